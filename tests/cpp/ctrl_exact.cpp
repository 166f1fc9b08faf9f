// ctrl_exact.cpp -- csrc/ctrl_math.h (the scalar rule of SPEC.md section 21) compiled for the host and put together the way
// k_ctrl puts it together (one ctrl_step per instance on its own state, play state and parameter row, command slot i, one
// count per fire), for tests/test_ctrl_exact.py to compare bit for bit with the numpy model.
//   usage: ctrl_exact <blob in> <result out>
// in : u32 n, C, S, T, nany, NP, dt (f32 bits), 0; C x 4 words of clips (period, flags, 0, key count); S x 4 words of nodes;
//      T x 12 words of transitions; n x 4 words of states; n x 8 words of play states; n x NP parameters; T counts
// out: n x 4 words of states, n x NP parameters, n x 4 words of commands, T counts
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blob_io.h"
#include <hip/hip_runtime.h>  // the stand-in of tests/cpp/hip_stub

#include "../../mt_renderer_amd/csrc/ctrl_math.h"

using namespace mtr;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    long size = 0;
    std::vector<uint32_t> blob = read_words(argv[1], &size);
    if (blob.size() < 8) return 2;
    const size_t n = blob[0], C = blob[1], S = blob[2], T = blob[3], nany = blob[4], NP = blob[5];
    float dt;
    std::memcpy(&dt, &blob[6], 4);
    if ((long)((8 + C * 4 + S * 4 + T * 12 + n * 4 + n * 8 + n * NP + T) * 4) != size || C == 0 || S == 0 || n == 0) {
        std::fprintf(stderr, "blob size\n");
        return 2;
    }
    const uint32_t* at = blob.data() + 8;
    std::vector<PlayClip> clips(C);
    std::memcpy(clips.data(), at, C * 16); at += C * 4;
    std::vector<CtrlWord> nodes(S), trans(T * 3 + 1);
    std::memcpy(nodes.data(), at, S * 16); at += S * 4;
    std::memcpy(trans.data(), at, T * 48); at += T * 12;
    std::vector<CtrlState> states(n);
    std::memcpy(states.data(), at, n * 16); at += n * 4;
    std::vector<PlayState> play(n);
    std::memcpy(play.data(), at, n * 32); at += n * 8;
    std::vector<float> params(n * NP + 1);
    std::memcpy(params.data(), at, n * NP * 4); at += n * NP;
    std::vector<uint32_t> counts(at, at + T);
    CtrlTables tb;
    tb.nodes = nodes.data(); tb.trans = trans.data(); tb.clips = clips.data();
    tb.nnodes = (uint32_t)S; tb.nany = (uint32_t)nany; tb.nclips = (uint32_t)C; tb.nparams = (uint32_t)NP;
    std::vector<uint32_t> out(n * 4 + n * NP + n * 4 + T);
    uint32_t* o_cmds = out.data() + n * 4 + n * NP;
    for (size_t inst = 0; inst < n; inst++) {
        const CtrlStep r = ctrl_step(states[inst], play[inst], NP ? params.data() + inst * NP : nullptr, (uint32_t)inst, dt, tb);
        std::memcpy(&out[inst * 4], &states[inst], 16);
        std::memcpy(o_cmds + inst * 4, &r.cmd, 16);
        if (r.fired != MTR_CTRL_NONE) {
            if (r.fired >= T) return 3;
            counts[r.fired] += 1u;
        }
    }
    std::memcpy(out.data() + n * 4, params.data(), n * NP * 4);
    if (T) std::memcpy(o_cmds + n * 4, counts.data(), T * 4);
    write_words(argv[2], out);
    return 0;
}
