// play_exact.cpp -- csrc/play_math.h (the scalar rule of SPEC.md section 20) compiled for the host and put together the way
// k_play puts it together (the largest command index + 1 per instance in a zeroed scratch array, then one play_advance per
// instance), for tests/test_player_exact.py to compare bit for bit with the numpy model.
//   usage: play_exact <blob in> <result out>
// in : u32 n, C, m, dt (f32 bits); C x 4 words of table (period, flags, rate, key count); n x 8 words of states; m x 4 words
//      of commands
// out: n x 8 words of states, then n x 9 words of frame (clip_a, clip_b, x_a', x_b', w_out, x0_a, dx_a, x0_b, dx_b)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blob_io.h"
#include <hip/hip_runtime.h>  // the stand-in of tests/cpp/hip_stub

#include "../../mt_renderer_amd/csrc/play_math.h"

using namespace mtr;

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    long size = 0;
    std::vector<uint32_t> blob = read_words(argv[1], &size);
    if (blob.size() < 4) return 2;
    const size_t n = blob[0], C = blob[1], m = blob[2];
    float dt;
    std::memcpy(&dt, &blob[3], 4);
    if ((long)((4 + C * 4 + n * 8 + m * 4) * 4) != size || C == 0 || n == 0) {
        std::fprintf(stderr, "blob size\n");
        return 2;
    }
    std::vector<PlayClip> table(C);
    std::memcpy(table.data(), blob.data() + 4, C * 16);
    std::vector<PlayState> states(n);
    std::memcpy(states.data(), blob.data() + 4 + C * 4, n * 32);
    std::vector<PlayCmd> cmds(m ? m : 1);
    std::memcpy(cmds.data(), blob.data() + 4 + C * 4 + n * 8, m * 16);
    std::vector<uint32_t> scratch(n, 0u);
    for (size_t i = 0; i < m; i++)
        if (cmds[i].instance < n && scratch[cmds[i].instance] < i + 1) scratch[cmds[i].instance] = (uint32_t)i + 1u;
    std::vector<uint32_t> out(n * 17);
    for (size_t inst = 0; inst < n; inst++) {
        const uint32_t slot = scratch[inst];
        const PlayFrame fr = play_advance(states[inst], slot ? &cmds[slot - 1] : nullptr, dt, table.data(), (uint32_t)C);
        std::memcpy(&out[inst * 8], &states[inst], 32);
        uint32_t* o = &out[n * 8 + inst * 9];
        o[0] = fr.clip_a; o[1] = fr.clip_b; o[2] = bits(fr.x_a); o[3] = bits(fr.x_b); o[4] = bits(fr.w);
        o[5] = bits(fr.x0_a); o[6] = bits(fr.dx_a); o[7] = bits(fr.x0_b); o[8] = bits(fr.dx_b);
    }
    write_words(argv[2], out);
    return 0;
}
