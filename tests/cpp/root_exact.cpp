// root_exact.cpp -- csrc/root_math.h (the scalar rule of SPEC.md section 19) compiled for the host and put together the way
// k_root puts it together (four samples per step, the step's delta, the blend in order, the delta matrix, one element of
// M * D per output element), for tests/test_root_exact.py to compare bit for bit with the numpy model.
//   usage: root_exact <blob in> <result out>
// in : u32 tracks, J, C, joint, n, S, nkeys (track sets: the key total), 0; C x 4 words of clip table (first key, keys or ticks,
//      0, 0); C root flag words; uniform: the keys (12 f32 per joint key) -- tracks: C * J * 3 descriptors of 8 words, nkeys x 2
//      value words, nkeys u16 times padded to a word; n * S steps of 4 words; n * 16 f32 instance matrices
// out: n * 16 f32 deltas D, then n * 16 f32 M * D
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blob_io.h"
#include <hip/hip_runtime.h>  // the stand-in of tests/cpp/hip_stub

#include "../../mt_renderer_amd/csrc/root_math.h"

using namespace mtr;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    long size = 0;
    std::vector<uint32_t> blob = read_words(argv[1], &size);
    if (blob.size() < 8) return 2;
    const bool tracks = blob[0] != 0;
    const size_t J = blob[1], C = blob[2], joint = blob[3], n = blob[4], S = blob[5], nkeys = blob[6];
    const uint32_t* clips = blob.data() + 8;
    const uint32_t* rflags = clips + C * 4;
    const uint32_t* src = rflags + C;
    size_t src_words = 0;
    if (tracks) {
        src_words = C * J * 24 + nkeys * 2 + (nkeys + 1) / 2;
    } else {
        for (size_t c = 0; c < C; c++) src_words += (size_t)clips[c * 4 + 1] * J * 12;
    }
    const uint32_t* steps = src + src_words;
    const float* mats = reinterpret_cast<const float*>(steps + n * S * 4);
    if ((long)((8 + C * 5 + src_words + n * S * 4 + n * 16) * 4) != size || C == 0 || S == 0 || S > MTR_ROOT_MAX_STEPS || joint >= J) {
        std::fprintf(stderr, "blob size\n");
        return 2;
    }
    const float* keys = reinterpret_cast<const float*>(src);
    const uint32_t* values = src + C * J * 24;
    const uint16_t* times = reinterpret_cast<const uint16_t*>(values + nkeys * 2);
    std::vector<float> out(n * 32);
    for (size_t inst = 0; inst < n; inst++) {
        RootXf d[MTR_ROOT_MAX_STEPS];
        float w[MTR_ROOT_MAX_STEPS];
        for (size_t i = 0; i < S; i++) {
            const uint32_t* rec = steps + (inst * S + i) * 4;
            const uint32_t ci = rec[0] < C ? rec[0] : (uint32_t)C - 1u;
            float x, dx;
            std::memcpy(&x, rec + 1, 4);
            std::memcpy(&dx, rec + 2, 4);
            std::memcpy(&w[i], rec + 3, 4);
            const uint32_t N = clips[ci * 4 + 1];
            const RootPos pos = root_positions(x, dx, N, rflags[ci]);
            RootXf s4[4];
            for (int r = 0; r < 4; r++)
                s4[r] = tracks ? root_sample_tracks(src + ((size_t)ci * J + joint) * 24, values, times, N, pos.r[r])
                               : root_sample_uniform(keys, clips[ci * 4], N, (uint32_t)J, (uint32_t)joint, pos.r[r]);
            d[i] = root_step_delta(s4, pos.kind);
        }
        RootXf acc = d[0];
        for (size_t i = 1; i < S; i++) root_blend(acc, d[i], w[i]);
        AnimVec D[4];
        root_matrix(acc, D);
        const float* M = mats + inst * 16;
        for (uint32_t e = 0; e < 16; e++) {
            const uint32_t i = e & 3u, c = e >> 2;
            const float m[4] = {M[i], M[4 + i], M[8 + i], M[12 + i]};
            const float Dc[4] = {D[c].x, D[c].y, D[c].z, D[c].w};
            out[inst * 16 + e] = Dc[i];
            out[(n + inst) * 16 + e] = attach_elem(m, Dc);
        }
    }
    write_words(argv[2], out);
    return 0;
}
