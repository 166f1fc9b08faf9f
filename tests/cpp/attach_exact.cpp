// attach_exact.cpp -- csrc/attach_math.h (the scalar rule of SPEC.md section 18) compiled for the host and put together the way
// k_attach puts it together (one row of A and one element of A * O per output element), for tests/test_attach_exact.py to
// compare bit for bit with the numpy model.
//   usage: attach_exact <blob in> <result out>
// in : u32 n, n_src, npal, 0; n_src * 16 f32 instance matrices; n_src * npal * 16 f32 palettes; n records of 20 words
// out: n * 16 f32
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blob_io.h"
#include <hip/hip_runtime.h>  // the stand-in of tests/cpp/hip_stub

#include "../../mt_renderer_amd/csrc/attach_math.h"

using namespace mtr;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    long size = 0;
    std::vector<uint32_t> blob = read_words(argv[1], &size);
    if (blob.size() < 4) return 2;
    const size_t n = blob[0], n_src = blob[1], npal = blob[2];
    if ((long)((4 + n_src * 16 + n_src * npal * 16 + n * MTR_ATTACH_WORDS) * 4) != size || n_src == 0) { std::fprintf(stderr, "blob size\n"); return 2; }
    const float* mats = reinterpret_cast<const float*>(blob.data() + 4);
    const float* pals = mats + n_src * 16;
    const uint32_t* recs = blob.data() + 4 + n_src * 16 + n_src * npal * 16;
    std::vector<float> out(n * 16);
    for (size_t r = 0; r < n; r++) {
        const uint32_t* rec = recs + r * MTR_ATTACH_WORDS;
        const uint32_t s = attach_instance(rec[0], (uint32_t)n_src), j = attach_joint(rec[1], (uint32_t)npal);
        const float* M = mats + (size_t)s * 16;
        const bool joint = j != MTR_ATTACH_NO_JOINT;
        float O[16], P[16] = {};
        if (joint) std::memcpy(P, pals + ((size_t)s * npal + j) * 16, 64);
        std::memcpy(O, rec + 4, 64);
        for (uint32_t e = 0; e < 16; e++) {
            const uint32_t i = e & 3u, c = e >> 2;
            const float m[4] = {M[i], M[4 + i], M[8 + i], M[12 + i]};
            float a[4];
            attach_joint_row(m, P, joint, rec[2], i, a);
            out[r * 16 + e] = attach_elem(a, O + c * 4);
        }
    }
    write_words(argv[2], out);
    return 0;
}
