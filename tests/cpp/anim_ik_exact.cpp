// anim_ik_exact.cpp -- csrc/anim_ik.h (the scalar solve of SPEC.md section 17), csrc/anim_blend.h's local matrix and
// csrc/pose_common.h's pose_mul compiled for the host, put together the way the k_anim_ik kernels put them together, for
// tests/test_anim_ik_exact.py to compare bit for bit with the numpy model.
//   usage: anim_ik_exact <blob in> <result out>
// in : u32 n, J, K, 0; J parent bytes padded to a word; K chains of 8 words; n * K targets of 8 words; then per instance and
//      joint 12 f32, the (T, Q, S) after the layer stack (t.xyz 0 | q.xyzw | s.xyz 0)
// out: per instance and joint 16 f32, the local matrix after the chains
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blob_io.h"
#include <hip/hip_runtime.h>  // the stand-in of tests/cpp/hip_stub: no vector types of floats
struct float4 {
    float x, y, z, w;
};
static inline float4 make_float4(float x, float y, float z, float w) {
    float4 r = {x, y, z, w};
    return r;
}

#include "../../mt_renderer_amd/csrc/anim_ik.h"
#include "../../mt_renderer_amd/csrc/pose_common.h"

using namespace mtr;

static float f32(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

static void rebuild(const AnimKey& r, float4* loc) {
    AnimVec M[4];
    anim_matrix(r, M);
    for (int c = 0; c < 4; c++) loc[c] = make_float4(M[c].x, M[c].y, M[c].z, M[c].w);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    long size = 0;
    std::vector<uint32_t> blob = read_words(argv[1], &size);
    const size_t n = blob[0], J = blob[1], K = blob[2], pw = (J + 3) / 4;
    if ((long)((4 + pw + K * 8 + n * K * 8 + n * J * 12) * 4) != size || J == 0 || J > 256 || K == 0 || K > 4) { std::fprintf(stderr, "blob size\n"); return 2; }
    const uint8_t* parents = reinterpret_cast<const uint8_t*>(blob.data() + 4);
    const uint32_t* chains = blob.data() + 4 + pw;
    const uint32_t* targets = chains + K * 8;
    const float* tqs = reinterpret_cast<const float*>(targets + n * K * 8);
    std::vector<std::vector<uint32_t>> paths(J);  // the root first, the joint last
    for (size_t j = 0; j < J; j++) {
        std::vector<uint32_t> up;
        for (size_t k = j;; k = parents[k]) {
            up.push_back((uint32_t)k);
            if (parents[k] == 255 || parents[k] == k) break;
        }
        paths[j].assign(up.rbegin(), up.rend());
    }
    std::vector<float> out(n * J * 16);
    std::vector<AnimKey> key(J);
    std::vector<float4> loc(J * 4);
    for (size_t i = 0; i < n; i++) {
        for (size_t j = 0; j < J; j++) {
            const float* p = tqs + (i * J + j) * 12;
            key[j].t = anim_vec(p[0], p[1], p[2], p[3]);
            key[j].q = anim_vec(p[4], p[5], p[6], p[7]);
            key[j].s = anim_vec(p[8], p[9], p[10], p[11]);
            rebuild(key[j], &loc[j * 4]);
        }
        for (size_t k = 0; k < K; k++) {
            const uint32_t* ch = chains + k * 8;
            const uint32_t* tg = targets + (i * K + k) * 8;
            const float e = anim_weight(f32(tg[3]));
            if (e == 0.0f) continue;
            const uint32_t a = ch[1], b = ch[2], c = ch[3];
            // the walk: pose_mul down a's path, parent on the left; P over the path without a
            const std::vector<uint32_t>& path = paths[a];
            float4 W[4], R[4];
            for (int q = 0; q < 4; q++) W[q] = loc[path[0] * 4 + q];
            AnimVec P = path.size() > 1 ? key[path[0]].q : anim_vec(0.0f, 0.0f, 0.0f, 1.0f);
            for (size_t s = 1; s < path.size(); s++) {
                float4 L[4];
                for (int q = 0; q < 4; q++) L[q] = loc[path[s] * 4 + q];
                if (s + 1 < path.size()) P = anim_qmul(P, key[path[s]].q);
                pose_mul(W, L, R);
                for (int q = 0; q < 4; q++) W[q] = R[q];
            }
            const IkVec3 pa = ik_vec3(W[3].x, W[3].y, W[3].z), g = ik_vec3(f32(tg[0]), f32(tg[1]), f32(tg[2]));
            if (ch[0] == 0u) {
                float4 L[4], Wb[4], Wc[4];
                for (int q = 0; q < 4; q++) L[q] = loc[b * 4 + q];
                pose_mul(W, L, Wb);
                for (int q = 0; q < 4; q++) L[q] = loc[c * 4 + q];
                pose_mul(Wb, L, Wc);
                ik_two_bone(pa, ik_vec3(Wb[3].x, Wb[3].y, Wb[3].z), ik_vec3(Wc[3].x, Wc[3].y, Wc[3].z), P, key[a].q, key[b].q, g,
                            ik_vec3(f32(tg[4]), f32(tg[5]), f32(tg[6])), (ch[7] & 1u) != 0u, e);
                rebuild(key[a], &loc[a * 4]);
                rebuild(key[b], &loc[b * 4]);
            } else {
                ik_aim(pa, P, key[a].q, ik_vec3(f32(ch[4]), f32(ch[5]), f32(ch[6])), g, e);
                rebuild(key[a], &loc[a * 4]);
            }
        }
        std::memcpy(&out[i * J * 16], loc.data(), J * 64);
    }
    write_words(argv[2], out);
    return 0;
}
