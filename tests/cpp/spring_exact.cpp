// spring_exact.cpp -- csrc/spring_math.h (the scalar rule of SPEC.md section 24), csrc/anim_blend.h's local matrix and
// csrc/pose_common.h's pose_mul compiled for the host, put together the way the k_anim_spring kernels put them together
// (by rounds, each spring over its own path), for tests/test_spring_exact.py to compare bit for bit with the numpy model.
//   usage: spring_exact <blob in> <result out>
// in : u32 n, J, K, has_motion; f32 dt, 3 words 0; J parent bytes padded to a word; K springs of 12 words; n * K states of
//      8 words; n * 16 f32 of motion if has_motion; then per instance and joint 12 f32, the (T, Q, S) after the chains
//      (t.xyz 0 | q.xyzw | s.xyz 0)
// out: per instance and joint 16 f32, the local matrix after the springs; then n * K states of 8 words
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

#include "../../mt_renderer_amd/csrc/spring_math.h"
#include "../../mt_renderer_amd/csrc/pose_common.h"

using namespace mtr;

static float f32(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static uint32_t u32(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
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
    const bool moved = blob[3] != 0;
    const float dt = f32(blob[4]);
    if ((long)((8 + pw + K * 12 + n * K * 8 + (moved ? n * 16 : 0) + n * J * 12) * 4) != size || J == 0 || J > 256 || K == 0 || K > 16) {
        std::fprintf(stderr, "blob size\n");
        return 2;
    }
    const uint8_t* parents = reinterpret_cast<const uint8_t*>(blob.data() + 8);
    const uint32_t* springs = blob.data() + 8 + pw;
    const uint32_t* states = springs + K * 12;
    const float* motion = reinterpret_cast<const float*>(states + n * K * 8);
    const float* tqs = motion + (moved ? n * 16 : 0);
    std::vector<std::vector<uint32_t>> paths(J);  // the root first, the joint last
    for (size_t j = 0; j < J; j++) {
        std::vector<uint32_t> up;
        for (size_t k = j;; k = parents[k]) {
            up.push_back((uint32_t)k);
            if (parents[k] == 255 || parents[k] == k) break;
        }
        paths[j].assign(up.rbegin(), up.rend());
    }
    // a spring's round: the spring joints among its joint's ancestors
    std::vector<int> spring_of(J, -1);
    for (size_t k = 0; k < K; k++) spring_of[springs[k * 12]] = (int)k;
    std::vector<uint32_t> round(K, 0);
    uint32_t R = 0;
    for (size_t k = 0; k < K; k++) {
        const std::vector<uint32_t>& path = paths[springs[k * 12]];
        for (size_t s = 0; s + 1 < path.size(); s++) round[k] += spring_of[path[s]] >= 0;
        if (round[k] + 1 > R) R = round[k] + 1;
    }
    std::vector<float> out(n * J * 16);
    std::vector<uint32_t> out_states(n * K * 8);
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
        SpringMotion D = {};
        if (moved) {
            const float* m = motion + i * 16;
            D.c0 = ik_vec3(m[0], m[1], m[2]); D.c1 = ik_vec3(m[4], m[5], m[6]); D.c2 = ik_vec3(m[8], m[9], m[10]); D.t = ik_vec3(m[12], m[13], m[14]);
        }
        for (uint32_t rd = 0; rd < R; rd++)
            for (size_t k = 0; k < K; k++) {
                if (round[k] != rd) continue;
                const uint32_t* sp = springs + k * 12;
                const uint32_t* st = states + (i * K + k) * 8;
                const uint32_t a = sp[0];
                // the walk: pose_mul down a's path, parent on the left; P over the path without a
                const std::vector<uint32_t>& path = paths[a];
                float4 W[4], Rm[4];
                for (int q = 0; q < 4; q++) W[q] = loc[path[0] * 4 + q];
                AnimVec P = path.size() > 1 ? key[path[0]].q : anim_vec(0.0f, 0.0f, 0.0f, 1.0f);
                for (size_t s = 1; s < path.size(); s++) {
                    float4 L[4];
                    for (int q = 0; q < 4; q++) L[q] = loc[path[s] * 4 + q];
                    if (s + 1 < path.size()) P = anim_qmul(P, key[path[s]].q);
                    pose_mul(W, L, Rm);
                    for (int q = 0; q < 4; q++) W[q] = Rm[q];
                }
                SpringState s;
                s.cur = ik_vec3(f32(st[0]), f32(st[1]), f32(st[2]));
                s.live = st[3];
                s.prev = ik_vec3(f32(st[4]), f32(st[5]), f32(st[6]));
                spring_step(ik_vec3(W[3].x, W[3].y, W[3].z), P, key[a].q, ik_vec3(f32(sp[4]), f32(sp[5]), f32(sp[6])), ik_vec3(f32(sp[8]), f32(sp[9]), f32(sp[10])),
                            f32(sp[2]), f32(sp[3]), dt, moved, D, s);
                rebuild(key[a], &loc[a * 4]);
                uint32_t* o = &out_states[(i * K + k) * 8];
                o[0] = u32(s.cur.x); o[1] = u32(s.cur.y); o[2] = u32(s.cur.z); o[3] = s.live;
                o[4] = u32(s.prev.x); o[5] = u32(s.prev.y); o[6] = u32(s.prev.z); o[7] = 0u;
            }
        std::memcpy(&out[i * J * 16], loc.data(), J * 64);
    }
    write_words(argv[2], out, out_states);
    return 0;
}
