// anim_layers_exact.cpp -- csrc/anim_blend.h (the scalar blend rules of SPEC.md sections 14 and 16 that k_anim.hip is made
// of) compiled for the host, for tests/test_anim_layers_exact.py to compare bit for bit with the numpy model.
//   usage: anim_layers_exact <blob in> <result out>
// in : u32 n, J, L, 0; then per instance and layer: f32 w, u32 mode; then per instance, layer and joint 28 f32: the mask
//      weight m, the fractions a of translation, rotation and scale, key 0 (t.xyz 0 | q.xyzw | s.xyz 0) and key 1
// out: per instance and joint 12 f32, the (T, Q, S) after the last layer; then per instance, layer and joint e
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blob_io.h"
#include "../../mt_renderer_amd/csrc/anim_blend.h"

static mtr::AnimKey key_at(const float* k) {
    mtr::AnimKey r;
    r.t = mtr::anim_vec(k[0], k[1], k[2], k[3]);
    r.q = mtr::anim_vec(k[4], k[5], k[6], k[7]);
    r.s = mtr::anim_vec(k[8], k[9], k[10], k[11]);
    return r;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    long size = 0;
    std::vector<uint32_t> blob = read_words(argv[1], &size);
    const size_t n = blob[0], J = blob[1], L = blob[2];
    const uint32_t* head = blob.data() + 4;
    const float* per = reinterpret_cast<const float*>(head + n * L * 2);
    if ((long)((4 + n * L * 2 + n * L * J * 28) * 4) != size) { std::fprintf(stderr, "blob size\n"); return 2; }
    std::vector<float> out(n * J * 12 + n * L * J);
    float* es = out.data() + n * J * 12;
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < J; j++) {
            mtr::AnimKey r = {};
            for (size_t l = 0; l < L; l++) {
                float w;
                std::memcpy(&w, &head[(i * L + l) * 2], 4);
                const uint32_t mode = head[(i * L + l) * 2 + 1];
                const float* p = per + ((i * L + l) * J + j) * 28;
                const mtr::AnimKey k0 = key_at(p + 4), k1 = key_at(p + 16);
                mtr::AnimKey v;  // what both sources of k_anim.hip make of two keys
                v.t = mtr::anim_lerp4(k0.t, k1.t, p[1]);
                v.q = mtr::anim_nlerp(k0.q, k1.q, p[2]);
                v.s = mtr::anim_lerp4(k0.s, k1.s, p[3]);
                const float e = l ? mtr::anim_layer_weight(w, p[0]) : 1.0f;
                es[(i * L + l) * J + j] = e;
                if (l == 0) r = v;
                else if (e != 0.0f) r = mtr::anim_layer_step(r, v, e, mode);
            }
            const float tqs[12] = {r.t.x, r.t.y, r.t.z, 0.0f, r.q.x, r.q.y, r.q.z, r.q.w, r.s.x, r.s.y, r.s.z, 0.0f};
            std::memcpy(&out[(i * J + j) * 12], tqs, sizeof(tqs));
        }
    write_words(argv[2], out);
    return 0;
}
