// anim_blend.h -- the scalar blend rules of SPEC.md sections 14 and 16 that k_anim.hip is made of: lerp, the dot product,
// nlerp, the local matrix, the Hamilton product, the layer weight and the two layer steps; the clamped weight itself is
// clip_math.h's.  Plain C++ besides the macro (clip_math.h's MTR_HD), so that tests/test_anim_layers_exact.py compiles this very source for the host (-ffp-contract=off) and compares it bit for bit
// with the numpy model of section 16.
//
// One rounded operation per operator; nothing here is fused (the including file is compiled with -ffp-contract=off).
#pragma once
#include "clip_math.h"

#if defined(__HIPCC__)
namespace mtr {
typedef float4 AnimVec;
}
#else
namespace mtr {
struct AnimVec {
    float x, y, z, w;
};
}
#endif

namespace mtr {

MTR_HD AnimVec anim_vec(float x, float y, float z, float w) {
    AnimVec r;
    r.x = x; r.y = y; r.z = z; r.w = w;
    return r;
}

// one joint's translation (xyz), rotation (xyzw) and scale (xyz)
struct AnimKey {
    AnimVec t, q, s;
};

MTR_HD float anim_lerp(float v0, float v1, float a) { return v0 + a * (v1 - v0); }

MTR_HD AnimVec anim_lerp4(const AnimVec& v0, const AnimVec& v1, float a) {
    return anim_vec(anim_lerp(v0.x, v1.x, a), anim_lerp(v0.y, v1.y, a), anim_lerp(v0.z, v1.z, a), anim_lerp(v0.w, v1.w, a));
}

MTR_HD float anim_dot(const AnimVec& p, const AnimVec& q) { return ((p.x * q.x + p.y * q.y) + p.z * q.z) + p.w * q.w; }

MTR_HD AnimVec anim_nlerp(const AnimVec& q0, AnimVec q1, float a) {
    if (anim_dot(q0, q1) < 0.0f) q1 = anim_vec(-q1.x, -q1.y, -q1.z, -q1.w);  // the shortest path; NaN compares false
    const AnimVec q = anim_lerp4(q0, q1, a);
    const float n2 = anim_dot(q, q);
    const float rn = 1.0f / sqrtf(n2);
    if (n2 == 0.0f || !(fabsf(rn) <= 3.402823466e38f)) return anim_vec(0.0f, 0.0f, 0.0f, 1.0f);
    return anim_vec(q.x * rn, q.y * rn, q.z * rn, q.w * rn);
}

// section 14's cross-fade of two (T, Q, S); section 16's OVERRIDE step is the same rule with e for the weight
MTR_HD AnimKey anim_mix(const AnimKey& k0, const AnimKey& k1, float a) {
    AnimKey r;
    r.t = anim_lerp4(k0.t, k1.t, a);
    r.q = anim_nlerp(k0.q, k1.q, a);
    r.s = anim_lerp4(k0.s, k1.s, a);
    return r;
}

// (T, Q, S) -> section 14's local matrix (column-major)
MTR_HD void anim_matrix(const AnimKey& r, AnimVec (&M)[4]) {
    const float x = r.q.x, y = r.q.y, z = r.q.z, qw = r.q.w;
    const float x2 = x + x, y2 = y + y, z2 = z + z;
    const float xx = x * x2, yy = y * y2, zz = z * z2, xy = x * y2, xz = x * z2, yz = y * z2;
    const float wx = qw * x2, wy = qw * y2, wz = qw * z2;
    M[0] = anim_vec((1.0f - (yy + zz)) * r.s.x, (xy + wz) * r.s.x, (xz - wy) * r.s.x, 0.0f);
    M[1] = anim_vec((xy - wz) * r.s.y, (1.0f - (xx + zz)) * r.s.y, (yz + wx) * r.s.y, 0.0f);
    M[2] = anim_vec((xz + wy) * r.s.z, (yz - wx) * r.s.z, (1.0f - (xx + yy)) * r.s.z, 0.0f);
    M[3] = anim_vec(r.t.x, r.t.y, r.t.z, 1.0f);
}

// the Hamilton product p q, in section 16's operation order
MTR_HD AnimVec anim_qmul(const AnimVec& p, const AnimVec& q) {
    return anim_vec(((p.w * q.x + p.x * q.w) + p.y * q.z) - p.z * q.y,
                    ((p.w * q.y - p.x * q.z) + p.y * q.w) + p.z * q.x,
                    ((p.w * q.z + p.x * q.y) - p.y * q.x) + p.z * q.w,
                    ((p.w * q.w - p.x * q.x) - p.y * q.y) - p.z * q.z);
}

// the effective weight of a layer on one joint: its clamped weight times the joint's mask weight
MTR_HD float anim_layer_weight(float w, float m) { return anim_weight(w) * m; }

// section 16's ADDITIVE step: the layer's (T, Q, S) are deltas from a reference pose
MTR_HD AnimKey anim_layer_additive(const AnimKey& r, const AnimKey& l, float e) {
    AnimKey o;
    const float p0 = e * l.t.x, p1 = e * l.t.y, p2 = e * l.t.z;
    o.t = anim_vec(r.t.x + p0, r.t.y + p1, r.t.z + p2, r.t.w);
    o.q = anim_nlerp(r.q, anim_qmul(r.q, l.q), e);
    const float d0 = e * (l.s.x - 1.0f), d1 = e * (l.s.y - 1.0f), d2 = e * (l.s.z - 1.0f);
    o.s = anim_vec(r.s.x * (1.0f + d0), r.s.y * (1.0f + d1), r.s.z * (1.0f + d2), r.s.w);
    return o;
}

// one layer over (T, Q, S) of a joint; e != 0 (a layer with e == 0 is skipped by the caller: nlerp(Q, ., 0) renormalises)
MTR_HD AnimKey anim_layer_step(const AnimKey& r, const AnimKey& l, float e, uint32_t mode) {
    return (mode & 1u) ? anim_layer_additive(r, l, e) : anim_mix(r, l, e);
}

}  // namespace mtr
