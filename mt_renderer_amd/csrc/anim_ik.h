// anim_ik.h -- the scalar solve of SPEC.md section 17 (inverse kinematics) that the k_anim_ik kernels are made of: dot3, the
// cross product, the rotation of a vector by a quaternion, the shortest arc between two vectors, the two-bone reach and
// the aim.  Plain C++ besides the macro, like anim_blend.h, so that tests/test_anim_ik_exact.py compiles this very source
// for the host (-ffp-contract=off) and compares it bit for bit with the numpy model of section 17.
//
// One rounded operation per operator; nothing here is fused (the including file is compiled with -ffp-contract=off), '/'
// and sqrtf are correctly rounded, and no trigonometric function is called.
#pragma once
#include "anim_blend.h"

namespace mtr {

struct IkVec3 {
    float x, y, z;
};

MTR_HD IkVec3 ik_vec3(float x, float y, float z) {
    IkVec3 r;
    r.x = x; r.y = y; r.z = z;
    return r;
}

MTR_HD IkVec3 ik_sub(const IkVec3& u, const IkVec3& v) { return ik_vec3(u.x - v.x, u.y - v.y, u.z - v.z); }
MTR_HD IkVec3 ik_add(const IkVec3& u, const IkVec3& v) { return ik_vec3(u.x + v.x, u.y + v.y, u.z + v.z); }
MTR_HD IkVec3 ik_scale(float s, const IkVec3& v) { return ik_vec3(s * v.x, s * v.y, s * v.z); }
MTR_HD IkVec3 ik_div(const IkVec3& v, float s) { return ik_vec3(v.x / s, v.y / s, v.z / s); }

MTR_HD float ik_dot3(const IkVec3& u, const IkVec3& v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
MTR_HD float ik_len(const IkVec3& v) { return sqrtf(ik_dot3(v, v)); }

MTR_HD IkVec3 ik_cross(const IkVec3& u, const IkVec3& v) {
    return ik_vec3(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x);
}

MTR_HD AnimVec ik_conj(const AnimVec& q) { return anim_vec(-q.x, -q.y, -q.z, q.w); }

// section 14's renormalisation: the identity when the norm is 0 or its reciprocal root is not finite
MTR_HD AnimVec ik_norm4(const AnimVec& q) {
    const float n2 = anim_dot(q, q);
    const float rn = 1.0f / sqrtf(n2);
    if (n2 == 0.0f || !(fabsf(rn) <= 3.402823466e38f)) return anim_vec(0.0f, 0.0f, 0.0f, 1.0f);
    return anim_vec(q.x * rn, q.y * rn, q.z * rn, q.w * rn);
}

// v rotated by q: t = 2 (q.xyz x v), v + q.w t + q.xyz x t
MTR_HD IkVec3 ik_qrot(const AnimVec& q, const IkVec3& v) {
    const IkVec3 a = ik_vec3(q.x, q.y, q.z);
    IkVec3 t = ik_cross(a, v);
    t = ik_add(t, t);
    return ik_add(ik_add(v, ik_scale(q.w, t)), ik_cross(a, t));
}

// the shortest arc that turns u towards v; exactly antiparallel vectors (and a zero vector) give the identity
MTR_HD AnimVec ik_fromto(const IkVec3& u, const IkVec3& v) {
    const IkVec3 c = ik_cross(u, v);
    const float w = sqrtf(ik_dot3(u, u) * ik_dot3(v, v)) + ik_dot3(u, v);
    return ik_norm4(anim_vec(c.x, c.y, c.z, w));
}

// TWO_BONE.  pa, pb, pc: the world positions of the chain's joints; P: the world rotation above a; qa, qb: the local
// rotations of a and b, replaced when the guard holds; g: the target position; pole: the pole position, read only with
// use_pole; e: the clamped weight, != 0 (the caller skips a chain with e == 0 before it reads anything).  Returns whether
// the guard held; when it did not, qa and qb are untouched bit for bit.
MTR_HD bool ik_two_bone(const IkVec3& pa, const IkVec3& pb, const IkVec3& pc, const AnimVec& P, AnimVec& qa, AnimVec& qb,
                              const IkVec3& g, const IkVec3& pole, bool use_pole, float e) {
    const IkVec3 ab = ik_sub(pb, pa), bc = ik_sub(pc, pb);
    const float la = ik_len(ab), lb = ik_len(bc);
    const IkVec3 d = ik_sub(g, pa);
    const float dist = ik_len(d);
    const float lo = fabsf(la - lb), hi = la + lb;
    float lt = dist;
    if (lt < lo) lt = lo;
    if (lt > hi) lt = hi;
    const IkVec3 n = ik_div(d, dist);
    const IkVec3 u = use_pole ? ik_sub(pole, pa) : ab;
    const IkVec3 h = ik_sub(u, ik_scale(ik_dot3(u, n), n));
    const float hl = ik_len(h);
    if (!(la > 0.0f && lb > 0.0f && dist > 0.0f && lt > 0.0f && hl > 0.0f && dist <= 3.402823466e38f)) return false;  // NaN compares false
    const IkVec3 hh = ik_div(h, hl);
    const float x = ((la * la - lb * lb) + lt * lt) / (lt + lt);
    const float y2 = la * la - x * x;
    const float y = y2 > 0.0f ? sqrtf(y2) : 0.0f;
    const IkVec3 pb1 = ik_add(ik_add(pa, ik_scale(x, n)), ik_scale(y, hh));
    const IkVec3 pc1 = ik_add(pa, ik_scale(lt, n));
    const AnimVec Ra = ik_fromto(ab, ik_sub(pb1, pa));
    const IkVec3 pcs = ik_add(pa, ik_qrot(Ra, ik_sub(pc, pa)));
    const AnimVec Rb = ik_fromto(ik_sub(pcs, pb1), ik_sub(pc1, pb1));
    const AnimVec A = anim_qmul(Ra, anim_qmul(P, qa));
    const AnimVec qa1 = anim_qmul(ik_conj(P), A);
    const AnimVec B = anim_qmul(Rb, anim_qmul(A, qb));
    const AnimVec qb1 = anim_qmul(ik_conj(A), B);
    qa = anim_nlerp(qa, qa1, e);
    qb = anim_nlerp(qb, qb1, e);
    return true;
}

// AIM.  pa: the world position of a; P: the world rotation above a; qa: the local rotation of a, replaced when the guard
// holds; axis: the chain's axis in a's local space; g: the target position; e != 0.
MTR_HD bool ik_aim(const IkVec3& pa, const AnimVec& P, AnimVec& qa, const IkVec3& axis, const IkVec3& g, float e) {
    const AnimVec A0 = anim_qmul(P, qa);
    const IkVec3 cur = ik_qrot(A0, axis);
    const IkVec3 v = ik_sub(g, pa);
    if (!(ik_len(v) > 0.0f && ik_len(cur) > 0.0f)) return false;  // NaN compares false
    const AnimVec qa1 = anim_qmul(ik_conj(P), anim_qmul(ik_fromto(cur, v), A0));
    qa = anim_nlerp(qa, qa1, e);
    return true;
}

}  // namespace mtr
