// spring_math.h -- the scalar rule of SPEC.md section 24 (spring bones) that the k_anim_spring kernels are made of: the
// freshness test of a state record, the carry of a particle by an instance's rigid delta, one integration step, the length
// constraint and the aim.  Plain C++ besides the macro, like anim_ik.h, so that tests/test_spring_exact.py compiles this
// very source for the host (-ffp-contract=off) and compares it bit for bit with the numpy model of section 24.
//
// One rounded operation per operator, section 17's operators throughout; nothing here is fused.
#pragma once
#include "anim_ik.h"

namespace mtr {

// a state record (mtr_spring_state) as the rule holds it; pad is written as 0
struct SpringState {
    IkVec3 cur;
    uint32_t live;
    IkVec3 prev;
};

// the rigid delta an instance moved by this frame (M_new = M_old o D): the columns of its rotation and its translation
struct SpringMotion {
    IkVec3 c0, c1, c2, t;
};

MTR_HD bool spring_finite(float x) { return fabsf(x) <= 3.402823466e38f; }  // NaN compares false
MTR_HD bool spring_finite3(const IkVec3& v) { return spring_finite(v.x) && spring_finite(v.y) && spring_finite(v.z); }

// p seen from the instance's new model space: R^T (p - t), the inverse of a rigid D
MTR_HD IkVec3 spring_carry(const SpringMotion& D, const IkVec3& p) {
    const IkVec3 u = ik_sub(p, D.t);
    return ik_vec3(ik_dot3(D.c0, u), ik_dot3(D.c1, u), ik_dot3(D.c2, u));
}

// One step of one spring.  pa: the world position of the joint; P: the world rotation above it; qa: the joint's local
// rotation, replaced when the aim's guard holds; tail, gravity, stiffness, drag: the spring's record, validated on the host
// (tail finite and not zero, stiffness finite and >= 0, drag in [0, 1], gravity finite); dt: the call's, any bit pattern;
// moved, D: whether the instance has a delta, and that delta (not read otherwise); st: the state record, any bit pattern
// in, the new record out (live = 1).  Returns whether the aim's guard held; when it did not, qa is untouched bit for bit.
MTR_HD bool spring_step(const IkVec3& pa, const AnimVec& P, AnimVec& qa, const IkVec3& tail, const IkVec3& gravity, float stiffness, float drag,
                              float dt, bool moved, const SpringMotion& D, SpringState& st) {
    const AnimVec A0 = anim_qmul(P, qa);
    const IkVec3 d0 = ik_qrot(A0, tail);
    const float L = ik_len(d0);
    const IkVec3 r = ik_add(pa, d0);  // where the particle rests
    const bool fresh = st.live == 0u || !spring_finite3(st.cur) || !spring_finite3(st.prev);
    const float h = dt > 0.0f && dt <= 3.402823466e38f ? dt : 0.0f;  // NaN, +inf, 0 and negative steps pause the spring
    IkVec3 c = r, p = r;
    if (!fresh) {
        c = st.cur; p = st.prev;
        if (moved) { c = spring_carry(D, c); p = spring_carry(D, p); }
        if (h > 0.0f) {
            const IkVec3 v = ik_scale(1.0f - drag, ik_sub(c, p));
            const float sh = stiffness * h;
            const float kk = sh < 1.0f ? sh : 1.0f;  // +inf clamps; sh is never NaN (both factors finite)
            const IkVec3 n = ik_add(ik_add(ik_add(c, v), ik_scale(kk, ik_sub(r, c))), ik_scale(h, gravity));
            p = c; c = n;
        }
    }
    const IkVec3 u = ik_sub(c, pa);
    const float ul = ik_len(u);
    c = ul > 0.0f && ul <= 3.402823466e38f && L > 0.0f ? ik_add(pa, ik_scale(L / ul, u)) : r;
    st.cur = c; st.live = 1u; st.prev = p;
    return ik_aim(pa, P, qa, tail, c, 1.0f);
}

}  // namespace mtr
