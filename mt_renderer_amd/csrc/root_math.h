// root_math.h -- the scalar rule of SPEC.md section 19 (root motion) that k_root.hip is made of: the positions of a step with
// its seam count m and the guard, the sample R(r) of the trajectory joint from either kind of animation set, the rigid delta
// between two samples, the composition of two deltas, the blend of an instance's steps and the delta matrix.  Plain C++
// besides the macro, like anim_ik.h, so that tests/test_root_exact.py compiles this very source for the host
// (-ffp-contract=off) and compares it bit for bit with the numpy model of section 19.
//
// One rounded operation per operator; nothing here is fused (the including file is compiled with -ffp-contract=off), '/'
// and sqrtf are correctly rounded, and no trigonometric function is called.  The helpers are those of anim_blend.h,
// anim_ik.h and anim_tracks.h; the one fma chain, M * D at the very end, is attach_math.h's attach_elem.
#pragma once
#include "anim_blend.h"
#include "anim_ik.h"
#include "anim_tracks.h"
#include "attach_math.h"

#ifndef MTR_ROOT_CYCLIC  // include/mtr.h has the same
#define MTR_ROOT_CYCLIC 1u
#define MTR_ROOT_MAX_STEPS 8
#endif

namespace mtr {

// a rigid transform: a translation and a rotation
struct RootXf {
    IkVec3 t;
    AnimVec q;
};

MTR_HD RootXf root_identity() {
    RootXf r;
    r.t = ik_vec3(0.0f, 0.0f, 0.0f);
    r.q = anim_vec(0.0f, 0.0f, 0.0f, 1.0f);
    return r;
}

// The four positions a step samples and how they combine.  kind ROOT_DIRECT: D = delta(r[0] -> r[3]).  ROOT_SEAM:
// D = delta(r[0] -> r[1]) o delta(r[2] -> r[3]), (r[1], r[2]) = (L, 0) for m = +1 and (0, L) for m = -1.  ROOT_IDENTITY:
// nothing sampled counts (a cyclic clip of one key, or the guard).  Every r is -0 or lies in [0, L] for every x and dx.
enum : uint32_t { ROOT_DIRECT = 0u, ROOT_SEAM = 1u, ROOT_IDENTITY = 2u };

struct RootPos {
    float r[4];
    uint32_t kind;
};

// n: the clip's key count or tick count (>= 1); flags: the root set's word of the clip (bit 0 is the only one set)
MTR_HD RootPos root_positions(float x, float dx, uint32_t n, uint32_t flags) {
    RootPos p;
    const float L = (float)(n - 1u);
    p.r[1] = L; p.r[2] = 0.0f;
    p.kind = ROOT_DIRECT;
    if (!(flags & MTR_ROOT_CYCLIC)) {
        const float y = x + dx;
        p.r[0] = track_position(x, n, 0u);  // section 14's clamp
        p.r[3] = track_position(y, n, 0u);
        return p;
    }
    p.r[0] = 0.0f; p.r[3] = 0.0f;
    if (n == 1u) {
        p.kind = ROOT_IDENTITY;
        return p;
    }
    const float r0 = clip_wrap(x, L);
    const float y = r0 + dx;
    float r1 = y;
    if (y < 0.0f) {
        r1 = y + L;
        p.kind = ROOT_SEAM; p.r[1] = 0.0f; p.r[2] = L;
    } else if (y >= L) {
        r1 = y - L;
        p.kind = ROOT_SEAM;
    }
    if (!(r1 >= 0.0f && r1 <= L)) {  // the guard: NaN compares false
        p.kind = ROOT_IDENTITY;
        return p;
    }
    p.r[0] = r0; p.r[3] = r1;
    return p;
}

MTR_HD RootXf root_mix(const AnimVec& t0, const AnimVec& t1, const AnimVec& q0, const AnimVec& q1, float at, float aq) {
    RootXf s;
    s.t = ik_vec3(anim_lerp(t0.x, t1.x, at), anim_lerp(t0.y, t1.y, at), anim_lerp(t0.z, t1.z, at));
    s.q = anim_nlerp(q0, q1, aq);
    return s;
}

// R(r) from uniform keys (12 floats per joint key, key-major, joint fastest); first: the clip's first key.  "One clip at r"
// of section 14 under the clamp rule: idempotent on a step's positions, and any float lands inside the clip
MTR_HD RootXf root_sample_uniform(const float* keys, uint32_t first, uint32_t nkeys, uint32_t J, uint32_t j, float r) {
    const AnimPos k = anim_position(r, nkeys, 0u);
    const float* p0 = keys + ((size_t)(first + k.i0) * J + j) * 12;
    const float* p1 = keys + ((size_t)(first + k.i1) * J + j) * 12;
    const AnimVec t0 = anim_vec(p0[0], p0[1], p0[2], 0.0f), q0 = anim_vec(p0[4], p0[5], p0[6], p0[7]);
    const AnimVec t1 = anim_vec(p1[0], p1[1], p1[2], 0.0f), q1 = anim_vec(p1[4], p1[5], p1[6], p1[7]);
    return root_mix(t0, t1, q0, q1, k.a, k.a);
}

// R(r) from a track set: desc points at the joint's three 8-word descriptors of the clip (translation, rotation, scale; the
// scale's is not read).  The two searches advance together, a step's probes in flight at once; then both time loads and
// the four value loads are issued before the first use.
MTR_HD RootXf root_sample_tracks(const uint32_t* desc, const uint32_t* values, const uint16_t* times, uint32_t nticks, float r) {
    const float pos = track_position(r, nticks, 0u);
    const uint32_t ft = desc[0], ct = desc[1], fq = desc[8], cq = desc[9];
    float lo[3], step[3];
    for (int i = 0; i < 3; i++) {
        __builtin_memcpy(&lo[i], desc + 2 + i, 4);
        __builtin_memcpy(&step[i], desc + 5 + i, 4);
    }
    TrackSearch st = track_search_begin(ft, ct), sq = track_search_begin(fq, cq);
    for (uint32_t left = ct | cq; left > 1u; left = track_search_left(left)) {
        const uint32_t tt = times[track_search_probe(st)], tq = times[track_search_probe(sq)];
        track_search_take(tt, pos, st);
        track_search_take(tq, pos, sq);
    }
    const uint32_t kt1 = track_next_key(ft, ct, st.base, 0u), kq1 = track_next_key(fq, cq, sq.base, 0u);
    const uint32_t tt1 = times[kt1], tq1 = times[kq1];
    const uint32_t vt0a = values[(size_t)st.base * 2], vt0b = values[(size_t)st.base * 2 + 1], vt1a = values[(size_t)kt1 * 2], vt1b = values[(size_t)kt1 * 2 + 1];
    const uint32_t vq0a = values[(size_t)sq.base * 2], vq0b = values[(size_t)sq.base * 2 + 1], vq1a = values[(size_t)kq1 * 2], vq1b = values[(size_t)kq1 * 2 + 1];
    const float at = track_fraction(pos, ft, ct, st.base, kt1, st.tk, tt1, nticks);
    const float aq = track_fraction(pos, fq, cq, sq.base, kq1, sq.tk, tq1, nticks);
    float t0[3], t1[3], q0[4], q1[4];
    track_decode_lin(vt0a, vt0b, lo, step, t0);
    track_decode_lin(vt1a, vt1b, lo, step, t1);
    track_decode_rot(vq0a, vq0b, q0);
    track_decode_rot(vq1a, vq1b, q1);
    return root_mix(anim_vec(t0[0], t0[1], t0[2], 0.0f), anim_vec(t1[0], t1[1], t1[2], 0.0f), anim_vec(q0[0], q0[1], q0[2], q0[3]),
                    anim_vec(q1[0], q1[1], q1[2], q1[3]), at, aq);
}

// delta(a -> b): b seen from a
MTR_HD RootXf root_delta(const RootXf& a, const RootXf& b) {
    const AnimVec ca = ik_conj(a.q);
    RootXf d;
    d.q = anim_qmul(ca, b.q);
    d.t = ik_qrot(ca, ik_sub(b.t, a.t));
    return d;
}

// d1 o d2: d2 carried out in the frame d1 ends in
MTR_HD RootXf root_compose(const RootXf& d1, const RootXf& d2) {
    RootXf d;
    d.t = ik_add(d1.t, ik_qrot(d1.q, d2.t));
    d.q = anim_qmul(d1.q, d2.q);
    return d;
}

// the delta of a step from the samples at its four positions; the rotation renormalised once
MTR_HD RootXf root_step_delta(const RootXf (&s)[4], uint32_t kind) {
    if (kind == ROOT_IDENTITY) return root_identity();
    RootXf d = kind == ROOT_SEAM ? root_compose(root_delta(s[0], s[1]), root_delta(s[2], s[3])) : root_delta(s[0], s[3]);
    d.q = ik_norm4(d.q);
    return d;
}

// one further step over the blend so far (section 16's OVERRIDE with mask 0); w as stored.  A step whose clamped weight is 0
// changes nothing: its delta is not read.
MTR_HD void root_blend(RootXf& acc, const RootXf& d, float w) {
    const float e = anim_weight(w);
    if (e == 0.0f) return;
    acc.t = ik_vec3(anim_lerp(acc.t.x, d.t.x, e), anim_lerp(acc.t.y, d.t.y, e), anim_lerp(acc.t.z, d.t.z, e));
    acc.q = anim_nlerp(acc.q, d.q, e);
}

// section 14's local matrix of (T, Q, S = (1, 1, 1)), column-major
MTR_HD void root_matrix(const RootXf& d, AnimVec (&M)[4]) {
    AnimKey k;
    k.t = anim_vec(d.t.x, d.t.y, d.t.z, 0.0f);
    k.q = d.q;
    k.s = anim_vec(1.0f, 1.0f, 1.0f, 0.0f);
    anim_matrix(k, M);
}

}  // namespace mtr
