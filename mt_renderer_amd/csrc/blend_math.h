// blend_math.h -- the scalar rule of SPEC.md section 23 (blend spaces) that k_blend.hip is made of: the smoothing of the
// parameters, the two or three samples around the point with their sequential weights (a bracket search in a 1-D space, the
// first triangle that holds the point in a 2-D space, the closest point on any edge where none does), the shared phase
// advanced at the blended rate, and the records of the frame.  Plain C++ besides the macro, like play_math.h, so that
// tests/test_blend_exact.py compiles this very source for the host (-ffp-contract=off) and compares it bit for bit with the
// numpy model of section 23.
//
// One rounded operation per operator; nothing here is fused (the including file is compiled with -ffp-contract=off; the section
// has no fma at all) and '/' is correctly rounded.  NaN compares false, which every test below is written for.
#pragma once
#include "play_math.h"

namespace mtr {

// mtr_blend_sample, mtr_blend_tri, mtr_blend_state: 16 bytes each
struct alignas(16) BlendSample {
    uint32_t clip;
    float px, py;
    uint32_t pad;
};
struct alignas(16) BlendTri {
    uint32_t v[3];
    uint32_t pad;
};
struct alignas(16) BlendState {
    float phase, px, py, speed;
};

// a blend set as its kernel sees it: the tables were validated at creation (a sample's clip < nclips and LOOP, a triangle's
// indices < nsamples, its doubled area finite and > 0, a 1-D space's px strictly increasing with finite differences)
struct BlendTables {
    const PlayClip* clips;       // nclips entries: period, flags, rate, key count
    const BlendSample* samples;  // nsamples (1..32)
    const BlendTri* tris;        // ntris (0..64); 0: a 1-D space
    uint32_t nclips, nsamples, ntris;
    uint32_t param_x, param_y, nparams;  // param_x, param_y < nparams (1..16)
    float damp;                  // > 0, +inf: no smoothing
};

// what a frame writes besides the state: per slot the clip, the position of the pose, the position before the advance and the
// step (motion), the sequential weight (e[0] = +0) and the effective share
struct BlendFrame {
    uint32_t clip[3];
    float x[3], x0[3], dx[3], e[3], share[3];
};

// the three slots and the two sequential weights of step 3
struct BlendSlots {
    uint32_t s[3];
    float e1, e2;
};

MTR_HD bool blend_finite(float v) { return fabsf(v) <= PLAY_FLT_MAX; }

// step 2: one parameter smoothed towards its target
MTR_HD float blend_smooth(float p, float t, float a) {
    if (a == 1.0f || !blend_finite(p)) return t;
    const float d = t - p, m = a * d;
    return p + m;
}

// the doubled area of a triangle, in the operation order of the creation check
MTR_HD float blend_area(float x0, float y0, float x1, float y1, float x2, float y2) {
    const float ax = x1 - x0, ay = y1 - y0, bx = x2 - x0, by = y2 - y0;
    const float m0 = ax * by, m1 = bx * ay;
    return m0 - m1;
}

MTR_HD float blend_dot2(float ux, float uy, float vx, float vy) {
    const float m0 = ux * vx, m1 = uy * vy;
    return m0 + m1;
}

// step 3 in a 1-D space
MTR_HD BlendSlots blend_slots_1d(float p, const BlendTables& t) {
    BlendSlots r;
    r.e1 = 0.0f; r.e2 = 0.0f;
    const uint32_t top = t.nsamples - 1u;
    if (!(p > t.samples[0].px)) { r.s[0] = r.s[1] = r.s[2] = 0u; return r; }
    if (p >= t.samples[top].px) { r.s[0] = r.s[1] = r.s[2] = top; return r; }
    uint32_t j = 0;  // px[0] < p < px[top]: top >= 1 and j ends in 0..top - 1
    for (uint32_t k = 1; k < top; k++)
        if (t.samples[k].px <= p) j = k;
    const float lo = t.samples[j].px, hi = t.samples[j + 1u].px;
    const float num = p - lo, den = hi - lo;
    r.s[0] = j; r.s[1] = j + 1u; r.s[2] = j;
    r.e1 = num / den;
    return r;
}

// step 3 in a 2-D space.  Both loops run over every triangle with a uniform index; a lane that has its triangle skips the
// rest of the first loop's bodies, and only a lane without one enters the second: what a lane computes does not depend on
// where the other lanes of its wave are.
MTR_HD BlendSlots blend_slots_2d(float px, float py, const BlendTables& t) {
    BlendSlots r;
    bool hit = false;
    for (uint32_t k = 0; k < t.ntris; k++) {
        if (hit) continue;
        const BlendTri tr = t.tris[k];
        const BlendSample a = t.samples[tr.v[0]], b = t.samples[tr.v[1]], c = t.samples[tr.v[2]];
        const float A = blend_area(a.px, a.py, b.px, b.py, c.px, c.py);
        const float qx = px - a.px, qy = py - a.py;
        const float bx = b.px - a.px, by = b.py - a.py, cx = c.px - a.px, cy = c.py - a.py;
        const float n1a = qx * cy, n1b = cx * qy, n1 = n1a - n1b;
        const float n2a = bx * qy, n2b = qx * by, n2 = n2a - n2b;
        const float l1 = n1 / A, l2 = n2 / A;
        const float h = 1.0f - l1, l0 = h - l2;
        if (l0 >= 0.0f && l1 >= 0.0f && l2 >= 0.0f) {
            hit = true;
            r.s[0] = tr.v[0]; r.s[1] = tr.v[1]; r.s[2] = tr.v[2];
            r.e2 = anim_weight(l2);
            const float om = 1.0f - l2;
            r.e1 = om == 0.0f ? 0.0f : anim_weight(l1 / om);
        }
    }
    if (hit) return r;
    // the fallback: the closest point on any edge; the first candidate wins ties and a NaN never wins
    uint32_t ba = t.tris[0].v[0], bb = ba;
    float bt = 0.0f, bd = INFINITY;
    for (uint32_t k = 0; k < t.ntris; k++) {
        const BlendTri tr = t.tris[k];
        for (uint32_t e = 0; e < 3u; e++) {
            const uint32_t ia = tr.v[e], ib = tr.v[e == 2u ? 0u : e + 1u];
            const BlendSample a = t.samples[ia], b = t.samples[ib];
            const float ex = b.px - a.px, ey = b.py - a.py;
            const float qx = px - a.px, qy = py - a.py;
            const float num = blend_dot2(qx, qy, ex, ey), den = blend_dot2(ex, ey, ex, ey);
            const float tt = anim_weight(num / den);
            const float mx = tt * ex, my = tt * ey;
            const float cx = a.px + mx, cy = a.py + my;
            const float dx = px - cx, dy = py - cy;
            const float d2 = blend_dot2(dx, dy, dx, dy);
            if (d2 < bd) { bd = d2; ba = ia; bb = ib; bt = tt; }
        }
    }
    r.s[0] = ba; r.s[1] = bb; r.s[2] = ba;
    r.e1 = bt; r.e2 = 0.0f;
    return r;
}

// Steps 1 to 6 of section 23 for one instance.  st: the stored state, rewritten (speed kept); row: the instance's nparams
// parameters, read only.
MTR_HD BlendFrame blend_advance(BlendState& st, const float* row, float dt, const BlendTables& t) {
    const bool two_d = t.ntris != 0u;
    // 1. target, 2. smooth
    const float dtp = dt > 0.0f ? dt : 0.0f;
    const float a = anim_weight(dtp * t.damp);
    const float px = blend_smooth(st.px, row[t.param_x], a);
    const float py = two_d ? blend_smooth(st.py, row[t.param_y], a) : st.py;
    // 3. slots
    const BlendSlots sl = two_d ? blend_slots_2d(px, py, t) : blend_slots_1d(px, t);
    BlendFrame f;
    f.e[0] = 0.0f; f.e[1] = sl.e1; f.e[2] = sl.e2;
    const float om2 = 1.0f - sl.e2, om1 = 1.0f - sl.e1;
    f.share[0] = om1 * om2; f.share[1] = sl.e1 * om2; f.share[2] = sl.e2;
    // 4. phase
    float s = dt * st.speed;
    if (!blend_finite(s)) s = 0.0f;
    float P[3], fr[3];
    for (int i = 0; i < 3; i++) {
        f.clip[i] = t.samples[sl.s[i]].clip;
        const PlayClip c = t.clips[f.clip[i]];
        P[i] = c.period;
        fr[i] = c.rate / c.period;
    }
    float fq = fr[0];
    if (sl.e1 != 0.0f) { const float d = fr[1] - fq, m = sl.e1 * d; fq = fq + m; }
    if (sl.e2 != 0.0f) { const float d = fr[2] - fq, m = sl.e2 * d; fq = fq + m; }
    const float dphi = s * fq;
    const float phi0 = (st.phase >= 0.0f && st.phase < 1.0f) ? st.phase : 0.0f;
    const float y = phi0 + dphi;
    float phi = y - floorf(y);
    if (!(phi >= 0.0f && phi < 1.0f)) phi = 0.0f;
    // 5. outputs
    for (int i = 0; i < 3; i++) {
        f.x[i] = phi * P[i];
        f.x0[i] = phi0 * P[i];
        f.dx[i] = dphi * P[i];
    }
    // 6. store
    st.phase = phi; st.px = px; st.py = py;
    return f;
}

}  // namespace mtr
