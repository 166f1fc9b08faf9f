// geom_cull.h -- conservative clip-space intervals of bone boxes and the tests of them against a rank's bins (k_cull.hip).
#pragma once
#include "mtr_internal.h"

namespace mtr {

// ---------------------------------------------------------------------------------------------
// Geometry culling of sharded frames (multi-GPU v2).  A rank must not spend vertex work on
// geometry that cannot reach one of its bins, and it must never skip geometry that does: the test is conservative.
//
// A BoneBox holds the object-space box (centre c, half extents e) of the vertices that one joint influences.  When the
// weight bytes of every vertex sum to 255 the skinned position is a convex combination of the points P_j * (p,1) over
// the joints j that carry weight, so every clip coordinate of every vertex lies in the union over those joints of
//     [ v_i - r_i - m_i ,  v_i + r_i + m_i ],     v_i = (C * (c,1))_i,   r_i = sum_c |C[c][i]| * e_c,   C = M * P_j,
// where m_i = 2^-16 * (|M| |P_j| (|c|+e, 1))_i covers the rounding of both this evaluation and of the vertex shader's own
// fma chains (about 40 operations at 2^-24 each, relative to the same sum of magnitudes), the error of the weight sum
// (4 * 2^-25) included.  Near-plane clipping only adds convex combinations of clip-space vertices, so the interval also
// holds for the vertices it creates.  With w_lo > 0 the screen rectangle follows by interval division; a pixel of
// slack and 2^-20 of the coordinate cover the divide, the viewport fma and the 1/256 snap.  Anything that cannot be
// bounded (w_lo <= 0, NaN, weights that are not normalised) is kept.
// m_i is a RELATIVE bound: a product or sum of the vertex shader that lands among the subnormals is rounded to a
// multiple of 2^-149 whatever its size, which no multiple of the magnitudes covers.  A clip coordinate whose sum of
// magnitudes lies below MTR_CULL_MIN_MAG = 2^-100 is therefore not bounded at all (infinite margin: the geometry is
// kept; tests/test_cull_model_premises.py has the matrices with subnormal rows that stepped out of the interval by
// thousands of margins).  Above it the shader's results are normal numbers unless the POSITIONS themselves are
// subnormal and a matrix element of 2^100 or more blows their rounding up again, which no model format produces.
// ---------------------------------------------------------------------------------------------
#define MTR_CULL_MIN_MAG 7.888609052210118e-31f  // 2^-100
struct ClipBox {
    float lo[3], hi[3];  // x, y, w
};

// element (row i, column c) of M * [P; 0 0 0 1] and of |M| * |P| (Pm: 16 floats column-major, rows 0..2 used; nullptr: identity)
__device__ __forceinline__ void comp_entry(const float* Pm, const float (&M)[16], int i, int c, float& C, float& A) {
    if (Pm) {
        C = M[0 + i] * Pm[c * 4 + 0] + M[4 + i] * Pm[c * 4 + 1] + M[8 + i] * Pm[c * 4 + 2];
        A = fabsf(M[0 + i]) * fabsf(Pm[c * 4 + 0]) + fabsf(M[4 + i]) * fabsf(Pm[c * 4 + 1]) + fabsf(M[8 + i]) * fabsf(Pm[c * 4 + 2]);
        if (c == 3) { C += M[12 + i]; A += fabsf(M[12 + i]); }
    } else {
        C = M[c * 4 + i];
        A = fabsf(C);
    }
}

// interval of one box under M * [P; 0 0 0 1]
__device__ __forceinline__ ClipBox box_clip_interval(const BoneBox& b, const float* Pm, const float (&M)[16]) {
    const float cen[3] = {b.cx, b.cy, b.cz}, ext[3] = {b.ex, b.ey, b.ez};
    ClipBox r;
#pragma unroll
    for (int t = 0; t < 3; t++) {
        const int i = t == 2 ? 3 : t;  // clip x, y, w
        float v = 0.0f, rad = 0.0f, mag = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            float C, A;
            comp_entry(Pm, M, i, c, C, A);
            if (c < 3) {
                v += C * cen[c];
                rad += fabsf(C) * ext[c];
                mag += A * (fabsf(cen[c]) + ext[c]);
            } else {
                v += C;
                mag += A;
            }
        }
        const float m = mag >= MTR_CULL_MIN_MAG ? mag * 1.52587890625e-05f : __builtin_inff();  // 2^-16; NaN: not bounded either
        r.lo[t] = v - rad - m;
        r.hi[t] = v + rad + m;
    }
    return r;
}

// the composite of one joint for the chunk tests: rows x, y, w of M * [P; 0 0 0 1] and of |M| * |P|
__device__ __forceinline__ CompMat make_comp(const float* Pm, const float (&M)[16]) {
    CompMat cm;
#pragma unroll
    for (int t = 0; t < 3; t++) {
        const int i = t == 2 ? 3 : t;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            float C, A;
            comp_entry(Pm, M, i, c, C, A);
            cm.C[c * 3 + t] = C;
            cm.A[c * 3 + t] = A;
        }
    }
    return cm;
}

// the same interval as box_clip_interval from a prepared composite: 11 multiply-adds per clip coordinate
__device__ __forceinline__ ClipBox box_comp_interval(const BoneBox& b, const CompMat& cm) {
    const float cen[3] = {b.cx, b.cy, b.cz}, ext[3] = {b.ex, b.ey, b.ez};
    ClipBox r;
#pragma unroll
    for (int t = 0; t < 3; t++) {
        float v = cm.C[9 + t], rad = 0.0f, mag = cm.A[9 + t];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            v += cm.C[c * 3 + t] * cen[c];
            rad += fabsf(cm.C[c * 3 + t]) * ext[c];
            mag += cm.A[c * 3 + t] * (fabsf(cen[c]) + ext[c]);
        }
        const float m = mag >= MTR_CULL_MIN_MAG ? mag * 1.52587890625e-05f : __builtin_inff();  // 2^-16; NaN: not bounded either
        r.lo[t] = v - rad - m;
        r.hi[t] = v + rad + m;
    }
    return r;
}

__device__ __forceinline__ bool clipbox_finite(const ClipBox& r) {
    bool ok = true;
#pragma unroll
    for (int t = 0; t < 3; t++) ok = ok && fabsf(r.lo[t]) < 3.0e38f && fabsf(r.hi[t]) < 3.0e38f;  // false for NaN and inf
    return ok;
}

// May geometry whose clip coordinates lie in `u` produce a fragment in a bin of this rank?  (wave-uniform arithmetic)
__device__ __forceinline__ bool clipbox_may_touch_rank(const ClipBox& u, const FrameBuffers& fb) {
    const float xlo = u.lo[0], xhi = u.hi[0], ylo = u.lo[1], yhi = u.hi[1], wlo = u.lo[2], whi = u.hi[2];
    if (!(wlo > 0.0f)) return true;  // reaches w <= 0 (or NaN): no screen bound
    const float sx_lo = xlo >= 0.0f ? xlo / whi : xlo / wlo, sx_hi = xhi >= 0.0f ? xhi / wlo : xhi / whi;
    const float sy_lo = ylo >= 0.0f ? ylo / whi : ylo / wlo, sy_hi = yhi >= 0.0f ? yhi / wlo : yhi / whi;
    const float fW = (float)fb.W, fH = (float)fb.H, hw = 0.5f * fW, hh = 0.5f * fH;
    float fx_lo = sx_lo * hw + hw, fx_hi = sx_hi * hw + hw;
    float fy_lo = hh - sy_hi * hh, fy_hi = hh - sy_lo * hh;
    const float mx = 1.0f + 9.5367431640625e-07f * fmaxf(fabsf(fx_lo), fabsf(fx_hi));  // 1 px + 2^-20 relative
    const float my = 1.0f + 9.5367431640625e-07f * fmaxf(fabsf(fy_lo), fabsf(fy_hi));
    fx_lo -= mx; fx_hi += mx; fy_lo -= my; fy_hi += my;
    if (fx_hi < 0.0f || fx_lo > fW || fy_hi < 0.0f || fy_lo > fH) return false;  // provably off the target (NaN: kept)
    if (!(fx_lo == fx_lo && fx_hi == fx_hi && fy_lo == fy_lo && fy_hi == fy_hi)) return true;
    const uint32_t bx0 = (uint32_t)fminf(fmaxf(fx_lo, 0.0f), fW) >> MTR_BIN_SHIFT, by0 = (uint32_t)fminf(fmaxf(fy_lo, 0.0f), fH) >> MTR_BIN_SHIFT;
    const uint32_t bx1 = min((uint32_t)fminf(fmaxf(fx_hi, 0.0f), fW) >> MTR_BIN_SHIFT, fb.nbx - 1u);
    const uint32_t by1 = min((uint32_t)fminf(fmaxf(fy_hi, 0.0f), fH) >> MTR_BIN_SHIFT, fb.nby - 1u);
    return rect_owned_any(fb.own, min(bx0, fb.nbx - 1u), min(by0, fb.nby - 1u), bx1, by1, fb.nbx);
}

// Is every bin that geometry with clip coordinates in `u` can produce a fragment in a bin of this rank?  (Then no part of
// it needs testing against the rank's border.)  Same rectangle as clipbox_may_touch_rank; false whenever in doubt.
__device__ __forceinline__ bool clipbox_all_in_rank(const ClipBox& u, const FrameBuffers& fb) {
    const float ylo = u.lo[1], yhi = u.hi[1], wlo = u.lo[2], whi = u.hi[2];
    if (!(wlo > 0.0f)) return false;
    const float sy_lo = ylo >= 0.0f ? ylo / whi : ylo / wlo, sy_hi = yhi >= 0.0f ? yhi / wlo : yhi / whi;
    const float fH = (float)fb.H, hh = 0.5f * fH;
    float fy_lo = hh - sy_hi * hh, fy_hi = hh - sy_lo * hh;
    const float my = 1.0f + 9.5367431640625e-07f * fmaxf(fabsf(fy_lo), fabsf(fy_hi));
    fy_lo -= my; fy_hi += my;
    if (!(fy_lo == fy_lo && fy_hi == fy_hi)) return false;
    if (fb.own.world <= 1) {  // an unsharded frame (MTR_GEOM_CULL_ALL_FRAMES): "all in" = wholly on the target, so that the
                              // chunks of an instance that hangs over its edge are still tested one by one
        const float xlo = u.lo[0], xhi = u.hi[0];
        const float sx_lo = xlo >= 0.0f ? xlo / whi : xlo / wlo, sx_hi = xhi >= 0.0f ? xhi / wlo : xhi / whi;
        const float fW = (float)fb.W, hw = 0.5f * fW;
        const float fx_lo = sx_lo * hw + hw, fx_hi = sx_hi * hw + hw;
        const float mx = 1.0f + 9.5367431640625e-07f * fmaxf(fabsf(fx_lo), fabsf(fx_hi));
        return fx_lo - mx >= 0.0f && fx_hi + mx <= fW && fy_lo >= 0.0f && fy_hi <= fH;  // false for NaN
    }
    const uint32_t by0 = (uint32_t)fminf(fmaxf(fy_lo, 0.0f), fH) >> MTR_BIN_SHIFT;
    const uint32_t by1 = min((uint32_t)fminf(fmaxf(fy_hi, 0.0f), fH) >> MTR_BIN_SHIFT, fb.nby - 1u);
    return rect_owned_all(fb.own, min(by0, fb.nby - 1u), by1);
}

// union of intervals inside each row of 16 lanes (every lane of a row ends up with the row's result): one wave bounds
// four chunks at once, a chunk has <= 16 boxes
__device__ __forceinline__ float row_min_f32(float v) { return row_reduce(v, [](float a, float b) { return fminf(a, b); }); }
__device__ __forceinline__ float row_max_f32(float v) { return row_reduce(v, [](float a, float b) { return fmaxf(a, b); }); }
// wave-wide union of the lanes' intervals (lanes that hold none pass lo = +inf, hi = -inf); every lane gets the result
__device__ __forceinline__ float wave_min_f32(float v) { return wave_reduce(v, [](float a, float b) { return fminf(a, b); }); }
__device__ __forceinline__ float wave_max_f32(float v) { return wave_reduce(v, [](float a, float b) { return fmaxf(a, b); }); }

// the instance's clip matrix M = VP * Model (VP itself without model matrices), every element by vp_model_elem
__device__ __forceinline__ void compose_vp_model(const float (&vp)[16], const float* model_mats, uint32_t inst, float (&M)[16]) {
    if (model_mats) {
#pragma unroll
        for (int e = 0; e < 16; e++) M[e] = vp_model_elem(vp, model_mats, inst, e);
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) M[i] = vp[i];
    }
}

}  // namespace mtr
