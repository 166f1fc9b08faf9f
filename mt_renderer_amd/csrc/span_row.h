// span_row.h -- the exact run of covered pixel centres in one bbox row of an i32-class triangle (k_tile_vis.hip's span
// walk).  Plain C++ besides the macros, so that tests/test_span_exact.py compiles it for the host and checks it
// against the per-pixel inside test.
//
// The row's edge functions are E_i(col) = e_i + A_i * col (e_i: the value at the bbox's first column, top-left bias
// included; A_i = 256 * dy_i, |dy_i| <= 2^14).  A triangle is convex, so { col : every E_i(col) >= 0 } is one run
// [lo, hi].  Each edge with A_i != 0 bounds one side at its zero crossing  q_i = -e_i / A_i:  col >= ceil(q_i) where E
// grows with the column, col <= floor(q_i) where it falls.  q_i is estimated in f32 and moved one eighth of a column
// toward the outside of the run before it is rounded, so the rounded estimate is the exact bound or one column outside
// it; one integer evaluation of E_i at the estimate decides which.  (Inside the range that matters, |q_i| <= 18, the
// estimate is within 18 * 2^-21 of q_i: one rounding of e_i, one v_rcp_f32 of at most 1 ulp, one rounded product.  The
// estimate is clamped to [-2, 17] first; a bound outside the bbox stays outside after the clamp and the correction.)
#pragma once
#include <cstdint>
#include <cmath>

#include "tri_setup.h"  // MTR_MUL24

#if defined(__HIPCC__)
#define MTR_SPAN_HD __host__ __device__ __forceinline__
#else
#define MTR_SPAN_HD inline
#endif

#ifndef MTR_SPAN_RCP  // the host build may substitute a reciprocal 1 ulp off either way (tests/test_span_exact.py)
#if defined(__HIP_DEVICE_COMPILE__)
#define MTR_SPAN_RCP(x) __builtin_amdgcn_rcpf(x)
#else
#define MTR_SPAN_RCP(x) (1.0f / (x))
#endif
#endif

namespace mtr {

// narrows [lo, hi] to the columns where e + A * col >= 0
MTR_SPAN_HD void span_edge(int32_t e, int32_t A, int32_t& lo, int32_t& hi) {
    const float q = (float)e * MTR_SPAN_RCP((float)(-A));  // ~ -e / A (A == 0: +-inf or NaN, replaced below)
    const float s = A > 0 ? -1.0f : 1.0f;                   // ceil(x) = -floor(-x): s * floor(s * q + 1/8)
    const float qc = fminf(fmaxf(q, -2.0f), 17.0f);
    int32_t c = (int32_t)(s * floorf(fmaf(s, qc, 0.125f)));
    if (e + MTR_MUL24(A, c) < 0) c += A > 0 ? 1 : -1;  // the estimate was one column outside: step in
    // selects, not branches: lo starts at 0 and hi at <= 15, so 0 and 16 bound nothing; A == 0 (an edge along the row): the
    // whole row is on one side of it
    const int32_t l = A > 0 ? c : 0, h = A < 0 ? c : (A == 0 && e < 0 ? -1 : 16);
    lo = l > lo ? l : lo;
    hi = h < hi ? h : hi;
}

// the covered columns [lo, hi] of a bbox row of bwm1 + 1 columns (empty: lo > hi)
MTR_SPAN_HD void span_of_row(int32_t e0, int32_t e1, int32_t e2, int32_t A0, int32_t A1, int32_t A2, int32_t bwm1, int32_t& lo, int32_t& hi) {
    lo = 0;
    hi = bwm1;
    span_edge(e0, A0, lo, hi);
    span_edge(e1, A1, lo, hi);
    span_edge(e2, A2, lo, hi);
}

}  // namespace mtr
