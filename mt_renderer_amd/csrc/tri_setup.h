// tri_setup.h -- the rasteriser's integer rules, once: triangle set-up against a bin, the three edge functions at a pixel,
// and the absolute-coordinate barycentrics of deferred shading.  k_tile.hip and k_tile_vis.hip use it unchanged, so "the
// same arithmetic per fragment, bit for bit" is one function.  Plain C++ besides the macros (as span_row.h):
// tests/test_tri_setup_exact.py compiles it for the host and holds every output to an int64 reference.
//
// Coordinates are snapped to 1/256 px.  Edge i runs from vertex i+1 to i+2:  E_i(lx, ly) = C_i + A_i * lx + B_i * ly  at
// pixel (lx, ly) of the bin, C_i taken at the centre of the bin's first pixel with the top-left bias (tl_i - 1) folded in:
// a centre is covered iff every E_i >= 0.  Small class (extent <= MTR_TRI_CLASS_LIMIT, 64 px): all i32, A / B pre-scaled
// by 256, 24-bit multiplies.  Large class: A / B are the unscaled (dy, -dx), C is i64 (Chi : Clo), 64-bit products.
#pragma once
#include <cstdint>
#include <cmath>

#if defined(__HIPCC__)
#define MTR_TRI_HD __host__ __device__ __forceinline__
#else
#define MTR_TRI_HD inline
#endif

// v_mul_i32_i24: the low 24 bits of each operand, sign-extended; the low 32 bits of their product.  The host form models
// the instruction in unsigned arithmetic (no overflow UB): an operand that does not fit is as wrong on the CPU as on the GPU
#if defined(__HIP_DEVICE_COMPILE__)
#define MTR_MUL24(a, b) __mul24((a), (b))
#else
#define MTR_MUL24(a, b) mtr::mul24_model((a), (b))
#endif
// c + MTR_MUL24(a, b), as the instruction itself (v_mad_i32_i24) on the device: where the compiler cannot see that an operand
// fits 24 bits it lowers __mul24 to a sign extension and a full 32-bit multiply, which issues at a quarter of the rate
#if defined(__HIP_DEVICE_COMPILE__)
#define MTR_MAD24(a, b, c) mtr::mad24_inst((a), (b), (c))
#else
#define MTR_MAD24(a, b, c) ((int32_t)((uint32_t)mtr::mul24_model((a), (b)) + (uint32_t)(c)))
#endif

#ifndef MTR_TRI_CLASS_LIMIT  // the test's mutant build raises it until 256 * dy leaves the 24 bits
#define MTR_TRI_CLASS_LIMIT 16384
#endif

namespace mtr {

MTR_TRI_HD int32_t mul24_model(int32_t a, int32_t b) {
    const uint32_t sa = (((uint32_t)a & 0xFFFFFFu) ^ 0x800000u) - 0x800000u, sb = (((uint32_t)b & 0xFFFFFFu) ^ 0x800000u) - 0x800000u;
    return (int32_t)(sa * sb);
}
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ int32_t mad24_inst(int32_t a, int32_t b, int32_t c) {
    int32_t r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
#endif
MTR_TRI_HD int32_t tri_min3(int32_t a, int32_t b, int32_t c) { const int32_t m = a < b ? a : b; return m < c ? m : c; }
MTR_TRI_HD int32_t tri_max3(int32_t a, int32_t b, int32_t c) { const int32_t m = a > b ? a : b; return m > c ? m : c; }

MTR_TRI_HD bool tri_is_large(int32_t xext, int32_t yext) { return xext > MTR_TRI_CLASS_LIMIT || yext > MTR_TRI_CLASS_LIMIT; }  // the 64-bit class

struct TriSetup {
    int32_t A[3], B[3], Clo[3], Chi[3];
    uint32_t flags;              // bit0 large, bits 4..6: (1 - tl_i), added back for barycentrics
    float area, rcpA;            // the signed doubled area as a float, and 1 / it
    float z0, dz1, dz2;          // z = fmaf(b2, dz2, fmaf(b1, dz1, z0))
    int32_t px0, px1, py0, py1;  // pixel-centre bbox relative to the bin, unclipped
};

// Set-up of one triangle against the bin whose first pixel is (binx0, biny0).  The small class relies on the bin
// overlapping the bbox: then every operand is < 2^16 and every product < 2^31.  A queued triangle whose bbox misses the
// bin may get meaningless C values from the 24-bit multiplies; its bbox says so (k_tile: submask == 0 and pad == 0,
// k_tile_vis: npx == 0) and its coefficients are never read.
// BOX (tri_setup_box below): the small class's C_i are taken at the first pixel of the bbox inside the bin instead.
template <bool BOX>
MTR_TRI_HD void tri_setup_at(const int32_t (&X)[3], const int32_t (&Y)[3], float z0, float z1, float z2, int32_t binx0, int32_t biny0, TriSetup& s) {
    const int32_t xmin = tri_min3(X[0], X[1], X[2]), xmax = tri_max3(X[0], X[1], X[2]);
    const int32_t ymin = tri_min3(Y[0], Y[1], Y[2]), ymax = tri_max3(Y[0], Y[1], Y[2]);
    const bool large = tri_is_large(xmax - xmin, ymax - ymin);
    s.flags = large ? 1u : 0u;
    // edge 0: v1->v2, edge 1: v2->v0, edge 2: v0->v1;  E = dy*(Px-Xa) - dx*(Py-Ya)
    if (!large) {
        int32_t Px = binx0 * 256 + 128, Py = biny0 * 256 + 128;
        if (BOX) {  // px0 / py0 below, clipped to the bin
            const int32_t bx = ((xmin + 127) >> 8) - binx0, by = ((ymin + 127) >> 8) - biny0;
            Px += ((bx > 0 ? bx : 0) & 15) * 256; Py += ((by > 0 ? by : 0) & 15) * 256;
        }
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int ia = (i + 1) % 3, ib = (i + 2) % 3;
            const int32_t dx = X[ib] - X[ia], dy = Y[ib] - Y[ia];
            const int32_t tl = (dy > 0 || (dy == 0 && dx < 0)) ? 1 : 0;
            s.flags |= (uint32_t)(1 - tl) << (4 + i);
            s.A[i] = dy * 256; s.B[i] = -dx * 256;
            s.Clo[i] = (int32_t)((uint32_t)MTR_MUL24(dy, Px - X[ia]) - (uint32_t)MTR_MUL24(dx, Py - Y[ia]) + (uint32_t)(tl - 1));
            s.Chi[i] = 0;
        }
        s.area = (float)(int32_t)((uint32_t)MTR_MUL24(X[2] - X[0], Y[1] - Y[0]) - (uint32_t)MTR_MUL24(X[1] - X[0], Y[2] - Y[0]));
    } else {
        const long long Px = (long long)binx0 * 256 + 128, Py = (long long)biny0 * 256 + 128;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            const int ia = (i + 1) % 3, ib = (i + 2) % 3;
            const int32_t dx = X[ib] - X[ia], dy = Y[ib] - Y[ia];
            const int32_t tl = (dy > 0 || (dy == 0 && dx < 0)) ? 1 : 0;
            const long long C = (long long)dy * (Px - X[ia]) - (long long)dx * (Py - Y[ia]) + (tl - 1);
            s.flags |= (uint32_t)(1 - tl) << (4 + i);
            s.A[i] = dy; s.B[i] = -dx;
            s.Clo[i] = (int32_t)(uint32_t)(unsigned long long)C;
            s.Chi[i] = (int32_t)(C >> 32);
        }
        s.area = (float)((long long)(X[2] - X[0]) * (long long)(Y[1] - Y[0]) - (long long)(X[1] - X[0]) * (long long)(Y[2] - Y[0]));
    }
    s.rcpA = 1.0f / s.area;
    s.z0 = z0; s.dz1 = z1 - z0; s.dz2 = z2 - z0;
    s.px0 = ((xmin + 127) >> 8) - binx0; s.px1 = ((xmax - 128) >> 8) - binx0;
    s.py0 = ((ymin + 127) >> 8) - biny0; s.py1 = ((ymax - 128) >> 8) - biny0;
}
MTR_TRI_HD void tri_setup(const int32_t (&X)[3], const int32_t (&Y)[3], float z0, float z1, float z2, int32_t binx0, int32_t biny0, TriSetup& s) {
    tri_setup_at<false>(X, Y, z0, z1, z2, binx0, biny0, s);
}
// tri_setup for the walks that evaluate E_i(col, row) in bbox coordinates (k_tile_vis.hip's flat walks): every output as
// tri_setup's, except that a small-class triangle's Clo[i] is E_i at the bbox's first pixel inside the bin, (ox, oy) =
// (max(px0, 0) & 15, max(py0, 0) & 15): the same integer expression at another point, so it equals tri_edge(C_i, A_i,
// B_i, ox, oy) of tri_setup's C_i in 32-bit arithmetic (tests/test_tri_setup_box_exact.py), with operands that are
// offsets inside the triangle's own extent (<= 2^14 + 2^8) rather than from the bin's corner.  The large class is left at
// the bin's first pixel, as its whole-wave walk reads it.
MTR_TRI_HD void tri_setup_box(const int32_t (&X)[3], const int32_t (&Y)[3], float z0, float z1, float z2, int32_t binx0, int32_t biny0, TriSetup& s) {
    tri_setup_at<true>(X, Y, z0, z1, z2, binx0, biny0, s);
}

struct TriEdges {  // the nine edge words as both kernels' LDS records lay them out
    int32_t A0, B0, C0, A1, B1, C1, A2, B2, C2;
};
MTR_TRI_HD int32_t tri_edge(int32_t C, int32_t A, int32_t B, int32_t lx, int32_t ly) {
    return (int32_t)((uint32_t)C + (uint32_t)MTR_MUL24(A, lx) + (uint32_t)MTR_MUL24(B, ly));
}
// small class: is the centre of pixel (lx, ly) covered; e1 / e2: edges 1 and 2 there, the barycentrics' integers
MTR_TRI_HD bool tri_inside(const TriEdges& t, int32_t lx, int32_t ly, int32_t& e1, int32_t& e2) {
    const int32_t e0 = tri_edge(t.C0, t.A0, t.B0, lx, ly);
    e1 = tri_edge(t.C1, t.A1, t.B1, lx, ly);
    e2 = tri_edge(t.C2, t.A2, t.B2, lx, ly);
    return (e0 | e1 | e2) >= 0;
}
// barycentric i of the small class: (e_i + (1 - tl_i)) * rcpA, the bias taken back out
MTR_TRI_HD float tri_bary(int32_t e, uint32_t one_minus_tl, float rcpA) { return (float)(e + (int32_t)one_minus_tl) * rcpA; }

// large class (C's high words in H0..H2, flags as in TriSetup): coverage and both barycentrics at pixel (lx, ly)
MTR_TRI_HD bool tri_inside_large(const TriEdges& t, int32_t H0, int32_t H1, int32_t H2, uint32_t flags, float rcpA, int32_t lx, int32_t ly, float& b1, float& b2) {
    const long long Xp = (long long)lx * 256, Yp = (long long)ly * 256;
    const long long e0 = (((long long)H0 << 32) | (unsigned long long)(uint32_t)t.C0) + (long long)t.A0 * Xp + (long long)t.B0 * Yp;
    const long long e1 = (((long long)H1 << 32) | (unsigned long long)(uint32_t)t.C1) + (long long)t.A1 * Xp + (long long)t.B1 * Yp;
    const long long e2 = (((long long)H2 << 32) | (unsigned long long)(uint32_t)t.C2) + (long long)t.A2 * Xp + (long long)t.B2 * Yp;
    const bool inside = (e0 | e1 | e2) >= 0;
    b1 = (float)(e1 + (long long)((flags >> 5) & 1u)) * rcpA;
    b2 = (float)(e2 + (long long)((flags >> 6) & 1u)) * rcpA;
    return inside;
}
MTR_TRI_HD float tri_depth(float b1, float b2, float z0, float dz1, float dz2) { return fmaf(b2, dz2, fmaf(b1, dz1, z0)); }

// Absolute coordinates (deferred shading has the record, not the bin's set-up): E1 / E2 at the centre of framebuffer pixel
// (px, py) are the integers e_i + (1 - tl_i) that the bin-relative form converts, so the barycentrics are the same floats
MTR_TRI_HD void tri_abs_edges(int32_t X0, int32_t Y0, int32_t X1, int32_t Y1, int32_t X2, int32_t Y2, int32_t px, int32_t py, long long& E1, long long& E2) {
    const long long Px = (long long)px * 256 + 128, Py = (long long)py * 256 + 128;
    E1 = (long long)(Y0 - Y2) * (Px - X2) - (long long)(X0 - X2) * (Py - Y2);
    E2 = (long long)(Y1 - Y0) * (Px - X0) - (long long)(X1 - X0) * (Py - Y0);
}
MTR_TRI_HD void tri_abs_bary(int32_t X0, int32_t Y0, int32_t X1, int32_t Y1, int32_t X2, int32_t Y2, int32_t px, int32_t py, float& b1, float& b2) {
    const float rcpA = 1.0f / (float)((long long)(X2 - X0) * (long long)(Y1 - Y0) - (long long)(X1 - X0) * (long long)(Y2 - Y0));
    long long E1, E2;
    tri_abs_edges(X0, Y0, X1, Y1, X2, Y2, px, py, E1, E2);
    b1 = (float)E1 * rcpA;
    b2 = (float)E2 * rcpA;
}

}  // namespace mtr
