// span_exact.cpp -- csrc/span_row.h (the span walk's exact covered run of a bbox row) against the per-pixel inside test,
// on triangles set up exactly as k_tile_vis.hip's setup_tri does for the i32 edge class.  Prints
// "<triangles> <rows> <non-empty rows> <rows with a bound inside the bbox> <mismatches>" and exits 1 on a mismatch.
// tests/test_span_exact.py builds it with the exact reciprocal and with reciprocals 1 ulp off either way.
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <algorithm>
#include <random>

#include "../../mt_renderer_amd/csrc/span_row.h"

static const int32_t BIN = 16;

struct Stats {
    long long tris = 0, rows = 0, nonempty = 0, inner = 0, bad = 0;
};

// setup_tri's small class: edge i from vertex i+1 to i+2, A = 256 dy, B = -256 dx, C at the bin's first pixel centre
// with the top-left bias, the bbox clipped to the bin and to the viewport; then k_tile_vis's rebase to the bbox origin
static void check(const int32_t X[3], const int32_t Y[3], int32_t binx0, int32_t biny0, int32_t vw, int32_t vh, Stats& st) {
    const int32_t xmin = std::min(X[0], std::min(X[1], X[2])), xmax = std::max(X[0], std::max(X[1], X[2]));
    const int32_t ymin = std::min(Y[0], std::min(Y[1], Y[2])), ymax = std::max(Y[0], std::max(Y[1], Y[2]));
    if ((xmax - xmin) > 16384 || (ymax - ymin) > 16384) return;  // the 64-bit class: not this walk
    const int32_t px0 = std::max(((xmin + 127) >> 8) - binx0, 0), px1 = std::min(((xmax - 128) >> 8) - binx0, std::min(BIN, vw) - 1);
    const int32_t py0 = std::max(((ymin + 127) >> 8) - biny0, 0), py1 = std::min(((ymax - 128) >> 8) - biny0, std::min(BIN, vh) - 1);
    if (px1 < px0 || py1 < py0) return;
    const int32_t Px = binx0 * 256 + 128, Py = biny0 * 256 + 128;
    int32_t A[3], B[3], C[3];
    for (int i = 0; i < 3; i++) {
        const int ia = (i + 1) % 3, ib = (i + 2) % 3;
        const int32_t dx = X[ib] - X[ia], dy = Y[ib] - Y[ia];
        const int32_t tl = (dy > 0 || (dy == 0 && dx < 0)) ? 1 : 0;
        A[i] = dy * 256;
        B[i] = -dx * 256;
        const long long c = (long long)dy * (Px - X[ia]) - (long long)dx * (Py - Y[ia]) + (tl - 1);
        if (c > INT32_MAX || c < INT32_MIN) { std::fprintf(stderr, "C out of i32\n"); std::exit(2); }
        C[i] = (int32_t)c + A[i] * px0 + B[i] * py0;
    }
    st.tris++;
    const int32_t bwm1 = px1 - px0;
    for (int32_t row = 0; row <= py1 - py0; row++) {
        int32_t e[3];
        for (int i = 0; i < 3; i++) e[i] = C[i] + B[i] * row;
        int32_t lo, hi;
        mtr::span_of_row(e[0], e[1], e[2], A[0], A[1], A[2], bwm1, lo, hi);
        st.rows++;
        if (lo <= hi) st.nonempty++;
        if (lo <= hi && (lo > 0 || hi < bwm1)) st.inner++;
        for (int32_t col = 0; col <= bwm1; col++) {
            bool inside = true;
            for (int i = 0; i < 3; i++) inside = inside && (long long)e[i] + (long long)A[i] * col >= 0;
            if (inside != (col >= lo && col <= hi)) {
                if (st.bad < 10)
                    std::fprintf(stderr, "mismatch: V=(%d,%d) (%d,%d) (%d,%d) bin=(%d,%d) vw=%d vh=%d row=%d col=%d lo=%d hi=%d inside=%d\n", X[0], Y[0], X[1],
                                 Y[1], X[2], Y[2], binx0, biny0, vw, vh, row, col, lo, hi, (int)inside);
                st.bad++;
            }
        }
    }
}

int main(int argc, char** argv) {
    const long long n = argc > 1 ? std::atoll(argv[1]) : 1000000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 12345);
    auto U = [&](int32_t lo, int32_t hi) { return (int32_t)(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1))); };
    Stats st;
    long long made = 0;
    while (st.tris < n) {
        made++;
        const int32_t binx0 = U(0, 40) * BIN, biny0 = U(0, 40) * BIN;
        // the viewport's right / bottom edge cuts the bin in a quarter of the cases
        const int32_t vw = U(0, 3) == 0 ? U(1, 16) : 1 << 20, vh = U(0, 3) == 0 ? U(1, 16) : 1 << 20;
        const int mode = (int)(made % 8);
        int32_t X[3], Y[3];
        // extent of the triangle in 1/256 px: mostly small, up to the class limit (16384 = 64 px)
        const int32_t ext = mode == 7 ? 16384 : (U(0, 2) == 0 ? U(64, 16384) : U(16, 1536));
        const int32_t cx = binx0 * 256 + U(-ext, BIN * 256 + ext), cy = biny0 * 256 + U(-ext, BIN * 256 + ext);
        for (int v = 0; v < 3; v++) {
            X[v] = cx + U(-ext / 2, ext / 2);
            Y[v] = cy + U(-ext / 2, ext / 2);
            if (mode == 1) { X[v] = (X[v] & ~255) + 128; Y[v] = (Y[v] & ~255) + 128; }           // on pixel centres
            if (mode == 2) { X[v] = (X[v] & ~(BIN * 256 - 1)); Y[v] = (Y[v] & ~(BIN * 256 - 1)); }  // on bin corners
            if (mode == 3 && v == 2) { X[v] = (X[v] & ~255) + 128; }                               // mixed
        }
        if (mode == 4) { Y[1] = Y[0]; }  // a horizontal edge (top or bottom: both top-left cases by winding)
        if (mode == 5) { X[1] = X[0]; }  // a vertical edge
        if (mode == 6) {                 // a long sliver across the bin: a thin wedge at a random slope
            const int32_t dx = U(-ext, ext), dy = U(-ext, ext);
            X[1] = X[0] + dx; Y[1] = Y[0] + dy;
            X[2] = X[0] + dx / 2 + U(-40, 40); Y[2] = Y[0] + dy / 2 + U(-40, 40);
        }
        if (mode == 7) {  // the class limit: vertices at the far ends, so that the edge values reach ~2^30
            X[0] = cx - ext / 2; X[1] = cx + ext / 2; X[2] = cx + U(-ext / 2, ext / 2);
            Y[0] = cy + U(-ext / 2, ext / 2); Y[1] = cy + U(-ext / 2, ext / 2); Y[2] = U(0, 1) ? cy - ext / 2 : cy + ext / 2;
        }
        if (made & 1) { std::swap(X[1], X[2]); std::swap(Y[1], Y[2]); }  // both windings: one of them covers nothing
        check(X, Y, binx0, biny0, vw, vh, st);
    }
    std::printf("%lld %lld %lld %lld %lld\n", st.tris, st.rows, st.nonempty, st.inner, st.bad);
    return st.bad ? 1 : 0;
}
