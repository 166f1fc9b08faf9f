// span_exact.cpp -- csrc/span_row.h (the span walk's exact covered run of a bbox row) against the per-pixel inside test,
// on i32-class triangles set up by the shared csrc/tri_setup.h, as k_tile_vis.hip's setup_tri does.  Prints
// "<triangles> <rows> <non-empty rows> <rows with a bound inside the bbox> <mismatches>" and exits 1 on a mismatch.
// tests/test_span_exact.py builds it with the exact reciprocal and with reciprocals 1 ulp off either way.
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <algorithm>

#include "../../mt_renderer_amd/csrc/span_row.h"
#include "tri_gen.h"

static const int32_t BIN = 16;

struct Stats {
    long long tris = 0, rows = 0, nonempty = 0, inner = 0, bad = 0;
};

// the shared set-up (csrc/tri_setup.h), then k_tile_vis's own: the bbox clipped to the bin and to the viewport, and the
// rebase of the edge functions to the bbox origin
static void check(const TriCase& c, Stats& st) {
    const int32_t(&X)[3] = c.X, (&Y)[3] = c.Y;
    const int32_t binx0 = c.binx0, biny0 = c.biny0, vw = c.vw, vh = c.vh;
    mtr::TriSetup g;
    mtr::tri_setup(X, Y, 0.0f, 0.0f, 0.0f, binx0, biny0, g);
    if (g.flags & 1u) return;  // the 64-bit class: not this walk
    const int32_t px0 = std::max(g.px0, 0), px1 = std::min(g.px1, std::min(BIN, vw) - 1);
    const int32_t py0 = std::max(g.py0, 0), py1 = std::min(g.py1, std::min(BIN, vh) - 1);
    if (px1 < px0 || py1 < py0) return;
    int32_t A[3], B[3], C[3];
    for (int i = 0; i < 3; i++) {
        A[i] = g.A[i];
        B[i] = g.B[i];
        C[i] = mtr::tri_edge(g.Clo[i], g.A[i], g.B[i], px0, py0);
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
    TriGen gen(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 12345);
    Stats st;
    while (st.tris < n) check(gen.next(), st);
    std::printf("%lld %lld %lld %lld %lld\n", st.tris, st.rows, st.nonempty, st.inner, st.bad);
    return st.bad ? 1 : 0;
}
