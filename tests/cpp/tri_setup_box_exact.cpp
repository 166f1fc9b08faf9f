// tri_setup_box_exact.cpp -- csrc/tri_setup.h's tri_setup_box (the set-up k_tile_vis.hip stages its flat walks from) against
// tri_setup, on the triangles of tri_gen.h that tri_setup_exact.cpp checks (bbox overlapping the bin): A, B, the flags,
// the area, rcpA, the z plane and the bbox are tri_setup's bit for bit; a small-class triangle's C_i are
// tri_edge(C_i, A_i, B_i, ox, oy) of tri_setup's C_i at the bbox's first pixel inside the bin, and the int64 edge value
// there; a large-class triangle's Chi:Clo are tri_setup's.
// Prints "<small triangles> <large triangles> <small ones whose origin is not the bin's> <mismatches>", exits 1 on a mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <algorithm>

#include "tri_gen.h"

static const int32_t BIN = TriGen::BIN;
typedef long long i64;

struct Stats {
    i64 small = 0, large = 0, moved = 0, bad = 0;
};

static void fail(Stats& st, const TriCase& c, const char* what, i64 got, i64 want, int i = -1) {
    if (st.bad++ < 10)
        std::fprintf(stderr, "mismatch %s[%d]: got %lld want %lld: V=(%d,%d) (%d,%d) (%d,%d) bin=(%d,%d)\n", what, i, got, want, c.X[0], c.Y[0], c.X[1],
                     c.Y[1], c.X[2], c.Y[2], c.binx0, c.biny0);
}
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static bool check(const TriCase& c, Stats& st) {
    mtr::TriSetup g, b;
    mtr::tri_setup(c.X, c.Y, 0.25f, 0.5f, 0.75f, c.binx0, c.biny0, g);
    if (g.px0 > BIN - 1 || g.px1 < 0 || g.py0 > BIN - 1 || g.py1 < 0) return false;  // set-up promises nothing (tri_setup_exact.cpp)
    std::memset(&b, 0xA5, sizeof b);
    mtr::tri_setup_box(c.X, c.Y, 0.25f, 0.5f, 0.75f, c.binx0, c.biny0, b);
    const bool large = (g.flags & 1u) != 0;
    if (b.flags != g.flags) fail(st, c, "flags", b.flags, g.flags);
    if (bits(b.area) != bits(g.area)) fail(st, c, "area", bits(b.area), bits(g.area));
    if (bits(b.rcpA) != bits(g.rcpA)) fail(st, c, "rcpA", bits(b.rcpA), bits(g.rcpA));
    if (bits(b.z0) != bits(g.z0) || bits(b.dz1) != bits(g.dz1) || bits(b.dz2) != bits(g.dz2)) fail(st, c, "z plane", 0, 0);
    if (b.px0 != g.px0 || b.px1 != g.px1 || b.py0 != g.py0 || b.py1 != g.py1) fail(st, c, "bbox", b.px0, g.px0);
    const int32_t ox = std::max(g.px0, 0) & 15, oy = std::max(g.py0, 0) & 15;  // k_tile_vis.hip: box bits 0..3, 4..7
    for (int i = 0; i < 3; i++) {
        if (b.A[i] != g.A[i]) fail(st, c, "A", b.A[i], g.A[i], i);
        if (b.B[i] != g.B[i]) fail(st, c, "B", b.B[i], g.B[i], i);
        if (b.Chi[i] != g.Chi[i]) fail(st, c, "Chi", b.Chi[i], g.Chi[i], i);
        if (large) {
            if (b.Clo[i] != g.Clo[i]) fail(st, c, "large Clo", b.Clo[i], g.Clo[i], i);
            continue;
        }
        const int32_t want = mtr::tri_edge(g.Clo[i], g.A[i], g.B[i], ox, oy);
        if (b.Clo[i] != want) fail(st, c, "Clo", b.Clo[i], want, i);
        // and the edge function itself there, in 64 bits
        const int ia = (i + 1) % 3, ib = (i + 2) % 3;
        const i64 dx = (i64)c.X[ib] - c.X[ia], dy = (i64)c.Y[ib] - c.Y[ia], tl = (dy > 0 || (dy == 0 && dx < 0)) ? 1 : 0;
        const i64 Px = ((i64)c.binx0 + ox) * 256 + 128, Py = ((i64)c.biny0 + oy) * 256 + 128;
        const i64 ref = dy * (Px - c.X[ia]) - dx * (Py - c.Y[ia]) + (tl - 1);
        if ((i64)b.Clo[i] != ref) fail(st, c, "Clo against int64", b.Clo[i], ref, i);
    }
    (large ? st.large : st.small)++;
    if (!large && (ox || oy)) st.moved++;
    return true;
}

int main(int argc, char** argv) {
    const i64 nsmall = argc > 1 ? std::atoll(argv[1]) : 1000000, nlarge = argc > 2 ? std::atoll(argv[2]) : 30000;
    TriGen gen(argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 12345);
    Stats st;
    while (st.small < nsmall) check(gen.next(), st);
    while (st.large < nlarge) check(gen.next(1 << 24), st);
    std::printf("%lld %lld %lld %lld\n", st.small, st.large, st.moved, st.bad);
    return st.bad ? 1 : 0;
}
