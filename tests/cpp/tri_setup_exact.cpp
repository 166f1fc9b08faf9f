// tri_setup_exact.cpp -- csrc/tri_setup.h (the set-up and edge evaluation both tile kernels use) against a plain int64
// reference written here, on the triangles of tri_gen.h.
//   small class: A, B, C of the three edges, the (1 - tl) bits, the signed area as a float and the bin-relative bbox; the
//     three edge values and the inside decision at all 256 pixels of the bin; and at every covered pixel the
//     absolute-coordinate E1 / E2 against the bin-relative e + (1 - tl) -- the identity that lets k_tile_vis defer shading;
//   large class (extents up to 2^24): A, B, the reassembled Chi:Clo, the inside decision and E1 / E2 alike.
// The header's host MTR_MUL24 models v_mul_i32_i24, so an operand beyond 24 bits is as wrong here as on the GPU.
// Prints "<small triangles> <large triangles> <covered pixels> <mismatches>" and exits 1 on a mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstdint>

#include "tri_gen.h"

static const int32_t BIN = TriGen::BIN;
typedef long long i64;

struct Stats {
    i64 small = 0, large = 0, covered = 0, bad = 0;
};

static i64 floor_div(i64 a, i64 b) { return a / b - ((a % b != 0 && (a % b < 0) != (b < 0)) ? 1 : 0); }

static void fail(Stats& st, const TriCase& c, const char* what, i64 got, i64 want, int lx = -1, int ly = -1) {
    if (st.bad++ < 10)
        std::fprintf(stderr, "mismatch %s: got %lld want %lld at (%d,%d): V=(%d,%d) (%d,%d) (%d,%d) bin=(%d,%d)\n", what, got, want, lx, ly, c.X[0], c.Y[0],
                     c.X[1], c.Y[1], c.X[2], c.Y[2], c.binx0, c.biny0);
}

// returns false when the triangle was not checked (its pixel-centre bbox misses the bin: set-up promises nothing)
static bool check(const TriCase& c, Stats& st) {
    // ---- the reference: 64-bit throughout, no 24-bit products, no pre-scaling ----
    i64 dx[3], dy[3], tl[3], C[3];  // edge i: vertex i+1 -> i+2; C at the centre of the bin's first pixel, bias included
    const i64 Px = (i64)c.binx0 * 256 + 128, Py = (i64)c.biny0 * 256 + 128;
    i64 xmin = c.X[0], xmax = c.X[0], ymin = c.Y[0], ymax = c.Y[0];
    for (int i = 0; i < 3; i++) {
        const int ia = (i + 1) % 3, ib = (i + 2) % 3;
        dx[i] = (i64)c.X[ib] - c.X[ia];
        dy[i] = (i64)c.Y[ib] - c.Y[ia];
        tl[i] = (dy[i] > 0 || (dy[i] == 0 && dx[i] < 0)) ? 1 : 0;
        C[i] = dy[i] * (Px - c.X[ia]) - dx[i] * (Py - c.Y[ia]) + (tl[i] - 1);
        if (c.X[i] < xmin) xmin = c.X[i];
        if (c.X[i] > xmax) xmax = c.X[i];
        if (c.Y[i] < ymin) ymin = c.Y[i];
        if (c.Y[i] > ymax) ymax = c.Y[i];
    }
    const bool large = xmax - xmin > MTR_TRI_CLASS_LIMIT || ymax - ymin > MTR_TRI_CLASS_LIMIT;
    const i64 area2 = ((i64)c.X[2] - c.X[0]) * ((i64)c.Y[1] - c.Y[0]) - ((i64)c.X[1] - c.X[0]) * ((i64)c.Y[2] - c.Y[0]);
    // pixel p's centre is at 256 p + 128: the first centre at or after xmin, the last at or before xmax
    const i64 px0 = -floor_div(128 - xmin, 256) - c.binx0, px1 = floor_div(xmax - 128, 256) - c.binx0;
    const i64 py0 = -floor_div(128 - ymin, 256) - c.biny0, py1 = floor_div(ymax - 128, 256) - c.biny0;
    if (px0 > BIN - 1 || px1 < 0 || py0 > BIN - 1 || py1 < 0) return false;

    mtr::TriSetup g;
    mtr::tri_setup(c.X, c.Y, 0.25f, 0.5f, 0.75f, c.binx0, c.biny0, g);
    if (((g.flags & 1u) != 0) != large) fail(st, c, "class", g.flags & 1u, large);
    if (g.px0 != px0) fail(st, c, "px0", g.px0, px0);
    if (g.px1 != px1) fail(st, c, "px1", g.px1, px1);
    if (g.py0 != py0) fail(st, c, "py0", g.py0, py0);
    if (g.py1 != py1) fail(st, c, "py1", g.py1, py1);
    if (g.area != (float)area2) fail(st, c, "area", (i64)g.area, area2);
    if (g.z0 != 0.25f || g.dz1 != 0.25f || g.dz2 != 0.5f) fail(st, c, "z plane", 0, 0);
    const i64 scale = large ? 1 : 256;
    for (int i = 0; i < 3; i++) {
        if (g.A[i] != dy[i] * scale) fail(st, c, "A", g.A[i], dy[i] * scale, i);
        if (g.B[i] != -dx[i] * scale) fail(st, c, "B", g.B[i], -dx[i] * scale, i);
        const i64 Cg = (i64)(((unsigned long long)(uint32_t)g.Chi[i] << 32) | (uint32_t)g.Clo[i]);
        if ((large ? Cg : (i64)g.Clo[i]) != C[i]) fail(st, c, "C", large ? Cg : (i64)g.Clo[i], C[i], i);
        if (((g.flags >> (4 + i)) & 1u) != (uint32_t)(1 - tl[i])) fail(st, c, "tl bit", (g.flags >> (4 + i)) & 1u, 1 - tl[i], i);
    }
    (large ? st.large : st.small)++;

    const mtr::TriEdges E = {g.A[0], g.B[0], g.Clo[0], g.A[1], g.B[1], g.Clo[1], g.A[2], g.B[2], g.Clo[2]};
    for (int32_t ly = 0; ly < BIN; ly++)
        for (int32_t lx = 0; lx < BIN; lx++) {
            i64 e[3];
            for (int i = 0; i < 3; i++) e[i] = C[i] + dy[i] * 256 * lx - dx[i] * 256 * ly;
            const bool inside = e[0] >= 0 && e[1] >= 0 && e[2] >= 0;
            bool got;
            if (!large) {
                int32_t e1, e2;
                got = mtr::tri_inside(E, lx, ly, e1, e2);
                const int32_t e0 = mtr::tri_edge(E.C0, E.A0, E.B0, lx, ly);
                if (e0 != e[0]) fail(st, c, "e0", e0, e[0], lx, ly);
                if (e1 != e[1]) fail(st, c, "e1", e1, e[1], lx, ly);
                if (e2 != e[2]) fail(st, c, "e2", e2, e[2], lx, ly);
            } else {
                float b1, b2;
                got = mtr::tri_inside_large(E, g.Chi[0], g.Chi[1], g.Chi[2], g.flags, g.rcpA, lx, ly, b1, b2);
                if (b1 != (float)(e[1] + 1 - tl[1]) * g.rcpA || b2 != (float)(e[2] + 1 - tl[2]) * g.rcpA) fail(st, c, "large barycentrics", 0, 0, lx, ly);
            }
            if (got != inside) fail(st, c, "inside", got, inside, lx, ly);
            if (!inside) continue;
            st.covered++;
            long long E1, E2;
            mtr::tri_abs_edges(c.X[0], c.Y[0], c.X[1], c.Y[1], c.X[2], c.Y[2], c.binx0 + lx, c.biny0 + ly, E1, E2);
            if (E1 != e[1] + 1 - tl[1]) fail(st, c, "E1", E1, e[1] + 1 - tl[1], lx, ly);
            if (E2 != e[2] + 1 - tl[2]) fail(st, c, "E2", E2, e[2] + 1 - tl[2], lx, ly);
            float a1, a2;  // and the floats made of them, with the same reciprocal of the area
            mtr::tri_abs_bary(c.X[0], c.Y[0], c.X[1], c.Y[1], c.X[2], c.Y[2], c.binx0 + lx, c.biny0 + ly, a1, a2);
            if (a1 != (float)E1 * g.rcpA || a2 != (float)E2 * g.rcpA) fail(st, c, "absolute barycentrics", 0, 0, lx, ly);
        }
    return true;
}

int main(int argc, char** argv) {
    const i64 nsmall = argc > 1 ? std::atoll(argv[1]) : 1000000, nlarge = argc > 2 ? std::atoll(argv[2]) : 30000;
    TriGen gen(argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 12345);
    Stats st;
    while (st.small < nsmall) check(gen.next(), st);
    while (st.large < nlarge) check(gen.next(1 << 24), st);
    std::printf("%lld %lld %lld %lld\n", st.small, st.large, st.covered, st.bad);
    return st.bad ? 1 : 0;
}
