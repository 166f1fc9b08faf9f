// tri_gen.h -- the random triangles of the exactness tests (span_exact.cpp, tri_setup_exact.cpp): a bin of a grid of up
// to 40 x 40, sometimes cut by the viewport's right / bottom edge, and a triangle near it in 1/256 px.  Eight modes in
// turn: vertices anywhere, on pixel centres, on bin corners, mixed, a horizontal edge, a vertical edge, a long sliver,
// extents at exactly the class limit; both windings alternate (one of them covers nothing).
#pragma once
#include <cstdint>
#include <random>
#include <utility>

#include "../../mt_renderer_amd/csrc/tri_setup.h"

struct TriCase {
    int32_t X[3], Y[3], binx0, biny0, vw, vh;
};

struct TriGen {
    static const int32_t BIN = 16, LIMIT = MTR_TRI_CLASS_LIMIT;
    std::mt19937_64 rng;
    long long made = 0;
    explicit TriGen(unsigned long long seed) : rng(seed) {}
    int32_t U(int32_t lo, int32_t hi) { return (int32_t)(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1))); }

    // max_ext == 0: extents mostly small, up to the class limit; otherwise extents above the limit, up to max_ext
    TriCase next(int32_t max_ext = 0) {
        TriCase c;
        made++;
        c.binx0 = U(0, 40) * BIN; c.biny0 = U(0, 40) * BIN;
        // the viewport's right / bottom edge cuts the bin in a quarter of the cases
        c.vw = U(0, 3) == 0 ? U(1, 16) : 1 << 20; c.vh = U(0, 3) == 0 ? U(1, 16) : 1 << 20;
        const int mode = (int)(made % 8);
        int32_t* X = c.X; int32_t* Y = c.Y;
        // extent of the triangle in 1/256 px: mostly small, up to the class limit (16384 = 64 px)
        const int32_t ext = max_ext ? U(LIMIT + 1, max_ext) : mode == 7 ? LIMIT : (U(0, 2) == 0 ? U(64, LIMIT) : U(16, 1536));
        const int32_t cx = c.binx0 * 256 + U(-ext, BIN * 256 + ext), cy = c.biny0 * 256 + U(-ext, BIN * 256 + ext);
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
        return c;
    }
};
