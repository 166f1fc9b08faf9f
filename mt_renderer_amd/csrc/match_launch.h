// match_launch.h -- the shape of k_match_search's grid and the reading of MTR_MATCH_TUNE.  The only copy of both rules:
// mtr_launch_match (k_match.hip) calls them and adds nothing.  Plain C++ with no HIP, so that tests/test_match_launch_plan.py
// compiles this very source for the host and pins the plan of a sweep of shapes and the parse of a list of strings.
//
// The grid.  Instances come in groups of 32 and rows in tiles of 32.  Crowds of up to share_groups groups run the SHARE layout
// (grid.x = groups: the four waves of a workgroup own the same 32 instances and a quarter of the slab each); larger crowds, and
// every call that stores the scores, the wave-owned one (grid.x = groups / 4 rounded up: wave w of workgroup x owns group
// 4 x + w).  grid.y splits the tiles into slabs of tiles_per_slab so that there are about `target` workgroups in all, never
// more slabs than tiles, and no slab without a tile.
#pragma once
#include <cstdint>
#include <cstdio>

struct MatchTune {
    uint32_t share_groups, target;
};

struct MatchGrid {
    bool share;
    uint32_t gx, gy, tiles_per_slab;
};

// "share_groups,target": two numbers and 1 <= target <= 65535, or the defaults (a null string too)
inline MatchTune match_tune_parse(const char* e) {
    MatchTune t{32u, 1024u};
    unsigned a = 0, b = 0;
    if (e && sscanf(e, "%u,%u", &a, &b) == 2 && b >= 1u && b <= 65535u) { t.share_groups = a; t.target = b; }
    return t;
}

// n >= 1 instances, R >= 1 rows (the launcher returns before this for an empty call)
inline MatchGrid match_grid(uint32_t n, uint32_t R, bool scores, uint32_t share_groups, uint32_t target) {
    const uint32_t ngroups = ((n + 31u) & ~31u) / 32u, ntiles = (R + 31u) / 32u;
    MatchGrid g;
    g.share = !scores && ngroups <= share_groups;
    g.gx = g.share ? ngroups : (ngroups + 3u) / 4u;
    uint32_t gy = (target + g.gx - 1u) / g.gx;
    if (gy > ntiles) gy = ntiles;
    g.tiles_per_slab = (ntiles + gy - 1u) / gy;
    g.gy = (ntiles + g.tiles_per_slab - 1u) / g.tiles_per_slab;
    return g;
}
