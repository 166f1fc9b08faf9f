// The grid of k_match_search and the reading of MTR_MATCH_TUNE, pinned on the CPU: csrc/match_launch.h compiled with
// AddressSanitizer and UBSan.  All grids give the same winners by design, so a changed rule, or a tuning string read
// differently, would go unseen everywhere else.  The program prints
//   - the parse of a list of strings: good ones, none, empty, one number, target 0, 65535 and 65536, junk in front and behind;
//   - for the default tuning and the four the GPU tests force (tests/test_gpu_match_grid.py), each read from its string as the
//     launcher reads it, for a search and for a scores call and for eight row counts, the plan of EVERY n in 1..1100 and
//     2040..2060, as runs of n with one plan (the plan depends on n through its groups of 32, so a run is a group or several).
// tests/test_match_launch_plan.py compares the text with tests/golden/match_launch_plan.txt, which was recorded from the
// launcher's own lines before this header replaced them, and holds the Python model's grid() to every n of every run.
#include "../../mt_renderer_amd/csrc/match_launch.h"
#include <cstdio>

static bool same(const MatchGrid& a, const MatchGrid& b) { return a.share == b.share && a.gx == b.gx && a.gy == b.gy && a.tiles_per_slab == b.tiles_per_slab; }

static void sweep(const MatchTune& t, bool scores, uint32_t R, uint32_t n0, uint32_t n1) {
    uint32_t from = n0;
    MatchGrid run = match_grid(n0, R, scores, t.share_groups, t.target);
    for (uint32_t n = n0 + 1u; n <= n1 + 1u; n++) {
        const bool end = n > n1;
        const MatchGrid g = end ? run : match_grid(n, R, scores, t.share_groups, t.target);
        if (end || !same(g, run)) {
            printf("  n=%u..%u: share=%d gx=%u gy=%u tiles_per_slab=%u\n", from, n - 1u, (int)run.share, run.gx, run.gy, run.tiles_per_slab);
            from = n;
            run = g;
        }
    }
}

int main() {
    const char* const strings[] = {nullptr, "", "32,1", "0,1", "32,6", "0,2", "8,2048", "4294967295,65535", " 7, 9", "32", "32,", ",5", "32,0", "32,65535",
                                   "32,65536", "32,6x", "32,6,7", "32,6 ", "x32,6", "32;6", "32 6", "3.5,6", "32,6.5", "0,0", "junk"};
    for (const char* e : strings) {
        const MatchTune t = match_tune_parse(e);
        if (e) printf("tune \"%s\": %u %u\n", e, t.share_groups, t.target);
        else printf("tune none: %u %u\n", t.share_groups, t.target);
    }
    const char* const tunes[] = {nullptr, "32,1", "0,1", "32,6", "0,2"};
    const uint32_t rows[] = {1u, 31u, 32u, 33u, 300u, 1025u, 4100u, 65536u};
    for (const char* e : tunes) {
        const MatchTune t = match_tune_parse(e);
        for (int scores = 0; scores < 2; scores++)
            for (uint32_t R : rows) {
                printf("plan tune=%s share_groups=%u target=%u scores=%d R=%u\n", e ? e : "none", t.share_groups, t.target, scores, R);
                sweep(t, scores != 0, R, 1u, 1100u);
                sweep(t, scores != 0, R, 2040u, 2060u);
            }
    }
    return 0;
}
