// tile_head_fill.cpp -- tile_fill_head (csrc/tile_common.h, the part that is plain C++) on the CPU: the head of the tile
// kernels' parameters (mtr_internal.h: TileHead) is a copy, and a stale or swapped copy would send a kernel to another
// frame's queues.  Over a list of parameter sets -- unsharded and sharded, own_list null and set, a rank without a bin,
// xcd_run 0 / 1 / 16 / 65536, both queue layouts -- every mirrored field must equal its source, the grid must be the whole
// runs the launchers used to compute, the divisor words must still give `/` and `%`, and nothing outside the head may change.
// Every source field holds a value of its own, so a copy taken from the wrong field shows.
// usage: tile_head_fill [mutant]   mutant: tile_fill_head's result with two fields swapped must be caught
// Prints "<parameter sets> <field checks> <mismatches>" and exits 1 on a mismatch.
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mt_renderer_amd/csrc/mtr_internal.h"
#include "../../mt_renderer_amd/csrc/tile_common.h"

static unsigned long long g_checks = 0, g_bad = 0;
#define HOLDS(cond)                                                                       \
    do {                                                                                  \
        g_checks++;                                                                       \
        if (!(cond)) { g_bad++; std::fprintf(stderr, "set %d: %s\n", g_set, #cond); }     \
    } while (0)
static int g_set = 0;

// distinct, recognisable pointers (never dereferenced)
template <class T>
static T* fake(uintptr_t k) { return reinterpret_cast<T*>((uintptr_t)0x100000 * (k + 1)); }

struct Case {
    uint32_t W, H, world, own_count, xcd_run, direct, nhint, zero_nwords;
    bool own_list, zero_words, zero_next, host_status;
};

static TileParams make(const Case& c) {
    TileParams p;
    std::memset(&p, 0xA5, sizeof p);  // whatever the caller left in the head (and everywhere else) must not matter
    FrameBuffers& fb = p.fb;
    fb.rec_hdr = fake<RecHdr>(1); fb.rec_a = fake<RecP>(2); fb.rec_l = fake<int4>(3); fb.rec_b = fake<RecB>(4);
    fb.chunk_info = fake<ChunkInfo>(5); fb.bin_count = fake<unsigned long long>(6); fb.bin_fill = fake<unsigned long long>(7);
    fb.bin_start = fake<uint32_t>(8); fb.seg_start = fake<uint32_t>(9); fb.entries = fake<uint32_t>(10); fb.segs = fake<Seg>(11);
    fb.counters = fake<uint32_t>(12);
    fb.rec_cap = 1001; fb.entry_cap = 1002; fb.seg_cap = 1003;
    fb.W = c.W; fb.H = c.H; fb.nbx = (c.W + 15) / 16; fb.nby = (c.H + 15) / 16;
    fb.own = Ownership{};
    fb.own.world = c.world; fb.own.rank = c.world > 1 ? 1 : 0; fb.own.own_count = c.own_count;
    fb.own.own_list = c.own_list ? fake<uint32_t>(13) : nullptr;
    fb.direct = c.direct; fb.qcap = 2048 + c.direct; fb.scap = 96 + c.direct; fb.unordered = 1;
    p.mats = fake<DMat>(14); p.color = fake<uint8_t>(15); p.depth = fake<float>(16);
    p.clear_rgba8 = 0x11223344u; p.clear_depth = 0.75f;
    p.bin_flag = fake<uint8_t>(17); p.mixed = 1;
    p.zero_next = c.zero_next ? fake<uint32_t>(18) : nullptr;
    p.host_status = c.host_status ? fake<uint32_t>(19) : nullptr;
    p.vis_waves = 4; p.xcd_run = c.xcd_run;
    p.zero_words = c.zero_words ? fake<uint32_t>(20) : nullptr;
    p.zero_nwords = c.zero_nwords;
    p.hint_out = fake<uint32_t>(21); p.nhint = c.nhint;
    for (int k = 0; k < 4; k++) { p.hint_word[k] = (uint16_t)(32 * k); p.hint_slot[k] = (uint16_t)(3 - k); }
    return p;
}

static void check(const Case& c, bool mutant) {
    const TileParams before = make(c);
    TileParams p;
    std::memcpy(&p, &before, sizeof p);  // padding included: the comparisons below are bytewise
    tile_fill_head(p);
    if (mutant) { uint32_t* t = p.head.bin_start; p.head.bin_start = p.head.seg_start; p.head.seg_start = t; }
    const TileHead& h = p.head;
    // the workgroups of the launch: the rank's bins, eight XCDs, whole runs
    uint32_t grid = (c.own_count + 7) / 8 * 8;
    if (c.xcd_run) grid = (grid / 8 + c.xcd_run - 1) / c.xcd_run * c.xcd_run * 8;
    HOLDS(h.grid == grid);
    HOLDS(h.grid % 8 == 0 && h.grid >= c.own_count && (c.own_count == 0 || c.xcd_run || h.grid - c.own_count < 8));
    HOLDS(h.own_count == p.fb.own.own_count);
    HOLDS(h.own_list == p.fb.own.own_list);
    HOLDS(h.nbx == p.fb.nbx);
    HOLDS(h.nbins == p.fb.nbx * p.fb.nby);
    HOLDS(h.W == p.fb.W);
    HOLDS(h.H == p.fb.H);
    HOLDS(h.direct == p.fb.direct);
    HOLDS(h.qcap == p.fb.qcap);
    HOLDS(h.scap == p.fb.scap);
    HOLDS(h.xcd_run == p.xcd_run);
    HOLDS(h.zero_nwords == p.zero_nwords);
    HOLDS(h.nhint == p.nhint);
    HOLDS(h.entries == p.fb.entries);
    HOLDS(h.bin_fill == p.fb.bin_fill);
    HOLDS(h.bin_start == p.fb.bin_start);
    HOLDS(h.seg_start == p.fb.seg_start);
    HOLDS(h.counters == p.fb.counters);
    HOLDS(h.rec_a == p.fb.rec_a);
    HOLDS(h.zero_next == p.zero_next);
    HOLDS(h.zero_words == p.zero_words);
    HOLDS(h.host_status == p.host_status);
    // the divisor words: bin / nbx and bin % nbx for every bin of the frame, i / run and i % run for every blockIdx.x >> 3
    for (uint32_t bin = 0; bin < h.nbins; bin++) {
        const uint32_t by = mtr::udiv_apply(bin, h.nbx_mul, h.nbx_shift);
        if (by != bin / h.nbx || bin - by * h.nbx != bin % h.nbx) { HOLDS(!"bin / nbx"); break; }
    }
    g_checks++;
    if (c.xcd_run) {
        for (uint32_t i = 0; i < h.grid / 8; i++) {
            const uint32_t q = mtr::udiv_apply(i, h.run_mul, h.run_shift);
            if (q != i / c.xcd_run || i - q * c.xcd_run != i % c.xcd_run) { HOLDS(!"i / run"); break; }
        }
        // ... and block_to_bin's slots with them: every bin of the rank is some workgroup's, once
        unsigned long long sum = 0, want = (unsigned long long)c.own_count * (c.own_count - (c.own_count ? 1 : 0)) / 2, taken = 0;
        for (uint32_t b = 0; b < h.grid; b++) {
            const uint32_t x = b & 7, i = b >> 3, q = mtr::udiv_apply(i, h.run_mul, h.run_shift);
            const uint32_t slot = (q * 8 + x) * c.xcd_run + (i - q * c.xcd_run);
            if (slot < c.own_count) { sum += slot; taken++; }
        }
        HOLDS(taken == c.own_count && sum == want);
    } else {
        HOLDS(h.run_mul == 0 && h.run_shift == 0);
    }
    // nothing but the head was written
    HOLDS(std::memcmp(&p.fb, &before.fb, sizeof p.fb) == 0);
    HOLDS(std::memcmp(&p.mats, &before.mats, sizeof(TileParams) - offsetof(TileParams, mats)) == 0);
    // filling twice, or over another launch's head, gives the same head (the mixed frame's second launch reuses the copy)
    TileParams again = p;
    again.nhint = 0;
    tile_fill_head(again);
    HOLDS(again.head.nhint == 0 && again.head.grid == h.grid && again.head.entries == p.fb.entries);
}

int main(int argc, char** argv) {
    const bool mutant = argc > 1 && !std::strcmp(argv[1], "mutant");
    static_assert(offsetof(TileParams, head) == 0, "the head is what the kernels fetch first");
    static_assert(offsetof(TileParams, fb) == sizeof(TileHead), "FrameBuffers follows the head unchanged");
    std::vector<Case> cases;
    const uint32_t runs[] = {0u, 1u, 16u, 65536u};
    for (uint32_t run : runs) {
        //              W     H    world own_count      run direct nhint nwords own_list zero_w zero_n status
        cases.push_back({1920, 1080, 1, 120 * 68, run, 1, 0, 0, false, false, true, true});      // the headline frame
        cases.push_back({1920, 1080, 1, 120 * 68, run, 0, 0, 0, false, false, true, true});      // ... on two-pass queues
        cases.push_back({272, 144, 1, 17 * 9, run, 1, 0, 0, false, false, false, false});        // 153 bins: no multiple of any run
        cases.push_back({16, 16, 1, 1, run, 1, 0, 0, false, false, true, true});                 // one bin
        cases.push_back({1920, 1080, 3, 2720, run, 1, 2, 7 * 32, true, true, true, true});       // rank 1 of 3, culling counters
        cases.push_back({1920, 1080, 3, 2720, run, 0, 4, 200 * 32, true, true, true, true});
        cases.push_back({640, 360, 8, 1, run, 1, 1, 129 * 32, true, true, true, true});          // a rank that owns one bin
        cases.push_back({640, 360, 8, 0, run, 1, 0, 0, true, false, true, true});                // a rank that owns none
        cases.push_back({16384, 16384, 1, 1024 * 1024, run, 1, 0, 0, false, false, true, true}); // the largest frame
    }
    for (const Case& c : cases) { check(c, mutant); g_set++; }
    std::printf("%d %llu %llu\n", g_set, g_checks, g_bad);
    return g_bad ? 1 : 0;
}
