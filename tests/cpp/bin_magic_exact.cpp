// bin_magic_exact.cpp -- the multiply-high divisions of csrc/tile_common.h (the part of the header that is plain C++)
// against `/` and `%`, exhaustively over what the tile kernels can meet:
//   nbx    bin / nbx, bin % nbx for every nbx = 1 .. 1024 (frames are at most 16384 px wide, bins 16 px) and every bin index
//          below nbx * 1024 (at most 16384 px high)
//   run    i / run, i % run for every run length 1 .. 65536 the host accepts (MTR_TILE_RUN) and every i = blockIdx.x >> 3 of
//          the launch: below ceil(2^20 / 8) bins per XCD rounded up to whole runs
//   magic  (k * row_magic(iw)) >> 16 == k / iw for iw = 1 .. 16, k < 256
// usage: bin_magic_exact <nbx|run|magic> [delta]   delta is added to every multiplier (the test's mutant: -1)
// Prints "<divisors> <dividends> <mismatches>" and exits 1 on a mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "../../mt_renderer_amd/csrc/tile_common.h"

static const uint32_t MAX_NB = 16384 / 16;            // bins per row / column
static const uint32_t MAX_RUN = 65536;                // host_device.cpp: MTR_TILE_RUN
static const uint32_t MAX_PER_XCD = MAX_NB * MAX_NB / 8;  // (own_count + 7) / 8

// every n below `count` against the quotient and remainder kept by counting (no division in the loop)
static uint64_t check_divisor(uint32_t d, uint32_t count, int delta) {
    const mtr::UDiv m = mtr::udiv_make(d);
    const uint32_t mul = m.mul + (uint32_t)delta;
    uint64_t bad = 0;
    uint32_t q = 0, r = 0;
    for (uint32_t n = 0; n < count; n++) {
        const uint32_t qq = mtr::udiv_apply(n, mul, m.shift);
        bad += (qq != q) | (n - qq * d != r);
        if (++r == d) { r = 0; q++; }
    }
    return bad;
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    const int delta = argc > 2 ? std::atoi(argv[2]) : 0;
    uint64_t divisors = 0, dividends = 0, bad = 0;
    if (!std::strcmp(mode, "magic")) {
        for (uint32_t iw = 1; iw <= 16; iw++, divisors++)
            for (uint32_t k = 0; k < 256; k++, dividends++) bad += ((k * (mtr::row_magic(iw) + (uint32_t)delta)) >> 16) != k / iw;
    } else if (!std::strcmp(mode, "nbx") || !std::strcmp(mode, "run")) {
        const bool run = mode[0] == 'r';
        const uint32_t dmax = run ? MAX_RUN : MAX_NB;
        // spot check of the bookkeeping above against the operators themselves
        for (uint32_t d = 1; d <= dmax; d += 37) {
            const mtr::UDiv m = mtr::udiv_make(d);
            for (uint32_t n = 0; n < (1u << 20); n += 4099) bad += mtr::udiv_apply(n, m.mul, m.shift) != n / d;
        }
        std::atomic<uint32_t> next(1);
        std::atomic<uint64_t> tot_bad(0), tot_n(0);
        const unsigned nthreads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < nthreads; t++)
            pool.emplace_back([&] {
                uint64_t b = 0, c = 0;
                for (uint32_t d; (d = next.fetch_add(1)) <= dmax;) {
                    const uint32_t count = run ? (MAX_PER_XCD + d - 1) / d * d : d * MAX_NB;
                    b += check_divisor(d, count, delta);
                    c += count;
                }
                tot_bad += b;
                tot_n += c;
            });
        for (auto& th : pool) th.join();
        divisors = dmax;
        dividends = tot_n;
        bad += tot_bad;
    } else {
        std::fprintf(stderr, "usage: bin_magic_exact <nbx|run|magic> [delta]\n");
        return 2;
    }
    std::printf("%llu %llu %llu\n", (unsigned long long)divisors, (unsigned long long)dividends, (unsigned long long)bad);
    return bad ? 1 : 0;
}
