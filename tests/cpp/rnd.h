// The seeded generator of the stand-alone programs of this directory (splitmix64): the including program gives the seed with
// #define MTR_RND_SEED, so its sequence is its own and the same in every run.
#pragma once
#include <cstdint>

static uint64_t rs = MTR_RND_SEED;
static inline uint64_t rnd() {
    uint64_t z = (rs += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static inline uint32_t pick(uint32_t lo, uint32_t hi) { return lo + (uint32_t)(rnd() % (hi - lo + 1)); }
