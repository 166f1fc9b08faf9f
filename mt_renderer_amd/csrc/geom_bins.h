// geom_bins.h -- the walk over a record's bins and the emission into the bin queues, shared by k_geom and k_fill.
#pragma once
#include "mtr_internal.h"

namespace mtr {

// ---------------------------------------------------------------------------------------------
// bin iteration shared by k_geom (count) and k_fill (fill): one round = up to 64 records, one per
// lane, in record order.  Lanes whose current bin equals the wave-minimum current bin form a group;
// f(bin, group_mask, is_member) runs once per group, groups in increasing bin order, so both
// kernels see identical (bin, count) sequences.
// ---------------------------------------------------------------------------------------------
// wave-wide minimum as a scalar (wave_reduce, mtr_internal.h)
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    return wave_reduce(v, [](uint32_t a, uint32_t b) { return min(a, b); });
}

template <class F>
__device__ __forceinline__ void for_each_bin_group(RecHdr h, bool act, const FrameBuffers& fb, F f) {
    const uint32_t nbx = fb.nbx;
    uint32_t bx = h.bx0, by = h.by0;
    // position on the first owned bin
    while (act && !bin_owned(fb.own, bx, by, nbx)) {
        if (++bx > h.bx1) { bx = h.bx0; if (++by > h.by1) act = false; }
    }
    for (;;) {
        uint64_t m_act = __ballot(act);
        if (!m_act) break;
        // every lane walks its bins in increasing order and the wave always serves the SMALLEST current
        // bin, so each bin is served exactly once per round, by all of its lanes together, in lane
        // (= submission) order: one ordered segment per (chunk, round, bin)
        uint32_t mybin = by * nbx + bx;
        uint32_t b = act ? mybin : 0xFFFFFFFFu;
        b = wave_min_u32(b);
        bool hit = act && mybin == b;
        uint64_t m = __ballot(hit);
        f(b, m, hit);
        if (hit) {
            do {
                if (++bx > h.bx1) { bx = h.bx0; if (++by > h.by1) act = false; }
            } while (act && !bin_owned(fb.own, bx, by, nbx));
        }
    }
}

// ---------------------------------------------------------------------------------------------
// One round = up to 64 records of a chunk's run, lane = record.  A record whose bin rectangle holds more
// than MTR_WIDE_BINS bins (a big triangle) is "wide": walking its bins with one lane would serialise the
// wave (a 12-triangle cube cost 1 ms that way), so wide records are emitted cooperatively, lane = bin.
// To keep submission order exact a wide record splits the round: the records before it are grouped and
// emitted first, then the wide record, then the rest.  Every segment is keyed by the submission order of
// its first entry, which makes segment keys unique and totally ordered per bin.
//   on_groups(act_sub): bin grouping of the lanes with act_sub set;  on_wide(wl): emit the record of lane wl.
// ---------------------------------------------------------------------------------------------
#define MTR_WIDE_BINS 16

template <class FG, class FW>
__device__ __forceinline__ void walk_round(RecHdr h, bool act, uint32_t lane, FG on_groups, FW on_wide) {
    const uint32_t nb = act ? (uint32_t)(h.bx1 - h.bx0 + 1) * (uint32_t)(h.by1 - h.by0 + 1) : 0u;
    uint64_t mw = __ballot(nb > MTR_WIDE_BINS);
    if (!mw) {
        on_groups(act);
        return;
    }
    uint32_t lo = 0;
    for (;;) {
        const uint32_t wl = mw ? __builtin_amdgcn_readfirstlane((uint32_t)__ffsll((long long)mw) - 1) : 64u;
        on_groups(act && lane >= lo && lane < wl && nb <= MTR_WIDE_BINS);
        if (wl == 64) break;
        on_wide(wl);
        mw &= mw - 1;
        lo = wl + 1;
    }
}

// bins of a wide record: lane i of a 64-lane step serves bin number `i` of the rectangle (row-major)
template <class F>
__device__ __forceinline__ void for_each_wide_bin(RecHdr hw, uint32_t lane, const FrameBuffers& fb, F f) {
    const uint32_t w = (uint32_t)(hw.bx1 - hw.bx0 + 1), n = w * (uint32_t)(hw.by1 - hw.by0 + 1);
    for (uint32_t i = lane; i < n; i += 64) {
        const uint32_t bx = hw.bx0 + i % w, by = hw.by0 + i / w;
        if (bin_owned(fb.own, bx, by, fb.nbx)) f(by * fb.nbx + bx);
    }
}

__device__ __forceinline__ RecHdr hdr_of_lane(RecHdr h, uint32_t wl) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)((uint32_t)h.bx0 | ((uint32_t)h.by0 << 16)), wl);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)((uint32_t)h.bx1 | ((uint32_t)h.by1 << 16)), wl);
    RecHdr r = {(uint16_t)(lo & 0xffff), (uint16_t)(lo >> 16), (uint16_t)(hi & 0xffff), (uint16_t)(hi >> 16)};
    return r;
}

// count pass of the two-pass path (k_geom<false>): one non-returning atomic per (wave, bin) group / wide bin
__device__ __forceinline__ void count_bins(const FrameBuffers& fb, RecHdr h, bool act, uint32_t lane) {
    walk_round(
        h, act, lane,
        [&](bool act_sub) {
            for_each_bin_group(h, act_sub, fb, [&](uint32_t bin, uint64_t m, bool hit) {
                if (hit && lane == (uint32_t)__ffsll((long long)m) - 1)
                    atomicAdd(&fb.bin_count[bin], (unsigned long long)__popcll(m) | (1ull << 32));
            });
        },
        [&](uint32_t wl) {
            for_each_wide_bin(hdr_of_lane(h, wl), lane, fb,
                              [&](uint32_t bin) { atomicAdd(&fb.bin_count[bin], 1ull | (1ull << 32)); });
        });
}

// ---------------------------------------------------------------------------------------------
// Hands one round of records (lane = record `round*64 + lane` of chunk `gid`'s run) to the bin queues.
// The (bin, lanes) groups are enumerated first; queue space for up to 64 groups is then reserved by ONE
// wave-wide returning atomic (lane g reserves for group g), so the atomic round trip is paid once per
// round instead of once per group; finally every member lane writes its entry and every group leader its
// segment descriptor.  DIRECT: bounded per-bin queues (single-pass binning, k_geom); otherwise the exact
// two-pass layout positioned by k_scan (k_fill).
// ---------------------------------------------------------------------------------------------
template <bool DIRECT>
__device__ __forceinline__ void emit_bins(const FrameBuffers& fb, RecHdr h, bool act, uint32_t gid, uint32_t round, uint32_t lane) {
    const uint32_t ord0 = gid * 128u + round * 64u;  // submission order of lane 0's record
    auto put = [&](uint32_t bin, unsigned long long t, uint32_t cnt, uint32_t rank, uint32_t order, bool leader, uint32_t key) {
        const uint32_t off = (uint32_t)t, si = (uint32_t)(t >> 32);
        const uint32_t qb = DIRECT ? bin * fb.qcap : fb.bin_start[bin];
        const uint32_t sb = DIRECT ? bin * fb.scap : fb.seg_start[bin];
        if (!DIRECT || (off + cnt <= fb.qcap && si < fb.scap)) {
            fb.entries[qb + off + rank] = order;
            if (leader) {
                Seg sg = {key, off, cnt, 0u};
                fb.segs[sb + si] = sg;
            }
        } else if (leader) {
            atomicOr(&fb.counters[CTR_OVERFLOW], 4u);
        }
    };
    walk_round(
        h, act, lane,
        [&](bool act_sub) {
            uint32_t gbin = 0, ng = 0;
            uint64_t gmask = 0;
            auto flush = [&]() {
                if (ng == 0) return;
                unsigned long long t = 0;
                if (lane < ng) t = atomicAdd(&fb.bin_fill[gbin], (unsigned long long)__popcll(gmask) | (1ull << 32));
                for (uint32_t gi = 0; gi < ng; gi++) {
                    const uint64_t m = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(gmask >> 32), gi) << 32) |
                                       (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)gmask, gi);
                    const unsigned long long tg = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(t >> 32), gi) << 32) |
                                                  (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)t, gi);
                    const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)gbin, gi);
                    if ((m >> lane) & 1ull) {
                        const uint32_t first = (uint32_t)__ffsll((long long)m) - 1;
                        put(b, tg, (uint32_t)__popcll(m), (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), ord0 + lane, lane == first,
                            ord0 + first);
                    }
                }
                ng = 0;
            };
            for_each_bin_group(h, act_sub, fb, [&](uint32_t bin, uint64_t m, bool) {
                if (lane == ng) { gbin = bin; gmask = m; }
                if (++ng == 64) flush();
            });
            flush();
        },
        [&](uint32_t wl) {
            for_each_wide_bin(hdr_of_lane(h, wl), lane, fb, [&](uint32_t bin) {
                const unsigned long long t = atomicAdd(&fb.bin_fill[bin], 1ull | (1ull << 32));
                put(bin, t, 1u, 0u, ord0 + wl, true, ord0 + wl);
            });
        });
}

// ---------------------------------------------------------------------------------------------
// Single-pass binning for frames the visibility-key tile kernel renders (every material opaque): the winner of a
// pixel does not depend on the order of the queue, so there is no order to keep and no segment to describe.
// Groups form around the FIRST ACTIVE lane's current bin (one v_readlane instead of a wave-wide minimum); a bin may
// then be served more than once per round, which only costs one more reservation.  Same queues, same fill words
// (entries in the low half, reservations in the high half) as the ordered builder.
// ---------------------------------------------------------------------------------------------
typedef unsigned short mtr_us2 __attribute__((ext_vector_type(2)));
// both 16-bit halves at once (v_pk_min_u16 / v_pk_max_u16): wave-wide minimum / maximum of a packed (x, y) pair
template <bool MAX>
__device__ __forceinline__ uint32_t pk_minmax(uint32_t a, uint32_t b) {
    const mtr_us2 x = __builtin_bit_cast(mtr_us2, a), y = __builtin_bit_cast(mtr_us2, b);
    return __builtin_bit_cast(uint32_t, MAX ? __builtin_elementwise_max(x, y) : __builtin_elementwise_min(x, y));
}
template <bool MAX>
__device__ __forceinline__ uint32_t wave_pk_minmax(uint32_t v) {
    return __builtin_amdgcn_readfirstlane(wave_reduce(v, [](uint32_t a, uint32_t b) { return pk_minmax<MAX>(a, b); }));
}

// `slot`: 128 dwords of LDS private to the wave (entry counts, then queue offsets, of an 8x8 window of bins).
__device__ __forceinline__ void emit_bins_unordered(const FrameBuffers& fb, RecHdr h, bool act, uint32_t gid, uint32_t round, uint32_t lane,
                                                    uint32_t* slot) {
    const uint32_t ord0 = gid * 128u + round * 64u;
    const uint32_t nb = act ? (uint32_t)(h.bx1 - h.bx0 + 1) * (uint32_t)(h.by1 - h.by0 + 1) : 0u;
    const uint64_t lt = (1ull << lane) - 1ull;
    // ---- fast path, lane-parallel: every record covers <= 4 bins and the round's bins fit an 8x8 window (a strip
    //      chunk of small triangles always does).  Each lane counts itself into the LDS slot of each of its bins
    //      (the returned count is its place in the group), lane s then reserves queue space for slot s with one
    //      global atomic, and every lane stores its entries: no loop over groups at all. ----
    {
        // The window: a chunk's triangles are neighbours on screen, so try the 8 x 8 bins that start three bins up and left of the
        // first active lane's rectangle (two v_readlane and a ballot); only when some lane does not fit is the round's true bounding
        // window worked out (two wave-wide packed min / max reductions, ~36 instructions: what every round used to pay).
        const uint64_t am = __ballot(act);
        if (!am) return;
        const uint32_t fl = (uint32_t)__ffsll((long long)am) - 1u;
        const uint32_t fx = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)h.bx0, fl), fy = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)h.by0, fl);
        uint32_t wx0 = fx > 3u ? fx - 3u : 0u, wy0 = fy > 3u ? fy - 3u : 0u;
        bool fits = !__ballot(act && !((uint32_t)h.bx0 >= wx0 && (uint32_t)h.bx1 < wx0 + 8u && (uint32_t)h.by0 >= wy0 && (uint32_t)h.by1 < wy0 + 8u));
        if (!fits) {
            const uint32_t lo = wave_pk_minmax<false>(act ? ((uint32_t)h.bx0 | ((uint32_t)h.by0 << 16)) : 0xFFFFFFFFu);
            const uint32_t hi = wave_pk_minmax<true>(act ? ((uint32_t)h.bx1 | ((uint32_t)h.by1 << 16)) : 0u);
            wx0 = lo & 0xffffu; wy0 = lo >> 16;
            fits = (hi & 0xffffu) - wx0 < 8u && (hi >> 16) - wy0 < 8u;
        }
        if (fits && !__ballot(nb > 4u)) {
            const uint32_t w = (uint32_t)(h.bx1 - h.bx0) + 1u;  // 1..4; w >= 3 means a single row
            slot[lane] = 0u;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            uint32_t ranks = 0, own = 0;
            for (uint32_t j = 0; j < 4u; j++) {
                const bool on = j < nb;
                if (!__ballot(on)) break;
                const uint32_t dx = w == 1u ? 0u : (w == 2u ? (j & 1u) : j), dy = w == 1u ? j : (w == 2u ? (j >> 1) : 0u);
                const uint32_t bx = h.bx0 + dx, by = h.by0 + dy;
                if (on && bin_owned(fb.own, bx, by, fb.nbx)) {
                    ranks |= atomicAdd(&slot[(by - wy0) * 8u + (bx - wx0)], 1u) << (8u * j);
                    own |= 1u << j;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint32_t c = slot[lane];
            if (c) {
                const uint32_t bin = (wy0 + (lane >> 3)) * fb.nbx + wx0 + (lane & 7u);
                const uint32_t o = (uint32_t)atomicAdd(&fb.bin_fill[bin], (unsigned long long)c | (1ull << 32));
                // the entry index of the reservation's first place, worked out here, once per bin of the window: the stores
                // below add their rank to it (the multiply by qcap issues at a quarter of the rate, and every store carried
                // one).  No entry has index 2^32 - 1 (the index is 32 bits wide and counts from 0), so it marks an overflow
                uint32_t q0 = bin * fb.qcap + o;
                if (o + c > fb.qcap) { atomicOr(&fb.counters[CTR_OVERFLOW], 4u); q0 = 0xFFFFFFFFu; }
                slot[64 + lane] = q0;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (uint32_t j = 0; j < 4u; j++) {
                if (!__ballot((own >> j) & 1u)) { if (!__ballot(j < nb)) break; continue; }
                const uint32_t dx = w == 1u ? 0u : (w == 2u ? (j & 1u) : j), dy = w == 1u ? j : (w == 2u ? (j >> 1) : 0u);
                const uint32_t bx = h.bx0 + dx, by = h.by0 + dy;
                if ((own >> j) & 1u) {
                    const uint32_t q0 = slot[64 + (by - wy0) * 8u + (bx - wx0)];
                    if (q0 != 0xFFFFFFFFu) fb.entries[q0 + ((ranks >> (8u * j)) & 0xffu)] = ord0 + lane;
                }
            }
            // the next round (or the caller) may reuse the slots at once: LDS operations of one wave are ordered
            return;
        }
    }
    uint32_t gbin = 0, ng = 0;
    uint64_t gmask = 0;
    auto flush = [&]() {
        if (ng == 0) return;
        uint32_t off = 0;
        if (lane < ng) {
            const uint32_t cnt = (uint32_t)__popcll(gmask);
            off = (uint32_t)atomicAdd(&fb.bin_fill[gbin], (unsigned long long)cnt | (1ull << 32));
            if (off + cnt > fb.qcap) atomicOr(&fb.counters[CTR_OVERFLOW], 4u);
        }
        for (uint32_t gi = 0; gi < ng; gi++) {
            const uint64_t m = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(gmask >> 32), gi) << 32) |
                               (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)gmask, gi);
            const uint32_t o = (uint32_t)__builtin_amdgcn_readlane((int)off, gi);
            const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)gbin, gi);
            if (((m >> lane) & 1ull) && o + (uint32_t)__popcll(m) <= fb.qcap)
                fb.entries[b * fb.qcap + o + (uint32_t)__popcll(m & lt)] = ord0 + lane;
        }
        ng = 0;
    };
    bool a = act && nb <= MTR_WIDE_BINS;
    uint32_t bx = h.bx0, by = h.by0;
    while (a && !bin_owned(fb.own, bx, by, fb.nbx)) {
        if (++bx > h.bx1) { bx = h.bx0; if (++by > h.by1) a = false; }
    }
    for (;;) {
        const uint64_t m_act = __ballot(a);
        if (!m_act) break;
        const uint32_t mybin = by * fb.nbx + bx;
        const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)mybin, (uint32_t)__ffsll((long long)m_act) - 1);
        const bool hit = a && mybin == b;
        const uint64_t m = __ballot(hit);
        if (lane == ng) { gbin = b; gmask = m; }
        if (++ng == 64) flush();
        if (hit) {
            do {
                if (++bx > h.bx1) { bx = h.bx0; if (++by > h.by1) a = false; }
            } while (a && !bin_owned(fb.own, bx, by, fb.nbx));
        }
    }
    flush();
    // big triangles: lane = bin of the rectangle, one reservation each
    for (uint64_t mw = __ballot(nb > MTR_WIDE_BINS); mw; mw &= mw - 1) {
        const uint32_t wl = (uint32_t)__ffsll((long long)mw) - 1;
        for_each_wide_bin(hdr_of_lane(h, wl), lane, fb, [&](uint32_t bin) {
            const uint32_t o = (uint32_t)atomicAdd(&fb.bin_fill[bin], 1ull | (1ull << 32));
            if (o < fb.qcap) fb.entries[bin * fb.qcap + o] = ord0 + wl;
            else atomicOr(&fb.counters[CTR_OVERFLOW], 4u);
        });
    }
}

}  // namespace mtr
