// k_events.hip -- animation events (SPEC.md section 22): the return channel of the players.  An event set holds sorted
// markers per clip; one call per frame takes the step records a player wrote (what k_root takes) and writes the compact list
// of the markers each instance arrived at or passed, ordered by instance, then step, then firing order, with a total and
// optionally a 32-bit mask per instance.  Every scalar rule lives in event_math.h, which the host test compiles too.
//
// Three launches on the caller's stream: count, scan, fill -- the bin queues' answer to ordered compaction (k_bin.hip).
//   k_events_count  one lane per instance, 256-thread workgroups.  A lane's count is a few binary searches over its clips'
//                   markers, never a walk; the workgroup's total (wave_incl_scan_u32 and four LDS words) goes to sums[block].
//   k_events_scan   one workgroup of 1024 scans the block sums exclusively in place, in turns of its own width with a carry,
//                   and writes count[0] (fired) and count[1] (written).
//   k_events_fill   the same lanes: offset = sums[block] + the workgroup-local exclusive prefix of the lanes' counts, which
//                   they recompute (DESIGN.md section 3 "k_events" says why); a lane that fired something walks its ranges
//                   and stores each record as one 16-byte word while the index is below the capacity, and ORs its mask.
// No spin-wait, no decoupled look-back, no atomics of any kind: the order of the list and every word written are functions
// of the inputs alone, whichever workgroup runs first.
//
// Memory safety.  n (1..max_instances <= 2^27), nsteps (1..8) and capacity are host values, validated.  A lane whose
// instance is >= n loads and stores nothing of its own; it still takes part in the workgroup's scan with a count of 0, so every
// barrier is reached by all 256 (1024) threads.  The steps hold n * nsteps records and are indexed by the lane's own instance
// and i < nsteps only.  From device memory comes the clip of a step, clamped to nclips - 1 in event_spans before it reaches
// the clip and range tables; positions, steps and weights reach no address.  Everything else that reaches an address was
// validated when the set was created and is immutable since: a clip's range [first, first + count) lies inside the marker
// array, and a search returns an index inside [0, count], so every marker index is inside the clip's own range.  sums holds
// ceil(max_instances / 256) words and is indexed by blockIdx.x < ceil(n / 256) (count, fill) or by b < ceil(n / 256) (scan).
// The list is written at indices < capacity only; the host rejects a call whose n * nsteps * (largest marker count of a clip)
// exceeds 2^32 - 1, so no count, sum or index wraps.  bits holds n words and is indexed by the lane's own instance.
#include "mtr_internal.h"
#include "event_math.h"

namespace mtr {

static_assert(MTR_EVENTS_BLOCK == 256u && MTR_EVENTS_SCAN == 1024u, "the kernels below are written for these widths");

__device__ __forceinline__ EventTables event_tables(const EventParams& p) {
    EventTables t;
    t.clips = reinterpret_cast<const PlayClip*>(p.clips);
    t.ranges = p.ranges;
    t.markers = reinterpret_cast<const EventMarker*>(p.markers);
    t.nclips = p.nclips;
    return t;
}

// the lane's count, and through s_w (four words) the sum of the counts of the waves below its own; *total: the workgroup's
__device__ __forceinline__ uint32_t block_excl_prefix(uint32_t c, uint32_t* s_w, uint32_t* total) {
    const uint32_t incl = wave_incl_scan_u32(c), wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) s_w[wave] = incl;
    __syncthreads();
    const uint32_t w0 = s_w[0], w1 = s_w[1], w2 = s_w[2], w3 = s_w[3];
    *total = w0 + w1 + w2 + w3;
    return (wave > 0u ? w0 : 0u) + (wave > 1u ? w1 : 0u) + (wave > 2u ? w2 : 0u) + incl - c;
}

__global__ __launch_bounds__(256) void k_events_count(EventParams p) {
    __shared__ uint32_t s_w[4];
    const uint32_t inst = blockIdx.x * 256u + threadIdx.x;
    uint32_t c = 0;
    if (inst < p.n) c = event_count(reinterpret_cast<const EventStepIn*>(p.steps) + (size_t)inst * p.nsteps, p.nsteps, p.min_weight, event_tables(p));
    uint32_t total;
    (void)block_excl_prefix(c, s_w, &total);
    if (threadIdx.x == 0) p.sums[blockIdx.x] = total;
}

// single workgroup: at most 2^27 / 256 = 2^19 sums, 512 turns
__global__ __launch_bounds__(1024) void k_events_scan(EventParams p) {
    __shared__ uint32_t s_w[16];
    __shared__ uint32_t s_carry;
    const uint32_t nb = (p.n + 255u) / 256u;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += 1024u) {
        const uint32_t b = base + threadIdx.x;
        const uint32_t v = b < nb ? p.sums[b] : 0u;
        const uint32_t incl = wave_incl_scan_u32(v);
        if (lane == 63u) s_w[wave] = incl;
        __syncthreads();
        uint32_t pre = s_carry;
        for (uint32_t w = 0; w < wave; w++) pre += s_w[w];
        if (b < nb) p.sums[b] = pre + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023u) s_carry = pre + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const uint32_t total = s_carry;
        p.count[0] = total;
        p.count[1] = total < p.capacity ? total : p.capacity;
    }
}

__global__ __launch_bounds__(256) void k_events_fill(EventParams p) {
    __shared__ uint32_t s_w[4];
    const uint32_t inst = blockIdx.x * 256u + threadIdx.x;
    const EventTables t = event_tables(p);
    const EventStepIn* steps = reinterpret_cast<const EventStepIn*>(p.steps) + (size_t)(inst < p.n ? inst : 0u) * p.nsteps;
    uint32_t c = 0;
    if (inst < p.n) c = event_count(steps, p.nsteps, p.min_weight, t);
    uint32_t total;
    const uint32_t off = p.sums[blockIdx.x] + block_excl_prefix(c, s_w, &total);
    if (inst >= p.n) return;
    uint32_t mask = 0;
    if (c != 0u && (p.bits || off < p.capacity)) {
        uint32_t idx = off;
        uint4* out = reinterpret_cast<uint4*>(p.out);
        const uint32_t cap = p.capacity;
        event_walk(steps, p.nsteps, p.min_weight, t, [&](const EventMarker& m, uint32_t where, float w) {
            const uint32_t id = m.id;
            if (idx < cap) out[idx] = make_uint4(inst, id, where, __float_as_uint(w));
            idx++;
            mask |= 1u << (id & 31u);
        });
    }
    if (p.bits) p.bits[inst] = mask;
}

}  // namespace mtr

void mtr_launch_events(const EventParams& p, hipStream_t s) {
    if (p.n == 0 || p.nclips == 0 || p.nsteps == 0) return;
    const dim3 grid((p.n + MTR_EVENTS_BLOCK - 1u) / MTR_EVENTS_BLOCK);
    hipLaunchKernelGGL(mtr::k_events_count, grid, dim3(256), 0, s, p);
    hipLaunchKernelGGL(mtr::k_events_scan, dim3(1), dim3(1024), 0, s, p);
    hipLaunchKernelGGL(mtr::k_events_fill, grid, dim3(256), 0, s, p);
}
