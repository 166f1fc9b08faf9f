// k_match.hip -- motion matching (SPEC.md section 25): per instance the database row whose features lie nearest to where the
// instance is and where it wants to go, and the command that fades there.  A match set holds R rows of D features; a call
// scores every row against the query of each of n instances, s = F q + c with c_r = -(|f_r|^2 / 2 + bias_r), keeps the
// greatest score among the rows the instance's filter admits, and writes command slot i of an n-slot mtr_play_cmd list as a
// controller does.  Every scalar rule lives in match_math.h, which the host test compiles too.
//
// Three launches in stream order, no spin-wait (as k_events):
//   k_match_query   one lane per instance: the lead of its play state, the binary search for its current row, its query
//                   written into the set's scratch in the lane order the search reads, its winner key cleared.
//   k_match_search  the hot path.  Database rows are M and instances N of v_mfma_f32_32x32x2_f32; c_r is the C input, so the
//                   chain of section 25 starts from it; k runs over the dimensions in order, two to an instruction.
//   k_match_decide  one lane per instance: the fmaf chain on its current row, the decision, the command and the result.
//
// Lanes of the search.  256-thread workgroups, two layouts.  Above 1024 instances wave w of workgroup x owns instances
// 32 (4 x + w) .. + 31, so a workgroup's four waves stream the same features (the later three from cache) and no two waves of
// a workgroup share an instance: no LDS and no barrier.  Up to 1024 instances the four waves own the SAME 32 instances and a
// quarter of the slab each and are joined through 1 KiB of LDS behind one barrier (SHARE).  grid.y splits the 32-row tiles
// into slabs, about 1024 workgroups in all, so that a crowd of 256 still fills the chip.  A wave
// keeps its instances' queries in Dp / 2 VGPRs for the whole slab (lane l: dimension 2 k + (l >> 5) of instance l & 31 for
// k-step k) and per tile loads Dp / 8 times 16 bytes of features per lane, stored at creation in exactly that lane order
// (match_slot), 16 c_r as four 16-byte loads, and with a filter 16 tag words the same way.  Dp is D rounded up to 8 with
// zeroes on both sides.  In the 32 x 32 result lane l holds rows 8 (i >> 2) + 4 (l >> 5) + (i & 3), i = 0..15, of instance
// l & 31: it keeps a running best over its registers in ascending row order (a strict compare keeps the lowest row among
// equals), one tile behind the matrix core, whose next chain is issued first.  At the end of the slab the two half-waves
// are joined by one cross-lane move and lanes 0..31 (SHARE: of wave 0) issue one 64-bit atomicMax per instance on the key
// (order of s) << 32 | ~row: a vector atomic on global memory, order-independent, so the result does not depend on which
// workgroup ran first.  Rows behind R carry c = NaN, and a NaN score never wins.
//
// Memory safety.  n (1..max_instances), instance_base and the shapes are host values, validated; lanes whose instance is >=
// n rounded up to 32 return before any access, and those in [n, that) touch the set's own scratch only, which is sized for
// max_instances rounded up to 32.  The play states, raw queries, filters, commands and results hold n records and are
// indexed by the lane's own instance only.  From device memory come (a) clip_a and clip_b of the play state, clamped to
// nclips - 1 before they reach the clip ranges; (b) the current row and the winner key in the set's scratch, written by
// this call's own first two launches and clamped to R - 1 again before they reach the rows.  The ranges of a clip lie in
// [0, R] by validation; tile and slab indices are formed from R and the grid.  Positions, features, scores and tags reach no
// address.
#include "mtr_internal.h"
#include "match_math.h"
#include "match_launch.h"

#include <cstdio>
#include <cstdlib>

namespace mtr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ MatchTables match_tables(const MatchParams& p) {
    MatchTables t;
    t.clips = reinterpret_cast<const PlayClip*>(p.clips);
    t.ranges = p.ranges;
    t.rows = reinterpret_cast<const MatchRow*>(p.rows);
    t.c = p.c; t.feat = p.feat; t.mean = p.mean; t.scale = p.scale;
    t.pose_dims = p.pose_dims;
    t.nclips = p.nclips; t.R = p.R; t.D = p.D; t.Dp = match_dp(p.D); t.flags = p.flags;
    t.seconds = p.seconds; t.near = p.near; t.margin = p.margin;
    return t;
}

__device__ __forceinline__ PlayState match_play(const MatchParams& p, uint32_t inst) {
    const uint4* pp = reinterpret_cast<const uint4*>(p.play) + (size_t)inst * 2;
    const uint4 p0 = pp[0], p1 = pp[1];
    PlayState pl;
    pl.clip_a = p0.x; pl.clip_b = p0.y; pl.x_a = __uint_as_float(p0.z); pl.x_b = __uint_as_float(p0.w);
    pl.w = __uint_as_float(p1.x); pl.fade = __uint_as_float(p1.y); pl.speed = __uint_as_float(p1.z); pl.flags = p1.w;
    return pl;
}

__global__ __launch_bounds__(256) void k_match_query(MatchParams p) {
    const uint32_t inst = blockIdx.x * 256u + threadIdx.x;
    const uint32_t np = (p.n + 31u) & ~31u, Dp = match_dp(p.D);
    if (inst >= np) return;
    if (inst >= p.n) {  // the rest of the last group of 32: queries of zeroes, so that the search multiplies nothing stale
        for (uint32_t d = 0; d < Dp; d++) p.query[match_slot(inst, d, Dp)] = 0.0f;
        return;
    }
    const MatchTables t = match_tables(p);
    const MatchLead l = match_lead(match_play(p, inst), p.nclips);
    const uint32_t cur = match_cur(t.rows, p.ranges[2u * l.clip], p.ranges[2u * l.clip + 1u], l.p);
    const float* raw = p.raw ? p.raw + (size_t)inst * p.D : nullptr;
    for (uint32_t d = 0; d < p.D; d++) p.query[match_slot(inst, d, Dp)] = match_query(t, cur, raw, d);
    for (uint32_t d = p.D; d < Dp; d++) p.query[match_slot(inst, d, Dp)] = 0.0f;
    p.cur[inst] = cur;
    p.keys[inst] = 0ull;
}

// the running best of one lane: 16 rows of one instance per tile, in ascending row order
struct MatchBest {
    float s;
    uint32_t row;
};

template <bool FILTER, bool SCORES>
__device__ __forceinline__ void match_take(const MatchParams& p, const f32x16& acc, uint32_t tile, uint32_t mask, uint32_t half, uint32_t inst, MatchBest& b) {
#pragma unroll
    for (uint32_t i = 0; i < 16u; i++) {
        const float s = acc[i];
        const uint32_t row = tile * 32u + 8u * (i >> 2) + 4u * half + (i & 3u);
        bool take = s > b.s || (b.row == MTR_MATCH_NONE && s >= b.s);  // -inf may win; NaN compares false
        if (FILTER) take = take && ((mask >> i) & 1u);
        b.s = take ? s : b.s;
        b.row = take ? row : b.row;
        if (SCORES) {
            if (inst < p.n && row < p.R) p.scores[(size_t)inst * p.R + row] = s + 0.0f;
        }
    }
}

// G: groups of 8 dimensions, Dp / 8.  SHARE: the four waves of a workgroup own the SAME 32 instances and a quarter of the slab's
// tiles each, and are joined through LDS before the one atomic per instance and workgroup: the layout for small crowds, whose
// few instance groups would otherwise need many slabs, and so many atomics on few addresses, to fill the chip.
template <int G, bool FILTER, bool SCORES, bool SHARE>
__global__ __launch_bounds__(256) void k_match_search(MatchParams p, uint32_t tiles_per_slab) {
    const uint32_t lane = threadIdx.x & 63u, half = lane >> 5, wave = threadIdx.x >> 6;
    const uint32_t group = SHARE ? blockIdx.x : blockIdx.x * 4u + wave;
    if (group >= ((p.n + 31u) >> 5)) return;  // SHARE: the whole workgroup; otherwise a whole wave, and nothing below synchronises
    const uint32_t inst = group * 32u + (lane & 31u);
    const uint32_t ntiles = (p.R + 31u) >> 5;
    uint32_t t0 = blockIdx.y * tiles_per_slab;
    uint32_t t1 = t0 + tiles_per_slab < ntiles ? t0 + tiles_per_slab : ntiles;
    if (SHARE) {
        const uint32_t quarter = (tiles_per_slab + 3u) >> 2;
        t0 += wave * quarter;
        if (t0 + quarter < t1) t1 = t0 + quarter;
    }
    MatchBest best;
    best.s = -INFINITY; best.row = MTR_MATCH_NONE;
    if (t0 < t1) {  // wave-uniform
        float4 q[G];
        const float4* qp = reinterpret_cast<const float4*>(p.query) + (size_t)group * G * 64u + lane;
#pragma unroll
        for (int g = 0; g < G; g++) q[g] = qp[g * 64];
        uint32_t require = 0u, exclude = 0u;
        if (FILTER) {
            if (inst < p.n) {
                const uint2 f = reinterpret_cast<const uint2*>(p.filter)[inst];
                require = f.x; exclude = f.y;
            }
        }
        const float4* fp = reinterpret_cast<const float4*>(p.feat) + lane;
        const float4* cp = reinterpret_cast<const float4*>(p.c) + half;
        const uint4* gp = reinterpret_cast<const uint4*>(p.tags) + half;
        f32x16 prev;
        uint32_t prev_mask = 0u;
        float4 a[G];
#pragma unroll
        for (int g = 0; g < G; g++) a[g] = fp[((size_t)t0 * G + g) * 64u];
        for (uint32_t t = t0; t < t1; t++) {
            f32x16 acc;
            uint32_t mask = 0u;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float4 c4 = cp[(size_t)t * 8u + 2u * k];
                acc[4 * k] = c4.x; acc[4 * k + 1] = c4.y; acc[4 * k + 2] = c4.z; acc[4 * k + 3] = c4.w;
                if (FILTER) {
                    const uint4 g4 = gp[(size_t)t * 8u + 2u * k];
                    mask |= (match_candidate(g4.x, require, exclude) ? 1u : 0u) << (4 * k);
                    mask |= (match_candidate(g4.y, require, exclude) ? 2u : 0u) << (4 * k);
                    mask |= (match_candidate(g4.z, require, exclude) ? 4u : 0u) << (4 * k);
                    mask |= (match_candidate(g4.w, require, exclude) ? 8u : 0u) << (4 * k);
                }
            }
            float4 an[G];
            const uint32_t tn = t + 1u < t1 ? t + 1u : t;  // the last tile loads itself again: no branch around the loads
#pragma unroll
            for (int g = 0; g < G; g++) an[g] = fp[((size_t)tn * G + g) * 64u];
#pragma unroll
            for (int g = 0; g < G; g++) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].x, q[g].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].y, q[g].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].z, q[g].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g].w, q[g].w, acc, 0, 0, 0);
            }
            if (t > t0) match_take<FILTER, SCORES>(p, prev, t - 1u, prev_mask, half, inst, best);  // while the matrix core runs
            prev = acc;
            prev_mask = mask;
#pragma unroll
            for (int g = 0; g < G; g++) a[g] = an[g];
        }
        match_take<FILTER, SCORES>(p, prev, t1 - 1u, prev_mask, half, inst, best);
    }
    if (SCORES) return;

    unsigned long long key = best.row != MTR_MATCH_NONE ? match_key(best.s, best.row) : 0ull;
    const unsigned long long other = __shfl_xor(key, 32, 64);
    key = other > key ? other : key;
    if (SHARE) {
        __shared__ unsigned long long join[4][32];
        if (half == 0u) join[wave][lane] = key;
        __syncthreads();
        if (wave != 0u) return;
#pragma unroll
        for (int w = 1; w < 4; w++) {
            const unsigned long long k = join[w][lane & 31u];
            key = k > key ? k : key;
        }
    }
    if (half == 0u && key != 0ull && inst < p.n) atomicMax(p.keys + inst, key);
}

__global__ __launch_bounds__(256) void k_match_decide(MatchParams p) {
    const uint32_t inst = blockIdx.x * 256u + threadIdx.x;
    if (inst >= p.n) return;
    const MatchTables t = match_tables(p);
    const MatchLead l = match_lead(match_play(p, inst), p.nclips);
    uint32_t cur = p.cur[inst];
    if (cur != MTR_MATCH_NONE && cur > p.R - 1u) cur = p.R - 1u;
    unsigned long long key = p.keys[inst];
    if (key != 0ull && ~(uint32_t)key > p.R - 1u) key = (key & 0xFFFFFFFF00000000ull) | (uint32_t)~(p.R - 1u);
    const float s_cur = cur != MTR_MATCH_NONE ? match_score(t, p.query, inst, cur) : 0.0f;
    PlayCmd cmd;
    MatchResult res;
    match_decide(t, l, cur, s_cur, key, p.instance_base + inst, cmd, res);
    reinterpret_cast<uint4*>(p.cmds)[inst] = make_uint4(cmd.instance, cmd.clip, __float_as_uint(cmd.x), __float_as_uint(cmd.seconds));
    if (p.results) reinterpret_cast<uint4*>(p.results)[inst] = make_uint4(res.row, res.cur, __float_as_uint(res.score), __float_as_uint(res.cur_score));
}

template <int G>
static void match_search_launch(const MatchParams& p, bool share, dim3 grid, uint32_t tps, hipStream_t s) {
    if (p.scores) hipLaunchKernelGGL((k_match_search<G, false, true, false>), grid, dim3(256), 0, s, p, tps);
    else if (share && p.filter) hipLaunchKernelGGL((k_match_search<G, true, false, true>), grid, dim3(256), 0, s, p, tps);
    else if (share) hipLaunchKernelGGL((k_match_search<G, false, false, true>), grid, dim3(256), 0, s, p, tps);
    else if (p.filter) hipLaunchKernelGGL((k_match_search<G, true, false, false>), grid, dim3(256), 0, s, p, tps);
    else hipLaunchKernelGGL((k_match_search<G, false, false, false>), grid, dim3(256), 0, s, p, tps);
}

}  // namespace mtr

// The shape of the search grid and the reading of MTR_MATCH_TUNE="share_groups,target" live in match_launch.h, which the host
// test compiles too; the variable overrides both numbers for timing ablations (tools/bench_match.py) and for the tests that
// force a grid shape, and is read once.
void mtr_launch_match(const MatchParams& p, hipStream_t s) {
    if (p.n == 0 || p.R == 0 || p.nclips == 0) return;
    static const MatchTune tune = match_tune_parse(getenv("MTR_MATCH_TUNE"));
    const uint32_t np = (p.n + 31u) & ~31u;
    hipLaunchKernelGGL(mtr::k_match_query, dim3((np + 255u) / 256u), dim3(256), 0, s, p);
    const MatchGrid g = match_grid(p.n, p.R, p.scores != nullptr, tune.share_groups, tune.target);
    const bool share = g.share;
    const uint32_t tps = g.tiles_per_slab;
    const dim3 grid(g.gx, g.gy);
    switch (mtr::match_dp(p.D) / 8u) {
    case 1: mtr::match_search_launch<1>(p, share, grid, tps, s); break;
    case 2: mtr::match_search_launch<2>(p, share, grid, tps, s); break;
    case 3: mtr::match_search_launch<3>(p, share, grid, tps, s); break;
    case 4: mtr::match_search_launch<4>(p, share, grid, tps, s); break;
    case 5: mtr::match_search_launch<5>(p, share, grid, tps, s); break;
    case 6: mtr::match_search_launch<6>(p, share, grid, tps, s); break;
    case 7: mtr::match_search_launch<7>(p, share, grid, tps, s); break;
    default: mtr::match_search_launch<8>(p, share, grid, tps, s); break;
    }
    if (!p.scores) hipLaunchKernelGGL(mtr::k_match_decide, dim3((p.n + 255u) / 256u), dim3(256), 0, s, p);
}
