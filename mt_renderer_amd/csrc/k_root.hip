// k_root.hip -- root motion (SPEC.md section 19).  For every instance: S steps (clip, x, dx, w) on the trajectory joint of an
// animation set of either kind; per step the rigid delta between position x and x + dx, across a cycle seam where the root
// set marks the clip cyclic; the deltas blended in order like section 16's OVERRIDE layers; out = M_in * D (k_root) or D itself
// (k_root_deltas).  Every scalar rule lives in root_math.h, which the host test compiles too; the product is
// attach_math.h's chain.
//
// Lanes.  G = 4 S rounded up to a power of two (4, 8, 16 or 32) lanes form the group of one instance, 256 / G instances per
// workgroup, a group never straddling a wave.  Lane g of a group belongs to step g / 4 (lanes past 4 S repeat the last
// step and their results are never fetched) and takes sample g % 4 of it: position r0, the two seam ends, r1.  A lane loads
// its step's record, then the clip's table entry and root flag, then the keys (or the track probes) of its one sample --
// a chain of three dependent steps (plus the search of a track set), every load of a step issued before the first use of
// any of them; row g % 4 of M_in is loaded at the very start.  Then the four samples of a step are exchanged inside its
// quad and every lane of the quad forms the step's delta; the lanes of the group fetch the deltas of steps 1 .. S - 1 in order
// from those steps' first lanes and blend them, all lanes alike; finally lane g forms the elements g, g + G, ... < 16 of
// M_in * D from its row of M_in and a column of D.  No LDS and no barrier: the cross-lane moves are wave shuffles that
// read inside the lane's own group, executed by all lanes outside any divergent branch.
//
// Memory safety.  nsteps is a host value validated to 1..8 and the step array holds n * nsteps records; the instance index
// is clamped to n - 1 and the step index to nsteps - 1, so inst * nsteps + step lies inside it (lanes of instances past n
// compute instance n - 1 again and store nothing).  From a record come (a) the clip index, clamped to nclips - 1 before it
// reaches the clip table, the root flags or a descriptor, (b) x and dx, which root_positions turns into positions that are
// -0 or lie in [0, N - 1] for every float pattern, and which anim_position / root_sample_tracks clamp once more into
// key indices inside the clip (the argument at track_clip_begin in k_anim.hip holds for the search), and (c) the weight,
// which reaches no address.  joint < njoints is validated on the host.  No device-side value forms an address unclamped.
#include "mtr_internal.h"
#include "root_math.h"

namespace mtr {

// lane `src` of the wave holds the value
__device__ __forceinline__ RootXf root_fetch(const RootXf& v, int src) {
    RootXf r;
    r.t.x = __shfl(v.t.x, src); r.t.y = __shfl(v.t.y, src); r.t.z = __shfl(v.t.z, src);
    r.q.x = __shfl(v.q.x, src); r.q.y = __shfl(v.q.y, src); r.q.z = __shfl(v.q.z, src); r.q.w = __shfl(v.q.w, src);
    return r;
}

// one of four values by a lane-dependent index, as selects between registers (an index into an array of them, or a choice
// between whole float4s, sends the array to scratch memory)
__device__ __forceinline__ float root_pick(float v0, float v1, float v2, float v3, uint32_t i) { return i == 0u ? v0 : i == 1u ? v1 : i == 2u ? v2 : v3; }

template <bool TRACKS, bool APPLY>
__global__ __launch_bounds__(256) void k_root(RootParams p, uint32_t G) {
    const uint32_t S = p.nsteps;
    const uint32_t g = threadIdx.x & (G - 1u), role = g & 3u;
    const uint32_t inst_raw = blockIdx.x * (256u / G) + threadIdx.x / G;
    const uint32_t inst = inst_raw < p.n ? inst_raw : p.n - 1u;
    const uint32_t step = (g >> 2) < S ? (g >> 2) : S - 1u;
    float m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (APPLY) {
        const float* Mp = p.mats_in + (size_t)inst * 16;
#pragma unroll
        for (int k = 0; k < 4; k++) m[k] = Mp[k * 4 + role];  // row `role` of M
    }
    const uint4 rec = reinterpret_cast<const uint4*>(p.steps)[(size_t)inst * S + step];  // clip, x, dx, w
    const uint32_t ci = rec.x < p.anim.nclips ? rec.x : p.anim.nclips - 1u;
    const uint4 ct = reinterpret_cast<const uint4*>(p.anim.clips)[ci];  // first key (uniform), keys or ticks, flags, 0
    const uint32_t rf = p.root_flags[ci];
    const RootPos pos = root_positions(__uint_as_float(rec.y), __uint_as_float(rec.z), ct.y, rf);
    const float r = role == 0u ? pos.r[0] : role == 1u ? pos.r[1] : role == 2u ? pos.r[2] : pos.r[3];
    const uint32_t J = p.anim.pose.njoints;
    RootXf smp;
    if constexpr (TRACKS) smp = root_sample_tracks(p.anim.tracks + ((size_t)ci * J + p.joint) * 24, p.anim.values, p.anim.times, ct.y, r);
    else smp = root_sample_uniform(p.anim.keys, ct.x, ct.y, J, p.joint, r);
    // the step's four samples, to every lane of its quad
    const int lane = (int)(threadIdx.x & 63u), quad = lane & ~3;
    RootXf s4[4];
#pragma unroll
    for (int i = 0; i < 4; i++) s4[i] = root_fetch(smp, quad + i);
    const RootXf d = root_step_delta(s4, pos.kind);
    // the blend: step 0's delta, then the others in order, from the first lane of each step's quad
    const int base = lane & ~(int)(G - 1u);
    RootXf acc = root_fetch(d, base);
    for (uint32_t i = 1; i < S; i++) {
        const RootXf di = root_fetch(d, base + (int)(i * 4u));
        const float w = __shfl(__uint_as_float(rec.w), base + (int)(i * 4u));
        root_blend(acc, di, w);
    }
    AnimVec D[4];
    root_matrix(acc, D);
    if (inst_raw >= p.n) return;
    float* out = p.out + (size_t)inst * 16;
#pragma unroll
    for (uint32_t t = 0; t < 4u; t++) {  // at most four elements per lane (G = 4)
        const uint32_t e = g + t * G;
        if (e >= 16u) break;
        const uint32_t c = e >> 2;
        const float Dc[4] = {root_pick(D[0].x, D[1].x, D[2].x, D[3].x, c), root_pick(D[0].y, D[1].y, D[2].y, D[3].y, c),
                             root_pick(D[0].z, D[1].z, D[2].z, D[3].z, c), root_pick(D[0].w, D[1].w, D[2].w, D[3].w, c)};  // column c
        if constexpr (APPLY) out[e] = attach_elem(m, Dc);
        else out[e] = root_pick(Dc[0], Dc[1], Dc[2], Dc[3], role);
    }
}

}  // namespace mtr

namespace {

template <bool APPLY>
void launch_root(const RootParams& p, hipStream_t s) {
    if (p.n == 0 || p.nsteps == 0 || p.nsteps > MTR_ROOT_MAX_STEPS) return;
    uint32_t G = 4;
    while (G < p.nsteps * 4u) G <<= 1;
    const uint32_t per = 256u / G;
    const dim3 grid((p.n + per - 1u) / per), block(256);
    if (p.anim.tracks) hipLaunchKernelGGL((mtr::k_root<true, APPLY>), grid, block, 0, s, p, G);
    else hipLaunchKernelGGL((mtr::k_root<false, APPLY>), grid, block, 0, s, p, G);
}

}  // namespace

void mtr_launch_root(const RootParams& p, hipStream_t s) { launch_root<true>(p, s); }
void mtr_launch_root_deltas(const RootParams& p, hipStream_t s) { launch_root<false>(p, s); }
