// k_cull.hip -- culling of sharded frames ahead of k_geom: which instances, and which chunks of
// them, may reach a bin of this rank.  The bounds and the tests are geom_cull.h; k_geom consumes the instance list and
// the per-group chunk masks written here.
#include "geom_cull.h"

#include <algorithm>

namespace mtr {

// Instance culling of a sharded batch draw, one wave per instance, lane = per-joint box of the whole model: the
// instances that may reach a bin of this rank are appended to `list` (in no particular order: k_geom takes the instance
// number from the work list, so submission-order keys do not change).
__global__ __launch_bounds__(64) void k_cull_instances(CullParams P) {
    const uint32_t inst = blockIdx.x, lane = threadIdx.x;
    if (inst >= P.ninst) return;
    float M[16];
    compose_vp_model(P.vp, P.model_mats, inst, M);
    const bool have_pal = P.palettes && P.npal;
    const float* pal = have_pal ? P.palettes + (size_t)inst * P.pal_stride : nullptr;
    ClipBox cb;
#pragma unroll
    for (int t = 0; t < 3; t++) { cb.lo[t] = __builtin_inff(); cb.hi[t] = -__builtin_inff(); }
    bool bad = false;
    for (uint32_t i = lane; i < P.nboxes; i += 64) {
        const BoneBox bx = P.boxes[i];
        const float* Pm = nullptr;
        if (bx.joint != MTR_BOX_UNSKINNED && have_pal) Pm = pal + (size_t)min(bx.joint, P.npal - 1u) * 16;
        const ClipBox one = box_clip_interval(bx, Pm, M);
        bad = bad || !clipbox_finite(one);
#pragma unroll
        for (int t = 0; t < 3; t++) { cb.lo[t] = fminf(cb.lo[t], one.lo[t]); cb.hi[t] = fmaxf(cb.hi[t], one.hi[t]); }
    }
    bool keep = true, inside = false;
    if (!__ballot(bad) && P.nboxes) {
        ClipBox u;
#pragma unroll
        for (int t = 0; t < 3; t++) { u.lo[t] = wave_min_f32(cb.lo[t]); u.hi[t] = wave_max_f32(cb.hi[t]); }
        FrameBuffers fb = {};
        fb.W = P.W; fb.H = P.H; fb.nbx = P.nbx; fb.nby = P.nby; fb.own = P.own;
        keep = clipbox_may_touch_rank(u, fb) || P.own.cull == 3u || P.own.cull == 4u;  // 3, 4: timing ablations (MTR_CULL_DEBUG), keep everything
        inside = (keep && (clipbox_all_in_rank(u, fb) || P.own.cull == 5u)) || P.own.cull == 4u;  // 5: no chunk tests for kept instances
    }
    if (!keep) {
        if (lane == 0) atomicAdd(&P.counters[MTR_CTR(CTR_CULL, inst)], P.nchunks);  // statistics only
        return;
    }
    uint32_t slot = 0;
    if (lane == 0) {
        slot = atomicAdd(P.count, 1u);
        P.list[slot] = inst;
        if (!inside) P.strad[atomicAdd(P.count + 1, 1u)] = slot;
    }
    if (inside) {  // every chunk of it is this rank's: no chunk tests (k_cull_chunks skips the slot)
        slot = (uint32_t)__builtin_amdgcn_readfirstlane((int)slot);
        const uint32_t nx = (P.nchunks + 15u) / 16u, tail = P.nchunks & 15u;
        for (uint32_t x = lane; x < nx; x += 64) P.work_mask[(size_t)slot * nx + x] = (uint16_t)((x == nx - 1u && tail) ? (1u << tail) - 1u : 0xFFFFu);
    }
    if (P.comp && !inside) {  // what the chunk tests of this instance read (k_cull_chunks tests the straddlers only)
        CompMat* out = P.comp + (size_t)inst * P.ncomp;
        for (uint32_t j = lane; j < P.ncomp; j += 64) out[j] = make_comp((have_pal && j + 1 < P.ncomp) ? pal + (size_t)j * 16 : nullptr, M);
    }
}

// Chunk culling of a sharded draw.  256 threads = 16 rows of 16 lanes: row = one chunk, lane = one of its boxes; the
// per-joint composites of the instance are built once per workgroup in LDS.  Which of the workgroup's 16 chunks may
// reach a bin of the rank is stored as one 16-bit mask per (instance slot, group of 16 chunks): no list to append to,
// no atomic; k_geom<.., true> launches four workgroups per mask, each taking four of its set bits (one palette in LDS,
// four waves).  A light kernel (no records, no binning state) at full occupancy: the test's chain of dependent loads
// is not paid inside k_geom's 80-register workgroups.
template <bool LDS_COMP>  // true: the workgroup builds its instance's composites in LDS (a single model); false: they come from k_cull_instances
__global__ __launch_bounds__(256, LDS_COMP ? 4 : 8) void k_cull_chunks(ChunkCullParams P) {
    extern __shared__ __align__(16) unsigned char s_raw[];
    CompMat* s_comp = reinterpret_cast<CompMat*>(s_raw);
    __shared__ uint32_t s_wmask[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane >> 4, sub = lane & 15u;
    const uint32_t c = blockIdx.x * 16u + wave * 4u + row;
    const bool has = c < P.nchunks;
    DChunk ch = {};
    if (has) ch = P.chunks[c];
    const bool have_pal = P.palettes && P.npal;
    const uint32_t ncomp = have_pal ? P.npal + 1u : 1u;
    const bool skinned = (ch.b_flags & 2u) && have_pal;
    // chunks that cannot be bounded are kept
    const bool unbounded = has && (ch.b_count == 0 || (skinned && (ch.b_flags & 1u)) || (skinned && ch.b_count < 2) || ch.b_count > MTR_CHUNK_MAX_BOXES + 1u);
    const uint32_t first = skinned ? ch.b_first + 1u : ch.b_first, n = has ? (skinned ? ch.b_count - 1u : 1u) : 0u;
    BoneBox bx = {};
    const bool tests = has && !unbounded && sub < n;
    if (tests) bx = P.boxes[first + sub];
    const uint32_t nlive = P.strad ? P.inst_count[1] : live_instances(P.inst_count, P.ninst);
    for (uint32_t si = blockIdx.y; si < nlive; si += gridDim.y) {
        const uint32_t ii = P.strad ? P.strad[si] : si;  // the instance's slot: where its masks go
        const uint32_t inst = P.inst_list ? P.inst_list[ii] : ii;
        __syncthreads();  // the composites and masks of the previous instance are no longer read
        if (LDS_COMP) {
            float M[16];
            compose_vp_model(P.vp, P.model_mats, inst, M);
            const float* pal = have_pal ? P.palettes + (size_t)inst * P.pal_stride : nullptr;
            for (uint32_t j = threadIdx.x; j < ncomp; j += 256) s_comp[j] = make_comp((have_pal && j + 1 < ncomp) ? pal + (size_t)j * 16 : nullptr, M);
        }
        __syncthreads();
        ClipBox cb;
#pragma unroll
        for (int t = 0; t < 3; t++) { cb.lo[t] = __builtin_inff(); cb.hi[t] = -__builtin_inff(); }
        bool bad = false;
        if (tests) {
            const uint32_t j = skinned ? min(bx.joint, P.npal - 1u) : ncomp - 1u;  // the last composite is M itself
            cb = box_comp_interval(bx, LDS_COMP ? s_comp[j] : P.comp[(size_t)inst * ncomp + j]);
            bad = !clipbox_finite(cb);
        }
        const uint64_t badm = __ballot(bad);
        const bool row_bad = ((badm >> (row * 16u)) & 0xFFFFull) != 0;
        ClipBox u;
#pragma unroll
        for (int t = 0; t < 3; t++) { u.lo[t] = row_min_f32(cb.lo[t]); u.hi[t] = row_max_f32(cb.hi[t]); }
        const bool keep = has && (unbounded || row_bad || P.keep_all || clipbox_may_touch_rank(u, P.fb));
        const uint64_t km = __ballot(keep);
        if (lane == 0)
            s_wmask[wave] = (uint32_t)(km & 1ull) | (uint32_t)((km >> 15) & 2ull) | (uint32_t)((km >> 30) & 4ull) | (uint32_t)((km >> 45) & 8ull);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t m16 = s_wmask[0] | (s_wmask[1] << 4) | (s_wmask[2] << 8) | (s_wmask[3] << 12);
            P.work_mask[(size_t)ii * gridDim.x + blockIdx.x] = (uint16_t)m16;
            const uint32_t k = (uint32_t)__popc(m16);
            const uint32_t nhave = blockIdx.x * 16u < P.nchunks ? min(16u, P.nchunks - blockIdx.x * 16u) : 0u;
            if (nhave > k) atomicAdd(&P.fb.counters[MTR_CTR(CTR_CULL, blockIdx.x + inst)], nhave - k);  // statistics only
        }
    }
}

}  // namespace mtr

void mtr_launch_cull_instances(const CullParams& p, hipStream_t s) {
    if (p.ninst == 0) return;
    hipLaunchKernelGGL(mtr::k_cull_instances, dim3(p.ninst), dim3(64), 0, s, p);
}

void mtr_launch_cull_chunks(const ChunkCullParams& p, hipStream_t s) {
    if (p.nchunks == 0 || p.ninst == 0) return;
    // instance slots: the kernel strides over the (possibly compacted) instance list; twice the rank's fair share
    uint32_t ny = p.ninst;
    if (p.inst_count && p.fb.own.world > 1) ny = std::max<uint32_t>(1u, std::min<uint32_t>(p.ninst, (2u * p.ninst + p.fb.own.world - 1) / p.fb.own.world));
    // the straddlers a recent frame of the batch reported (the kernel strides over the list: any ny is correct)
    if (p.strad && (p.strad_hint & 0x80000000u)) ny = std::max<uint32_t>(1u, std::min<uint32_t>(p.ninst, (p.strad_hint & 0x7FFFFFFFu) + (p.strad_hint & 0x7FFFFFFFu) / 8u + 2u));
    ny = std::min<uint32_t>(ny, 65535u);
    const uint32_t ncomp = (p.palettes && p.npal) ? p.npal + 1u : 1u;
    if (p.comp) hipLaunchKernelGGL(mtr::k_cull_chunks<false>, dim3((p.nchunks + 15) / 16, ny), dim3(256), 0, s, p);
    else hipLaunchKernelGGL(mtr::k_cull_chunks<true>, dim3((p.nchunks + 15) / 16, ny), dim3(256), (size_t)ncomp * sizeof(CompMat), s, p);
}
