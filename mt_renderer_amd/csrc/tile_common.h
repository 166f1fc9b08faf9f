// tile_common.h -- fragment-stage helpers shared by the ordered (k_tile.hip) and visibility
// (k_tile_vis.hip) tile kernels.  Every formula is SPEC.md section 7, bit for bit.
#pragma once
#include <cstdint>

// ---- divisions by multiply-high: plain C++, so that tests/cpp/bin_magic_exact.cpp compiles this part for the host and
//      holds it to `/` and `%` over every value the kernels can meet (tests/test_bin_magic_exact.py) ----
#if defined(__HIP_DEVICE_COMPILE__)
#define MTR_UMULHI(a, b) __umulhi((a), (b))
#else
#define MTR_UMULHI(a, b) ((uint32_t)(((uint64_t)(uint32_t)(a) * (uint64_t)(uint32_t)(b)) >> 32))
#endif
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MTR_DIV_HD __host__ __device__ __forceinline__
#else
#define MTR_DIV_HD inline
#endif

namespace mtr {

// n / d for a divisor fixed per launch (the scalar unit has no divide; on a uniform n this is s_lshl + s_mul_hi_u32 +
// s_lshr).  With s = floor(log2 d) and mul = ceil(2^(31 + s) / d) <= 2^31:  2n * mul / 2^(32 + s) = n / d + n * e / (d *
// 2^(31 + s)), e = mul * d - 2^(31 + s) < d, and the excess stays below 1 / d -- the floor is exact -- while n * e <
// 2^(31 + s), which n < 2^30 guarantees (e < d < 2^(s + 1)).  EXACT FOR EVERY d >= 1 AND EVERY n < 2^30: a bin index is
// below 2^20 (frames are at most 16384 x 16384: nbx, nby <= 1024) and blockIdx.x >> 3 below 2^18 (at most 2^17 bins per
// XCD, rounded up to whole runs of at most 65536).  d == 0 (no runs: the divisor is not used) gives {0, 0}.
struct UDiv {
    uint32_t mul, shift;
};
MTR_DIV_HD UDiv udiv_make(uint32_t d) {
    UDiv r = {0u, 0u};
    if (d == 0u) return r;
    while ((d >> r.shift) > 1u) r.shift++;
    r.mul = (uint32_t)((((uint64_t)1 << (31u + r.shift)) + d - 1u) / d);
    return r;
}
MTR_DIV_HD uint32_t udiv_apply(uint32_t n, uint32_t mul, uint32_t shift) { return MTR_UMULHI(n << 1, mul) >> shift; }

// the pair walks' item -> bbox row:  k / iw = k * row_magic(iw) >> 16, exact for k < 256 and iw = 1 .. 16 (items per bbox
// row), with magic = ceil(65536 / iw):  k * magic / 65536 = k / iw + k * e / (iw * 65536), e = magic * iw - 65536 < iw, and
// the excess stays below 1 / iw because k * e < 256 * 16 < 65536.  A lane-varying u32 division (28 VALU, three of them
// quarter-rate), so the kernels compute it only for the triangles whose walk reads it
MTR_DIV_HD uint32_t row_magic(uint32_t iw) { return (65536u + iw - 1u) / iw; }

}  // namespace mtr

#if defined(__HIPCC__)  // everything below is device code
#include "bc_sample.h"
#include "mtr_internal.h"
#include "span_row.h"

namespace mtr {

// The head of the parameters (mtr_internal.h: TileHead) in scalar registers.  Naming every field in one empty asm makes the
// compiler fetch them together at the top of the kernel -- wide scalar loads, one wait -- where it would otherwise fetch each
// argument alone in the block that first uses it and wait for it at once: some sixteen dependent round trips in front of a
// wave's first queue load, and most of the life of the waves of an empty bin.  The kernels read these copies, not P.fb, up
// to the end of their raster loops; what k_tile_vis reads after its loop it fetches there (tile_late).
__device__ __forceinline__ TileHead tile_head(const TileParams& P) {
    const TileHead h = P.head;
    asm volatile("" ::"s"(h.grid), "s"(h.own_count), "s"(h.nbx), "s"(h.nbins), "s"(h.W), "s"(h.H), "s"(h.direct), "s"(h.qcap), "s"(h.scap),
                 "s"(h.xcd_run), "s"(h.nbx_mul), "s"(h.nbx_shift), "s"(h.run_mul), "s"(h.run_shift), "s"(h.zero_nwords), "s"(h.nhint),
                 "s"(h.own_list), "s"(h.entries), "s"(h.bin_fill), "s"(h.bin_start), "s"(h.seg_start), "s"(h.counters), "s"(h.rec_a),
                 "s"(h.zero_next), "s"(h.zero_words), "s"(h.host_status));
    return h;
}

// every workgroup of a tile kernel clears its slice of the counter blocks the next frame on these framebuffers will use.
// BLOCK: threads per workgroup (the kernel's template knows it; blockDim.x is a vector load from the implicit arguments).
// A workgroup first tests, on the scalar unit, whether it owns a word at all: of the headline's 8 160 only the first 33 do.
// The grid-stride loops stay: a launch with fewer threads than words (a rank that owns one bin) still clears them all.
template <uint32_t BLOCK>
__device__ __forceinline__ void zero_next_counters(const TileParams& P, const TileHead& h) {
    const uint32_t b0 = blockIdx.x * BLOCK, step = h.grid * BLOCK;  // < 2^30: at most 2^20 + 2^19 workgroups of 512
    if (h.zero_words && b0 < h.zero_nwords) {
        const auto pack4 = [](const uint16_t (&a)[4]) { return (uint64_t)a[0] | (uint64_t)a[1] << 16 | (uint64_t)a[2] << 32 | (uint64_t)a[3] << 48; };
        const uint64_t hint_words = pack4(P.hint_word), hint_slots = pack4(P.hint_slot);
        for (uint32_t i = b0 + threadIdx.x; i < h.zero_nwords; i += step) {
            for (uint32_t k = 0; k < h.nhint; k++) {  // the thread that clears a word the host wants to see publishes it first
                // (the 16-bit arguments picked out of their words on the scalar unit: indexed by k they are vector loads)
                const uint32_t hw = (uint32_t)(hint_words >> (16u * k)) & 0xffffu, hs = (uint32_t)(hint_slots >> (16u * k)) & 0xffffu;
                if (i - hw < 2u)
                    __hip_atomic_store(&P.hint_out[2u * hs + (i - hw)], 0x80000000u | h.zero_words[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
            h.zero_words[i] = 0u;
        }
    }
    if (h.zero_next && b0 < (uint32_t)CTR_NUM)
        for (uint32_t i = b0 + threadIdx.x; i < (uint32_t)CTR_NUM; i += step) h.zero_next[i] = 0u;
}

// What k_tile_vis reads after its raster loop, fetched once more where the loop ends.  An argument read through P is a load the
// compiler may hoist to the top of the kernel (the segment is known to be readable), and what the resolve reads -- the material
// table, the colour and depth planes, rec_b, ... -- then sits in scalar registers across the whole raster loop, next to the
// head: the allocator ran out and spilled to vector lanes, which cost the kernel a wave per SIMD.  Through a pointer whose
// origin the compiler does not see they are fetched where this is called -- together, with one wait, like the head: left to
// the blocks that use them they were eight round trips one after another.  (The tile kernels take one argument: it starts the
// kernel-argument segment.)
struct TileLate {
    const DMat* mats;
    uint8_t* color;
    float* depth;
    uint8_t* bin_flag;
    RecP* rec_a;
    int4* rec_l;
    RecB* rec_b;
    unsigned long long* bin_count;
    unsigned long long* bin_fill;
    uint32_t* counters;
    uint32_t W, clear_rgba8, mixed, direct;
};
__device__ __forceinline__ TileLate tile_late() {
    typedef const TileParams __attribute__((address_space(4)))* TileArgs;
    TileArgs q = (TileArgs)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(q));
    const TileLate t = {q->mats,         q->color,        q->depth,       q->bin_flag, q->fb.rec_a,    q->fb.rec_l, q->fb.rec_b,
                        q->fb.bin_count, q->fb.bin_fill,  q->fb.counters, q->fb.W,     q->clear_rgba8, q->mixed,    q->fb.direct};
    asm volatile("" ::"s"(t.mats), "s"(t.color), "s"(t.depth), "s"(t.bin_flag), "s"(t.rec_a), "s"(t.rec_l), "s"(t.rec_b), "s"(t.bin_count),
                 "s"(t.bin_fill), "s"(t.counters), "s"(t.W), "s"(t.clear_rgba8), "s"(t.mixed), "s"(t.direct));
    return t;
}
// bin_queue_done (mtr_internal.h) on them
__device__ __forceinline__ void bin_queue_done(const TileLate& t, uint32_t bin) {
    if (t.direct) {
        t.bin_count[bin] = t.bin_fill[bin];
        t.bin_fill[bin] = 0ull;
    }
}

// one record, decoded (the rare long-edged triangle costs a second, dependent load)
__device__ __forceinline__ RecA load_rec(const RecP* rec_a, const int4* rec_l, uint32_t r) {
    const RecP p = rec_a[r];
    int4 l = make_int4(0, 0, 0, 0);
    if ((p.q0.z & 0xFFFFu) == MTR_REC_LARGE_SENTINEL) l = rec_l[r];
    return rec_unpack(p, l);
}

// byte / 255, bit-identical to the IEEE division SPEC.md spells, in three instructions instead of the ten of the
// correctly rounded divide expansion: q0 = x * r, e = fma(-q0, 255, x), q = fma(e, r, q0), r = RN(1 / 255).  Verified
// for all 256 bytes with exact rational arithmetic (tests/test_div_exact.py; the bare product x * r is wrong for 126
// of them).  Texel decode and blending do 4-19 of these per fragment: C5 translucent 2.75 -> 2.40 ms.  (The same
// sequence for the SNORM16 / UNORM8 vertex decode made k_geom SLOWER, 37.8 -> 41.9 us, and is not used there.)
__device__ __forceinline__ float unorm8f(uint32_t v) {
    const float x = (float)(v & 0xffu), r = __uint_as_float(0x3b808081u);
    const float q0 = x * r;
    return fmaf(fmaf(-q0, 255.0f, x), r, q0);
}
__device__ __forceinline__ uint32_t quant8(float x) {
    if (!(x > 0.0f)) x = 0.0f;
    if (x > 1.0f) x = 1.0f;
    return (uint32_t)rintf(x * 255.0f);
}
__device__ __forceinline__ int32_t clamp_texel(float f, uint32_t n) {
    if (!(f >= 0.0f)) f = 0.0f;
    if (f > (float)(n - 1)) f = (float)(n - 1);
    return (int32_t)f;
}
struct TexRef {
    const uint8_t* tex;
    uint32_t tw, th;
    uint32_t levels;  // DMat::tlevels: mip levels present (the reference uploads one, src/texture.rs:21; more: row f-4)
                      // in the low byte, MTR_TR_* (what `tex` holds) above it
};
// one texel of mip level `level` (lw x lh) as RGBA8: from the image decoded at upload, or from the BC block it lives in
__device__ __forceinline__ uint32_t texel_u32(const TexRef& m, int level, uint32_t lw, int32_t x, int32_t y) {
    const uint32_t res = m.levels >> 8;
    uint32_t w = m.tw, h = m.th;
    size_t off = 0;
    if (res == MTR_TR_RGBA8) {
        for (int l = 0; l < level; l++) { off += (size_t)w * h; w = w > 1u ? w >> 1 : 1u; h = h > 1u ? h >> 1 : 1u; }
        return reinterpret_cast<const uint32_t*>(m.tex)[off + (size_t)y * lw + (size_t)x];
    }
    for (int l = 0; l < level; l++) { off += (size_t)((w + 3u) >> 2) * ((h + 3u) >> 2); w = w > 1u ? w >> 1 : 1u; h = h > 1u ? h >> 1 : 1u; }
    const size_t b = off + (size_t)((uint32_t)y >> 2) * ((lw + 3u) >> 2) + ((uint32_t)x >> 2);
    const uint32_t i = ((uint32_t)y & 3u) * 4u + ((uint32_t)x & 3u);
    if (res == MTR_TR_BC1) return bc1_texel(reinterpret_cast<const uint2*>(m.tex)[b], i);
    return bc7_texel(reinterpret_cast<const ulonglong2*>(m.tex)[b], i);
}
__device__ __forceinline__ void texel_f(const TexRef& m, int32_t x, int32_t y, float (&o)[4]) {
    const uint32_t t = texel_u32(m, 0, m.tw, x, y);
    o[0] = unorm8f(t); o[1] = unorm8f(t >> 8); o[2] = unorm8f(t >> 16); o[3] = unorm8f(t >> 24);
}

// textureSample: clamp-to-edge, mag linear / min nearest (src/texture.rs:33-42).  flt < 0: linear on level 0
// (magnification); flt >= 0: the nearest texel of mip level flt (level 0 always when the texture has one level).
__device__ __forceinline__ void sample_texture(const TexRef& m, float u, float v, int flt, float (&o)[4]) {
    const float fw = (float)m.tw, fh = (float)m.th;
    if (flt >= 0) {
        uint32_t lw = m.tw, lh = m.th;
        for (int l = 0; l < flt; l++) { lw = lw > 1u ? lw >> 1 : 1u; lh = lh > 1u ? lh >> 1 : 1u; }
        const int32_t x = clamp_texel(floorf(u * (float)lw), lw), y = clamp_texel(floorf(v * (float)lh), lh);
        const uint32_t t = texel_u32(m, flt, lw, x, y);
        o[0] = unorm8f(t); o[1] = unorm8f(t >> 8); o[2] = unorm8f(t >> 16); o[3] = unorm8f(t >> 24);
        return;
    }
    float x = u * fw - 0.5f, y = v * fh - 0.5f;
    float x0 = floorf(x), y0 = floorf(y);
    float fx = x - x0, fy = y - y0;
    int32_t ix0 = clamp_texel(x0, m.tw), ix1 = clamp_texel(x0 + 1.0f, m.tw);
    int32_t iy0 = clamp_texel(y0, m.th), iy1 = clamp_texel(y0 + 1.0f, m.th);
    float c00[4], c10[4], c01[4], c11[4];
    texel_f(m, ix0, iy0, c00); texel_f(m, ix1, iy0, c10); texel_f(m, ix0, iy1, c01); texel_f(m, ix1, iy1, c11);
#pragma unroll
    for (int c = 0; c < 4; c++) {
        float top = fmaf(fx, c10[c] - c00[c], c00[c]);
        float bot = fmaf(fx, c11[c] - c01[c], c01[c]);
        o[c] = fmaf(fy, bot - top, top);
    }
}

// SPEC.md section 7: -1 = linear (every derivative product <= 1: magnification), else the mip level of a nearest
// sample: level l while m > 2^(l - 1/2), i.e. m * m > 2^(2l - 1), m = the largest product (NaN: level 0)
__device__ __forceinline__ int filter_select(float dudx, float dvdx, float dudy, float dvdy, uint32_t tw, uint32_t th, uint32_t levels) {
    levels &= 0xffu;  // DMat::tlevels carries MTR_TR_* above the count
    const float fw = (float)tw, fh = (float)th;
    const float a = fabsf(dudx) * fw, b = fabsf(dvdx) * fh, c = fabsf(dudy) * fw, d = fabsf(dvdy) * fh;
    if ((a <= 1.0f) && (b <= 1.0f) && (c <= 1.0f) && (d <= 1.0f)) return -1;
    int level = 0;
    if (levels > 1u) {
        const float m = fmaxf(fmaxf(a, b), fmaxf(c, d));
        const float m2 = m * m;
        float thr = 2.0f;
        while ((uint32_t)level + 1u < levels && m2 > thr) { level++; thr *= 4.0f; }
    }
    return level;
}

// blend 1: SrcAlpha / OneMinusSrcAlpha colour, One / Zero alpha (src/model.rs:243-246); 2: additive, SrcAlpha / One
// (material state, SPEC.md section 10); 0: replace.  UNORM8 store.
__device__ __forceinline__ uint32_t blend_store(uint32_t dst, const float (&src)[4], uint32_t blend) {
    uint32_t out = 0;
    if (blend == 2u) {
        const float a = src[3];
#pragma unroll
        for (int c = 0; c < 3; c++) out |= quant8(fmaf(src[c], a, unorm8f(dst >> (8 * c)))) << (8 * c);
        out |= quant8(src[3]) << 24;
    } else if (blend) {
        const float a = src[3], ia = 1.0f - a;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            float d = unorm8f(dst >> (8 * c));
            float t = d * ia;
            out |= quant8(fmaf(src[c], a, t)) << (8 * c);
        }
        out |= quant8(src[3]) << 24;
    } else {
#pragma unroll
        for (int c = 0; c < 4; c++) out |= quant8(src[c]) << (8 * c);
    }
    return out;
}

// LDS traffic between lanes of ONE wave: ds operations of a wave complete in order; this only stops
// the compiler from moving accesses across the hand-off point.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the flattened walk: work items (pairs, rows) of up to 64 triangles spread over the wave 64 at a time.  The item ->
//      triangle map needs no search: triangle t sets bit (prefix_t mod 64) of a 64-bit start mask per batch of 64 items
//      (one ds_or_b64), and item p's triangle is  #starts before its batch + popcount(mask bits <= p) - 1  (v_mbcnt), an
//      index into the triangles that have items, in lane order. ----
// a lane with `mine` items after `pre` items of lower lanes marks its start in s_start[nmask].  The caller stages its
// triangle records next and then calls wave_lds_sync()
__device__ __forceinline__ void flat_stage_starts(unsigned long long* s_start, uint32_t nmask, uint32_t lane, uint32_t mine, uint32_t pre) {
    if (lane < nmask) s_start[lane] = 0ull;
    wave_lds_sync();
    if (mine) atomicOr(&s_start[pre >> 6], 1ull << (pre & 63u));
}
// body(item, compacted triangle index) for every item below total, lane = item of the batch
template <typename F>
__device__ __forceinline__ void flat_for_each(const unsigned long long* s_start, uint32_t nmask, uint32_t lane, uint32_t total, F&& body) {
    const unsigned long long my_start = lane < nmask ? s_start[lane] : 0ull;
    const uint32_t nb = (total + 63u) >> 6;
    uint32_t base = 0;
    for (uint32_t b = 0; b < nb; b++) {
        const uint32_t mlo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)my_start, b);
        const uint32_t mhi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(my_start >> 32), b);
        const uint64_t m = ((uint64_t)mhi << 32) | mlo;
        // triangles started before this batch + starts at or below this lane - 1
        const uint32_t tri = base + __builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u)) + (uint32_t)((m >> lane) & 1ull) - 1u;
        base += (uint32_t)__popcll(m);
        const uint32_t p = b * 64u + lane;
        if (p < total) body(p, tri);
    }
}
// this lane's rank among the lanes of a ballot: its compacted triangle index
__device__ __forceinline__ uint32_t lane_rank(uint64_t m) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u)); }

// ---- perspective-correct texcoords from barycentrics, and their quad derivatives from the plane equations ----
struct UVPlanes { float iw0, diw1, diw2, up0, dup1, dup2, vp0, dvp1, dvp2; };
__device__ __forceinline__ UVPlanes uv_planes(const RecB& b) {
    return {b.iw0, b.iw1 - b.iw0, b.iw2 - b.iw0, b.up0, b.up1 - b.up0, b.up2 - b.up0, b.vp0, b.vp1 - b.vp0, b.vp2 - b.vp0};
}
__device__ __forceinline__ void uv_at_bary(const UVPlanes& p, float b1, float b2, float& u, float& v) {
    const float iw = fmaf(b2, p.diw2, fmaf(b1, p.diw1, p.iw0));
    const float up = fmaf(b2, p.dup2, fmaf(b1, p.dup1, p.up0));
    const float vp = fmaf(b2, p.dvp2, fmaf(b1, p.dvp1, p.vp0));
    u = up / iw;
    v = vp / iw;
}
struct QuadUV { float u, v, dudx, dvdx, dudy, dvdy; };
// fine quad differences at pixel (x, y): (odd position) - (even position) along each axis; the pixel is one end of both,
// so two more evaluations give all four derivatives.  bary(x, y, b1, b2): the triangle's barycentrics at a pixel
template <typename B>
__device__ __forceinline__ QuadUV quad_uv(const UVPlanes& p, int32_t x, int32_t y, B&& bary) {
    auto uv_at = [&](int32_t qx, int32_t qy, float& u, float& v) {
        float b1, b2;
        bary(qx, qy, b1, b2);
        uv_at_bary(p, b1, b2, u, v);
    };
    float u, v, uh, vh, uw, vw;
    uv_at(x, y, u, v);
    uv_at(x ^ 1, y, uh, vh);
    uv_at(x, y ^ 1, uw, vw);
    return {u, v, (x & 1) ? u - uh : uh - u, (x & 1) ? v - vh : vh - v, (y & 1) ? u - uw : uw - u, (y & 1) ? v - vw : vw - v};
}

// XCD-aware bin order: blocks b, b+8, ... share an XCD's L2: give each XCD a contiguous run of this rank's bins
// (own_list is row-major for interleaved / band ownership and super-tile-major for super-tiles).
// Returns false when this block has no bin.  The divisions by the run length and (bin_xy) by the bins per row are
// multiply-highs by the launcher's multipliers (tile_fill_head): every value here is uniform over the workgroup, and
// a scalar division is a float-reciprocal sequence of some 25 instructions that every wave of every bin would pay.
__device__ __forceinline__ bool block_to_bin(const TileHead& h, uint32_t& bin) {
    const uint32_t run = h.xcd_run;
    const uint32_t per = (h.grid + 7) / 8;
    const uint32_t x = blockIdx.x & 7, i = blockIdx.x >> 3;
    // run == 0: XCD x takes one contiguous eighth of the bins; run > 0: runs of `run` consecutive bins are dealt to the
    // XCDs in turn (the launch covers whole runs), so every XCD sees every region of the frame
    uint32_t slot = x * per + i;
    if (run) {
        const uint32_t q = udiv_apply(i, h.run_mul, h.run_shift);  // i / run
        slot = (q * 8 + x) * run + (i - q * run);
    }
    bin = 0;
    if (slot >= h.own_count) return false;
    bin = h.own_list ? h.own_list[slot] : slot;
    return bin < h.nbins;
}
// bin -> its column and row in the grid of bins
__device__ __forceinline__ void bin_xy(const TileHead& h, uint32_t bin, uint32_t& bx, uint32_t& by) {
    by = udiv_apply(bin, h.nbx_mul, h.nbx_shift);  // bin / nbx
    bx = bin - by * h.nbx;
}

// Start of every tile workgroup, shared by both kernels.  Fetches the head, finds the workgroup's bin and issues everything
// the bin's first pass waits for back to back -- the frame's overflow flags, the bin's fill word (or its two-pass bounds)
// and, SPEC, this wave's first two entry loads (direct mode: bin b's queue starts at b * qcap whatever its fill, so they
// need not wait for the fill word) -- then does the workgroup's bookkeeping, the counter clearing and the host's status
// word, while those loads are in flight.
//   ovf      the frame's overflow flags (final: the kernels that raise them precede this one on the stream), also published
//            to the host's status word.  A frame with a flag set has incomplete queues -- slots that were reserved and never
//            written -- so the tile kernels must not read them: they clear their bin, park the fill word and leave; the
//            host re-runs the frame (mtr_frame_wait, the exchange thread) or latches an error.
//   spec0/1  entries [first + lane] and [first + BLOCK + lane] of the bin's queue where they are below qcap (direct mode),
//            valid where they are below n_ent
// Returns false when the workgroup has no bin (uniform over the workgroup; no barrier has been met).
struct TileEntry {
    TileHead h;
    uint32_t ovf, bin, bin_x, bin_y;
    uint32_t ent_lo, n_ent, seg_lo, n_seg;
    uint32_t spec0, spec1;
};
template <uint32_t BLOCK, bool SPEC>
__device__ __forceinline__ bool tile_enter(const TileParams& P, uint32_t first, uint32_t lane, TileEntry& e) {
    e.h = tile_head(P);
    const TileHead& h = e.h;
    const bool has_bin = block_to_bin(h, e.bin);
    const uint32_t bin = e.bin;
    const uint32_t ovf_v = h.counters[CTR_OVERFLOW];
    unsigned long long fill = 0ull;
    uint32_t e0 = 0, e1 = 0, s0 = 0, s1 = 0;
    e.spec0 = e.spec1 = 0u;
    if (has_bin) {
        if (h.direct) {
            // every lane of the bin's workgroup reads the same word; the caller cleans it afterwards (bin_queue_done)
            fill = h.bin_fill[bin];
            if (SPEC) {
                const uint32_t qb = bin * h.qcap;
                if (first + lane < h.qcap) e.spec0 = h.entries[qb + first + lane];
                if (first + BLOCK + lane < h.qcap) e.spec1 = h.entries[qb + first + BLOCK + lane];
            }
        } else {
            e0 = h.bin_start[bin]; e1 = h.bin_start[bin + 1];
            s0 = h.seg_start[bin]; s1 = h.seg_start[bin + 1];
        }
    }
    zero_next_counters<BLOCK>(P, h);
    if (blockIdx.x == 0 && threadIdx.x == 0 && h.host_status)
        __hip_atomic_store(h.host_status, 0x80000000u | ovf_v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (!has_bin) return false;
    bin_xy(h, bin, e.bin_x, e.bin_y);
    // every lane has loaded the same words: the bounds go on in scalar registers
    const auto uni = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); };
    e.ovf = uni(ovf_v);
    if (h.direct) {
        e.ent_lo = bin * h.qcap; e.seg_lo = bin * h.scap;
        e.n_ent = min(uni((uint32_t)fill), h.qcap); e.n_seg = min(uni((uint32_t)(fill >> 32)), h.scap);
    } else {
        e.ent_lo = uni(e0); e.n_ent = uni(e1) - e.ent_lo;
        e.seg_lo = uni(s0); e.n_seg = uni(s1) - e.seg_lo;
    }
    return true;
}

}  // namespace mtr

#endif  // __HIPCC__

#if defined(MTR_TILE_PARAMS)  // mtr_internal.h has been included: always above, and by the host test in front of this header
// What both launchers do to their copy of the parameters: the workgroups of the launch, the multipliers of the two
// launch-invariant divisors, and a copy of everything else the kernels' entry path reads.  Plain C++
// (tests/cpp/tile_head_fill.cpp holds every field to its source).
inline void tile_fill_head(TileParams& p) {
    TileHead& h = p.head;
    const uint32_t mine = p.fb.own.own_count;
    h.grid = (mine + 7) / 8 * 8;
    if (p.xcd_run) h.grid = (h.grid / 8 + p.xcd_run - 1) / p.xcd_run * p.xcd_run * 8;  // whole runs
    h.own_count = mine; h.own_list = p.fb.own.own_list;
    h.nbx = p.fb.nbx; h.nbins = p.fb.nbx * p.fb.nby;
    h.W = p.fb.W; h.H = p.fb.H;
    h.direct = p.fb.direct; h.qcap = p.fb.qcap; h.scap = p.fb.scap;
    h.xcd_run = p.xcd_run;
    const mtr::UDiv n = mtr::udiv_make(p.fb.nbx), r = mtr::udiv_make(p.xcd_run);
    h.nbx_mul = n.mul; h.nbx_shift = n.shift;
    h.run_mul = r.mul; h.run_shift = r.shift;
    h.zero_nwords = p.zero_nwords; h.nhint = p.nhint;
    h.entries = p.fb.entries; h.bin_fill = p.fb.bin_fill; h.bin_start = p.fb.bin_start; h.seg_start = p.fb.seg_start;
    h.counters = p.fb.counters; h.rec_a = p.fb.rec_a;
    h.zero_next = p.zero_next; h.zero_words = p.zero_words; h.host_status = p.host_status;
}
#endif
