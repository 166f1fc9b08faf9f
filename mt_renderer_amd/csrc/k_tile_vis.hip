// k_tile_vis.hip -- visibility-key tile kernel for frames whose every material is opaque
// (debug-id / overlay colours, or textures with alpha == 255 everywhere: blend = replace).
//
// For such frames the per-pixel result of the ordered pipeline (depth LessEqual + write, blend with
// a = 1) is a pure reduction: the winner of a pixel is the fragment with the smallest z, the LATEST
// in submission order among equals.  So each pixel keeps one 64-bit key  (~bits(z) : order+1)  in
// LDS and every fragment is an order-independent, fire-and-forget `ds_max_u64`:
//   * 64 triangles are set up per pass, one per lane;
//   * a pass whose boxes are mostly larger than four pixels flattens (triangle, bbox row) items instead, and each row walks
//     only the run of columns its triangle covers (span_row.h; see the walk below);
//   * otherwise the (triangle, pixel-of-bbox) pairs of every i32-edge-class triangle are FLATTENED over the wave, in rounds of
//     <= 4096 pairs: a pass costs sum(bbox pixels)/64 iterations whatever the mix of 1-pixel slivers and bin-filling
//     triangles (a lane = triangle walk ran max(bbox pixels) iterations at 29 % lane efficiency on the headline scene).
//     The pair -> triangle map needs no search (start masks, tile_common.h).  Triangles over 64 px across (64-bit edge
//     functions) are rasterised by the whole wave, one at a time (v_readlane);
//   * shading is deferred: the winner's record is addressable from its order (chunk runs live at
//     chunk * MTR_CHUNK_SLOTS), so the resolve does one colour lookup -- or one texture sample with the
//     quad derivatives evaluated from the winner's plane equations exactly as SPEC.md section 7
//     defines them -- per pixel, then the only framebuffer write of the frame.
// Same arithmetic per fragment as k_tile.hip, bit for bit: the set-up, the edge evaluation and the absolute-coordinate
// barycentrics are tri_setup.h's functions in both kernels, the flattened walk tile_common.h's; the host picks this kernel only when the
// frame is eligible (host_submit.cpp); tests run both kernels on the same scenes.
// VIS_WAVES waves per 16x16 bin (passes dealt round-robin, two workgroup barriers in total), no segment
// sort (the submission order rides in the entry).
//
// STAIR (frames with translucent materials, round 3): alpha blending in the default depth state (test LessEqual + write)
// depends on submission order only through the fragments that PASS the depth test, and those are exactly the prefix
// minima of z in submission order: fragment f passes iff z_f <= z_e for every earlier fragment e of the pixel (a
// fragment that fails leaves the depth buffer alone, so the depth f meets is the minimum over all its predecessors).
// The set is order-independent to build: next to the max key each pixel keeps a short list of submission orders; a
// fragment is appended unless the key it meets proves it dominated (an EARLIER fragment that is STRICTLY nearer -- with
// entries arriving roughly in order that leaves little more than the prefix minima themselves).  The resolve walks a
// pixel's list in increasing order, recomputes z from the record, keeps the running minimum, and shades + blends the
// fragments that pass -- the ordered kernel's arithmetic, without its segment sort, ordered passes and per-pass set-up
// (C5 with translucent textures: tile stage 675 -> see DESIGN.md).  A bin with a HARD order-dependent triangle (additive
// blend, depth write or test off) or a pixel whose list overflows is flagged and left to the ordered kernel.
#include "tile_common.h"

namespace mtr {

// LDS triangle record of one pass (64 B): everything a (triangle, pixel) work item needs
struct VisTri {
    int32_t A0, B0, C0, A1;  // edge i: E_i = C_i + A_i*x + B_i*y, top-left bias folded into C_i
    int32_t B1, C1, A2, B2;  // small class: i32, A/B pre-scaled by 256, (x, y) from the bbox origin; large class: unscaled, from the bin's first pixel, C high words in chi
    int32_t C2;
    uint32_t flags;          // bit0 large, bits 4..6: 1 - tl_i
    float z0, dz1;
    float dz2, rcpA;
    uint32_t ordk;           // submission order + 1
    uint32_t box;            // px0 | py0 << 4 | (bw-1) << 8 [| row_magic(iw) << 12 where the walk reads it; iw: items per bbox row]
};
static_assert(sizeof(VisTri) == 64, "VisTri is 64 B");

struct Setup {
    VisTri t;
    int4 chi;
    int32_t npx;   // pixels of the triangle's bbox in this bin
    uint32_t bhm1; // bbox height - 1
};

// the shared set-up (tri_setup.h) plus this kernel's own: the bbox clipped to the bin and the viewport, and the order.
// A triangle whose bbox misses the bin gets npx == 0: its coefficients (meaningless, tri_setup.h) are never read.
// An i32-class triangle's C_i are taken at the bbox origin (box bits 0..7), where the flat walks evaluate them; a
// large-class one's at the bin's first pixel, for the whole-wave walk (tri_setup_box)
__device__ __forceinline__ void setup_tri(const RecA& a, uint32_t ord, int32_t binx0, int32_t biny0, int32_t vw, int32_t vh, Setup& s) {
    const int32_t X[3] = {a.X0, a.X1, a.X2}, Y[3] = {a.Y0, a.Y1, a.Y2};
    TriSetup g;
    tri_setup_box(X, Y, a.z0, a.z1, a.z2, binx0, biny0, g);
    const int32_t px0 = max(g.px0, 0), px1 = min(g.px1, min(MTR_BIN, vw) - 1);
    const int32_t py0 = max(g.py0, 0), py1 = min(g.py1, min(MTR_BIN, vh) - 1);
    const int32_t bw = px1 - px0 + 1, bh = py1 - py0 + 1;
    s.npx = (bw > 0 && bh > 0) ? MTR_MAD24(bw, bh, 0) : 0;  // pixels of the bbox in this bin (both <= 16: no full-width multiply); the caller turns it into work items
    s.bhm1 = (uint32_t)max(bh - 1, 0);
    s.t.A0 = g.A[0]; s.t.B0 = g.B[0]; s.t.C0 = g.Clo[0];
    s.t.A1 = g.A[1]; s.t.B1 = g.B[1]; s.t.C1 = g.Clo[1];
    s.t.A2 = g.A[2]; s.t.B2 = g.B[2]; s.t.C2 = g.Clo[2];
    s.t.flags = g.flags;
    s.t.z0 = g.z0; s.t.dz1 = g.dz1; s.t.dz2 = g.dz2; s.t.rcpA = g.rcpA;
    s.t.ordk = ord + 1u;
    s.t.box = (uint32_t)(px0 & 15) | ((uint32_t)(py0 & 15) << 4) | ((uint32_t)((bw - 1) & 15) << 8);  // + magic << 12 (walk_items)
    s.chi = make_int4(g.Chi[0], g.Chi[1], g.Chi[2], 0);
}

// a triangle of the flattened walks in s_flat: its record, whose edge functions setup_tri took at the bbox origin (an item
// evaluates E(col, row) with no bin coordinates), `pre` in place of flags, whose bits 5 / 6 (1 - tl) go to box bits 29 / 30
__device__ __forceinline__ void stage_flat(uint4* dst, const VisTri& t, uint32_t pre) {
    dst[0] = make_uint4((uint32_t)t.A0, (uint32_t)t.B0, (uint32_t)t.C0, (uint32_t)t.A1);
    dst[1] = make_uint4((uint32_t)t.B1, (uint32_t)t.C1, (uint32_t)t.A2, (uint32_t)t.B2);
    dst[2] = make_uint4((uint32_t)t.C2, pre, __float_as_uint(t.z0), __float_as_uint(t.dz1));
    dst[3] = make_uint4(__float_as_uint(t.dz2), __float_as_uint(t.rcpA), t.ordk, t.box | ((t.flags & 0x60u) << 24));
}

#define STAIR_K 8u  // submission orders kept per pixel (STAIR)

// one fragment that passed coverage and the z range.  STAIR: also remember its order unless the key it meets proves it
// dominated: `old` is SOME fragment of this pixel; if it is earlier and strictly nearer, this one fails the depth test
// whatever else arrives (the depth it meets is <= z_old < z).
template <bool STAIR>
__device__ __forceinline__ void put_fragment(unsigned long long* s_key, uint32_t* s_cnt, uint32_t* s_list, uint32_t pix, unsigned long long key) {
    if (!STAIR) {
        atomicMax(&s_key[pix], key);
        return;
    }
    const unsigned long long old = atomicMax(&s_key[pix], key);
    if (old != 0ull && (uint32_t)old < (uint32_t)key && (uint32_t)(old >> 32) > (uint32_t)(key >> 32)) return;
    const uint32_t slot = atomicAdd(&s_cnt[pix], 1u);
    if (slot < STAIR_K) s_list[pix * STAIR_K + slot] = (uint32_t)key;
}

__device__ __forceinline__ unsigned long long make_key(float z, uint32_t ordk) {
    // 0 <= z <= 1 and z is never -0 (SPEC.md: vertex z comes from an fma chain started at +0), so the bit
    // pattern is monotonic; larger key = nearer, then later
    return ((unsigned long long)(~__float_as_uint(z)) << 32) | ordk;
}

// deferred textured shading of the winner at pixel (px,py): SPEC.md section 7, same operations as the
// per-fragment path (the quad neighbours are evaluated from the same triangle's plane equations)
__device__ __forceinline__ void sample_textured(const RecA& a, const RecB& b, const DMat& mat, int32_t px, int32_t py, float (&src)[4]) {
    const QuadUV q = quad_uv(uv_planes(b), px, py, [&](int32_t qx, int32_t qy, float& b1, float& b2) { tri_abs_bary(a.X0, a.Y0, a.X1, a.Y1, a.X2, a.Y2, qx, qy, b1, b2); });
    const TexRef tr = {mat.tex, mat.tw, mat.th, mat.tlevels};
    sample_texture(tr, q.u, q.v, filter_select(q.dudx, q.dvdx, q.dudy, q.dvdy, mat.tw, mat.th, mat.tlevels), src);
}
// z of the record's triangle at the centre of pixel (px, py): the edge values are the exact integers the rasteriser
// compares, so this is the float the flattened walk computed from its bin-relative form (SPEC.md section 6)
__device__ __forceinline__ float z_at(const RecA& a, int32_t px, int32_t py) {
    float b1, b2;
    tri_abs_bary(a.X0, a.Y0, a.X1, a.Y1, a.X2, a.Y2, px, py, b1, b2);
    return tri_depth(b1, b2, a.z0, a.z1 - a.z0, a.z2 - a.z0);
}

// waves per bin: the passes (64 triangles each) of a bin are dealt round-robin to the waves of its workgroup;
// the keys are order-independent, so the waves only meet at the two barriers around the raster loop.
// measured on the unsharded headline scene (tools/sweep_vis_waves.sh): 1 wave per bin: 104 us, 2: 73 us, 4: 83 us, 8: 129 us
#ifndef VIS_OCC
#define VIS_OCC 6    // waves per SIMD the register allocator must leave room for (no spills at 6)
#endif

// VIS_WAVES: 2 for unsharded frames (see above); a sharded rank has few bins and the frame then takes as long as its
// heaviest bin (629 triangles = 183 batches of 64 pairs on the headline scene: 23 us with two waves), so the host
// gives such frames 4 or 8 waves per bin (mtr_launch_tile_vis).
// QW: always false.  It selected a 2 x 2 quad walk for frames alone on the GPU until the span walk below replaced it; the
// parameter stays so that the kernel keeps the name bench.py and profiles/ refer to it by (k_tile_vis<false, 2, false, false>).
template <bool TEX, int VIS_WAVES, bool STAIR, bool QW>
__global__ __launch_bounds__(64 * VIS_WAVES, VIS_OCC) void k_tile_vis(TileParams P) {
    __shared__ unsigned long long s_key[MTR_BIN * MTR_BIN];
    __shared__ uint4 s_flat[VIS_WAVES][64 * 4];              // flat-class triangles of the current pass, 64 B each
    __shared__ unsigned long long s_start[VIS_WAVES][64];     // per batch of 64 pairs: which pairs start a triangle
    __shared__ uint32_t s_trans;                               // mixed frames: the queue holds an order-dependent triangle
    __shared__ uint32_t s_hard;                                // ... one that prefix minima of z do not resolve: the ordered kernel's bin
    __shared__ uint32_t s_cnt[STAIR ? MTR_BIN * MTR_BIN : 1];                      // STAIR: orders listed per pixel
    __shared__ __align__(16) uint32_t s_list[STAIR ? MTR_BIN * MTR_BIN * STAIR_K : 4];  // STAIR: the orders (+ 1)

    static_assert(!QW, "the quad walk is retired");
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the shared entry (tile_common.h): the head of the parameters in one fetch, this workgroup's bin, and -- direct mode --
    // this wave's first two entry loads issued together with the fill-count load instead of after it
    const uint32_t stride = 64 * VIS_WAVES, first = wv * 64;
    TileEntry te;
    if (!tile_enter<64 * VIS_WAVES, true>(P, first, lane, te)) return;  // uniform over the workgroup, before any barrier
    const TileHead& hd = te.h;
    const uint32_t ovf = te.ovf, bin = te.bin, ent_lo = te.ent_lo, n_seg = te.n_seg;
    const uint32_t spec0 = te.spec0, spec1 = te.spec1;
    uint32_t N = te.n_ent;
    const int32_t binx0 = (int32_t)te.bin_x * MTR_BIN, biny0 = (int32_t)te.bin_y * MTR_BIN;
    const float cd = P.clear_depth;
    // fragments pass 0 <= z <= 1 and z <= clear depth (nothing else is in the depth buffer before the resolve)
    const bool zlim_ok = cd >= 0.0f;
    const uint32_t zlim = __float_as_uint(fminf(cd, 1.0f));
    const int32_t vw = (int32_t)hd.W - binx0, vh = (int32_t)hd.H - biny0;  // viewport edge in bin coordinates
    if (ovf) {  // incomplete queues: read nothing, leave the bin cleared and its fill word parked for the next frame
        N = 0;
        __syncthreads();  // every thread has read the fill word
        if (threadIdx.x == 0) bin_queue_done(P.fb, bin);
    }
    if (N == 0) {
        // an empty bin (a third of the headline frame): clear colour / depth and leave, no LDS, no barrier
        for (uint32_t pidx = threadIdx.x; pidx < MTR_BIN * MTR_BIN; pidx += 64 * VIS_WAVES) {
            const int32_t lx = (int32_t)(pidx & (MTR_BIN - 1)), ly = (int32_t)(pidx >> MTR_BIN_SHIFT);
            if (lx >= vw || ly >= vh) continue;
            const size_t pi = (size_t)(biny0 + ly) * hd.W + (size_t)(binx0 + lx);
            reinterpret_cast<uint32_t*>(P.color)[pi] = P.clear_rgba8;
            P.depth[pi] = cd;
        }
        if (P.mixed && threadIdx.x == 0) P.bin_flag[bin] = 0;
        // the parked count of an empty bin is 0 too (mtr_frame_read_bin_counts: what bench.py balances bands by); without
        // this store the word keeps whatever the allocation, or an earlier scene, left there
        if (hd.direct && threadIdx.x == 0 && !ovf) P.fb.bin_count[bin] = 0ull;
        return;
    }
    const RecA zero_rec = {0, 0, 0, 0, 0, 0, 0.0f, 0.0f, 0.0f, 0u, 0u, 0u};
    // two-deep software pipeline over the dependent loads entries[] -> rec_a[]: while pass k is rasterised the
    // record loads of this wave's next pass and the entry loads of the one after are in flight.  The record of an
    // entry is addressable from its submission order: chunk run base = chunk * MTR_CHUNK_SLOTS.
    uint32_t ord_cur = 0, ord_nxt = 0;
    if (hd.direct) {
        if (first + lane < N) ord_cur = spec0;
        if (first + stride + lane < N) ord_nxt = spec1;
    } else {
        if (first + lane < N) ord_cur = hd.entries[ent_lo + first + lane];
        if (first + stride + lane < N) ord_nxt = hd.entries[ent_lo + first + stride + lane];
    }
    RecA a_cur = zero_rec;
    if (first + lane < N) a_cur = load_rec(hd.rec_a, P.fb.rec_l, (ord_cur >> 7) * MTR_CHUNK_SLOTS + (ord_cur & 127u));
    // ... and the first record load is in flight while the workgroup clears its keys and meets
    for (uint32_t i = threadIdx.x; i < MTR_BIN * MTR_BIN; i += 64 * VIS_WAVES) {
        s_key[i] = 0ull;
        if (STAIR) s_cnt[i] = 0u;
    }
    if (threadIdx.x == 0) { s_trans = 0u; s_hard = 0u; }
    __syncthreads();
    for (uint32_t e0 = first; e0 < N; e0 += stride) {
        const bool valid = e0 + lane < N;
        RecA a_nxt = zero_rec;
        if (e0 + stride + lane < N) a_nxt = load_rec(hd.rec_a, P.fb.rec_l, (ord_nxt >> 7) * MTR_CHUNK_SLOTS + (ord_nxt & 127u));
        uint32_t ord_nn = 0;
        if (e0 + 2 * stride + lane < N) ord_nn = hd.entries[ent_lo + e0 + 2 * stride + lane];

        if (P.mixed && valid && (a_cur.pad1 >> 16)) {  // benign races: every writer stores 1
            s_trans = 1u;
            if (!STAIR || (a_cur.pad1 >> 17)) s_hard = 1u;
        }
        Setup s = {};
        if (valid) setup_tri(a_cur, ord_cur, binx0, biny0, vw, vh, s);
        const bool large = (s.t.flags & 1u) != 0;
        const uint32_t iw = ((s.t.box >> 8) & 15u) + 1u;  // bbox width
        const uint32_t npx = (uint32_t)s.npx;
        // k / iw = k * magic >> 16 (row_magic, tile_common.h) is read by the whole-wave walk of large triangles and by the
        // pair walk only, so it is computed in their branches: the span walk, which takes nearly every pass of a frame of
        // small triangles, never pays for the division.  (A span pass can still hold a large triangle.)
        // ---- lane = pixel of the bbox: triangles that need 64-bit edge functions (more than 64 px across: rare),
        //      broadcast one at a time with v_readlane ----
        const uint64_t mlarge = __ballot(npx != 0 && large);
        uint32_t lbox = s.t.box;
        if (mlarge) lbox |= row_magic(iw) << 12;  // uniform branch
        for (uint64_t mb = mlarge; mb; mb &= mb - 1) {
            const uint32_t t = __builtin_amdgcn_readfirstlane((uint32_t)__ffsll((long long)mb) - 1);
#define RL(x) __builtin_amdgcn_readlane((int)(x), t)
            const TriEdges E = {RL(s.t.A0), RL(s.t.B0), RL(s.t.C0), RL(s.t.A1), RL(s.t.B1), RL(s.t.C1), RL(s.t.A2), RL(s.t.B2), RL(s.t.C2)};
            const uint32_t flags = (uint32_t)RL(s.t.flags), box = (uint32_t)RL(lbox), tord = (uint32_t)RL(s.t.ordk), tn = (uint32_t)RL(npx);
            const float z0 = __int_as_float(RL(__float_as_int(s.t.z0))), dz1 = __int_as_float(RL(__float_as_int(s.t.dz1)));
            const float dz2 = __int_as_float(RL(__float_as_int(s.t.dz2))), rcpA = __int_as_float(RL(__float_as_int(s.t.rcpA)));
            const int32_t H0 = RL(s.chi.x), H1 = RL(s.chi.y), H2 = RL(s.chi.z);
#undef RL
            const uint32_t bw = ((box >> 8) & 15u) + 1u, magic = box >> 12;
            for (uint32_t k = lane; k < tn; k += 64) {
                const uint32_t row = (k * magic) >> 16;
                const int32_t lx = (int32_t)((box & 15u) + (k - row * bw)), ly = (int32_t)(((box >> 4) & 15u) + row);
                float b1, b2;
                const bool inside = tri_inside_large(E, H0, H1, H2, flags, rcpA, lx, ly, b1, b2);
                const float z = tri_depth(b1, b2, z0, dz1, dz2);
                if (inside && z >= 0.0f && z <= 1.0f && z <= cd) put_fragment<STAIR>(s_key, s_cnt, s_list, (uint32_t)(ly * MTR_BIN + lx), make_key(z, tord));
            }
        }

        // ---- lane = (triangle, bbox row), 64 rows per step, for every i32-class triangle of a pass whose boxes are mostly
        //      larger than four pixels.  A row finds the exact run of columns its triangle covers (span_row.h: three
        //      zero crossings, each estimated in f32 and settled by one integer evaluation of its edge) and walks just
        //      that run: no (eb0 | eb1 | eb2) test, and the pairs of the bbox that cover no pixel centre -- 78 % of them on
        //      the headline scene (tools/span_stats.py) -- are never visited.  The headline's covered runs are one pixel
        //      long on average, so the run is walked by its own lane rather than flattened a second time.  A pass holds
        //      at most 64 x 16 rows: one round, at most 16 start masks, the pair walk's scheme.  Uniform over the wave;
        //      passes of one-pixel boxes (the instanced configs) keep the pair walk below. ----
        const uint32_t ncand = (uint32_t)__popcll(__ballot(npx != 0 && !large));
        const bool spans = zlim_ok && ncand != 0u && (uint32_t)__popcll(__ballot(!large && npx > 4)) * 2u >= ncand;
        if (spans) {
            const bool cand = npx != 0 && !large;
            const uint32_t cidx = lane_rank(__ballot(cand));
            const uint32_t rows = cand ? s.bhm1 + 1u : 0u;
            const uint32_t inc = wave_incl_scan_u32(rows);
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);  // <= 64 x 16
            flat_stage_starts(s_start[wv], 64, lane, rows, inc - rows);
            if (cand) stage_flat(&s_flat[wv][cidx * 4], s.t, inc - rows);  // the triangle's first row item in place of its first pair
            wave_lds_sync();
            flat_for_each(s_start[wv], 64, lane, total, [&](uint32_t p, uint32_t tri) {
                const uint4* src = &s_flat[wv][tri * 4];
                const uint4 q0 = src[0], q1 = src[1], q2 = src[2], q3 = src[3];
                const uint32_t box = q3.w;
                const int32_t row = (int32_t)(p - q2.y);
                const int32_t A1 = (int32_t)q0.w, A2 = (int32_t)q1.z;
                int32_t e1 = (int32_t)q1.y + MTR_MUL24((int32_t)q1.x, row), e2 = (int32_t)q2.x + MTR_MUL24((int32_t)q1.w, row);
                int32_t lo, hi;
                span_of_row((int32_t)q0.z + MTR_MUL24((int32_t)q0.y, row), e1, e2, (int32_t)q0.x, A1, A2, (int32_t)((box >> 8) & 15u), lo, hi);
                // eb1 / eb2 of the run's first pixel, + (1 - tl): the pair walk's integers, stepped along the row
                e1 = MTR_MAD24(A1, lo, e1 + (int32_t)((box >> 29) & 1u));  // lo in [0, 15], A = 256 * dy, |dy| <= 2^14
                e2 = MTR_MAD24(A2, lo, e2 + (int32_t)((box >> 30) & 1u));
                const float rcp = __uint_as_float(q3.y), dz1 = __uint_as_float(q2.w), dz2 = __uint_as_float(q3.x), z0 = __uint_as_float(q2.z);
                uint32_t pix = (box & 0xffu) + (uint32_t)(row * MTR_BIN + lo);
                for (int32_t c = lo; c <= hi; c++, pix++, e1 += A1, e2 += A2) {
                    const float b1 = (float)e1 * rcp, b2 = (float)e2 * rcp;
                    const float z = tri_depth(b1, b2, z0, dz1, dz2);
                    if (__float_as_uint(z) <= zlim) put_fragment<STAIR>(s_key, s_cnt, s_list, pix, make_key(z, q3.z));
                }
            });
        }
        // ---- lane = (triangle, pixel) pair, 64 pairs per step, for every i32-class triangle.  A round stages a
        //      prefix of the remaining triangles holding <= 4096 pairs (64 start masks, one per lane); one round
        //      is the rule.  Fewer than half of this walk's boxes are over four pixels, so a pass holds at most
        //      31 x 256 + 33 x 4 pairs and needs three rounds at the most (64 bin-filling triangles take the span walk). ----
        for (uint64_t todo = (zlim_ok && !spans) ? __ballot(npx != 0 && !large) : 0ull; todo;) {
            const bool cand = (todo >> lane) & 1ull;
            const uint32_t mine = cand ? npx : 0u;
            const uint32_t inc = wave_incl_scan_u32(mine);
            const bool take = cand && inc <= 4096u;  // npx <= 256: the first candidate always fits
            const uint64_t tm = __ballot(take);
            todo &= ~tm;
            const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63 - __builtin_clzll(tm));
            const uint32_t cidx = lane_rank(tm);
            flat_stage_starts(s_start[wv], 64, lane, take ? mine : 0u, inc - mine);
            if (take) {
                s.t.box |= row_magic(iw) << 12;  // a triangle is taken by one round only
                stage_flat(&s_flat[wv][cidx * 4], s.t, inc - mine);
            }
            wave_lds_sync();
            flat_for_each(s_start[wv], 64, lane, total, [&](uint32_t p, uint32_t tri) {
                const uint4* src = &s_flat[wv][tri * 4];
                const uint4 q0 = src[0], q1 = src[1], q2 = src[2], q3 = src[3];
                const TriEdges E = {(int32_t)q0.x, (int32_t)q0.y, (int32_t)q0.z, (int32_t)q0.w, (int32_t)q1.x, (int32_t)q1.y, (int32_t)q1.z, (int32_t)q1.w, (int32_t)q2.x};
                const uint32_t box = q3.w, k = p - q2.y;
                const int32_t row = (int32_t)((k * ((box >> 12) & 0x1ffffu)) >> 16);
                const int32_t col = (int32_t)k - __mul24(row, (int32_t)((box >> 8) & 15u) + 1);
                int32_t e1, e2;
                const bool inside = tri_inside(E, col, row, e1, e2);
                const float rcpA = __uint_as_float(q3.y);
                const float z = tri_depth(tri_bary(e1, (box >> 29) & 1u, rcpA), tri_bary(e2, (box >> 30) & 1u, rcpA), __uint_as_float(q2.z), __uint_as_float(q2.w),
                                          __uint_as_float(q3.x));
                // 0 <= z <= min(1, clear depth) as ONE unsigned compare of the bit patterns (z is never -0, SPEC.md;
                // negative and NaN patterns are above every non-negative bound)
                if (inside && __float_as_uint(z) <= zlim)
                    put_fragment<STAIR>(s_key, s_cnt, s_list, (box & 0xffu) + (uint32_t)(row * MTR_BIN + col), make_key(z, q3.z));
            });
        }
        a_cur = a_nxt;
        ord_cur = ord_nxt;
        ord_nxt = ord_nn;
    }
    const TileLate Q = tile_late();  // what the resolve reads: fetched here, under the barrier, not carried across the raster loop
    __syncthreads();
    bool stair = false;  // this bin resolves through its per-pixel order lists
    if (Q.mixed) {  // an order-dependent triangle in the queue
        bool leave = s_hard != 0u;  // leave the bin (and its queue) to the ordered kernel
        if (STAIR && !leave && s_trans) {
            bool over = false;
            for (uint32_t i = threadIdx.x; i < MTR_BIN * MTR_BIN; i += 64 * VIS_WAVES) over = over || s_cnt[i] > STAIR_K;
            leave = __syncthreads_or(over ? 1 : 0) != 0;  // a pixel listed more orders than it has room for
            stair = !leave;
        }
        if (threadIdx.x == 0) Q.bin_flag[bin] = leave ? 1 : 0;
        if (leave) return;
    }
    if (threadIdx.x == 0) {
        if (Q.direct && N) {  // queue statistics (direct mode has no scan to count them)
            atomicAdd(&Q.counters[MTR_CTR(CTR_ENT, bin)], N);
            atomicAdd(&Q.counters[MTR_CTR(CTR_SEG, bin)], n_seg);
        }
        bin_queue_done(Q, bin);  // every wave has read its queue bounds by now
    }

    // ---- resolve: deferred shading of each pixel's winner, the only framebuffer traffic of the frame;
    //      one pixel per thread, rows of 16 pixels = 64 contiguous bytes ----
    // (unrolled: a thread's pixels are independent, so their winner-record loads are in flight together)
#pragma unroll
    for (uint32_t pidx = threadIdx.x; pidx < MTR_BIN * MTR_BIN; pidx += 64 * VIS_WAVES) {
        const int32_t lx = (int32_t)(pidx & (MTR_BIN - 1)), ly = (int32_t)(pidx >> MTR_BIN_SHIFT);
        if (lx >= vw || ly >= vh) continue;
        const uint32_t x = (uint32_t)(binx0 + lx), y = (uint32_t)(biny0 + ly);
        const unsigned long long key = s_key[ly * MTR_BIN + lx];
        uint32_t col = Q.clear_rgba8;
        float dep = cd;
        if (STAIR && stair) {
            // the pixel's listed fragments in submission order; those that pass the depth test (z <= every earlier one's:
            // running minimum, starting from the clear depth) are shaded and blended, exactly as the ordered kernel does
            const uint32_t pix = (uint32_t)(ly * MTR_BIN + lx);
            const uint32_t n = s_cnt[pix];
            const uint4 l0 = reinterpret_cast<const uint4*>(&s_list[pix * STAIR_K])[0], l1 = reinterpret_cast<const uint4*>(&s_list[pix * STAIR_K])[1];
            const uint32_t lst[STAIR_K] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
            uint32_t last = 0;  // orders are stored + 1
            for (;;) {
                uint32_t best = 0xFFFFFFFFu;  // the smallest listed order above `last`
#pragma unroll
                for (uint32_t j = 0; j < STAIR_K; j++)
                    if (j < n && lst[j] > last && lst[j] < best) best = lst[j];
                if (best == 0xFFFFFFFFu) break;
                last = best;
                const uint32_t ord = best - 1u;
                const uint32_t r = (ord >> 7) * MTR_CHUNK_SLOTS + (ord & 127u);
                const RecA a = load_rec(Q.rec_a, Q.rec_l, r);
                const float z = z_at(a, (int32_t)x, (int32_t)y);
                if (!(z <= dep)) continue;  // fails LessEqual against the nearest of its predecessors
                dep = z;
                if (a.pad1 & 1u) {  // solid: its colour replaces the pixel
                    col = a.pad0;
                } else {
                    const DMat mat = Q.mats[a.mat];
                    if (TEX && mat.shader == MTR_SH_TEXTURED) {
                        const RecB b = Q.rec_b[r];
                        float src[4];
                        sample_textured(a, b, mat, (int32_t)x, (int32_t)y, src);
                        col = blend_store(col, src, mat.blend == MTR_DB_ALPHA ? 1u : 0u);
                    } else {
                        col = mat.rgba8;
                    }
                }
            }
        } else if (key != 0ull) {
            dep = __uint_as_float(~(uint32_t)(key >> 32));
            const uint32_t ord = (uint32_t)key - 1u;
            const uint32_t r = (ord >> 7) * MTR_CHUNK_SLOTS + (ord & 127u);
            // the last word of the record: the source colour of a solid triangle (top byte 0xFF) or a material id
            const uint32_t payload = Q.rec_a[r].q1.w;
            if ((payload >> 24) != 0xFFu) {  // needs its material: in this kernel (order-free triangles only) a textured one
                const DMat mat = Q.mats[payload & 0xFFFFFFu];
                if (TEX && mat.shader == MTR_SH_TEXTURED) {
                    const RecA a = load_rec(Q.rec_a, Q.rec_l, r);
                    const RecB b = Q.rec_b[r];
                    float src[4];
                    sample_textured(a, b, mat, (int32_t)x, (int32_t)y, src);
                    col = blend_store(0u, src, 0u);  // order-free: blending is off, or the texture is opaque (a == 1 exactly) and the blend a replace
                } else {
                    col = mat.rgba8;
                }
            } else {
                col = payload;
            }
        }
        const size_t pi = (size_t)y * Q.W + x;
        reinterpret_cast<uint32_t*>(Q.color)[pi] = col;
        Q.depth[pi] = dep;
    }
}

}  // namespace mtr

void mtr_launch_tile_vis(const TileParams& p_in, bool textured, hipStream_t s) {
    TileParams p = p_in;
    tile_fill_head(p);
    const uint32_t mine = p.fb.own.own_count, grid = p.head.grid;
    if (mine == 0) return;
    const int waves = (int)mtr_vis_waves_for(p.vis_waves, mine);
#define MTR_LAUNCH_VIS(T, W, S) hipLaunchKernelGGL((mtr::k_tile_vis<T, W, S, false>), dim3(grid), dim3(64 * W), 0, s, p)
#define MTR_LAUNCH_VIS_W(T, S) do { if (waves >= 8) MTR_LAUNCH_VIS(T, 8, S); else if (waves >= 4) MTR_LAUNCH_VIS(T, 4, S); else MTR_LAUNCH_VIS(T, 2, S); } while (0)
    // frames with translucent materials keep per-pixel order lists (STAIR); all-opaque frames need only the key
    if (p.mixed) { if (textured) MTR_LAUNCH_VIS_W(true, true); else MTR_LAUNCH_VIS_W(false, true); }
    else { if (textured) MTR_LAUNCH_VIS_W(true, false); else MTR_LAUNCH_VIS_W(false, false); }
#undef MTR_LAUNCH_VIS_W
#undef MTR_LAUNCH_VIS
}
