// k_blend.hip -- blend spaces (SPEC.md section 23): one or two float parameters per instance mix phase-locked LOOP clips.  Per
// instance a 16-byte blend state that lives on the device (a phase, two smoothed parameters, a speed) is advanced by dt: the
// parameters are read from the instance's controller row and smoothed, the two or three samples around the point are found
// with their sequential weights, one shared phase moves at the blended rate, and the records the animate, root-motion and
// event calls take are written: layers 0 to 2 of a layer stack, three mtr_root_steps, optionally the three shares.  Every
// scalar rule lives in blend_math.h, which the host test compiles too.
//
// Lanes.  One lane per instance, 256-thread workgroups, no LDS, no barrier, no cross-lane traffic.  A lane loads its state as
// one 16-byte word and one or two parameters, and stores the state as one 16-byte word, three layers and three steps as one
// 16-byte word each and the shares as three 4-byte words: 16 + 8 bytes in and at most 16 + 48 + 48 + 12 out.
//
// Tables.  The samples (at most 32), the triangles (at most 64) and the clip entries are read-only and small: 1.5 KiB of
// samples and triangles at the most.  They are left to loads through the caches, not staged in LDS: the triangle loops run
// over every triangle with an index that is uniform across the wave, so the triangle and its three samples come from
// addresses every lane shares (the compiler reads them, and the samples of the 1-D search, with scalar loads: the loops branch
// on the scalar unit and skip a body with no live lane) and stay in the scalar cache after the first trip, while a stage in LDS
// would cost every workgroup a barrier that lanes >= n would have to reach and 1.5 KiB of loads even for a 1-D space of two
// samples.  Without the barrier a lane >= n returns before any access.  The loads that are not uniform -- the samples around a
// 1-D bracket, the clips of the three slots -- are per lane from the same few cache lines.
//
// Divergence.  Lanes of one wave that are inside different triangles, or outside the hull, are masked at different trips; a
// lane's result is made of its own registers only (no cross-lane operation, no vote), so it does not depend on that.
//
// Memory safety.  n (1..max_instances), nlayers (3..8), nparams (1..16), param_x and param_y (< nparams) are host values,
// validated; a lane whose index is >= n returns before any access.  The state, parameter and output arrays hold n records
// and are indexed by the lane's own instance only.  The tables were validated at creation and live in the set's own memory,
// which no caller can write: a sample's clip is < nclips, a triangle's indices are < nsamples.  The 1-D bracket j is kept in
// 0..nsamples - 2 by the two comparisons ahead of the search.  From caller-writable device memory come only the state and the
// parameters, all floats: they reach comparisons and arithmetic, never an address.
#include "mtr_internal.h"
#include "blend_math.h"

namespace mtr {

__global__ __launch_bounds__(256) void k_blend(BlendParams p) {
    const uint32_t inst = blockIdx.x * 256u + threadIdx.x;
    if (inst >= p.n) return;
    uint4* sp = reinterpret_cast<uint4*>(p.states) + inst;
    const uint4 s0 = *sp;
    BlendState st;
    st.phase = __uint_as_float(s0.x); st.px = __uint_as_float(s0.y); st.py = __uint_as_float(s0.z); st.speed = __uint_as_float(s0.w);
    BlendTables t;
    t.clips = reinterpret_cast<const PlayClip*>(p.clips);
    t.samples = reinterpret_cast<const BlendSample*>(p.samples);
    t.tris = reinterpret_cast<const BlendTri*>(p.tris);
    t.nclips = p.nclips; t.nsamples = p.nsamples; t.ntris = p.ntris;
    t.param_x = p.param_x; t.param_y = p.param_y; t.nparams = p.nparams;
    t.damp = p.damp;
    const BlendFrame f = blend_advance(st, p.params + (size_t)inst * p.nparams, p.dt, t);
    *sp = make_uint4(__float_as_uint(st.phase), __float_as_uint(st.px), __float_as_uint(st.py), s0.w);
    if (p.out_layers) {  // clip, x, w, mask 0 and MTR_LAYER_OVERRIDE (0) in one word; layers 3.. are not touched
        uint4* o = reinterpret_cast<uint4*>(p.out_layers) + (size_t)inst * p.nlayers;
        o[0] = make_uint4(f.clip[0], __float_as_uint(f.x[0]), 0u, 0u);
        o[1] = make_uint4(f.clip[1], __float_as_uint(f.x[1]), __float_as_uint(f.e[1]), 0u);
        o[2] = make_uint4(f.clip[2], __float_as_uint(f.x[2]), __float_as_uint(f.e[2]), 0u);
    }
    if (p.out_steps) {  // clip, x, dx, w
        uint4* o = reinterpret_cast<uint4*>(p.out_steps) + (size_t)inst * 3;
        o[0] = make_uint4(f.clip[0], __float_as_uint(f.x0[0]), __float_as_uint(f.dx[0]), 0u);
        o[1] = make_uint4(f.clip[1], __float_as_uint(f.x0[1]), __float_as_uint(f.dx[1]), __float_as_uint(f.e[1]));
        o[2] = make_uint4(f.clip[2], __float_as_uint(f.x0[2]), __float_as_uint(f.dx[2]), __float_as_uint(f.e[2]));
    }
    if (p.out_shares) {
        float* o = p.out_shares + (size_t)inst * 3;
        o[0] = f.share[0]; o[1] = f.share[1]; o[2] = f.share[2];
    }
}

}  // namespace mtr

void mtr_launch_blend(const BlendParams& p, hipStream_t s) {
    if (p.n == 0 || p.nsamples == 0 || p.nclips == 0) return;
    hipLaunchKernelGGL(mtr::k_blend, dim3((p.n + 255u) / 256u), dim3(256), 0, s, p);
}
