// k_anim.hip -- skin palettes from animation clips (SPEC.md section 14).  For every instance: sample one or two clips at
// the instance's key positions, cross-fade them, turn each joint's (translation, quaternion, scale) into its local matrix
// and fold the skeleton as k_pose does (section 12).  The local matrices exist in LDS only.
//
// Same shape as k_pose: one workgroup per instance, one thread per joint.  The 24-byte state is the same for the whole
// workgroup; thread j reads its joint's keys (3 x 16 bytes each: 2 keys, or 4 with a cross-fade) with every load issued
// before the first use.  Section 14 has no fused multiply-add: every operator below is one rounded operation (the file
// is compiled with -ffp-contract=off), so a plain binary32 model reproduces the local matrices bit for bit.
//
// Two sources of channel values: clips of uniformly spaced 48-byte keys (section 14), and track sets (section 15: per joint
// and channel a track with its own key times and 16-bit keys).  Everything after "one clip's (T, Q, S)" is one copy.
//
// Layers (section 16): the k_anim_layers kernels evaluate a stack of up to 8 layers per instance on either source -- a
// base clip, then per layer a clip blended over it per joint (override or additive) by its weight times a mask weight.
// The scalar blend rules of both sections live in anim_blend.h.
//
// Inverse kinematics (section 17): the k_anim_ik kernels evaluate the same stack through the same code, keep each joint's
// (T, Q, S) in registers and, between the stack and the fold, solve up to 4 chains per instance (two-bone reach, aim) in
// order over the local matrices and rotations in LDS.  The scalar solve lives in anim_ik.h.
//
// Spring bones (section 24): the k_anim_spring kernels go on from there -- after the chains, joints that carry a spring are
// aimed at a particle whose state lives in device memory from call to call.  The scalar rule lives in spring_math.h.
#include "anim_blend.h"
#include "anim_ik.h"
#include "anim_launch.h"
#include "spring_math.h"
#include "anim_tracks.h"
#include "pose_common.h"

namespace mtr {

__device__ __forceinline__ AnimKey anim_load_key(const float4* keys, uint32_t key, uint32_t J, uint32_t j) {
    const float4* k = keys + ((size_t)key * J + j) * 3;
    AnimKey r;
    r.t = k[0]; r.q = k[1]; r.s = k[2];
    return r;
}

// ---- the track source (section 15) ----
// What one thread holds of one clip's three tracks of its joint while they are searched
struct TrackClip {
    float r;
    uint32_t nticks, flags;
    uint32_t first[3], count[3];
    float lo[2][3], step[2][3];  // [0] translation, [1] scale; the rotation's are never read
    TrackSearch s[3];
};

// Memory safety by construction.  Every index below is formed from a descriptor of the set, which mtr_anim_create_tracks
// validated on the host before the upload (count >= 1, first + count <= the key total, times[first] == 0, strictly
// increasing times, the last one <= N - 1) and which nothing writes afterwards.  The device-side state only chooses
// (a) the clip, and the index is clamped to nclips - 1, and (b) the position x, and track_position() returns -0 or a
// value of [0, N) for every x (NaN, +-inf, huge, -0).  The search keeps base + n <= first + count and probes inside that
// range whatever r is; k is its base, k1 is k + 1 < first + count, first or k.  So no state can move a read of times[] or
// values[] outside [first, first + count) of a validated track, and the descriptor index (clip * J + j) * 3 + ch lies
// inside the nclips * J * 3 descriptors because j < J.
__device__ __forceinline__ void track_clip_begin(const AnimParams& p, uint32_t clip, float x, uint32_t j, TrackClip& c) {
    const uint32_t ci = clip < p.nclips ? clip : p.nclips - 1u;
    const uint4 ct = reinterpret_cast<const uint4*>(p.clips)[ci];
    c.nticks = ct.y; c.flags = ct.z;
    c.r = track_position(x, ct.y, ct.z);
    const uint4* d = reinterpret_cast<const uint4*>(p.tracks) + ((size_t)ci * p.pose.njoints + j) * 6;  // 3 x 32 bytes
    const uint4 t0 = d[0], t1 = d[1], s0 = d[4], s1 = d[5];
    const uint2 q0 = *reinterpret_cast<const uint2*>(d + 2);
    c.first[0] = t0.x; c.count[0] = t0.y;
    c.first[1] = q0.x; c.count[1] = q0.y;
    c.first[2] = s0.x; c.count[2] = s0.y;
    c.lo[0][0] = __uint_as_float(t0.z); c.lo[0][1] = __uint_as_float(t0.w); c.lo[0][2] = __uint_as_float(t1.x);
    c.step[0][0] = __uint_as_float(t1.y); c.step[0][1] = __uint_as_float(t1.z); c.step[0][2] = __uint_as_float(t1.w);
    c.lo[1][0] = __uint_as_float(s0.z); c.lo[1][1] = __uint_as_float(s0.w); c.lo[1][2] = __uint_as_float(s1.x);
    c.step[1][0] = __uint_as_float(s1.y); c.step[1][1] = __uint_as_float(s1.z); c.step[1][2] = __uint_as_float(s1.w);
#pragma unroll
    for (int ch = 0; ch < 3; ch++) c.s[ch] = track_search_begin(c.first[ch], c.count[ch]);
}

// the (T, Q, S) of NC clips at once: the 3 * NC searches advance in one loop, a step's loads in flight together; then
// every time and value load is issued before the first use
template <int NC>
__device__ __forceinline__ void track_sample(const AnimParams& p, TrackClip (&c)[NC], AnimKey (&out)[NC]) {
    const uint16_t* times = p.times;
    const uint2* values = reinterpret_cast<const uint2*>(p.values);
    uint32_t left = 0u;
#pragma unroll
    for (int i = 0; i < NC; i++) left |= c[i].count[0] | c[i].count[1] | c[i].count[2];
    for (; left > 1u; left = track_search_left(left)) {  // as many steps as the longest of this thread's tracks takes
#pragma unroll
        for (int i = 0; i < NC; i++)
#pragma unroll
            for (int ch = 0; ch < 3; ch++) track_search_step(times, c[i].r, c[i].s[ch]);
    }
    uint32_t k1[NC][3], tk1[NC][3];
    uint2 v0[NC][3], v1[NC][3];
#pragma unroll
    for (int i = 0; i < NC; i++)
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            const uint32_t k = c[i].s[ch].base;
            k1[i][ch] = track_next_key(c[i].first[ch], c[i].count[ch], k, c[i].flags);
            tk1[i][ch] = times[k1[i][ch]];
            v0[i][ch] = values[k];
            v1[i][ch] = values[k1[i][ch]];
        }
#pragma unroll
    for (int i = 0; i < NC; i++) {
        float a[3];
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
            a[ch] = track_fraction(c[i].r, c[i].first[ch], c[i].count[ch], c[i].s[ch].base, k1[i][ch], c[i].s[ch].tk, tk1[i][ch], c[i].nticks);
        float t0[3], t1[3], q0[4], q1[4], s0[3], s1[3];
        track_decode_lin(v0[i][0].x, v0[i][0].y, c[i].lo[0], c[i].step[0], t0);
        track_decode_lin(v1[i][0].x, v1[i][0].y, c[i].lo[0], c[i].step[0], t1);
        track_decode_rot(v0[i][1].x, v0[i][1].y, q0);
        track_decode_rot(v1[i][1].x, v1[i][1].y, q1);
        track_decode_lin(v0[i][2].x, v0[i][2].y, c[i].lo[1], c[i].step[1], s0);
        track_decode_lin(v1[i][2].x, v1[i][2].y, c[i].lo[1], c[i].step[1], s1);
        out[i].t = make_float4(anim_lerp(t0[0], t1[0], a[0]), anim_lerp(t0[1], t1[1], a[0]), anim_lerp(t0[2], t1[2], a[0]), 0.0f);
        out[i].q = anim_nlerp(make_float4(q0[0], q0[1], q0[2], q0[3]), make_float4(q1[0], q1[1], q1[2], q1[3]), a[1]);
        out[i].s = make_float4(anim_lerp(s0[0], s1[0], a[2]), anim_lerp(s0[1], s1[1], a[2]), anim_lerp(s0[2], s1[2], a[2]), 0.0f);
    }
}

// The local matrix of joint j of instance inst (column-major); TRACKS: the set is a track set
template <bool TRACKS>
__device__ __forceinline__ void anim_local(const AnimParams& p, uint32_t inst, uint32_t j, float4 (&M)[4]) {
    const uint32_t J = p.pose.njoints;
    const uint2* st = reinterpret_cast<const uint2*>(p.states + (size_t)inst * 6);
    const uint2 sc = st[0], sx = st[1], sw = st[2];
    const float w = anim_weight(__uint_as_float(sw.x));
    AnimKey r;
    if constexpr (TRACKS) {
        if (w == 0.0f) {  // clip B is not read
            TrackClip c[1];
            AnimKey v[1];
            track_clip_begin(p, sc.x, __uint_as_float(sx.x), j, c[0]);
            track_sample<1>(p, c, v);
            r = v[0];
        } else {
            TrackClip c[2];
            AnimKey v[2];
            track_clip_begin(p, sc.x, __uint_as_float(sx.x), j, c[0]);
            track_clip_begin(p, sc.y, __uint_as_float(sx.y), j, c[1]);
            track_sample<2>(p, c, v);
            r = anim_mix(v[0], v[1], w);
        }
    } else {
        const uint4* clips = reinterpret_cast<const uint4*>(p.clips);
        const float4* keys = reinterpret_cast<const float4*>(p.keys);
        const uint4 ca = clips[sc.x < p.nclips ? sc.x : p.nclips - 1u];
        const AnimPos pa = anim_position(__uint_as_float(sx.x), ca.y, ca.z);
        if (w == 0.0f) {  // clip B is not read
            const AnimKey a0 = anim_load_key(keys, ca.x + pa.i0, J, j), a1 = anim_load_key(keys, ca.x + pa.i1, J, j);
            r = anim_mix(a0, a1, pa.a);
        } else {
            const uint4 cb = clips[sc.y < p.nclips ? sc.y : p.nclips - 1u];
            const AnimPos pb = anim_position(__uint_as_float(sx.y), cb.y, cb.z);
            const AnimKey a0 = anim_load_key(keys, ca.x + pa.i0, J, j), a1 = anim_load_key(keys, ca.x + pa.i1, J, j);
            const AnimKey b0 = anim_load_key(keys, cb.x + pb.i0, J, j), b1 = anim_load_key(keys, cb.x + pb.i1, J, j);
            r = anim_mix(anim_mix(a0, a1, pa.a), anim_mix(b0, b1, pb.a), w);
        }
    }
    anim_matrix(r, M);
}

// ---- layers (section 16) ----
// What one thread holds of one layer between the issue of its loads and its blend: the layer's weight and mode, the
// joint's mask weight and the source's values -- both keys of the joint and their fraction (uniform keys), or the sampled
// (T, Q, S) in k0 (tracks).  Two of these are live at a time, in named registers: the layer being blended and the next
// one, whose loads are in flight.
struct LayerFetch {
    float w, m;  // the weight as stored and the mask weight: e = anim_layer_weight(w, m), formed when the layer is blended
    uint32_t mode;
    AnimKey k0, k1;
    float a;
};

// Issues the loads of layer l of instance inst for joint j.  The 16-byte record, the clip table entry and the position
// are the same for the whole workgroup (scalar loads and arithmetic); the mask weight and the keys are per lane.  A
// layer whose clamped weight is 0 returns before any further load for the whole workgroup (m = 0 stands for e = 0).
// The base (l == 0) reads its clip and x only.
//
// Memory safety, extending the argument at track_clip_begin: nlayers is a host value validated to 1..8 and the layer
// array holds ninst * nlayers records, so inst * nlayers + l lies inside it.  From a record come (a) the clip index,
// clamped to nclips - 1, (b) the position x, which anim_position / track_position turn into key indices inside the
// clip for every x, (c) the mask index, clamped to nmasks -- 0 without a mask set, and index 0 reads nothing -- so that
// (mask - 1) * J + j lies inside the nmasks * J weights because j < J, and (d) the weight and the mode, which reach no
// address.  No device-side value forms an address unclamped.
template <bool TRACKS>
__device__ __forceinline__ LayerFetch anim_layer_fetch(const AnimLayerParams& p, uint32_t inst, uint32_t l, uint32_t j) {
    const AnimParams& ap = p.anim;
    const uint32_t J = ap.pose.njoints;
    const uint4 rec = reinterpret_cast<const uint4*>(p.layers)[(size_t)inst * p.nlayers + l];  // clip, x, w, mask | mode << 16
    LayerFetch f;  // the keys stay unset where no load is issued: they are read only where e != 0 (a zero fill would be merged
                   // with the loaded registers by copies that wait for the loads, ahead of the previous layer's arithmetic)
    f.mode = rec.w >> 16;
    f.w = __uint_as_float(rec.z);
    f.m = 0.0f;
    if (l != 0u) {
        if (anim_weight(f.w) == 0.0f) return f;
        uint32_t mask = rec.w & 0xFFFFu;
        mask = mask < p.nmasks ? mask : p.nmasks;
        f.m = mask ? p.masks[(size_t)(mask - 1u) * J + j] : 1.0f;
        // Tracks: a lane whose e is 0 takes no part in the searches.  Uniform keys: every lane issues the key loads at once
        // with the mask weight's, without waiting for it (one memory latency less per layer on a chain of dependent
        // layers); a lane whose e turns out 0 leaves what it loaded unused.
        if constexpr (TRACKS) {
            if (anim_layer_weight(f.w, f.m) == 0.0f) return f;
        }
    }
    if constexpr (TRACKS) {
        TrackClip c[1];
        AnimKey v[1];
        track_clip_begin(ap, rec.x, __uint_as_float(rec.y), j, c[0]);
        track_sample<1>(ap, c, v);
        f.k0 = v[0];
    } else {
        const float4* keys = reinterpret_cast<const float4*>(ap.keys);
        const uint4 ct = reinterpret_cast<const uint4*>(ap.clips)[rec.x < ap.nclips ? rec.x : ap.nclips - 1u];
        const AnimPos pos = anim_position(__uint_as_float(rec.y), ct.y, ct.z);
        f.k0 = anim_load_key(keys, ct.x + pos.i0, J, j);
        f.k1 = anim_load_key(keys, ct.x + pos.i1, J, j);
        f.a = pos.a;
    }
    return f;
}

template <bool TRACKS>
__device__ __forceinline__ AnimKey anim_layer_value(const LayerFetch& f) {
    if constexpr (TRACKS) return f.k0;
    else return anim_mix(f.k0, f.k1, f.a);
}

// The (T, Q, S) of joint j of instance inst after its layer stack: layer l + 1's loads are issued before layer l's blend
// arithmetic
template <bool TRACKS>
__device__ __forceinline__ AnimKey anim_layer_tqs(const AnimLayerParams& p, uint32_t inst, uint32_t j) {
    const uint32_t L = p.nlayers;
    LayerFetch cu, nx = anim_layer_fetch<TRACKS>(p, inst, 0u, j);
    AnimKey r = {};
    for (uint32_t l = 0u; l < L; l++) {
        cu = nx;
        if (l + 1u < L) nx = anim_layer_fetch<TRACKS>(p, inst, l + 1u, j);
        if (l == 0u) {
            r = anim_layer_value<TRACKS>(cu);
        } else {
            const float e = anim_layer_weight(cu.w, cu.m);
            if (e != 0.0f) r = anim_layer_step(r, anim_layer_value<TRACKS>(cu), e, cu.mode);  // e == 0: untouched, bit for bit
        }
    }
    return r;
}

// The local matrix of joint j of instance inst from its layer stack
template <bool TRACKS>
__device__ __forceinline__ void anim_local(const AnimLayerParams& p, uint32_t inst, uint32_t j, float4 (&M)[4]) {
    anim_matrix(anim_layer_tqs<TRACKS>(p, inst, j), M);
}

__device__ __forceinline__ const PoseParams& anim_pose(const AnimParams& p) { return p.pose; }
__device__ __forceinline__ const PoseParams& anim_pose(const AnimLayerParams& p) { return p.anim.pose; }

template <bool TRACKS, class P>
__device__ __forceinline__ void anim_palettes(const P& p) {
    const PoseParams& pose = anim_pose(p);
    __shared__ float4 loc[MTR_POSE_MAX_JOINTS * 4];
    extern __shared__ uint32_t path_lds[];  // p.pose.path_bytes / 4 words
    const uint32_t inst = blockIdx.x, t = threadIdx.x, J = pose.njoints;
    if (t < J) {
        float4 M[4];
        anim_local<TRACKS>(p, inst, t, M);
#pragma unroll
        for (int c = 0; c < 4; c++) loc[t * 4 + c] = M[c];
    }
    for (uint32_t i = t; i < pose.path_bytes / 4; i += blockDim.x) path_lds[i] = pose.path_words[i];
    __syncthreads();
    if (t >= J) return;
    pose_fold_store(pose, loc, path_lds, inst, t);
}

// the local matrices themselves (mtr_anim_sample): the same sampling function, stored instead of folded
template <bool TRACKS, class P>
__device__ __forceinline__ void anim_locals(const P& p) {
    const PoseParams& pose = anim_pose(p);
    const uint32_t inst = blockIdx.x, t = threadIdx.x, J = pose.njoints;
    if (t >= J) return;
    float4 M[4];
    anim_local<TRACKS>(p, inst, t, M);
    float4* out = reinterpret_cast<float4*>(pose.out + ((size_t)inst * J + t) * 16);
#pragma unroll
    for (int c = 0; c < 4; c++) out[c] = M[c];
}

// ---- inverse kinematics (section 17) ----
// The world matrix W of joint a and the world rotation P above it, from the local matrices and rotations in LDS: the
// joint's path root first, as pose_fold_store walks it -- the same k-ordered fma chain, parent on the left, so W is bit for
// bit what the fold will produce for a.  P is the product of the rotations of the path without a itself, the identity for
// a root.  Every lane that calls it reads the same LDS addresses (broadcasts).
__device__ __forceinline__ void ik_walk(const float4* loc, const float4* rot, const uint32_t* path_lds, uint32_t pw, float4 (&W)[4], AnimVec& P) {
    const uint8_t* path = reinterpret_cast<const uint8_t*>(path_lds) + (pw & 0xFFFFu);
    const uint32_t len = pw >> 16;  // >= 1: the root first, a itself last
    uint32_t j = path[0];
#pragma unroll
    for (int c = 0; c < 4; c++) W[c] = loc[j * 4 + c];
    P = len > 1 ? rot[j] : make_float4(0.0f, 0.0f, 0.0f, 1.0f);
    for (uint32_t s = 1; s < len; s++) {
        j = path[s];
        float4 L[4], R[4];
#pragma unroll
        for (int c = 0; c < 4; c++) L[c] = loc[j * 4 + c];
        if (s + 1 < len) P = anim_qmul(P, rot[j]);
        pose_mul(W, L, R);
#pragma unroll
        for (int c = 0; c < 4; c++) W[c] = R[c];
    }
}

// One workgroup per instance, one thread per joint, as anim_palettes.  Thread j keeps the (T, Q, S) of its layer stack in
// registers and puts its local matrix into loc[] and its rotation into rot[].  Then the chains are evaluated in order.  A
// chain whose clamped weight is 0 is skipped by the whole workgroup before any other read.  Otherwise the wave that owns
// joint a walks a's path (every lane of it the same walk: broadcast reads, no divergence, nothing to share afterwards),
// solves, and lane a writes the new rotations of a and b into rot[]; after a barrier the owners of a and b take their
// rotation from rot[] and rebuild their local matrix into loc[] from their registers; a second barrier ends the chain.
// A chain whose guard fails writes nothing, and the owners rebuild the matrix they had.
//
// Memory safety, extending the argument at anim_layer_fetch: nchains is a host value validated to 1..4 and the target
// array holds ninst * nchains records of 32 bytes, so inst * nchains + k lies inside it.  From a target come the weight,
// the position and the pole, which reach no address.  The chain records come from the IK set, which mtr_anim_ik_create
// validated on the host (kind 0 or 1, every joint that is read < njoints, b and c the child and grandchild of a) and
// nothing writes afterwards; a, b and c index loc[], rot[] and paths[], all of njoints entries.  paths[] and the path bytes
// were built on the host from validated parents: an offset plus a length stays inside path_bytes, and every path byte is
// a joint < njoints.  No device-side value forms an address.
//
// ik_chains is that chain loop, shared with the spring kernels (section 24): r is the calling thread's (T, Q, S), every
// thread of the workgroup calls it (the barriers), and nchains == 0 (a spring call without an IK set) reads nothing.
__device__ __forceinline__ void ik_chains(const AnimIkParams& p, float4* loc, float4* rot, const uint32_t* path_lds, AnimKey& r, uint32_t inst, uint32_t t) {
    const uint32_t K = p.nchains;
    const uint4* chains = reinterpret_cast<const uint4*>(p.chains);
    const uint4* targets = reinterpret_cast<const uint4*>(p.targets) + (size_t)inst * K * 2;
    for (uint32_t k = 0; k < K; k++) {  // uniform for the workgroup: every barrier below is met by every wave
        const uint4 g0 = targets[k * 2];  // pos, w
        const float e = anim_weight(__uint_as_float(g0.w));
        if (e == 0.0f) continue;  // untouched, bit for bit; no other target field is read
        const uint4 g1 = targets[k * 2 + 1];  // pole, pad
        const uint4 c0 = chains[k * 2], c1 = chains[k * 2 + 1];  // kind, a, b, c | axis, flags
        const bool two = c0.x == 0u;  // MTR_IK_TWO_BONE; otherwise MTR_IK_AIM, which reads neither b nor c
        const uint32_t a = c0.y, b = c0.z;
        if ((t >> 6) == (a >> 6)) {
            float4 W[4];
            AnimVec P, qa = rot[a];
            ik_walk(loc, rot, path_lds, p.paths[a], W, P);
            const IkVec3 pa = ik_vec3(W[3].x, W[3].y, W[3].z);
            const IkVec3 g = ik_vec3(__uint_as_float(g0.x), __uint_as_float(g0.y), __uint_as_float(g0.z));
            if (two) {
                const uint32_t c = c0.w;
                float4 L[4], Wb[4], Wc[4];
#pragma unroll
                for (int i = 0; i < 4; i++) L[i] = loc[b * 4 + i];
                pose_mul(W, L, Wb);
#pragma unroll
                for (int i = 0; i < 4; i++) L[i] = loc[c * 4 + i];
                pose_mul(Wb, L, Wc);
                AnimVec qb = rot[b];
                const IkVec3 pole = ik_vec3(__uint_as_float(g1.x), __uint_as_float(g1.y), __uint_as_float(g1.z));
                const bool hit = ik_two_bone(pa, ik_vec3(Wb[3].x, Wb[3].y, Wb[3].z), ik_vec3(Wc[3].x, Wc[3].y, Wc[3].z), P, qa, qb, g, pole,
                                             (c1.w & 1u) != 0u, e);
                if (hit && t == a) { rot[a] = qa; rot[b] = qb; }
            } else {
                const IkVec3 axis = ik_vec3(__uint_as_float(c1.x), __uint_as_float(c1.y), __uint_as_float(c1.z));
                const bool hit = ik_aim(pa, P, qa, axis, g, e);
                if (hit && t == a) rot[a] = qa;
            }
        }
        __syncthreads();
        if (t == a || (two && t == b)) {
            r.q = rot[t];
            float4 M[4];
            anim_matrix(r, M);
#pragma unroll
            for (int c = 0; c < 4; c++) loc[t * 4 + c] = M[c];
        }
        __syncthreads();
    }
}

// what the IK and the spring kernels begin with: thread t's (T, Q, S) after the layer stack, its matrix and rotation in LDS,
// the path table in LDS, a barrier
template <bool TRACKS>
__device__ __forceinline__ AnimKey anim_stack_to_lds(const AnimIkParams& p, float4* loc, float4* rot, uint32_t* path_lds, uint32_t inst, uint32_t t) {
    AnimKey r = {};
    if (t < p.layers.anim.pose.njoints) {
        r = anim_layer_tqs<TRACKS>(p.layers, inst, t);
        float4 M[4];
        anim_matrix(r, M);
#pragma unroll
        for (int c = 0; c < 4; c++) loc[t * 4 + c] = M[c];
        rot[t] = r.q;
    }
    for (uint32_t i = t; i < p.path_bytes / 4; i += blockDim.x) path_lds[i] = p.path_words[i];
    __syncthreads();
    return r;
}

// and what they end with: the fold, or the local matrices themselves
template <bool FOLD>
__device__ __forceinline__ void anim_lds_out(const PoseParams& pose, const float4* loc, const uint32_t* path_lds, uint32_t inst, uint32_t t) {
    if (t >= pose.njoints) return;
    if constexpr (FOLD) {
        pose_fold_store(pose, loc, path_lds, inst, t);
    } else {
        float4* out = reinterpret_cast<float4*>(pose.out + ((size_t)inst * pose.njoints + t) * 16);
#pragma unroll
        for (int c = 0; c < 4; c++) out[c] = loc[t * 4 + c];
    }
}

template <bool TRACKS, bool FOLD>
__device__ __forceinline__ void anim_ik(const AnimIkParams& p) {
    __shared__ float4 loc[MTR_POSE_MAX_JOINTS * 4];
    __shared__ float4 rot[MTR_POSE_MAX_JOINTS];
    extern __shared__ uint32_t path_lds[];  // p.path_bytes / 4 words
    const uint32_t inst = blockIdx.x, t = threadIdx.x;
    AnimKey r = anim_stack_to_lds<TRACKS>(p, loc, rot, path_lds, inst, t);
    ik_chains(p, loc, rot, path_lds, r, inst, t);
    anim_lds_out<FOLD>(p.layers.anim.pose, loc, path_lds, inst, t);
}

__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_anim_ik(AnimIkParams p) { anim_ik<false, true>(p); }
__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_anim_ik_sample(AnimIkParams p) { anim_ik<false, false>(p); }
__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_anim_ik_tracks(AnimIkParams p) { anim_ik<true, true>(p); }
__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_anim_ik_tracks_sample(AnimIkParams p) { anim_ik<true, false>(p); }

// ---- spring bones (section 24) ----
// The shape of anim_ik: the layer stack, then the chains (ik_chains; none without an IK set), then the springs, then the
// fold.  A joint carries at most one spring, so thread t owns at most one: it simulates it itself -- it holds the joint's
// (T, Q, S) in registers, walks its own path (ik_walk), runs the rule of spring_math.h on its state record, writes rot[t]
// and rebuilds loc[t].  The springs run by ROUNDS: a spring's round is the number of spring joints among its joint's
// ancestors (the host counted it), R = 1 + the largest one is the same for the whole workgroup, and one barrier ends a
// round.  That suffices: within a round no spring joint is an ancestor of another (an ancestor has fewer spring ancestors),
// so no thread reads an entry of loc[] or rot[] that another thread of the round writes -- a walk reads the joint's ancestors
// and the joint itself --, and the joints without a spring read loc[] only in the fold, behind the last barrier.  Four
// strands of three joints cost three rounds, not twelve steps.  The spring record, the state record, the path word and the
// instance's delta depend on nothing computed, so their loads are issued ahead of the layer stack.
//
// Memory safety, extending the argument at anim_ik: joint_tab holds njoints words and t < njoints; the host built it from
// the validated springs (a spring index k < nsprings, nsprings validated to 1..16, each joint named once), so the record
// k * 3 lies inside the nsprings records of the set and the state (inst * nsprings + k) * 2 inside the ninst * nsprings
// records of 32 bytes the caller owns; two threads never share a state record.  motion is indexed by inst alone and holds
// ninst * 16 floats.  From the spring and state records, dt and motion come positions, rotations and factors, which reach
// no address; paths[t] is the host's, as for a chain.  No device-side value forms an address.
template <bool TRACKS, bool FOLD>
__device__ __forceinline__ void anim_spring(const AnimSpringParams& p) {
    const AnimIkParams& ip = p.ik;
    __shared__ float4 loc[MTR_POSE_MAX_JOINTS * 4];
    __shared__ float4 rot[MTR_POSE_MAX_JOINTS];
    extern __shared__ uint32_t path_lds[];  // ip.path_bytes / 4 words
    const uint32_t inst = blockIdx.x, t = threadIdx.x, J = ip.layers.anim.pose.njoints, R = p.nrounds;
    const uint32_t tab = t < J ? p.joint_tab[t] : MTR_SPRING_NONE;
    const bool mine = tab != MTR_SPRING_NONE;
    uint4 s0 = {}, s1 = {}, s2 = {}, st0 = {}, st1 = {};
    float4 d0 = {}, d1 = {}, d2 = {}, d3 = {};
    uint4* state = nullptr;
    uint32_t pw = 0u;
    if (mine) {
        const uint32_t k = tab & 0xFFu;
        const uint4* sp = reinterpret_cast<const uint4*>(p.springs) + k * 3;
        s0 = sp[0]; s1 = sp[1]; s2 = sp[2];  // joint, flags, stiffness, drag | tail, pad | gravity, pad
        state = reinterpret_cast<uint4*>(p.states) + ((size_t)inst * p.nsprings + k) * 2;
        st0 = state[0]; st1 = state[1];  // cur, live | prev, pad
        pw = ip.paths[t];
        if (p.motion) {
            const float4* D = reinterpret_cast<const float4*>(p.motion) + (size_t)inst * 4;
            d0 = D[0]; d1 = D[1]; d2 = D[2]; d3 = D[3];
        }
    }
    AnimKey r = anim_stack_to_lds<TRACKS>(ip, loc, rot, path_lds, inst, t);
    ik_chains(ip, loc, rot, path_lds, r, inst, t);
    for (uint32_t rd = 0; rd < R; rd++) {  // uniform for the workgroup: the barrier is met by every wave
        if (mine && (tab >> 8) == rd) {
            float4 W[4];
            AnimVec P;
            ik_walk(loc, rot, path_lds, pw, W, P);
            SpringMotion D;
            D.c0 = ik_vec3(d0.x, d0.y, d0.z); D.c1 = ik_vec3(d1.x, d1.y, d1.z); D.c2 = ik_vec3(d2.x, d2.y, d2.z); D.t = ik_vec3(d3.x, d3.y, d3.z);
            SpringState st;
            st.cur = ik_vec3(__uint_as_float(st0.x), __uint_as_float(st0.y), __uint_as_float(st0.z));
            st.live = st0.w;
            st.prev = ik_vec3(__uint_as_float(st1.x), __uint_as_float(st1.y), __uint_as_float(st1.z));
            spring_step(ik_vec3(W[3].x, W[3].y, W[3].z), P, r.q, ik_vec3(__uint_as_float(s1.x), __uint_as_float(s1.y), __uint_as_float(s1.z)),
                        ik_vec3(__uint_as_float(s2.x), __uint_as_float(s2.y), __uint_as_float(s2.z)), __uint_as_float(s0.z), __uint_as_float(s0.w), p.dt,
                        p.motion != nullptr, D, st);
            state[0] = make_uint4(__float_as_uint(st.cur.x), __float_as_uint(st.cur.y), __float_as_uint(st.cur.z), st.live);
            state[1] = make_uint4(__float_as_uint(st.prev.x), __float_as_uint(st.prev.y), __float_as_uint(st.prev.z), 0u);
            rot[t] = r.q;  // a failed guard left r.q as it was: the same matrix again
            float4 M[4];
            anim_matrix(r, M);
#pragma unroll
            for (int c = 0; c < 4; c++) loc[t * 4 + c] = M[c];
        }
        __syncthreads();
    }
    anim_lds_out<FOLD>(ip.layers.anim.pose, loc, path_lds, inst, t);
}

__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_anim_spring(AnimSpringParams p) { anim_spring<false, true>(p); }
__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_anim_spring_sample(AnimSpringParams p) { anim_spring<false, false>(p); }
__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_anim_spring_tracks(AnimSpringParams p) { anim_spring<true, true>(p); }
__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_anim_spring_tracks_sample(AnimSpringParams p) { anim_spring<true, false>(p); }

__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_anim(AnimParams p) { anim_palettes<false>(p); }
__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_anim_sample(AnimParams p) { anim_locals<false>(p); }
__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_anim_tracks(AnimParams p) { anim_palettes<true>(p); }
__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_anim_tracks_sample(AnimParams p) { anim_locals<true>(p); }
__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_anim_layers(AnimLayerParams p) { anim_palettes<false>(p); }
__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_anim_layers_sample(AnimLayerParams p) { anim_locals<false>(p); }
__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_anim_layers_tracks(AnimLayerParams p) { anim_palettes<true>(p); }
__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_anim_layers_tracks_sample(AnimLayerParams p) { anim_locals<true>(p); }

}  // namespace mtr

// One launcher per stage: the kernel by the set's kind (tracks) and by fold or sample; whether it is launched, and with how
// many threads and how much LDS for the path table, is anim_launch.h's to say.  A block per instance.
template <class P>
static void anim_launch(void (*const (&kernels)[2][2])(P), const P& p, bool tracks, bool fold, uint32_t ninst, hipStream_t s) {
    const AnimLaunchPlan plan = anim_launch_plan(p, tracks, fold, ninst);
    if (plan.ok) hipLaunchKernelGGL(kernels[tracks][fold], dim3(ninst), dim3(plan.threads), plan.lds_bytes, s, p);
}

void mtr_launch_anim(const AnimParams& p, bool tracks, bool fold, uint32_t ninst, hipStream_t s) {
    static void (*const k[2][2])(AnimParams) = {{mtr::k_anim_sample, mtr::k_anim}, {mtr::k_anim_tracks_sample, mtr::k_anim_tracks}};
    anim_launch(k, p, tracks, fold, ninst, s);
}
void mtr_launch_anim_layers(const AnimLayerParams& p, bool tracks, bool fold, uint32_t ninst, hipStream_t s) {
    static void (*const k[2][2])(AnimLayerParams) = {{mtr::k_anim_layers_sample, mtr::k_anim_layers}, {mtr::k_anim_layers_tracks_sample, mtr::k_anim_layers_tracks}};
    anim_launch(k, p, tracks, fold, ninst, s);
}
void mtr_launch_anim_ik(const AnimIkParams& p, bool tracks, bool fold, uint32_t ninst, hipStream_t s) {
    static void (*const k[2][2])(AnimIkParams) = {{mtr::k_anim_ik_sample, mtr::k_anim_ik}, {mtr::k_anim_ik_tracks_sample, mtr::k_anim_ik_tracks}};
    anim_launch(k, p, tracks, fold, ninst, s);
}
void mtr_launch_anim_spring(const AnimSpringParams& p, bool tracks, bool fold, uint32_t ninst, hipStream_t s) {
    static void (*const k[2][2])(AnimSpringParams) = {{mtr::k_anim_spring_sample, mtr::k_anim_spring}, {mtr::k_anim_spring_tracks_sample, mtr::k_anim_spring_tracks}};
    anim_launch(k, p, tracks, fold, ninst, s);
}
