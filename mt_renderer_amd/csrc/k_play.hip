// k_play.hip -- players (SPEC.md section 20): the library's clock.  Per instance a 32-byte play state that lives on the
// device is advanced by dt -- clip indices clamped, at most one command applied (a cut or the start of a cross-fade), the
// positions of clip A (and of clip B while a fade runs) advanced and wrapped or clamped, the fade weight moved, the clips
// swapped when the fade is complete -- and the records the animate and root-motion calls take are written: an
// mtr_anim_state, layers 0 and 1 of a layer stack, two mtr_root_steps.  Every scalar rule lives in play_math.h, which the
// host test compiles too.
//
// Lanes.  One lane per instance, 256-thread workgroups, no LDS, no barrier, no cross-lane traffic.  The work is memory-bound:
// a lane loads its state as two 16-byte words and the table entries of its two clips as one 16-byte word each (the table is
// a few cache lines that every lane shares), and stores the state as two 16-byte words, the animation state as three 8-byte
// words (24 bytes per instance: 8-byte aligned, not 16), the two layers and the two steps as two 16-byte words each: at most
// 32 bytes in and 32 + 24 + 32 + 32 out, plus 4 bytes of scratch in a call that carries commands.  The state and the
// scratch word are loaded together; the command depends on the scratch word and the table entries on the clip indices.
//
// Commands.  "The last command in array order that names an instance wins" must not depend on which thread runs first, so
// commands are resolved in two kernels.  k_play_cmds, one lane per command, does atomicMax(scratch[instance], index + 1): a
// maximum is the same whatever the order.  k_play's lane of an instance reads its word, clears it when it is not 0 and
// applies command word - 1.  The scratch array starts zeroed, every call leaves it zeroed, so a call without commands runs
// one kernel and does not read it.
//
// Memory safety.  n (1..max_instances) and nlayers (2..8) are host values, validated; a lane whose index is >= n returns
// before any access.  The state, output and scratch arrays hold n records (the scratch max_instances >= n words) and are
// indexed by the lane's own instance only.  From device memory come (a) clip_a, clip_b and a command's clip, each clamped to
// nclips - 1 in play_advance before it reaches the table, (b) a command's instance, compared with n before it indexes the
// scratch, and (c) the scratch word, which k_play_cmds makes at most ncmds and which is compared with ncmds again before
// word - 1 indexes the commands.  Positions, weights, rates and dt reach no address.
#include "mtr_internal.h"
#include "play_math.h"

namespace mtr {

__global__ __launch_bounds__(256) void k_play_cmds(const uint4* __restrict__ cmds, uint32_t ncmds, uint32_t* __restrict__ scratch, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= ncmds) return;
    const uint32_t inst = reinterpret_cast<const uint32_t*>(cmds)[(size_t)i * 4];
    if (inst < n) atomicMax(scratch + inst, i + 1u);
}

__global__ __launch_bounds__(256) void k_play(PlayParams p) {
    const uint32_t inst = blockIdx.x * 256u + threadIdx.x;
    if (inst >= p.n) return;
    uint4* sp = reinterpret_cast<uint4*>(p.states) + (size_t)inst * 2;
    const uint4 s0 = sp[0], s1 = sp[1];
    uint32_t slot = 0;
    if (p.ncmds) slot = p.scratch[inst];
    PlayState st;
    st.clip_a = s0.x; st.clip_b = s0.y; st.x_a = __uint_as_float(s0.z); st.x_b = __uint_as_float(s0.w);
    st.w = __uint_as_float(s1.x); st.fade = __uint_as_float(s1.y); st.speed = __uint_as_float(s1.z); st.flags = s1.w;
    PlayCmd cmd;
    const bool have = slot != 0u && slot <= p.ncmds;
    if (slot != 0u) p.scratch[inst] = 0u;
    if (have) {
        const uint4 c = reinterpret_cast<const uint4*>(p.cmds)[slot - 1u];
        cmd.instance = c.x; cmd.clip = c.y; cmd.x = __uint_as_float(c.z); cmd.seconds = __uint_as_float(c.w);
    }
    const PlayFrame f = play_advance(st, have ? &cmd : nullptr, p.dt, reinterpret_cast<const PlayClip*>(p.table), p.nclips);
    sp[0] = make_uint4(st.clip_a, st.clip_b, __float_as_uint(st.x_a), __float_as_uint(st.x_b));
    sp[1] = make_uint4(__float_as_uint(st.w), __float_as_uint(st.fade), __float_as_uint(st.speed), st.flags);
    const uint32_t xa = __float_as_uint(f.x_a), xb = __float_as_uint(f.x_b), w = __float_as_uint(f.w);
    if (p.out_states) {
        uint2* o = reinterpret_cast<uint2*>(p.out_states) + (size_t)inst * 3;
        o[0] = make_uint2(f.clip_a, f.clip_b);
        o[1] = make_uint2(xa, xb);
        o[2] = make_uint2(w, 0u);
    }
    if (p.out_layers) {  // clip, x, w, mask 0 and MTR_LAYER_OVERRIDE (0) in one word
        uint4* o = reinterpret_cast<uint4*>(p.out_layers) + (size_t)inst * p.nlayers;
        o[0] = make_uint4(f.clip_a, xa, 0u, 0u);
        o[1] = make_uint4(f.clip_b, xb, w, 0u);
    }
    if (p.out_steps) {  // clip, x, dx, w
        uint4* o = reinterpret_cast<uint4*>(p.out_steps) + (size_t)inst * 2;
        o[0] = make_uint4(f.clip_a, __float_as_uint(f.x0_a), __float_as_uint(f.dx_a), 0u);
        o[1] = make_uint4(f.clip_b, __float_as_uint(f.x0_b), __float_as_uint(f.dx_b), w);
    }
}

}  // namespace mtr

void mtr_launch_play(const PlayParams& p, hipStream_t s) {
    if (p.n == 0 || p.nclips == 0) return;
    if (p.ncmds) hipLaunchKernelGGL(mtr::k_play_cmds, dim3((p.ncmds + 255u) / 256u), dim3(256), 0, s, reinterpret_cast<const uint4*>(p.cmds), p.ncmds, p.scratch, p.n);
    hipLaunchKernelGGL(mtr::k_play, dim3((p.n + 255u) / 256u), dim3(256), 0, s, p);
}
