// k_ctrl.hip -- controllers (SPEC.md section 21): what each instance plays next is decided on the device.  A controller is a
// graph of nodes and transitions shared by all instances; per instance a 16-byte state and a row of float parameters live
// in device memory.  One call per frame evaluates the transitions of each instance's node in priority order (the any-state
// ones first) against its parameters and its play state, which is read and never written, and writes command slot `inst` of
// an n-slot mtr_play_cmd list: the command of the transition that fired, or one the player ignores.  The next
// mtr_anim_player_advance_device_cmds consumes the list.  Every scalar rule lives in ctrl_math.h, which the host test
// compiles too.
//
// Lanes.  One lane per instance, 256-thread workgroups, no LDS, no barrier, no cross-lane traffic, no spin-wait.  The work is
// memory-bound: a lane loads its state as one 16-byte word and its play state as two, the table entry of its lead clip and
// its node as one 16-byte word each, and per candidate a transition as up to three 16-byte words (the tables are a few
// cache lines that every lane shares; the second and third word are loaded only for a candidate that is not skipped); a user
// parameter is loaded where a condition names it (a wave's rows are contiguous, nparams * 4 bytes each, at most 64).  It
// stores the state and the command as one 16-byte word each, a parameter as 4 bytes where CONSUME names it, and adds 1 to
// one counter where a transition fired and counters were given: at most 16 + 32 + 64 bytes in and 16 + 16 out per instance
// besides the tables.  The candidate loop runs to each lane's own count, nany + the node's; lanes of a wave whose nodes
// differ diverge there and nowhere else.
//
// Memory safety.  n (1..2^27) is a host value, validated; a lane whose index is >= n returns before any access.  The state,
// play-state and command arrays hold n records, the parameter array n rows of nparams floats, and all are indexed by the
// lane's own instance only.  From device memory come (a) state.node, clamped to nnodes - 1 in ctrl_step before it reaches
// the node table, and (b) clip_a and clip_b of the play state, clamped to nclips - 1 before they reach the clip table.
// Everything else that reaches an address was validated when the controller was created and is immutable since: a node's
// clip < nclips and its range of transitions inside [nany, ntrans], a transition's target < nnodes and ncond <= 3, a
// condition's parameter < nparams unless it is a built-in.  The counters hold ntrans words and are indexed by the index of
// the transition that fired, < ntrans by the same validation.  Times, positions, values and dt reach no address.
#include "mtr_internal.h"
#include "ctrl_math.h"

namespace mtr {

__global__ __launch_bounds__(256) void k_ctrl(CtrlParams p) {
    const uint32_t inst = blockIdx.x * 256u + threadIdx.x;
    if (inst >= p.n) return;
    uint4* sp = reinterpret_cast<uint4*>(p.states) + inst;
    const uint4* pp = reinterpret_cast<const uint4*>(p.play) + (size_t)inst * 2;
    const uint4 s = sp[0], p0 = pp[0], p1 = pp[1];
    CtrlState st;
    st.node = s.x; st.t = __uint_as_float(s.y); st.fired = s.z; st.user = s.w;
    PlayState pl;
    pl.clip_a = p0.x; pl.clip_b = p0.y; pl.x_a = __uint_as_float(p0.z); pl.x_b = __uint_as_float(p0.w);
    pl.w = __uint_as_float(p1.x); pl.fade = __uint_as_float(p1.y); pl.speed = __uint_as_float(p1.z); pl.flags = p1.w;
    CtrlTables tb;
    tb.nodes = reinterpret_cast<const CtrlWord*>(p.nodes);
    tb.trans = reinterpret_cast<const CtrlWord*>(p.trans);
    tb.clips = reinterpret_cast<const PlayClip*>(p.clips);
    tb.nnodes = p.nnodes; tb.nany = p.nany; tb.nclips = p.nclips; tb.nparams = p.nparams;
    float* row = p.params ? p.params + (size_t)inst * p.nparams : nullptr;
    const CtrlStep r = ctrl_step(st, pl, row, inst, p.dt, tb);
    sp[0] = make_uint4(st.node, __float_as_uint(st.t), st.fired, st.user);
    reinterpret_cast<uint4*>(p.cmds)[inst] = make_uint4(r.cmd.instance, r.cmd.clip, __float_as_uint(r.cmd.x), __float_as_uint(r.cmd.seconds));
    if (p.counts && r.fired != MTR_CTRL_NONE) atomicAdd(p.counts + r.fired, 1u);
}

}  // namespace mtr

void mtr_launch_ctrl(const CtrlParams& p, hipStream_t s) {
    if (p.n == 0 || p.nnodes == 0 || p.nclips == 0) return;
    hipLaunchKernelGGL(mtr::k_ctrl, dim3((p.n + 255u) / 256u), dim3(256), 0, s, p);
}
