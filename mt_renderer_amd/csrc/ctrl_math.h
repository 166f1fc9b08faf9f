// ctrl_math.h -- the scalar rule of SPEC.md section 21 (controllers) that k_ctrl.hip is made of: the clamp of the node, the
// lead of the play state and the built-in values made from it, the candidates in priority order with their skips, the
// conditions, and what a fire and no fire store.  Plain C++ besides the macro, like play_math.h, so that
// tests/test_ctrl_exact.py compiles this very source for the host (-ffp-contract=off) and compares it bit for bit with the
// numpy model of section 21.
//
// One rounded operation per operator; the section rounds two of them (the quotient x_l / P_l and, with SYNC, its product with
// P_c) and one sum (t + dtp).  NaN compares false, and NE is IEEE !=, true against NaN.
//
// Registers.  A transition is read as three 16-byte words and its three conditions sit at fixed places in them, so nothing
// here indexes a local array with a value known only at run time: user parameters are read from memory where a condition
// names them and the tables are read through pointers.
#pragma once
#include "play_math.h"

#ifndef MTR_CTRL_MAX_COND  // include/mtr.h has the same
#define MTR_CTRL_MAX_COND 3
#define MTR_TR_INTERRUPT 1u
#define MTR_TR_SELF 2u
#define MTR_TR_SYNC 4u
#define MTR_TR_CONSUME 8u
#define MTR_CTRL_TIME 0xFFFFu
#define MTR_CTRL_POS 0xFFFEu
#define MTR_CTRL_PHASE 0xFFFDu
#define MTR_CTRL_ENDED 0xFFFCu
#define MTR_CTRL_FADING 0xFFFBu
#define MTR_CTRL_NONE 0xFFFFFFFFu
#endif

namespace mtr {

enum : uint32_t { CTRL_OP_LT = 0, CTRL_OP_LE = 1, CTRL_OP_GT = 2, CTRL_OP_GE = 3, CTRL_OP_EQ = 4, CTRL_OP_NE = 5 };

// one 16-byte word of a table
struct alignas(16) CtrlWord {
    uint32_t x, y, z, w;
};

// mtr_ctrl_state, 16 bytes
struct alignas(16) CtrlState {
    uint32_t node;
    float t;
    uint32_t fired, user;
};

// The tables of a controller, immutable and validated at creation: nodes of one word {clip < nclips, first, count, pad} with
// nany <= first and first + count <= ntrans; transitions of three words {target < nnodes, flags, seconds, x}, {ncond <= 3,
// pad, cond 0}, {cond 1, cond 2}, a condition being {param | op << 16, value} with op <= 5 and param < nparams or a
// built-in; clips as a player set holds them (period, flags, 0, key count).
struct CtrlTables {
    const CtrlWord* nodes;
    const CtrlWord* trans;
    const PlayClip* clips;
    uint32_t nnodes, nany, nclips, nparams;
};

// what a step hands to the player and to the counters: command slot `inst`, and the index of the transition that fired
struct CtrlStep {
    PlayCmd cmd;
    uint32_t fired;  // MTR_CTRL_NONE: none
};

MTR_HD float ctrl_float(uint32_t u) {
    union { uint32_t u; float f; } c;
    c.u = u;
    return c.f;
}

// what the step knows of the play state: step 2 of section 21
struct CtrlLead {
    float t, x, phase, ended, fading, period;
    bool running;
};

// v op value for one condition word pair; params: the instance's row, read only where the condition names a user parameter
MTR_HD bool ctrl_cond(uint32_t po, uint32_t value_bits, const CtrlLead& l, const float* params) {
    const uint32_t p = po & 0xFFFFu, op = po >> 16;
    const float value = ctrl_float(value_bits);
    float v;
    if (p == MTR_CTRL_TIME) v = l.t;
    else if (p == MTR_CTRL_POS) v = l.x;
    else if (p == MTR_CTRL_PHASE) v = l.phase;
    else if (p == MTR_CTRL_ENDED) v = l.ended;
    else if (p == MTR_CTRL_FADING) v = l.fading;
    else v = params[p];
    switch (op) {
    case CTRL_OP_LT: return v < value;
    case CTRL_OP_LE: return v <= value;
    case CTRL_OP_GT: return v > value;
    case CTRL_OP_GE: return v >= value;
    case CTRL_OP_EQ: return v == value;
    default: return v != value;
    }
}

// CONSUME: the user parameter a condition names is stored as +0.0
MTR_HD void ctrl_consume(uint32_t po, float* params) {
    const uint32_t p = po & 0xFFFFu;
    if (p < MTR_CTRL_FADING) params[p] = 0.0f;
}

// Steps 1 to 6 of section 21 for one instance.  st: the stored state, rewritten; play: its play state, read only; params: its
// row of nparams floats (nullptr when nparams == 0), written only by CONSUME.
MTR_HD CtrlStep ctrl_step(CtrlState& st, const PlayState& play, float* params, uint32_t inst, float dt, const CtrlTables& tb) {
    // 1. node
    const uint32_t node = st.node < tb.nnodes - 1u ? st.node : tb.nnodes - 1u;
    // 2. lead
    const uint32_t top = tb.nclips - 1u;
    const uint32_t ca = play.clip_a < top ? play.clip_a : top, cb = play.clip_b < top ? play.clip_b : top;
    CtrlLead l;
    l.running = play.fade > 0.0f;
    const PlayClip lc = tb.clips[l.running ? cb : ca];
    l.t = st.t;
    l.x = l.running ? play.x_b : play.x_a;
    l.period = lc.period;
    l.phase = l.x / l.period;
    l.ended = (!(lc.flags & MTR_CLIP_LOOP) && l.x >= l.period) ? 1.0f : 0.0f;
    l.fading = l.running ? 1.0f : 0.0f;
    // 3. candidates: the any-state transitions, then the node's own
    const CtrlWord nd = tb.nodes[node];
    const uint32_t ncand = tb.nany + nd.z;
    CtrlStep r;
    r.fired = MTR_CTRL_NONE;
    for (uint32_t j = 0; j < ncand; j++) {
        const bool any = j < tb.nany;
        const uint32_t idx = any ? j : nd.y + (j - tb.nany);
        const CtrlWord* tp = tb.trans + (size_t)idx * 3;
        const CtrlWord w0 = tp[0];
        if (l.running && !(w0.y & MTR_TR_INTERRUPT)) continue;
        if (any && w0.x == node && !(w0.y & MTR_TR_SELF)) continue;
        const CtrlWord w1 = tp[1], w2 = tp[2];
        const uint32_t nc = w1.x;
        if (nc > 0u && !ctrl_cond(w1.z, w1.w, l, params)) continue;
        if (nc > 1u && !ctrl_cond(w2.x, w2.y, l, params)) continue;
        if (nc > 2u && !ctrl_cond(w2.z, w2.w, l, params)) continue;
        // 4. fire
        const uint32_t c = tb.nodes[w0.x].x;
        float x = ctrl_float(w0.w);
        if (w0.y & MTR_TR_SYNC) x = l.phase * tb.clips[c].period;
        r.cmd.instance = inst; r.cmd.clip = c; r.cmd.x = x; r.cmd.seconds = ctrl_float(w0.z);
        if (w0.y & MTR_TR_CONSUME) {
            if (nc > 0u) ctrl_consume(w1.z, params);
            if (nc > 1u) ctrl_consume(w2.x, params);
            if (nc > 2u) ctrl_consume(w2.z, params);
        }
        st.node = w0.x; st.t = 0.0f; st.fired = idx;
        r.fired = idx;
        return r;
    }
    // 5. no fire
    r.cmd.instance = 0xFFFFFFFFu; r.cmd.clip = 0u; r.cmd.x = 0.0f; r.cmd.seconds = 0.0f;
    const float dtp = dt > 0.0f ? dt : 0.0f;
    st.node = node; st.t = st.t + dtp; st.fired = MTR_CTRL_NONE;
    return r;
}

}  // namespace mtr
