// play_math.h -- the scalar rule of SPEC.md section 20 (players) that k_play.hip is made of: the clamp of the clip indices, the
// command (cut or fade), the time step, the advance of a position on a LOOP clip or a one-shot clip, the fade weight, the
// records of the frame and the state that is stored.  Plain C++ besides the macro, like root_math.h, so that
// tests/test_player_exact.py compiles this very source for the host (-ffp-contract=off) and compares it bit for bit with the
// numpy model of section 20.
//
// One rounded operation per operator; nothing here is fused (the including file is compiled with -ffp-contract=off) and '/'
// is correctly rounded.  NaN compares false, which every test below is written for.
#pragma once
#include "clip_math.h"

#ifndef MTR_PLAY_ENDED  // include/mtr.h has the same
#define MTR_PLAY_ENDED 1u
#endif

namespace mtr {

constexpr float PLAY_FLT_MAX = 3.402823466e+38f;

// one clip of a player set, 16 bytes: the period P (float(N) for a LOOP clip, float(N - 1) otherwise), the flag word,
// the rate in positions per second and the key count the period was made from
struct alignas(16) PlayClip {
    float period;
    uint32_t flags;
    float rate;
    uint32_t nkeys;
};

// mtr_play_state, 32 bytes
struct alignas(16) PlayState {
    uint32_t clip_a, clip_b;
    float x_a, x_b, w, fade, speed;
    uint32_t flags;
};

// mtr_play_cmd, 16 bytes
struct alignas(16) PlayCmd {
    uint32_t instance, clip;
    float x, seconds;
};

// what a frame writes besides the state: the clips and the weight of the frame before the swap, the advanced positions
// (pose) and the positions before the advance with their steps (motion)
struct PlayFrame {
    uint32_t clip_a, clip_b;
    float x_a, x_b, w;      // x_a', x_b' (the stored x_b where no fade runs), w_out
    float x0_a, dx_a, x0_b, dx_b;
};

// x' = adv(x, dx, clip): on a LOOP clip section 14's wrap of y = x + dx with its fallback, otherwise its clamp to [0, P]
MTR_HD float play_adv(float x, float dx, const PlayClip& c) {
    const float y = x + dx;
    return (c.flags & MTR_CLIP_LOOP) ? clip_wrap(y, c.period) : clip_clamp(y, c.period);
}

// Steps 1 to 8 of section 20 for one instance.  st: the stored state, rewritten; cmd: the one command that reaches the
// instance, or nullptr; table: nclips >= 1 entries, read through clamped indices only.
MTR_HD PlayFrame play_advance(PlayState& st, const PlayCmd* cmd, float dt, const PlayClip* table, uint32_t nclips) {
    const uint32_t top = nclips - 1u;
    // 1. clamp
    uint32_t ca = st.clip_a < top ? st.clip_a : top, cb = st.clip_b < top ? st.clip_b : top;
    float xa = st.x_a, xb = st.x_b, w = st.w, fade = st.fade;
    // 2. command
    if (cmd) {
        const uint32_t c = cmd->clip < top ? cmd->clip : top;
        const float r = 1.0f / cmd->seconds;
        if (cmd->seconds > 0.0f && r > 0.0f && r <= PLAY_FLT_MAX) {  // a fade
            if (fade > 0.0f && anim_weight(w) >= 0.5f) { ca = cb; xa = xb; }
            cb = c; xb = cmd->x; w = 0.0f; fade = r;
        } else {  // a cut
            ca = c; xa = cmd->x; w = 0.0f; fade = 0.0f;
        }
    }
    const bool running = fade > 0.0f;
    // 3. time
    float s = dt * st.speed;
    if (!(fabsf(s) <= PLAY_FLT_MAX)) s = 0.0f;
    const float dtp = dt > 0.0f ? dt : 0.0f;
    PlayFrame f;
    f.clip_a = ca; f.clip_b = cb;
    // 4. advance A
    const PlayClip ta = table[ca];
    f.dx_a = s * ta.rate;
    f.x0_a = xa;
    f.x_a = play_adv(xa, f.dx_a, ta);
    // 5. advance B, 6. weight
    const PlayClip tb = table[cb];
    float w1 = 0.0f;
    if (running) {
        f.dx_b = s * tb.rate;
        f.x0_b = xb;
        f.x_b = play_adv(xb, f.dx_b, tb);
        w1 = anim_weight(w) + dtp * fade;
        f.w = w1 > 1.0f ? 1.0f : w1;
    } else {
        f.dx_b = 0.0f;
        f.x0_b = xb;
        f.x_b = xb;
        f.w = 0.0f;
    }
    // 8. store
    st.clip_a = ca; st.clip_b = cb; st.x_b = xb; st.w = w; st.fade = fade;
    PlayClip tl = ta;
    if (running && w1 >= 1.0f) {
        st.clip_a = cb; st.x_a = f.x_b; st.w = 0.0f; st.fade = 0.0f;
        tl = tb;
    } else {
        st.x_a = f.x_a;
        if (running) { st.x_b = f.x_b; st.w = w1; }
    }
    const bool ended = !(tl.flags & MTR_CLIP_LOOP) && st.x_a >= tl.period;
    st.flags = (st.flags & ~MTR_PLAY_ENDED) | (ended ? MTR_PLAY_ENDED : 0u);
    return f;
}

}  // namespace mtr
