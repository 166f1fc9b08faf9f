// event_math.h -- the scalar rule of SPEC.md section 22 (animation events) that k_events.hip is made of: the weight of a
// step, the positions a step starts and ends at, and per step the one or two ranges of the clip's sorted markers that the
// position arrives at or passes, with a direction.  The ranges come from lower / upper bound searches, never from a walk.
// Plain C++ besides the macro, like play_math.h (whose PlayClip it reuses; the clamp and the wrap of a position and the
// clamp of a weight are clip_math.h's), so that
// tests/test_events_exact.py compiles this very source for the host (-ffp-contract=off) and compares it bit for bit with
// the numpy model of section 22.
//
// One rounded operation per operator; nothing here is fused.  NaN compares false, which every test below is written for.
#pragma once
#include "play_math.h"

#ifndef MTR_EVENT_MAX_STEPS  // include/mtr.h has the same (MTR_ROOT_MAX_STEPS)
#define MTR_EVENT_MAX_STEPS 8
#endif
#define MTR_EVENT_BACKWARD 0x80000000u

namespace mtr {

// mtr_event_marker, 8 bytes
struct alignas(8) EventMarker {
    float x;
    uint32_t id;
};

// mtr_root_step, 16 bytes: what section 20 step 7 writes
struct alignas(16) EventStepIn {
    uint32_t clip;
    float x, dx, w;
};

// mtr_anim_event, 16 bytes
struct alignas(16) EventRecord {
    uint32_t instance, id, where;
    float w;
};

// the tables of an event set, all validated at creation and immutable: nclips >= 1 clips (period and flags are read),
// per clip {first, count} with first + count <= the marker total, and the markers, clip after clip, x non-decreasing per clip
struct EventTables {
    const PlayClip* clips;
    const uint32_t* ranges;  // nclips x 2 words
    const EventMarker* markers;
    uint32_t nclips;
};

// what a step fires: the markers [lo0, hi0) and then [lo1, hi1) (indices into EventTables::markers), each range walked
// upwards when the step runs forward and downwards when it runs backward; `where` is the word of the records
struct EventSpans {
    uint32_t lo0, hi0, lo1, hi1;
    uint32_t where;
    MTR_HD uint32_t count() const { return (hi0 - lo0) + (hi1 - lo1); }
};

// how many of the n markers at m lie below v (x < v), and how many do not lie above it (x <= v)
MTR_HD uint32_t event_lower(const EventMarker* m, uint32_t n, float v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (m[mid].x < v) lo = mid + 1u; else hi = mid;
    }
    return lo;
}
MTR_HD uint32_t event_upper(const EventMarker* m, uint32_t n, float v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (m[mid].x <= v) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// The weights of an instance's S steps (1..8): E[i] = e_i (1 - e_{i+1}) ... (1 - e_{S-1}) with e_0 = 1 and e_i the clamped
// w of step i, the products taken in increasing index; returns the mask of the steps that fire at all: e_i != 0 (i >= 1)
// and E_i >= min_weight.  w: the S raw weights; w[0] is not read.
MTR_HD uint32_t event_weights(const float* w, uint32_t S, float min_weight, float* E) {
    float e[MTR_EVENT_MAX_STEPS];
    e[0] = 1.0f;
#pragma unroll
    for (uint32_t i = 1; i < MTR_EVENT_MAX_STEPS; i++) e[i] = i < S ? anim_weight(w[i]) : 0.0f;
    uint32_t live = 0;
#pragma unroll
    for (uint32_t i = 0; i < MTR_EVENT_MAX_STEPS; i++) {
        float p = e[i];
#pragma unroll
        for (uint32_t j = i + 1; j < MTR_EVENT_MAX_STEPS; j++)
            if (j < S) p = p * (1.0f - e[j]);
        E[i] = p;
        if (i < S && (i == 0 || e[i] != 0.0f) && p >= min_weight) live |= 1u << i;
    }
    return live;
}

// The ranges of step i of an instance.  The clip index is clamped; everything else that reaches an address is a search
// result inside the clip's own range of markers.
MTR_HD EventSpans event_spans(const EventStepIn& s, uint32_t i, const EventTables& t) {
    const uint32_t top = t.nclips - 1u, c = s.clip < top ? s.clip : top;
    const float x = s.x, dx = s.dx;
    const bool fwd = dx > 0.0f, back = dx < 0.0f;
    EventSpans r;
    r.lo0 = r.hi0 = r.lo1 = r.hi1 = 0u;
    r.where = c | (i << 24) | (back ? MTR_EVENT_BACKWARD : 0u);
    if (!fwd && !back) return r;  // +-0 and NaN
    const uint32_t first = t.ranges[2u * c], n = t.ranges[2u * c + 1u];
    if (n == 0u) return r;
    const PlayClip pc = t.clips[c];
    const EventMarker* m = t.markers + first;
    const float P = pc.period;
    uint32_t lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
    if (!(pc.flags & MTR_CLIP_LOOP)) {
        const float a = clip_clamp(x, P), y = x + dx, b = clip_clamp(y, P);
        if (fwd) { lo0 = event_upper(m, n, a); hi0 = event_upper(m, n, b); }  // (a, b]
        else { lo0 = event_lower(m, n, b); hi0 = event_lower(m, n, a); }       // [b, a)
    } else {
        const float r0 = clip_wrap(x, P), y = r0 + dx;
        if (fabsf(dx) >= P) {  // a cycle or more: every marker once, from behind r0 round to r0
            const uint32_t k = fwd ? event_upper(m, n, r0) : event_lower(m, n, r0);
            if (fwd) { lo0 = k; hi0 = n; lo1 = 0; hi1 = k; }
            else { lo0 = 0; hi0 = k; lo1 = k; hi1 = n; }
        } else if (fwd) {
            lo0 = event_upper(m, n, r0);
            if (y < P) hi0 = event_upper(m, n, y);
            else { hi0 = n; lo1 = 0; hi1 = event_upper(m, n, y - P); }
        } else {
            hi0 = event_lower(m, n, r0);
            if (y >= 0.0f) lo0 = event_lower(m, n, y);
            else { lo0 = 0; lo1 = event_lower(m, n, y + P); hi1 = n; }
        }
    }
    if (hi0 < lo0) hi0 = lo0;  // an inverted interval is empty
    if (hi1 < lo1) hi1 = lo1;
    r.lo0 = first + lo0; r.hi0 = first + hi0; r.lo1 = first + lo1; r.hi1 = first + hi1;
    return r;
}

// the raw weights of an instance's steps, for event_weights
MTR_HD void event_load_weights(const EventStepIn* steps, uint32_t S, float* w) {
#pragma unroll
    for (uint32_t i = 0; i < MTR_EVENT_MAX_STEPS; i++) w[i] = (i >= 1u && i < S) ? steps[i].w : 0.0f;
}

// how many events the S steps of an instance fire
MTR_HD uint32_t event_count(const EventStepIn* steps, uint32_t S, float min_weight, const EventTables& t) {
    float w[MTR_EVENT_MAX_STEPS], E[MTR_EVENT_MAX_STEPS];
    event_load_weights(steps, S, w);
    const uint32_t live = event_weights(w, S, min_weight, E);
    uint32_t total = 0;
    for (uint32_t i = 0; i < S; i++)
        if (live & (1u << i)) total += event_spans(steps[i], i, t).count();
    return total;
}

// The events of an instance in their order: step after step, range 0 then range 1, each in its direction.  emit(marker,
// where, w) is called once per event; returns their number.
template <class Emit>
MTR_HD uint32_t event_walk(const EventStepIn* steps, uint32_t S, float min_weight, const EventTables& t, Emit&& emit) {
    float w[MTR_EVENT_MAX_STEPS], E[MTR_EVENT_MAX_STEPS];
    event_load_weights(steps, S, w);
    const uint32_t live = event_weights(w, S, min_weight, E);
    uint32_t total = 0;
    for (uint32_t i = 0; i < S; i++) {
        if (!(live & (1u << i))) continue;
        const EventSpans sp = event_spans(steps[i], i, t);
        const bool back = (sp.where & MTR_EVENT_BACKWARD) != 0u;
        float Ei = E[0];  // E[i] by selects: the array stays in registers
#pragma unroll
        for (uint32_t k = 1; k < MTR_EVENT_MAX_STEPS; k++) Ei = i == k ? E[k] : Ei;
        for (uint32_t part = 0; part < 2u; part++) {
            const uint32_t lo = part ? sp.lo1 : sp.lo0, hi = part ? sp.hi1 : sp.hi0;
            for (uint32_t k = lo; k < hi; k++) emit(t.markers[back ? hi - 1u - (k - lo) : k], sp.where, Ei);
        }
        total += sp.count();
    }
    return total;
}

}  // namespace mtr
