// anim_tracks.h -- the scalar rules of SPEC.md section 15 (animation tracks) that k_anim.hip's track source is made of:
// position -> r (and -> keys, for section 14's uniform clips), the key search with (k, k1, a), and the two key decodes.
// The wrap and the clamp of a position are clip_math.h's.  Plain C++ besides the macro, on plain
// pointers, so that tests/test_anim_tracks_exact.py compiles this very source for the host (-ffp-contract=off) and
// compares it bit for bit with the numpy model of the section.
//
// One rounded operation per operator.  The only fused operations are the two of snorm16, a spelled-out IEEE division
// by 32767 (tests/test_div_exact.py proves the sequence equal to `/` for every 16-bit code).
#pragma once
#include "clip_math.h"

namespace mtr {

// Position -> r (section 14's r, N = the clip's length in ticks, 1..65536).  For every x -- NaN, +-inf, huge, -0 --
// the result is -0 or lies in [0, N): LOOP by the explicit range test, clamp because r <= float(N - 1).
MTR_HD float track_position(float x, uint32_t nticks, uint32_t flags) {
    return (flags & MTR_CLIP_LOOP) ? clip_wrap(x, (float)nticks) : clip_clamp(x, (float)(nticks - 1u));
}

// Position -> keys for a clip of uniformly spaced keys (section 14): nkeys >= 1 keys, x in keys.  The same two rules, each
// followed by its own key pair; k_anim.hip's uniform source and root_math.h's sample call this.
struct AnimPos {
    uint32_t i0, i1;  // key indices inside the clip
    float a;          // fraction towards i1
};

MTR_HD AnimPos anim_position(float x, uint32_t nkeys, uint32_t flags) {
    AnimPos r;
    float pos;
    if (flags & MTR_CLIP_LOOP) {
        pos = clip_wrap(x, (float)nkeys);
        r.i0 = (uint32_t)floorf(pos);
        r.i1 = r.i0 + 1u == nkeys ? 0u : r.i0 + 1u;
    } else {
        pos = clip_clamp(x, (float)(nkeys - 1u));
        r.i0 = (uint32_t)floorf(pos);
        r.i1 = r.i0 + 1u < nkeys ? r.i0 + 1u : nkeys - 1u;
    }
    r.a = pos - (float)r.i0;
    return r;
}

// The search for the largest key k of the track [first, first + count) with float(times[k]) <= r, as a lower-bound loop
// whose steps are separate calls so that several searches advance together, each step's loads in flight at once.
// Invariant: float(times[base]) <= r (times[first] == 0 <= r at the start, -0 included) and the answer lies in
// [base, base + n), n >= 1; the probe base + n / 2 lies inside it.  n == 1: the step probes base itself and changes
// nothing, so a finished search may be stepped again.  A step leaves at most ceil(n / 2) keys (track_search_left).
// tk follows times[base].
struct TrackSearch {
    uint32_t base, n, tk;
};

MTR_HD TrackSearch track_search_begin(uint32_t first, uint32_t count) {
    TrackSearch s;
    s.base = first; s.n = count; s.tk = 0u;
    return s;
}

MTR_HD void track_search_step(const uint16_t* times, float r, TrackSearch& s) {
    const uint32_t half = s.n >> 1;
    const uint32_t t = times[s.base + half];
    const bool le = (float)t <= r;
    s.base = le ? s.base + half : s.base;
    s.tk = le ? t : s.tk;
    s.n -= half;
}

// The same step in two halves, for a caller that issues the probes of several searches before it uses any of them
// (root_math.h): the key the step probes, and the step taken with the time t read there.
MTR_HD uint32_t track_search_probe(const TrackSearch& s) { return s.base + (s.n >> 1); }

MTR_HD void track_search_take(uint32_t t, float r, TrackSearch& s) {
    const uint32_t half = s.n >> 1;
    const bool le = (float)t <= r;
    s.base = le ? s.base + half : s.base;
    s.tk = le ? t : s.tk;
    s.n -= half;
}

// an upper bound of n after a step, for any n up to `left`: the number of steps a loop over several searches runs
MTR_HD uint32_t track_search_left(uint32_t left) { return left - (left >> 1); }

// the key the track interpolates towards from its key k: the next one; past the last key the first one when the clip
// loops (over the ticks up to N), else k itself
MTR_HD uint32_t track_next_key(uint32_t first, uint32_t count, uint32_t k, uint32_t flags) {
    if (k + 1u < first + count) return k + 1u;
    return (flags & MTR_CLIP_LOOP) ? first : k;
}

// a, from the time of k, the time read at k1 and the clip: t1 = N on the wrap (N may be 65536: u32, not u16)
MTR_HD float track_fraction(float r, uint32_t first, uint32_t count, uint32_t k, uint32_t k1, uint32_t tk, uint32_t time_k1, uint32_t nticks) {
    if (k1 == k) return 0.0f;
    const uint32_t t1 = k + 1u < first + count ? time_k1 : nticks;
    return (r - (float)tk) / (float)(t1 - tk);  // the difference is exact (both below 2^17 with r's fraction bits to spare)
}

struct TrackPos {
    uint32_t k, k1;
    float a;
};

// the whole rule for one track, one search after the other (the host harness; the kernel interleaves the steps)
MTR_HD TrackPos track_locate(const uint16_t* times, float r, uint32_t first, uint32_t count, uint32_t nticks, uint32_t flags) {
    TrackSearch s = track_search_begin(first, count);
    while (s.n > 1u) track_search_step(times, r, s);
    TrackPos p;
    p.k = s.base;
    p.k1 = track_next_key(first, count, p.k, flags);
    p.a = track_fraction(r, first, count, p.k, p.k1, s.tk, times[p.k1], nticks);
    return p;
}

// section 2's Snorm16: max(float(v) / 32767, -1)
MTR_HD float track_snorm16(uint32_t lo16) {
    const float x = (float)(int16_t)lo16, d = 32767.0f;
    uint32_t rb = 0x38000100u;  // RN(1 / 32767)
    float r;
    __builtin_memcpy(&r, &rb, 4);
    const float q0 = x * r;
    const float q = fmaf(fmaf(-q0, d, x), r, q0);
    return q < -1.0f ? -1.0f : q;
}

// a translation / scale key (w0 = words 0 and 1, w1 = words 2 and 3 of the key, little-endian): lo + float(v) * step,
// product then sum; the fourth word is not read
MTR_HD void track_decode_lin(uint32_t w0, uint32_t w1, const float* lo, const float* step, float* out) {
    const float p0 = (float)(w0 & 0xFFFFu) * step[0], p1 = (float)(w0 >> 16) * step[1], p2 = (float)(w1 & 0xFFFFu) * step[2];
    out[0] = lo[0] + p0;
    out[1] = lo[1] + p1;
    out[2] = lo[2] + p2;
}

// a rotation key: (x, y, z, w) as Snorm16
MTR_HD void track_decode_rot(uint32_t w0, uint32_t w1, float* out) {
    out[0] = track_snorm16(w0 & 0xFFFFu);
    out[1] = track_snorm16(w0 >> 16);
    out[2] = track_snorm16(w1 & 0xFFFFu);
    out[3] = track_snorm16(w1 >> 16);
}

}  // namespace mtr
