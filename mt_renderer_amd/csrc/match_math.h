// match_math.h -- the scalar rule of SPEC.md section 25 (motion matching) that k_match.hip is made of: where a feature or a
// query component lies in the tile-major image, the lead of the play state, the search for the current row, the query, the
// reference chain of a score, the order key of the arg-max and the decision.  Plain C++ besides the macro, like ctrl_math.h,
// so that tests/test_match_exact.py compiles this very source for the host (-ffp-contract=off) and compares it bit for bit
// with the numpy model of section 25.
//
// One rounded operation per operator; every fused multiply-add is an explicit fmaf.  NaN compares false, which every test
// below is written for.
#pragma once
#include "play_math.h"

#ifndef MTR_MATCH_INTERRUPT  // include/mtr.h has the same
#define MTR_MATCH_INTERRUPT 1u
#define MTR_MATCH_NONE 0xFFFFFFFFu
#define MTR_MATCH_MAX_DIMS 64
#endif

namespace mtr {

// mtr_match_row, 16 bytes
struct alignas(16) MatchRow {
    uint32_t clip;
    float x, bias;
    uint32_t tags;
};

// mtr_match_result, 16 bytes
struct alignas(16) MatchResult {
    uint32_t row, cur;
    float score, cur_score;
};

// The tables of a match set, immutable and validated at creation, and the scratch its three launches share.
struct MatchTables {
    const PlayClip* clips;   // nclips
    const uint32_t* ranges;  // nclips x {first row, row count}
    const MatchRow* rows;    // R, sorted by clip, x strictly increasing within a clip
    const float* c;          // Rp: c_r, NaN behind R
    const float* feat;       // Rp x Dp floats, tile-major (match_slot), zero behind R and behind D
    const float* mean;       // D
    const float* scale;      // D
    uint64_t pose_dims;
    uint32_t nclips, R, D, Dp, flags;
    float seconds, near, margin;
};

constexpr uint32_t MATCH_QNAN = 0x7FC00000u;

MTR_HD uint32_t match_bits(float f) {
    union { float f; uint32_t u; } c;
    c.f = f;
    return c.u;
}
MTR_HD float match_float(uint32_t u) {
    union { uint32_t u; float f; } c;
    c.u = u;
    return c.f;
}

// D rounded up to the 8 dimensions one 16-byte load of a lane covers; the dimensions behind D hold zeroes on both sides, and
// fmaf(0, 0, s) is s for every s but -0, which the rule reads as +0 anyway
MTR_HD uint32_t match_dp(uint32_t D) { return (D + 7u) & ~7u; }

// Where component d of row (or instance) r lies in a tile-major image of Dp dimensions: tiles of 32 rows; in a tile, groups
// of 8 dimensions; in a group, 64 lanes of 4 floats.  Lane l of a wave holds, as float j of its 16 bytes, dimension
// 8g + 2j + (l >> 5) of row (l & 31): operand k = l >> 5 of k-step 4g + j of v_mfma_f32_32x32x2_f32.
MTR_HD size_t match_slot(uint32_t r, uint32_t d, uint32_t Dp) {
    const uint32_t tile = r >> 5, g = d >> 3, j = (d & 7u) >> 1, lane = (r & 31u) + ((d & 1u) << 5);
    return (((size_t)tile * (Dp >> 3) + g) * 64u + lane) * 4u + j;
}

// c_r = -(0.5 * n2 + bias), n2 the fma chain of f_d * f_d from 0 in d order; f: the row's D features, row-major
inline float match_c(const float* f, uint32_t D, float bias) {
    float n2 = 0.0f;
    for (uint32_t d = 0; d < D; d++) n2 = fmaf(f[d], f[d], n2);
    const float h = 0.5f * n2;
    return -(h + bias);
}

// step 1: what plays
struct MatchLead {
    uint32_t clip;
    float p;
    bool running;
};
MTR_HD MatchLead match_lead(const PlayState& play, uint32_t nclips) {
    const uint32_t top = nclips - 1u;
    MatchLead l;
    l.running = play.fade > 0.0f;
    const uint32_t c = l.running ? play.clip_b : play.clip_a;
    l.clip = c < top ? c : top;
    l.p = l.running ? play.x_b : play.x_a;
    return l;
}

// step 1: the row of the lead clip with the largest x <= p, or MTR_MATCH_NONE (no rows, p NaN, p below the first row).  x is
// strictly increasing, so the answer is first + (the number of rows with x <= p) - 1 however it is counted: a 16-way search
// whose up to 16 pivots per round are independent loads, five rounds for 65 536 rows where a binary search has 16 dependent ones.
MTR_HD uint32_t match_cur(const MatchRow* rows, uint32_t first, uint32_t count, float p) {
    uint32_t lo = 0u, n = count;  // rows [0, lo) are <= p, rows [lo + n, count) are not
    while (n > 0u) {
        const uint32_t step = (n + 15u) >> 4;
        float v[16];  // pivots lo + k * step - 1, k = 1..16; those past the range read its last row instead: no load waits for a test
        for (uint32_t k = 1u; k <= 16u; k++) v[k - 1u] = rows[first + lo + (k * step <= n ? k * step : n) - 1u].x;
        uint32_t c = 0u;  // how many pivots inside the range are <= p: a prefix of them
        for (uint32_t k = 1u; k <= 16u; k++) c += (k * step <= n && v[k - 1u] <= p) ? 1u : 0u;
        const uint32_t rest = n - c * step;
        lo += c * step;
        n = rest < step ? rest : step - 1u;  // behind the last pivot, or before the first pivot that is not <= p
    }
    return lo ? first + lo - 1u : MTR_MATCH_NONE;
}

// step 2: component d of the query of an instance whose current row is cur; raw: its D floats, or nullptr when every
// dimension is a pose dimension (a difference, then a product)
MTR_HD float match_query(const MatchTables& t, uint32_t cur, const float* raw, uint32_t d) {
    if (cur != MTR_MATCH_NONE && ((t.pose_dims >> d) & 1u)) return t.feat[match_slot(cur, d, t.Dp)];
    const float r = raw ? raw[d] : 0.0f;
    const float diff = r - t.mean[d];
    return diff * t.scale[d];
}

// step 3: the score of row r against query slot i of the image q, the chain in d order from c_r; -0 is stored as +0
MTR_HD float match_score(const MatchTables& t, const float* q, uint32_t i, uint32_t r) {
    float s = t.c[r];
    for (uint32_t d = 0; d < t.D; d += 4u) {  // D is a multiple of 4: eight loads in flight, then four links of the chain
        float a[4], b[4];
        for (uint32_t k = 0; k < 4u; k++) { a[k] = q[match_slot(i, d + k, t.Dp)]; b[k] = t.feat[match_slot(r, d + k, t.Dp)]; }
        for (uint32_t k = 0; k < 4u; k++) s = fmaf(a[k], b[k], s);
    }
    return s + 0.0f;
}

// step 5: the order of scores as unsigned words: 0 for NaN (never wins), else increasing with s, -0 and +0 alike
MTR_HD uint32_t match_order(float s) {
    if (!(s == s)) return 0u;
    const uint32_t u = match_bits(s + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
MTR_HD float match_unorder(uint32_t k) { return match_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
// the 64-bit key slabs are joined by: the greater score wins, then the lower row; 0: no winner
MTR_HD unsigned long long match_key(float s, uint32_t row) {
    const uint32_t k = match_order(s);
    return k ? ((unsigned long long)k << 32) | (uint32_t)~row : 0ull;
}

// step 4
MTR_HD bool match_candidate(uint32_t tags, uint32_t require, uint32_t exclude) { return (tags & require) == require && (tags & exclude) == 0u; }

// steps 6 and 7 for instance i of a call: key is the joined winner key, s_cur the chain on row cur (any value when there is
// none)
MTR_HD void match_decide(const MatchTables& t, const MatchLead& l, uint32_t cur, float s_cur, unsigned long long key, uint32_t instance, PlayCmd& cmd,
                         MatchResult& res) {
    const bool have = key != 0ull;
    const uint32_t win = have ? ~(uint32_t)key : MTR_MATCH_NONE;
    const float s_win = have ? match_unorder((uint32_t)(key >> 32)) : match_float(MATCH_QNAN);
    const bool have_cur = cur != MTR_MATCH_NONE;
    res.row = win; res.cur = cur;
    res.score = s_win;
    res.cur_score = (have_cur && s_cur == s_cur) ? s_cur : match_float(MATCH_QNAN);
    bool ignore = !have;
    if (l.running && !(t.flags & MTR_MATCH_INTERRUPT)) ignore = true;
    if (!ignore) {
        const MatchRow w = t.rows[win];
        if (have_cur && w.clip == l.clip && fabsf(w.x - l.p) <= t.near) ignore = true;
        if (have_cur && s_cur == s_cur && !(s_win - s_cur > t.margin)) ignore = true;
        if (!ignore) { cmd.instance = instance; cmd.clip = w.clip; cmd.x = w.x; cmd.seconds = t.seconds; }
    }
    if (ignore) { cmd.instance = 0xFFFFFFFFu; cmd.clip = 0u; cmd.x = 0.0f; cmd.seconds = 0.0f; }
}

}  // namespace mtr
