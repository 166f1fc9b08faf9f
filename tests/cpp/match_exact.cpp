// match_exact.cpp -- csrc/match_math.h (the scalar rule of SPEC.md section 25) compiled for the host and put together the way
// k_match puts it together (the image of the set as mtr_anim_match_create builds it, then per instance the lead, the current
// row, the query written into the tile-major scratch, every row's chain, the maximum of the candidates' 64-bit keys, the
// decision), for tests/test_match_exact.py to compare bit for bit with the numpy model.
//   usage: match_exact <blob in> <result out>
// in : u32 n, C, R, D, flags, base, has_raw, has_filter, pose lo, pose hi, seconds, near, margin (f32 bits), 0, 0, 0; C x 4 words
//      of clips (period, flags, 0, key count); R x 4 words of rows; R x D features; D means; D scales; n x 8 words of play states;
//      n x D raw queries (has_raw); n x 2 words of filters (has_filter)
// out: n x R scores, n x 4 words of commands, n x 4 words of results
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blob_io.h"
#include <hip/hip_runtime.h>  // the stand-in of tests/cpp/hip_stub

#include "../../mt_renderer_amd/csrc/match_math.h"

using namespace mtr;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    long size = 0;
    std::vector<uint32_t> blob = read_words(argv[1], &size);
    if (blob.size() < 16) return 2;
    const size_t n = blob[0], C = blob[1], R = blob[2], D = blob[3];
    const uint32_t flags = blob[4], base = blob[5];
    const bool has_raw = blob[6] != 0, has_filter = blob[7] != 0;
    if ((long)((16 + C * 4 + R * 4 + R * D + 2 * D + n * 8 + (has_raw ? n * D : 0) + (has_filter ? n * 2 : 0)) * 4) != size || C == 0 || R == 0 || n == 0) {
        std::fprintf(stderr, "blob size\n");
        return 2;
    }
    const uint32_t* at = blob.data() + 16;
    std::vector<PlayClip> clips(C);
    std::memcpy(clips.data(), at, C * 16); at += C * 4;
    std::vector<MatchRow> rows(R);
    std::memcpy(rows.data(), at, R * 16); at += R * 4;
    const float* feats = reinterpret_cast<const float*>(at); at += R * D;
    const uint32_t Dp = match_dp((uint32_t)D);
    const size_t Rp = (R + 31) & ~(size_t)31, np = (n + 31) & ~(size_t)31;
    std::vector<float> mean(Dp, 0.0f), scale(Dp, 0.0f);
    std::memcpy(mean.data(), at, D * 4); at += D;
    std::memcpy(scale.data(), at, D * 4); at += D;
    std::vector<PlayState> play(n);
    std::memcpy(play.data(), at, n * 32); at += n * 8;
    const float* raw = has_raw ? reinterpret_cast<const float*>(at) : nullptr;
    if (has_raw) at += n * D;
    const uint32_t* filt = has_filter ? at : nullptr;
    // the image
    std::vector<uint32_t> ranges(C * 2, 0u);
    std::vector<float> c(Rp, match_float(MATCH_QNAN)), image(Rp * Dp, 0.0f), query(np * Dp, 0.0f);
    for (size_t r = 0; r < R; r++) {
        c[r] = match_c(feats + r * D, (uint32_t)D, rows[r].bias);
        for (size_t d = 0; d < D; d++) image[match_slot((uint32_t)r, (uint32_t)d, Dp)] = feats[r * D + d];
        if (rows[r].clip >= C) return 3;
        if (ranges[2 * rows[r].clip + 1] == 0u) ranges[2 * rows[r].clip] = (uint32_t)r;
        ranges[2 * rows[r].clip + 1] += 1u;
    }
    MatchTables t;
    t.clips = clips.data(); t.ranges = ranges.data(); t.rows = rows.data(); t.c = c.data(); t.feat = image.data();
    t.mean = mean.data(); t.scale = scale.data();
    t.pose_dims = (uint64_t)blob[8] | ((uint64_t)blob[9] << 32);
    t.nclips = (uint32_t)C; t.R = (uint32_t)R; t.D = (uint32_t)D; t.Dp = Dp; t.flags = flags;
    std::memcpy(&t.seconds, &blob[10], 4);
    std::memcpy(&t.near, &blob[11], 4);
    std::memcpy(&t.margin, &blob[12], 4);
    std::vector<uint32_t> out(n * R + n * 8);
    float* o_scores = reinterpret_cast<float*>(out.data());
    uint32_t* o_cmds = out.data() + n * R;
    uint32_t* o_res = o_cmds + n * 4;
    for (size_t i = 0; i < n; i++) {
        const MatchLead l = match_lead(play[i], t.nclips);
        const uint32_t cur = match_cur(t.rows, ranges[2 * l.clip], ranges[2 * l.clip + 1], l.p);
        for (size_t d = 0; d < D; d++) query[match_slot((uint32_t)i, (uint32_t)d, Dp)] = match_query(t, cur, raw ? raw + i * D : nullptr, (uint32_t)d);
        unsigned long long key = 0ull;
        for (size_t r = 0; r < R; r++) {
            const float s = match_score(t, query.data(), (uint32_t)i, (uint32_t)r);
            o_scores[i * R + r] = s;
            if (filt && !match_candidate(rows[r].tags, filt[2 * i], filt[2 * i + 1])) continue;
            const unsigned long long k = match_key(s, (uint32_t)r);
            if (k > key) key = k;
        }
        const float s_cur = cur != MTR_MATCH_NONE ? match_score(t, query.data(), (uint32_t)i, cur) : 0.0f;
        PlayCmd cmd;
        MatchResult res;
        match_decide(t, l, cur, s_cur, key, base + (uint32_t)i, cmd, res);
        std::memcpy(o_cmds + i * 4, &cmd, 16);
        std::memcpy(o_res + i * 4, &res, 16);
    }
    write_words(argv[2], out);
    return 0;
}
