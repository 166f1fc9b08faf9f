// host_match.cpp -- motion matching (SPEC.md section 25): the match set, its validated rows and the device image of its
// features, and the search calls that run k_match on play states, queries and filters in device memory.
#include "host.h"
#include "match_math.h"

// k_match.hip.  Weak: the host-only builds of this file (tests/cpp, over the HIP stub runtime) link no kernels; libmtr.so
// links k_match.o.
void mtr_launch_match(const MatchParams& p, hipStream_t s) __attribute__((weak));

namespace mtr_host {

namespace {

constexpr size_t kMatchMaxInstances = (size_t)1 << 20, kMatchMaxRows = (size_t)1 << 22;

size_t pad4(size_t words) { return (words + 3) & ~(size_t)3; }

// what every search call checks before it touches anything; device: the pointers are device memory and must be aligned
int32_t match_check(const mtr_anim_match* m, const void* play, const void* query, const void* filter, size_t n, uint32_t instance_base, const void* cmds,
                    const void* results, bool device) {
    mtr_device* d = m->dev;
    if (!play || !cmds) return fail(d, MTR_E_INVALID, "match search: no play states or no commands");
    if (n == 0 || n > m->max_instances) return fail(d, MTR_E_INVALID, "match search: 1 to max_instances instances");
    if ((uint64_t)instance_base + n > 0xFFFFFFFFull) return fail(d, MTR_E_INVALID, "match search: instance_base + n lies above 2^32 - 1");
    if (!query) {
        for (uint32_t k = 0; k < m->D; k++)
            if (!((m->pose_dims >> k) & 1u))
                return fail(d, MTR_E_INVALID, "match search: no query, and dimension " + std::to_string(k) + " is not a pose dimension");
    }
    if (device) {
        if (((uintptr_t)play & 15u) || ((uintptr_t)query & 15u) || ((uintptr_t)cmds & 15u) || ((uintptr_t)results & 15u))
            return fail(d, MTR_E_INVALID, "match search: device play states, queries, commands and results must be 16-byte aligned");
        if ((uintptr_t)filter & 7u) return fail(d, MTR_E_INVALID, "match search: device filters must be 8-byte aligned");
    }
    if (!mtr_launch_match) return fail(d, MTR_E_UNSUPPORTED, "match search: built without k_match");
    return set_device(d);
}

// the three launches of k_match on `s` between the set's events: they write the set's scratch, so a call on another stream
// than the one before first waits for it, and the destroy parks the image behind the one event (DeviceSet::last)
int32_t match_launch(mtr_anim_match* m, const void* play_dev, const float* query_dev, const void* filter_dev, size_t n, uint32_t instance_base, void* cmds_dev,
                     void* results_dev, float* scores_dev, hipStream_t s) {
    mtr_device* d = m->dev;
    int32_t rc = set_before(m, s);
    if (rc) return rc;
    const size_t Rp = (m->R + 31u) & ~(size_t)31, Dp = mtr::match_dp(m->D), np = (m->max_instances + 31u) & ~(size_t)31;
    MatchParams mp{};
    mp.clips = m->d;
    mp.ranges = mp.clips + (size_t)m->nclips * 4;
    mp.rows = mp.ranges + m->w_ranges;
    mp.c = reinterpret_cast<const float*>(mp.rows + (size_t)m->R * 4);
    mp.tags = reinterpret_cast<const uint32_t*>(mp.c + Rp);
    mp.feat = reinterpret_cast<const float*>(mp.tags + Rp);
    mp.mean = mp.feat + Rp * Dp;
    mp.scale = mp.mean + Dp;
    mp.query = const_cast<float*>(mp.scale + Dp);
    mp.cur = reinterpret_cast<uint32_t*>(mp.query + np * Dp);
    mp.keys = reinterpret_cast<unsigned long long*>(mp.cur + pad4(m->max_instances));
    mp.play = static_cast<const uint32_t*>(play_dev);
    mp.raw = query_dev;
    mp.filter = static_cast<const uint32_t*>(filter_dev);
    mp.cmds = static_cast<uint32_t*>(cmds_dev);
    mp.results = static_cast<uint32_t*>(results_dev);
    mp.scores = scores_dev;
    mp.pose_dims = m->pose_dims;
    mp.nclips = m->nclips; mp.R = m->R; mp.D = m->D; mp.flags = m->flags; mp.n = (uint32_t)n; mp.instance_base = instance_base;
    mp.seconds = m->seconds; mp.near = m->near_x; mp.margin = m->margin;
    mtr_launch_match(mp, s);
    HIPCHK(d, hipGetLastError());
    return set_after(m, s);
}

}  // namespace

}  // namespace mtr_host

using namespace mtr_host;

extern "C" {

static_assert(sizeof(mtr_match_row) == 16 && sizeof(mtr_match_filter) == 8 && sizeof(mtr_match_result) == 16, "mtr_match_row, mtr_match_filter, mtr_match_result");

int32_t mtr_anim_match_create(mtr_device* d, size_t nclips, const uint32_t* nkeys, const uint32_t* clip_flags, size_t D, uint64_t pose_dims, uint32_t flags,
                              float seconds, float near_x, float margin, const mtr_match_row* rows, size_t nrows, const float* features, const float* mean,
                              const float* scale, size_t max_instances, mtr_anim_match** out) {
    if (!d || !out) return MTR_E_INVALID;
    *out = nullptr;
    if (nclips == 0 || nclips > kClipMaxKeys) return fail(d, MTR_E_INVALID, "anim match: 1 to 2^24 clips");
    if (!nkeys) return fail(d, MTR_E_INVALID, "anim match: no key counts");
    if (D < 4 || D > MTR_MATCH_MAX_DIMS || (D & 3u)) return fail(d, MTR_E_INVALID, "anim match: the dimensions are a multiple of 4 in 4 to 64");
    if (!rows || !features || nrows == 0 || nrows > kMatchMaxRows) return fail(d, MTR_E_INVALID, "anim match: 1 to 2^22 rows with their features");
    if (max_instances == 0 || max_instances > kMatchMaxInstances) return fail(d, MTR_E_INVALID, "anim match: 1 to 2^20 instances");
    if (flags & ~MTR_MATCH_INTERRUPT) return fail(d, MTR_E_INVALID, "anim match: unknown flag bits");
    if (D < 64 && (pose_dims >> D)) {
        size_t k = D;
        while (!((pose_dims >> k) & 1u)) k++;
        return fail(d, MTR_E_INVALID, "anim match: pose dimension " + std::to_string(k) + " lies at or above the dimensions");
    }
    if (!(near_x >= 0.0f) || !std::isfinite(near_x) || !(margin >= 0.0f) || !std::isfinite(margin))
        return fail(d, MTR_E_INVALID, "anim match: near and margin are finite and not negative");
    const size_t Rp = (nrows + 31) & ~(size_t)31, Dp = mtr::match_dp((uint32_t)D), np = (max_instances + 31) & ~(size_t)31;
    const size_t w_ranges = pad4(nclips * 2);
    std::vector<uint32_t> head(nclips * 4 + w_ranges + nrows * 4, 0u);
    uint32_t* ranges = head.data() + nclips * 4;
    int32_t rc;
    for (size_t c = 0; c < nclips; c++)
        if ((rc = clip_entry(d, "anim match", c, nkeys, clip_flags ? clip_flags[c] : 0u, nullptr, &head[c * 4]))) return rc;
    for (size_t k = 0; k < D; k++) {
        if (mean && !std::isfinite(mean[k])) return fail(d, MTR_E_INVALID, "anim match: dimension " + std::to_string(k) + " has a mean that is not finite");
        if (scale && !std::isfinite(scale[k])) return fail(d, MTR_E_INVALID, "anim match: dimension " + std::to_string(k) + " has a scale that is not finite");
    }
    std::vector<float> body(Rp * 2 + Rp * Dp + Dp * 2, 0.0f);  // c, tags, features, mean, scale
    float* cs = body.data();
    uint32_t* tags = reinterpret_cast<uint32_t*>(cs + Rp);
    float* feat = cs + Rp * 2;
    float* mean_out = feat + Rp * Dp;
    float* scale_out = mean_out + Dp;
    for (size_t k = 0; k < D; k++) { mean_out[k] = mean ? mean[k] : 0.0f; scale_out[k] = scale ? scale[k] : 1.0f; }
    for (size_t r = 0; r < nrows; r++) {
        const mtr_match_row& row = rows[r];
        const std::string who = "anim match: row " + std::to_string(r) + " ";
        if (row.clip >= nclips) return fail(d, MTR_E_INVALID, who + "names a clip the set does not have");
        if (r > 0 && row.clip < rows[r - 1].clip) return fail(d, MTR_E_INVALID, who + "names a clip below the row before it");
        const bool loop = (clip_flags ? clip_flags[row.clip] : 0u) & MTR_CLIP_LOOP;
        float period;
        std::memcpy(&period, &head[(size_t)row.clip * 4], 4);
        if (!std::isfinite(row.x) || row.x < 0.0f || row.x > period || (loop && row.x >= period))
            return fail(d, MTR_E_INVALID, who + "has a position that is not finite or lies outside its clip");
        if (r > 0 && row.clip == rows[r - 1].clip && !(row.x > rows[r - 1].x)) return fail(d, MTR_E_INVALID, who + "does not lie above the row before it in its clip");
        if (!std::isfinite(row.bias)) return fail(d, MTR_E_INVALID, who + "has a bias that is not finite");
        const float* f = features + r * D;
        for (size_t k = 0; k < D; k++)
            if (!std::isfinite(f[k])) return fail(d, MTR_E_INVALID, who + "has a feature that is not finite in dimension " + std::to_string(k));
        const float c = mtr::match_c(f, (uint32_t)D, row.bias);
        if (!std::isfinite(c)) return fail(d, MTR_E_INVALID, who + "has a norm and bias whose sum is not finite");
        cs[r] = c;
        tags[r] = row.tags;
        for (size_t k = 0; k < D; k++) feat[mtr::match_slot((uint32_t)r, (uint32_t)k, (uint32_t)Dp)] = f[k];
        if (ranges[2 * row.clip + 1] == 0u) ranges[2 * row.clip] = (uint32_t)r;
        ranges[2 * row.clip + 1] += 1u;
        std::memcpy(&head[nclips * 4 + w_ranges + r * 4], &row, 16);
    }
    for (size_t r = nrows; r < Rp; r++) cs[r] = mtr::match_float(mtr::MATCH_QNAN);  // rows that can never win
    if ((rc = set_device(d))) return rc;
    auto m = std::make_unique<mtr_anim_match>();
    m->dev = d; m->nclips = (uint32_t)nclips; m->R = (uint32_t)nrows; m->D = (uint32_t)D; m->flags = flags; m->max_instances = (uint32_t)max_instances;
    m->pose_dims = pose_dims; m->seconds = seconds; m->near_x = near_x; m->margin = margin; m->w_ranges = w_ranges;
    const size_t scratch = (np * Dp + pad4(max_instances) + max_instances * 2) * 4;
    if ((rc = set_upload(m.get(), "anim match", {{head.data(), head.size() * 4}, {body.data(), body.size() * 4}, {nullptr, scratch}}))) return rc;
    *out = m.release();
    return MTR_OK;
}

void mtr_anim_match_destroy(mtr_anim_match* m) { set_destroy(m); }

int32_t mtr_anim_match_search_device(mtr_anim_match* m, const mtr_play_state* play_dev, const float* query_dev, const mtr_match_filter* filter_dev, size_t n,
                                     uint32_t instance_base, mtr_play_cmd* cmds_out_dev, mtr_match_result* results_dev, void* hip_stream) {
    if (!m) return MTR_E_INVALID;
    int32_t rc = match_check(m, play_dev, query_dev, filter_dev, n, instance_base, cmds_out_dev, results_dev, true);
    if (rc) return rc;
    return match_launch(m, play_dev, query_dev, filter_dev, n, instance_base, cmds_out_dev, results_dev, nullptr, caller_stream(m->dev, hip_stream));
}

int32_t mtr_anim_match_search_host(mtr_anim_match* m, const mtr_play_state* play, const float* query, const mtr_match_filter* filter, size_t n, uint32_t instance_base,
                                   mtr_play_cmd* cmds_out, mtr_match_result* results) {
    if (!m) return MTR_E_INVALID;
    mtr_device* d = m->dev;
    int32_t rc = match_check(m, play, query, filter, n, instance_base, cmds_out, results, false);
    if (rc) return rc;
    // one block: the play states, the commands, the results and the queries (16-byte words), then the filters
    StagedBlock blk(d);
    StagedPart &p_play = blk.part(play, n * 8), &p_cmds = blk.part(cmds_out, n * 4), &p_res = blk.part(results, results ? n * 4 : 0),
               &p_query = blk.part(query, query ? n * m->D : 0), &p_filter = blk.part(filter, filter ? n * 2 : 0);
    return blk.run([&]() -> int32_t {
        int32_t r2;
        if ((r2 = blk.up({&p_play, &p_query, &p_filter})) ||
            (r2 = match_launch(m, p_play.at, p_query.dev<float>(), p_filter.dev<void>(), n, instance_base, p_cmds.at, p_res.dev<void>(), nullptr, d->s_copy)))
            return r2;
        return blk.down({&p_cmds, &p_res});
    });
}

int32_t mtr_anim_match_scores_host(mtr_anim_match* m, const mtr_play_state* play, const float* query, size_t n, float* out) {
    if (!m) return MTR_E_INVALID;
    mtr_device* d = m->dev;
    if (!out) return fail(d, MTR_E_INVALID, "match scores: no room for the scores");
    int32_t rc = match_check(m, play, query, nullptr, n, 0u, out, nullptr, false);
    if (rc) return rc;
    StagedBlock blk(d);
    StagedPart &p_play = blk.part(play, n * 8), &p_query = blk.part(query, query ? n * m->D : 0), &p_out = blk.part(out, n * m->R);
    return blk.run([&]() -> int32_t {
        int32_t r2;
        if ((r2 = blk.up({&p_play, &p_query})) ||
            (r2 = match_launch(m, p_play.at, p_query.dev<float>(), nullptr, n, 0u, nullptr, nullptr, p_out.dev<float>(), d->s_copy)))
            return r2;
        return blk.down({&p_out});
    });
}

}  // extern "C"
