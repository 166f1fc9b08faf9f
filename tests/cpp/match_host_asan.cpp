// AddressSanitizer / UBSan run of the HOST side of motion matching (csrc/host_match.cpp: mtr_anim_match_create / _destroy,
// mtr_anim_match_search_device, mtr_anim_match_search_host, mtr_anim_match_scores_host) over the stand-in HIP runtime
// (tests/cpp/hip_stub: device memory = host heap), a stand-alone program.  The k_match launcher here does what the three
// kernels do, with csrc/match_math.h on exactly the words MatchParams hands it: the query and the cleared key per instance,
// every row's chain and the maximum of the candidates' keys, the decision.  A wrong size, offset or stride on the host side
// is an ASan report, and the results are compared with a second run of the rule on the caller's copies.  Every rejected
// creation and call of include/mtr.h's table is made and must launch nothing and leave commands and results as they were,
// the error naming the clip, row or dimension; sets are created and destroyed with searches queued.
//   usage: match_host_asan <iterations>
#define MTR_RND_SEED 0x243F6A8885A308D3ull
#include "harness.h"

static uint64_t g_launches = 0;
static const void* g_last_stream = nullptr;

static mtr::MatchTables tables_of(const MatchParams& p) {
    mtr::MatchTables t;
    t.clips = reinterpret_cast<const mtr::PlayClip*>(p.clips);
    t.ranges = p.ranges;
    t.rows = reinterpret_cast<const mtr::MatchRow*>(p.rows);
    t.c = p.c; t.feat = p.feat; t.mean = p.mean; t.scale = p.scale;
    t.pose_dims = p.pose_dims;
    t.nclips = p.nclips; t.R = p.R; t.D = p.D; t.Dp = mtr::match_dp(p.D); t.flags = p.flags;
    t.seconds = p.seconds; t.near = p.near; t.margin = p.margin;
    return t;
}

void mtr_launch_match(const MatchParams& p, hipStream_t s) {
    if (!p.clips || !p.ranges || !p.rows || !p.c || !p.tags || !p.feat || !p.mean || !p.scale || !p.query || !p.cur || !p.keys || !p.play || !p.n || !p.R || !p.nclips) abort();
    if (!p.scores && !p.cmds) abort();
    if (((uintptr_t)p.clips & 15u) || ((uintptr_t)p.rows & 15u) || ((uintptr_t)p.c & 15u) || ((uintptr_t)p.tags & 15u) || ((uintptr_t)p.feat & 15u) ||
        ((uintptr_t)p.query & 15u) || ((uintptr_t)p.keys & 7u) || ((uintptr_t)p.play & 15u) || ((uintptr_t)p.raw & 15u) || ((uintptr_t)p.filter & 7u) ||
        ((uintptr_t)p.cmds & 15u) || ((uintptr_t)p.results & 15u))
        abort();
    g_launches++;
    g_last_stream = s;
    const mtr::MatchTables t = tables_of(p);
    const uint32_t np = (p.n + 31u) & ~31u;
    // k_match_query
    for (uint32_t inst = 0; inst < np; inst++) {
        if (inst >= p.n) {
            for (uint32_t d = 0; d < t.Dp; d++) p.query[mtr::match_slot(inst, d, t.Dp)] = 0.0f;
            continue;
        }
        mtr::PlayState pl;
        memcpy(&pl, p.play + (size_t)inst * 8, 32);
        const mtr::MatchLead l = mtr::match_lead(pl, p.nclips);
        const uint32_t cur = mtr::match_cur(t.rows, p.ranges[2 * l.clip], p.ranges[2 * l.clip + 1], l.p);
        for (uint32_t d = 0; d < p.D; d++) p.query[mtr::match_slot(inst, d, t.Dp)] = mtr::match_query(t, cur, p.raw ? p.raw + (size_t)inst * p.D : nullptr, d);
        for (uint32_t d = p.D; d < t.Dp; d++) p.query[mtr::match_slot(inst, d, t.Dp)] = 0.0f;
        p.cur[inst] = cur;
        p.keys[inst] = 0ull;
    }
    // k_match_search: every tile of 32 rows, the ones behind R included (c = NaN there: they never win)
    const uint32_t Rp = (p.R + 31u) & ~31u;
    for (uint32_t inst = 0; inst < p.n; inst++)
        for (uint32_t r = 0; r < Rp; r++) {
            const float sc = mtr::match_score(t, p.query, inst, r);
            if (p.scores) { if (r < p.R) p.scores[(size_t)inst * p.R + r] = sc; continue; }
            if (p.filter && !mtr::match_candidate(p.tags[r], p.filter[2 * inst], p.filter[2 * inst + 1])) continue;
            const unsigned long long k = mtr::match_key(sc, r);
            if (k > p.keys[inst]) p.keys[inst] = k;
        }
    if (p.scores) return;
    // k_match_decide
    for (uint32_t inst = 0; inst < p.n; inst++) {
        mtr::PlayState pl;
        memcpy(&pl, p.play + (size_t)inst * 8, 32);
        const mtr::MatchLead l = mtr::match_lead(pl, p.nclips);
        const uint32_t cur = p.cur[inst];
        const float s_cur = cur != MTR_MATCH_NONE ? mtr::match_score(t, p.query, inst, cur) : 0.0f;
        mtr::PlayCmd cmd;
        mtr::MatchResult res;
        mtr::match_decide(t, l, cur, s_cur, p.keys[inst], p.instance_base + inst, cmd, res);
        memcpy(p.cmds + (size_t)inst * 4, &cmd, 16);
        if (p.results) memcpy(p.results + (size_t)inst * 4, &res, 16);
    }
}

static float unit() { return (float)(rnd() % 2001) / 1000.0f - 1.0f; }
static float edge() {
    static const float e[] = {0.0f, -0.0f, 0.3f, 1.5f, 29.8f, -1e-7f, 1e30f, NAN, INFINITY, -1.0f, 0.05f, 1e-41f, 0.5f, 1.0f};
    return e[rnd() % (sizeof e / sizeof e[0])];
}

int main(int argc, char** argv) {
    const long iters = argc > 1 ? strtol(argv[1], nullptr, 10) : 40;
    mtr_device* dev = nullptr;
    if (mtr_device_create(0, &dev)) return 3;
    hipStream_t caller = nullptr, caller2 = nullptr;
    if (hipStreamCreateWithFlags(&caller, hipStreamNonBlocking) || hipStreamCreateWithFlags(&caller2, hipStreamNonBlocking)) return 3;
    const float clear[4] = {1, 1, 1, 1};
    long searched = 0, rejected = 0;
    for (long it = 0; it < iters; it++) {
        const uint32_t C = pick(1, 5), D = 4u * pick(1, it % 6 == 0 ? 16 : 4), n = pick(1, 70), cap = n + pick(0, 40);
        const uint64_t all = D == 64 ? ~0ull : (1ull << D) - 1ull;
        const uint64_t pose = it % 3 == 0 ? all : it % 3 == 1 ? 0ull : (rnd() & all);
        const bool need_query = pose != all;
        const uint32_t flags = it & 1;
        std::vector<uint32_t> nk(C), fl(C);
        for (uint32_t c = 0; c < C; c++) { nk[c] = pick(2, 40); fl[c] = (uint32_t)(rnd() & 1); }
        std::vector<mtr_match_row> rows;
        for (uint32_t c = 0; c < C; c++) {
            if (C > 1 && c == it % C) continue;  // a clip without rows
            const uint32_t k = pick(1, 12);
            const float P = (float)(nk[c] - 1);  // inside the clip with and without LOOP: the set is also created with NULL flags
            for (uint32_t j = 0; j < k; j++) rows.push_back({c, P * (float)j / (float)(k + 1), unit() * 0.1f, (uint32_t)rnd() & 0xFFu});
        }
        const uint32_t R = (uint32_t)rows.size();
        std::vector<float> feats((size_t)R * D), mean(D), scale(D);
        for (auto& v : feats) v = unit();
        for (auto& v : mean) v = unit() * 0.1f;
        for (auto& v : scale) v = 1.0f + unit() * 0.5f;
        if (R > 1) memcpy(&feats[(size_t)(R - 1) * D], &feats[0], D * 4);  // an exact tie where the biases agree
        const float seconds = 0.2f, near_x = it % 4 ? 0.5f : 0.0f, margin = it % 5 ? 0.01f : 0.0f;
        // ---- every invalid creation ----
        mtr_anim_match* none = (mtr_anim_match*)1;
        auto create = [&](size_t nclips, const uint32_t* k, const uint32_t* f, size_t d, uint64_t pd, uint32_t fg, float nr, float mg, const mtr_match_row* rw, size_t nr_,
                          const float* ft, const float* mn, const float* sc, size_t ni) {
            return mtr_anim_match_create(dev, nclips, k, f, d, pd, fg, seconds, nr, mg, rw, nr_, ft, mn, sc, ni, &none);
        };
        auto ok_but = [&](auto&& change) {
            size_t nclips = C, d = D, nrows = R, ni = cap;
            const uint32_t *k = nk.data(), *f = fl.data();
            uint64_t pd = pose; uint32_t fg = flags; float nr = near_x, mg = margin;
            const mtr_match_row* rw = rows.data();
            const float *ft = feats.data(), *mn = mean.data(), *sc = scale.data();
            change(nclips, k, f, d, pd, fg, nr, mg, rw, nrows, ft, mn, sc, ni);
            return create(nclips, k, f, d, pd, fg, nr, mg, rw, nrows, ft, mn, sc, ni);
        };
#define BUT(stmt) ok_but([&](size_t& nclips, const uint32_t*& k, const uint32_t*& f, size_t& d, uint64_t& pd, uint32_t& fg, float& nr, float& mg, const mtr_match_row*& rw, \
                             size_t& nrows, const float*& ft, const float*& mn, const float*& sc, size_t& ni) { (void)nclips; (void)k; (void)f; (void)d; (void)pd; (void)fg; \
                             (void)nr; (void)mg; (void)rw; (void)nrows; (void)ft; (void)mn; (void)sc; (void)ni; stmt; })
        EXPECT(mtr_anim_match_create(nullptr, C, nk.data(), fl.data(), D, pose, flags, seconds, near_x, margin, rows.data(), R, feats.data(), nullptr, nullptr, cap, &none), MTR_E_INVALID);
        EXPECT(mtr_anim_match_create(dev, C, nk.data(), fl.data(), D, pose, flags, seconds, near_x, margin, rows.data(), R, feats.data(), nullptr, nullptr, cap, nullptr), MTR_E_INVALID);
        EXPECT(BUT(nclips = 0), MTR_E_INVALID);
        EXPECT(BUT(nclips = ((size_t)1 << 24) + 1), MTR_E_INVALID);
        EXPECT(BUT(k = nullptr), MTR_E_INVALID);
        EXPECT(BUT(d = 0), MTR_E_INVALID);
        EXPECT(BUT(d = D + 2), MTR_E_INVALID);
        EXPECT(BUT(d = 68), MTR_E_INVALID);
        EXPECT(BUT(rw = nullptr), MTR_E_INVALID);
        EXPECT(BUT(ft = nullptr), MTR_E_INVALID);
        EXPECT(BUT(nrows = 0), MTR_E_INVALID);
        EXPECT(BUT(nrows = ((size_t)1 << 22) + 1), MTR_E_INVALID);
        EXPECT(BUT(ni = 0), MTR_E_INVALID);
        EXPECT(BUT(ni = ((size_t)1 << 20) + 1), MTR_E_INVALID);
        EXPECT(BUT(fg = flags | (2u << pick(0, 30))), MTR_E_INVALID);
        EXPECT(BUT(nr = -0.5f), MTR_E_INVALID);
        EXPECT(BUT(nr = NAN), MTR_E_INVALID);
        EXPECT(BUT(nr = INFINITY), MTR_E_INVALID);
        EXPECT(BUT(mg = -1e-3f), MTR_E_INVALID);
        EXPECT(BUT(mg = NAN), MTR_E_INVALID);
        EXPECT(BUT(mg = INFINITY), MTR_E_INVALID);
        rejected += 21;
        if (D < 64) {
            const uint32_t b = pick(D, 63);
            char want[32];
            snprintf(want, sizeof want, "dimension %u ", b);
            EXPECT(BUT(pd = pose | (1ull << b)), MTR_E_INVALID); NAMES(want);
            rejected++;
        }
        {
            const uint32_t c = pick(0, C - 1);
            char want[32];
            snprintf(want, sizeof want, "clip %u ", c);
            std::vector<uint32_t> bad_n = nk, bad_f = fl;
            bad_n[c] = rnd() & 1 ? 0u : (1u << 24) + 1u;
            bad_f[c] |= 2u << pick(0, 29);
            EXPECT(BUT(k = bad_n.data()), MTR_E_INVALID); NAMES(want);
            EXPECT(BUT(f = bad_f.data()), MTR_E_INVALID); NAMES(want);
            rejected += 2;
        }
        {
            const uint32_t r = pick(0, R - 1), dim = pick(0, D - 1);
            char want[32], wantd[32];
            snprintf(want, sizeof want, "row %u ", r);
            snprintf(wantd, sizeof wantd, "dimension %u", dim);
            std::vector<mtr_match_row> b;
            const float P = (float)(fl[rows[r].clip] ? nk[rows[r].clip] : nk[rows[r].clip] - 1);
            b = rows; b[r].clip = rnd() & 1 ? C : 0xFFFFFFFFu;
            EXPECT(BUT(rw = b.data()), MTR_E_INVALID); NAMES(want);
            b = rows; b[r].x = NAN;
            EXPECT(BUT(rw = b.data()), MTR_E_INVALID); NAMES(want);
            b = rows; b[r].x = -1e-3f;
            EXPECT(BUT(rw = b.data()), MTR_E_INVALID); NAMES(want);
            b = rows; b[r].x = fl[rows[r].clip] ? P : P + 0.5f;  // LOOP: at the period; otherwise above it
            EXPECT(BUT(rw = b.data()), MTR_E_INVALID); NAMES(want);
            b = rows; b[r].bias = rnd() & 1 ? NAN : -INFINITY;
            EXPECT(BUT(rw = b.data()), MTR_E_INVALID); NAMES(want);
            std::vector<float> bf = feats;
            bf[(size_t)r * D + dim] = rnd() & 1 ? NAN : INFINITY;
            EXPECT(BUT(ft = bf.data()), MTR_E_INVALID); NAMES(want); NAMES(wantd);
            bf = feats;
            for (uint32_t k2 = 0; k2 < D; k2++) bf[(size_t)r * D + k2] = 1.5e19f;  // finite features, a norm that is not
            EXPECT(BUT(ft = bf.data()), MTR_E_INVALID); NAMES(want);
            rejected += 7;
            if (r > 0) {
                b = rows; b[r].clip = b[r - 1].clip; b[r].x = b[r - 1].x;  // not above the row before it in its clip
                EXPECT(BUT(rw = b.data()), MTR_E_INVALID); NAMES(want);
                rejected++;
                if (rows[r - 1].clip > 0) {  // clips out of order
                    b = rows; b[r].clip = rows[r - 1].clip - 1u;
                    EXPECT(BUT(rw = b.data()), MTR_E_INVALID); NAMES(want);
                    rejected++;
                }
            }
            std::vector<float> bm = mean;
            bm[dim] = NAN;
            snprintf(wantd, sizeof wantd, "dimension %u ", dim);
            EXPECT(BUT(mn = bm.data()), MTR_E_INVALID); NAMES(wantd);
            bm = scale; bm[dim] = INFINITY;
            EXPECT(BUT(sc = bm.data()), MTR_E_INVALID); NAMES(wantd);
            rejected += 2;
        }
        if (none) { fprintf(stderr, "a failed create must clear *out\n"); return 1; }
        mtr_anim_match *mt = nullptr, *mt0 = nullptr;
        EXPECT(mtr_anim_match_create(dev, C, nk.data(), fl.data(), D, pose, flags, seconds, near_x, margin, rows.data(), R, feats.data(), mean.data(), scale.data(), cap, &mt), MTR_OK);
        EXPECT(mtr_anim_match_create(dev, C, nk.data(), nullptr, D, pose, flags, seconds, near_x, margin, rows.data(), R, feats.data(), nullptr, nullptr, cap, &mt0), MTR_OK);  // NULL flags, mean, scale
        for (uint32_t c = 0; c < C; c++) {  // the image: the clips (period, flags, 0, key count)
            float P;
            memcpy(&P, mt->d + c * 4, 4);
            CHECK(P == (float)(fl[c] ? nk[c] : nk[c] - 1) && mt->d[c * 4 + 1] == fl[c] && mt->d[c * 4 + 2] == 0 && mt->d[c * 4 + 3] == nk[c] && mt0->d[c * 4 + 1] == 0);
        }
        CHECK(same(mt->d + C * 4 + mt->w_ranges, rows.data(), (size_t)R * 16));
        // ---- inputs, exactly sized: one record too many read or written is a report ----
        std::vector<mtr_play_state> pl(n);
        for (auto& s : pl) {
            s.clip_a = rnd() % 5 ? pick(0, C - 1) : (uint32_t)rnd(); s.clip_b = rnd() % 5 ? pick(0, C - 1) : (uint32_t)rnd();
            s.x_a = rnd() & 1 ? unit() * 20.0f + 10.0f : edge(); s.x_b = rnd() & 1 ? unit() * 20.0f + 10.0f : edge();
            s.w = edge(); s.fade = rnd() & 1 ? 0.0f : edge(); s.speed = edge(); s.flags = (uint32_t)rnd();
        }
        std::vector<float> raw((size_t)n * D);
        for (auto& v : raw) v = rnd() % 16 ? unit() : edge();
        std::vector<mtr_match_filter> filt(n);
        for (auto& f : filt) { f.require = rnd() % 3 ? 0u : 1u << pick(0, 7); f.exclude = rnd() % 4 ? 0u : rnd() % 8 ? 1u << pick(0, 7) : 0xFFFFFFFFu; }
        const uint32_t base = it % 2 ? pick(0, 1000) : 0u;
        // what the rule makes of them, on copies: the launcher above on memory of the test's own
        std::vector<mtr_play_cmd> want_cm(n), want_cm_nf(n);
        std::vector<mtr_match_result> want_rs(n), want_rs_nf(n);
        std::vector<float> want_sc((size_t)n * R);
        {
            const uint32_t Dp = mtr::match_dp(D);
            const size_t np = ((size_t)n + 31) & ~(size_t)31;
            std::vector<float> q(np * Dp);
            std::vector<uint32_t> cur(n);
            std::vector<unsigned long long> keys(n);
            MatchParams p{};
            const size_t Rp = ((size_t)R + 31) & ~(size_t)31;
            p.clips = mt->d; p.ranges = mt->d + C * 4; p.rows = p.ranges + mt->w_ranges;
            p.c = reinterpret_cast<const float*>(p.rows + (size_t)R * 4); p.tags = reinterpret_cast<const uint32_t*>(p.c + Rp);
            p.feat = reinterpret_cast<const float*>(p.tags + Rp); p.mean = p.feat + Rp * Dp; p.scale = p.mean + Dp;
            float* qa = static_cast<float*>(aligned_alloc(16, q.size() * 4));
            p.query = qa; p.cur = cur.data(); p.keys = keys.data();
            mtr_play_state* pla = dev_copy(pl);
            float* rawa = dev_copy(raw);
            p.play = reinterpret_cast<const uint32_t*>(pla); p.raw = need_query ? rawa : nullptr;
            p.pose_dims = pose; p.nclips = C; p.R = R; p.D = D; p.flags = flags; p.n = n; p.seconds = seconds; p.near = near_x; p.margin = margin;
            const uint64_t keep = g_launches;
            mtr_play_cmd* cma = dev_copy(want_cm);
            mtr_match_result* rsa = dev_copy(want_rs);
            p.cmds = reinterpret_cast<uint32_t*>(cma); p.results = reinterpret_cast<uint32_t*>(rsa);
            p.filter = reinterpret_cast<const uint32_t*>(filt.data()); p.instance_base = base;
            mtr_launch_match(p, nullptr);
            memcpy(want_cm.data(), cma, (size_t)n * 16); memcpy(want_rs.data(), rsa, (size_t)n * 16);
            p.filter = nullptr; p.instance_base = 0;
            mtr_launch_match(p, nullptr);
            memcpy(want_cm_nf.data(), cma, (size_t)n * 16); memcpy(want_rs_nf.data(), rsa, (size_t)n * 16);
            p.scores = want_sc.data();
            mtr_launch_match(p, nullptr);
            g_launches = keep;
            free(qa); free(pla); free(rawa); free(cma); free(rsa);
        }
        mtr_play_state* pl_dev = dev_copy(pl);
        float* raw_dev = dev_copy(raw);
        mtr_match_filter* fl_dev = dev_copy(filt);
        std::vector<mtr_play_cmd> cm(n);
        memset(cm.data(), 0x5A, cm.size() * 16);
        mtr_play_cmd* cm_dev = dev_copy(cm);
        mtr_match_result* rs_dev = reinterpret_cast<mtr_match_result*>(dev_copy(cm));
        const float* rq = need_query ? raw_dev : nullptr;
        // ---- the valid calls ----
        EXPECT(mtr_anim_match_search_device(mt, pl_dev, rq, fl_dev, n, base, cm_dev, rs_dev, caller), MTR_OK);
        CHECK(g_last_stream == caller && mt->recorded && mt->last_stream == caller);
        CHECK(same(cm_dev, want_cm.data(), (size_t)n * 16) && same(rs_dev, want_rs.data(), (size_t)n * 16));
        CHECK(same(pl_dev, pl.data(), (size_t)n * 32));  // the play states are read only
        // another stream (a second one, or the device's own), filter and results NULL: the stream first waits for the set's
        // event, since the searches share the set's scratch, and the one event covers both when the destroy parks the image
        memset(rs_dev, 0x5A, (size_t)n * 16);
        const hipStream_t other = it & 1 ? caller2 : dev->stream;
        g_ops.clear();
        hipStubTrace() = trace;
        EXPECT(mtr_anim_match_search_device(mt, pl_dev, rq, nullptr, n, 0, cm_dev, nullptr, it & 1 ? caller2 : nullptr), MTR_OK);
        hipStubTrace() = nullptr;
        {
            bool waited = false;
            for (const Op& o : g_ops) waited |= o.op == "hipStreamWaitEvent" && o.what == mt->last && o.stream == other;
            CHECK(waited && g_last_stream == other && mt->last_stream == other);
        }
        CHECK(same(cm_dev, want_cm_nf.data(), (size_t)n * 16));
        for (size_t i = 0; i < (size_t)n * 16; i++) CHECK(reinterpret_cast<uint8_t*>(rs_dev)[i] == 0x5A);
        // the host hooks: everything in host memory, unaligned on purpose
        {
            std::vector<uint8_t> praw((size_t)n * 32 + 4), qraw(raw.size() * 4 + 5), fraw((size_t)n * 8 + 3), craw((size_t)n * 16 + 4, 0x5A), rraw((size_t)n * 16 + 2, 0x5A),
                sraw((size_t)n * R * 4 + 1);
            memcpy(praw.data() + 4, pl.data(), (size_t)n * 32);
            memcpy(qraw.data() + 1, raw.data(), raw.size() * 4);
            memcpy(fraw.data() + 3, filt.data(), (size_t)n * 8);
            EXPECT(mtr_anim_match_search_host(mt, reinterpret_cast<const mtr_play_state*>(praw.data() + 4), need_query ? reinterpret_cast<const float*>(qraw.data() + 1) : nullptr,
                                              reinterpret_cast<const mtr_match_filter*>(fraw.data() + 3), n, base, reinterpret_cast<mtr_play_cmd*>(craw.data() + 4),
                                              reinterpret_cast<mtr_match_result*>(rraw.data() + 2)), MTR_OK);
            CHECK(same(craw.data() + 4, want_cm.data(), (size_t)n * 16) && same(rraw.data() + 2, want_rs.data(), (size_t)n * 16));
            EXPECT(mtr_anim_match_scores_host(mt, reinterpret_cast<const mtr_play_state*>(praw.data() + 4), need_query ? reinterpret_cast<const float*>(qraw.data() + 1) : nullptr, n,
                                              reinterpret_cast<float*>(sraw.data() + 1)), MTR_OK);
            CHECK(same(sraw.data() + 1, want_sc.data(), want_sc.size() * 4));
        }
        searched += 4;
        // ---- every invalid call: nothing is launched, nothing changes ----
        const uint64_t launches = g_launches;
        memset(cm_dev, 0x5A, (size_t)n * 16);
        auto odd = [](auto* p, int by) { return reinterpret_cast<decltype(p)>(reinterpret_cast<char*>(p) + by); };
        EXPECT(mtr_anim_match_search_device(nullptr, pl_dev, rq, fl_dev, n, base, cm_dev, rs_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_match_search_device(mt, nullptr, rq, fl_dev, n, base, cm_dev, rs_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_match_search_device(mt, pl_dev, rq, fl_dev, n, base, nullptr, rs_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_match_search_device(mt, pl_dev, rq, fl_dev, 0, base, cm_dev, rs_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_match_search_device(mt, pl_dev, rq, fl_dev, (size_t)cap + 1, base, cm_dev, rs_dev, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_match_search_device(mt, pl_dev, rq, fl_dev, n, 0xFFFFFFFFu - n + 1u, cm_dev, rs_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_match_search_device(mt, odd(pl_dev, 8), rq, fl_dev, n, base, cm_dev, rs_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_match_search_device(mt, pl_dev, odd(raw_dev, 4), fl_dev, n, base, cm_dev, rs_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_match_search_device(mt, pl_dev, rq, odd(fl_dev, 4), n, base, cm_dev, rs_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_match_search_device(mt, pl_dev, rq, fl_dev, n, base, odd(cm_dev, 8), rs_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_match_search_device(mt, pl_dev, rq, fl_dev, n, base, cm_dev, odd(rs_dev, 4), caller), MTR_E_INVALID);
        EXPECT(mtr_anim_match_search_host(nullptr, pl.data(), raw.data(), nullptr, n, 0, cm.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_match_search_host(mt, nullptr, raw.data(), nullptr, n, 0, cm.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_match_search_host(mt, pl.data(), raw.data(), nullptr, n, 0, nullptr, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_match_search_host(mt, pl.data(), raw.data(), nullptr, 0, 0, cm.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_match_scores_host(mt, pl.data(), raw.data(), n, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_match_scores_host(nullptr, pl.data(), raw.data(), n, want_sc.data()), MTR_E_INVALID);
        rejected += 17;
        if (need_query) {
            uint32_t first = 0;
            while ((pose >> first) & 1u) first++;
            char want[32];
            snprintf(want, sizeof want, "dimension %u ", first);
            EXPECT(mtr_anim_match_search_device(mt, pl_dev, nullptr, fl_dev, n, base, cm_dev, rs_dev, caller), MTR_E_INVALID); NAMES(want);
            EXPECT(mtr_anim_match_search_host(mt, pl.data(), nullptr, nullptr, n, 0, cm.data(), nullptr), MTR_E_INVALID); NAMES(want);
            rejected += 2;
        }
        CHECK(launches == g_launches && same(pl_dev, pl.data(), (size_t)n * 32));
        for (size_t i = 0; i < (size_t)n * 16; i++) CHECK(reinterpret_cast<uint8_t*>(cm_dev)[i] == 0x5A && reinterpret_cast<uint8_t*>(rs_dev)[i] == 0x5A && reinterpret_cast<uint8_t*>(cm.data())[i] == 0x5A);
        // ---- sets created and destroyed with searches queued; a frame collects the garbage ----
        for (int k = 0; k < 3; k++) {
            mtr_anim_match* tmp = nullptr;
            EXPECT(mtr_anim_match_create(dev, C, nk.data(), fl.data(), D, pose, flags, seconds, near_x, margin, rows.data(), R, feats.data(), mean.data(), scale.data(), cap, &tmp), MTR_OK);
            for (int q = 0; q < k; q++) {
                EXPECT(mtr_anim_match_search_device(tmp, pl_dev, rq, q ? fl_dev : nullptr, n, base, cm_dev, q ? rs_dev : nullptr, q ? caller : caller2), MTR_OK);
                searched++;
            }
            mtr_anim_match_destroy(tmp);  // straight after the call: the kernels are queued (k == 0: never searched)
            mtr_frame* f = nullptr;
            EXPECT(mtr_frame_begin(dev, 64, 48, clear, 1.0f, &f), MTR_OK);
            EXPECT(mtr_frame_submit(f), MTR_OK);
            EXPECT(mtr_frame_wait(f), MTR_OK);
            mtr_frame_destroy(f);
        }
        mtr_anim_match_destroy(mt);
        mtr_anim_match_destroy(mt0);
        mtr_anim_match_destroy(nullptr);
        free(pl_dev); free(raw_dev); free(fl_dev); free(cm_dev); free(rs_dev);
    }
    hipStreamDestroy(caller);
    hipStreamDestroy(caller2);
    mtr_device_destroy(dev);
    printf("searched=%ld rejected=%ld launches=%llu failed=%d\n", searched, rejected, (unsigned long long)g_launches, g_failed);
    return g_failed ? 1 : 0;
}
