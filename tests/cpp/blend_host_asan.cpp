// AddressSanitizer / UBSan run of the HOST side of blend spaces (csrc/host_blend.cpp: mtr_anim_blend_create / _destroy,
// mtr_anim_blend_advance_device, mtr_anim_blend_advance_host) over the stand-in HIP runtime (tests/cpp/hip_stub: device memory
// = host heap), a stand-alone program.  The k_blend launcher here does what the kernel does, with csrc/blend_math.h on exactly
// the words BlendParams hands it.  A wrong size, offset or stride on the host side is an ASan report, and the results are
// compared with a second run of the rule on the caller's copies.  Every rejected creation and call of include/mtr.h's table is
// made and must launch nothing and leave the states, the layers, the steps and the shares as they were, the error naming the
// clip, the sample or the triangle; sets are created and destroyed with calls queued.
//   usage: blend_host_asan <iterations>
#define MTR_RND_SEED 0x13198A2E03707344ull
#include "harness.h"

static uint64_t g_launches = 0;
static const void* g_last_stream = nullptr;

// the rule on the words of p
static void run_rule(const BlendParams& p) {
    mtr::BlendTables t;
    t.clips = reinterpret_cast<const mtr::PlayClip*>(p.clips);
    t.samples = reinterpret_cast<const mtr::BlendSample*>(p.samples);
    t.tris = reinterpret_cast<const mtr::BlendTri*>(p.tris);
    t.nclips = p.nclips; t.nsamples = p.nsamples; t.ntris = p.ntris;
    t.param_x = p.param_x; t.param_y = p.param_y; t.nparams = p.nparams; t.damp = p.damp;
    for (uint32_t i = 0; i < p.n; i++) {
        mtr::BlendState st;
        memcpy(&st, p.states + (size_t)i * 4, 16);
        const uint32_t speed = p.states[(size_t)i * 4 + 3];
        const mtr::BlendFrame f = mtr::blend_advance(st, p.params + (size_t)i * p.nparams, p.dt, t);
        memcpy(p.states + (size_t)i * 4, &st, 12);
        p.states[(size_t)i * 4 + 3] = speed;
        for (uint32_t s = 0; s < 3; s++) {
            if (p.out_layers) {
                uint32_t* l = p.out_layers + ((size_t)i * p.nlayers + s) * 4;
                l[0] = f.clip[s]; memcpy(l + 1, &f.x[s], 4); memcpy(l + 2, &f.e[s], 4); l[3] = 0u;
            }
            if (p.out_steps) {
                uint32_t* q = p.out_steps + ((size_t)i * 3 + s) * 4;
                q[0] = f.clip[s]; memcpy(q + 1, &f.x0[s], 4); memcpy(q + 2, &f.dx[s], 4); memcpy(q + 3, &f.e[s], 4);
            }
            if (p.out_shares) p.out_shares[(size_t)i * 3 + s] = f.share[s];
        }
    }
}

void mtr_launch_blend(const BlendParams& p, hipStream_t s) {
    if (!p.clips || !p.samples || !p.states || !p.params || !p.n || !p.nclips || !p.nsamples || p.nsamples > 32 || p.ntris > 64 || !p.nparams || p.nparams > 16) abort();
    if (p.param_x >= p.nparams || p.param_y >= p.nparams || (p.out_layers && (p.nlayers < 3 || p.nlayers > 8)) || !(p.damp > 0.0f)) abort();
    if (((uintptr_t)p.clips & 15u) || ((uintptr_t)p.samples & 15u) || ((uintptr_t)p.tris & 15u) || ((uintptr_t)p.states & 15u) || ((uintptr_t)p.params & 3u) ||
        ((uintptr_t)p.out_layers & 15u) || ((uintptr_t)p.out_steps & 15u) || ((uintptr_t)p.out_shares & 3u))
        abort();
    g_launches++;
    g_last_stream = s;
    run_rule(p);
}

static float unit() { return (float)(rnd() % 100001) / 100000.0f; }
static float edge() {
    static const float e[] = {0.0f, -0.0f, 0.3f, 1.5f, 0.99f, -1e-7f, 1e30f, NAN, INFINITY, -INFINITY, -1.0f, 0.05f, 1e-41f, -1e-41f, 0.5f, 1.0f, -0.37f, 3e38f};
    return e[rnd() % (sizeof e / sizeof e[0])];
}

int main(int argc, char** argv) {
    const long iters = argc > 1 ? strtol(argv[1], nullptr, 10) : 40;
    mtr_device* dev = nullptr;
    if (mtr_device_create(0, &dev)) return 3;
    hipStream_t caller = nullptr, caller2 = nullptr;
    if (hipStreamCreateWithFlags(&caller, hipStreamNonBlocking) || hipStreamCreateWithFlags(&caller2, hipStreamNonBlocking)) return 3;
    const float clear[4] = {1, 1, 1, 1};
    long advanced = 0, rejected = 0;
    for (long it = 0; it < iters; it++) {
        const bool two_d = it % 2 == 1;
        const uint32_t C = pick(1, 4), NP = pick(two_d ? 2 : 1, 16), n = it % 4 == 3 ? pick(257, 600) : pick(1, 70), maxn = n + pick(0, 300);
        const uint32_t nl = pick(3, 8), px = pick(0, NP - 1), py = (px + 1) % NP;
        const float damp = it % 3 == 0 ? INFINITY : it % 3 == 1 ? 4.0f : 1e-41f, dt = it % 5 == 4 ? edge() : 1.0f / 30.0f;
        std::vector<uint32_t> nk(C), fl(C, MTR_CLIP_LOOP);
        std::vector<float> rt(C);
        for (uint32_t c = 0; c < C; c++) {
            nk[c] = rnd() % 4 ? pick(1, 40) : (1u << 24);
            rt[c] = rnd() % 5 ? 30.0f * unit() + 1.0f : -7.5f;
        }
        std::vector<mtr_blend_sample> sm;
        std::vector<mtr_blend_tri> tr;
        if (two_d) {  // a fan around sample 0: K - 1 rim points in counter-clockwise order
            const uint32_t rim = pick(3, 31);
            sm.push_back({pick(0, C - 1), 0.1f, 0.2f, 0});
            for (uint32_t k = 0; k < rim; k++) {
                const float a = 6.2831853f * (float)k / (float)rim, r = 1.0f + unit();
                sm.push_back({pick(0, C - 1), 0.1f + r * cosf(a), 0.2f + r * sinf(a), 0});
            }
            for (uint32_t k = 0; k < rim; k++) {
                const uint32_t v[3] = {0u, 1u + k, 1u + (k + 1u) % rim}, r = k % 3;
                tr.push_back({{v[r], v[(r + 1) % 3], v[(r + 2) % 3]}, 0});
            }
        } else {
            const uint32_t K = pick(1, 32);
            float x = -3.0f;
            for (uint32_t k = 0; k < K; k++) { x += 0.01f + unit(); sm.push_back({pick(0, C - 1), x, edge(), 0}); }
        }
        const uint32_t K = (uint32_t)sm.size(), T = (uint32_t)tr.size();
        const mtr_blend_tri* tp = T ? tr.data() : nullptr;
        // ---- every invalid creation ----
        mtr_anim_blend* none = (mtr_anim_blend*)1;
        auto create = [&](size_t nclips, const uint32_t* k, const uint32_t* f, const float* r, const mtr_blend_sample* s, size_t ns, const mtr_blend_tri* t, size_t nt,
                          size_t np, uint32_t x, uint32_t y, float dmp, size_t mi) { return mtr_anim_blend_create(dev, nclips, k, f, r, s, ns, t, nt, np, x, y, dmp, mi, &none); };
        EXPECT(mtr_anim_blend_create(nullptr, C, nk.data(), fl.data(), rt.data(), sm.data(), K, tp, T, NP, px, py, damp, maxn, &none), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_create(dev, C, nk.data(), fl.data(), rt.data(), sm.data(), K, tp, T, NP, px, py, damp, maxn, nullptr), MTR_E_INVALID);
        EXPECT(create(0, nk.data(), fl.data(), rt.data(), sm.data(), K, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID);
        EXPECT(create(((size_t)1 << 24) + 1, nk.data(), fl.data(), rt.data(), sm.data(), K, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID);
        EXPECT(create(C, nullptr, fl.data(), rt.data(), sm.data(), K, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), nullptr, sm.data(), K, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), rt.data(), nullptr, K, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), rt.data(), sm.data(), 0, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), rt.data(), sm.data(), 33, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), rt.data(), sm.data(), K, tp, 65, NP, px, py, damp, maxn), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), rt.data(), sm.data(), K, nullptr, 1, NP, px, py, damp, maxn), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), rt.data(), sm.data(), K, tp, T, 0, px, py, damp, maxn), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), rt.data(), sm.data(), K, tp, T, 17, px, py, damp, maxn), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), rt.data(), sm.data(), K, tp, T, NP, NP, py, damp, maxn), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), rt.data(), sm.data(), K, tp, T, NP, px, py, 0.0f, maxn), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), rt.data(), sm.data(), K, tp, T, NP, px, py, -4.0f, maxn), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), rt.data(), sm.data(), K, tp, T, NP, px, py, NAN, maxn), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), rt.data(), sm.data(), K, tp, T, NP, px, py, damp, 0), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), rt.data(), sm.data(), K, tp, T, NP, px, py, damp, ((size_t)1 << 27) + 1), MTR_E_INVALID);
        rejected += 19;
        if (two_d) { EXPECT(create(C, nk.data(), fl.data(), rt.data(), sm.data(), K, tp, T, NP, px, NP, damp, maxn), MTR_E_INVALID); rejected++; }
        {   // a clip without keys, with unknown flag bits, with a rate that is not finite
            const uint32_t c = pick(0, C - 1);
            char want[32];
            snprintf(want, sizeof want, "clip %u ", c);
            std::vector<uint32_t> bad_n = nk, bad_f = fl;
            std::vector<float> bad_r = rt;
            bad_n[c] = rnd() & 1 ? 0u : (1u << 24) + 1u;
            bad_f[c] |= 2u << pick(0, 29);
            bad_r[c] = rnd() & 1 ? NAN : INFINITY;
            EXPECT(create(C, bad_n.data(), fl.data(), rt.data(), sm.data(), K, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID); NAMES(want);
            EXPECT(create(C, nk.data(), bad_f.data(), rt.data(), sm.data(), K, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID); NAMES(want);
            EXPECT(create(C, nk.data(), fl.data(), bad_r.data(), sm.data(), K, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID); NAMES(want);
            rejected += 3;
        }
        {   // a sample on a clip the set does not have, on a clip that is not LOOP (flags given or NULL), at a position that is not finite
            const uint32_t k = pick(0, K - 1);
            char want[32];
            snprintf(want, sizeof want, "sample %u ", k);
            std::vector<mtr_blend_sample> bs = sm;
            bs[k].clip = rnd() & 1 ? C : 0xFFFFFFFFu;
            EXPECT(create(C, nk.data(), fl.data(), rt.data(), bs.data(), K, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID); NAMES(want);
            std::vector<uint32_t> bad_f = fl;
            bad_f[sm[k].clip] = 0u;
            EXPECT(create(C, nk.data(), bad_f.data(), rt.data(), sm.data(), K, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID); NAMES("sample ");
            EXPECT(create(C, nk.data(), nullptr, rt.data(), sm.data(), K, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID); NAMES("sample 0 ");
            bs = sm;
            bs[k].px = rnd() & 1 ? NAN : -INFINITY;
            EXPECT(create(C, nk.data(), fl.data(), rt.data(), bs.data(), K, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID); NAMES(want);
            rejected += 4;
            if (two_d) {
                bs = sm;
                bs[k].py = INFINITY;
                EXPECT(create(C, nk.data(), fl.data(), rt.data(), bs.data(), K, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID); NAMES(want);
                rejected++;
            } else if (K >= 2) {  // 1-D: not above the sample before it, or further above it than binary32 holds
                const uint32_t j = pick(1, K - 1);
                snprintf(want, sizeof want, "sample %u ", j);
                bs = sm;
                bs[j].px = rnd() & 1 ? bs[j - 1].px : bs[j - 1].px - 1.0f;
                EXPECT(create(C, nk.data(), fl.data(), rt.data(), bs.data(), K, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID); NAMES(want);
                bs = sm;
                for (uint32_t q = 0; q < K; q++) bs[q].px = q < j ? -3e38f + (float)q * 1e32f : 3e38f - (float)(K - q) * 1e32f;
                EXPECT(create(C, nk.data(), fl.data(), rt.data(), bs.data(), K, tp, T, NP, px, py, damp, maxn), MTR_E_INVALID); NAMES(want);
                rejected += 2;
            }
        }
        if (two_d) {  // a triangle with an index past the samples, with one twice, clockwise, without an area
            const uint32_t k = pick(0, T - 1);
            char want[32];
            snprintf(want, sizeof want, "triangle %u ", k);
            std::vector<mtr_blend_tri> bt = tr;
            bt[k].v[pick(0, 2)] = rnd() & 1 ? K : 0xFFFFFFFFu;
            EXPECT(create(C, nk.data(), fl.data(), rt.data(), sm.data(), K, bt.data(), T, NP, px, py, damp, maxn), MTR_E_INVALID); NAMES(want);
            bt = tr;
            bt[k].v[1] = bt[k].v[0];
            EXPECT(create(C, nk.data(), fl.data(), rt.data(), sm.data(), K, bt.data(), T, NP, px, py, damp, maxn), MTR_E_INVALID); NAMES(want);
            bt = tr;
            std::swap(bt[k].v[1], bt[k].v[2]);
            EXPECT(create(C, nk.data(), fl.data(), rt.data(), sm.data(), K, bt.data(), T, NP, px, py, damp, maxn), MTR_E_INVALID); NAMES(want);
            std::vector<mtr_blend_sample> bs = sm;  // the three on one line: the area is 0
            bs[tr[k].v[0]] = {sm[tr[k].v[0]].clip, 0.0f, 0.0f, 0}; bs[tr[k].v[1]] = {sm[tr[k].v[1]].clip, 1.0f, 1.0f, 0}; bs[tr[k].v[2]] = {sm[tr[k].v[2]].clip, 2.0f, 2.0f, 0};
            EXPECT(create(C, nk.data(), fl.data(), rt.data(), bs.data(), K, tr.data(), T, NP, px, py, damp, maxn), MTR_E_INVALID); NAMES("triangle ");
            rejected += 4;
        }
        if (none) { fprintf(stderr, "a failed create must clear *out\n"); return 1; }
        mtr_anim_blend* bl = nullptr;
        EXPECT(mtr_anim_blend_create(dev, C, nk.data(), fl.data(), rt.data(), sm.data(), K, tp, T, NP, px, py, damp, maxn, &bl), MTR_OK);
        {   // the image: the clips (period, flags, rate, key count), the samples, the triangles
            for (uint32_t c = 0; c < C; c++) {
                float P, r;
                memcpy(&P, bl->d + c * 4, 4);
                memcpy(&r, bl->d + c * 4 + 2, 4);
                CHECK(P == (float)nk[c] && bl->d[c * 4 + 1] == MTR_CLIP_LOOP && r == rt[c] && bl->d[c * 4 + 3] == nk[c]);
            }
            for (uint32_t k = 0; k < K; k++) CHECK(bl->d[(C + k) * 4] == sm[k].clip && same(bl->d + (C + k) * 4 + 1, &sm[k].px, 4) && bl->d[(C + k) * 4 + 3] == 0);
            for (uint32_t k = 0; k < T; k++) CHECK(same(bl->d + (C + K + k) * 4, tr[k].v, 12) && bl->d[(C + K + k) * 4 + 3] == 0);
            CHECK(bl->nsamples == K && bl->ntris == T && bl->nparams == NP && bl->param_x == px && bl->max_instances == maxn);
        }
        // ---- inputs, exactly sized: one record too many read or written is a report ----
        std::vector<mtr_blend_state> st(n);
        std::vector<float> pr((size_t)n * NP);
        for (auto& s : st) {
            s.phase = rnd() % 3 ? unit() : edge();
            s.px = rnd() % 4 ? 2.0f * unit() - 1.0f : edge();
            s.py = rnd() % 4 ? 2.0f * unit() - 1.0f : edge();
            s.speed = rnd() % 4 ? 2.0f * unit() - 0.5f : edge();
        }
        for (auto& v : pr) v = rnd() % 5 ? 5.0f * unit() - 2.5f : edge();
        std::vector<mtr_anim_layer> ly((size_t)n * nl);
        memset(ly.data(), 0x5A, ly.size() * 16);
        std::vector<mtr_root_step> sp((size_t)n * 3);
        memset(sp.data(), 0x5A, sp.size() * 16);
        std::vector<float> sh((size_t)n * 3, 7.0f);
        // what the rule makes of them, on copies
        std::vector<mtr_blend_state> want_st = st;
        std::vector<mtr_anim_layer> want_ly = ly;
        std::vector<mtr_root_step> want_sp = sp;
        std::vector<float> want_sh = sh;
        {
            BlendParams p{};
            p.clips = bl->d; p.samples = bl->d + C * 4; p.tris = p.samples + K * 4;
            p.states = reinterpret_cast<uint32_t*>(want_st.data()); p.params = pr.data();
            p.out_layers = reinterpret_cast<uint32_t*>(want_ly.data()); p.out_steps = reinterpret_cast<uint32_t*>(want_sp.data()); p.out_shares = want_sh.data();
            p.nclips = C; p.nsamples = K; p.ntris = T; p.nparams = NP; p.param_x = px; p.param_y = two_d ? py : 0; p.nlayers = nl; p.n = n; p.damp = damp; p.dt = dt;
            run_rule(p);
            for (uint32_t i = 0; i < n; i++)  // layers 3.. are not touched, the speed is never written
                CHECK(same(&want_ly[(size_t)i * nl + 3], &ly[(size_t)i * nl + 3], (size_t)(nl - 3) * 16) && same(&want_st[i].speed, &st[i].speed, 4));
        }
        mtr_blend_state* st_dev = dev_copy(st);
        float* pr_dev = dev_copy(pr);
        mtr_anim_layer* ly_dev = dev_copy(ly);
        mtr_root_step* sp_dev = dev_copy(sp);
        float* sh_dev = dev_copy(sh);
        // ---- the valid calls ----
        EXPECT(mtr_anim_blend_advance_device(bl, st_dev, pr_dev, n, dt, ly_dev, nl, sp_dev, sh_dev, caller), MTR_OK);
        CHECK(g_last_stream == caller && bl->recorded && bl->last_stream == caller);
        CHECK(same(st_dev, want_st.data(), (size_t)n * 16) && same(ly_dev, want_ly.data(), ly.size() * 16) && same(sp_dev, want_sp.data(), sp.size() * 16));
        CHECK(same(sh_dev, want_sh.data(), sh.size() * 4) && same(pr_dev, pr.data(), pr.size() * 4));  // the parameters are read only
        // another stream (a second one, or the device's own), the layers and the shares NULL: they stay, and the stream first
        // waits for the set's event, so that one event covers every reader and the destroy can park the set behind it
        memcpy(st_dev, st.data(), (size_t)n * 16);
        memcpy(ly_dev, ly.data(), ly.size() * 16);
        memcpy(sp_dev, sp.data(), sp.size() * 16);
        memcpy(sh_dev, sh.data(), sh.size() * 4);
        const hipStream_t other = it & 1 ? caller2 : dev->stream;
        g_ops.clear();
        hipStubTrace() = trace;
        EXPECT(mtr_anim_blend_advance_device(bl, st_dev, pr_dev, n, dt, nullptr, 0, sp_dev, nullptr, it & 1 ? caller2 : nullptr), MTR_OK);
        hipStubTrace() = nullptr;
        {
            bool waited = false;
            for (const Op& o : g_ops) waited |= o.op == "hipStreamWaitEvent" && o.what == bl->last && o.stream == other;
            CHECK(waited && g_last_stream == other && bl->last_stream == other);
        }
        CHECK(same(st_dev, want_st.data(), (size_t)n * 16) && same(ly_dev, ly.data(), ly.size() * 16) && same(sp_dev, want_sp.data(), sp.size() * 16));
        CHECK(same(sh_dev, sh.data(), sh.size() * 4));
        // the host hook: everything in host memory, unaligned on purpose; layers 3.. come back as they went in
        {
            std::vector<uint8_t> sraw((size_t)n * 16 + 4), praw(pr.size() * 4 + 5), lraw(ly.size() * 16 + 4), qraw(sp.size() * 16 + 4), hraw(sh.size() * 4 + 5);
            memcpy(sraw.data() + 4, st.data(), (size_t)n * 16);
            memcpy(praw.data() + 1, pr.data(), pr.size() * 4);
            memcpy(lraw.data() + 4, ly.data(), ly.size() * 16);
            memcpy(qraw.data() + 4, sp.data(), sp.size() * 16);
            memcpy(hraw.data() + 1, sh.data(), sh.size() * 4);
            EXPECT(mtr_anim_blend_advance_host(bl, reinterpret_cast<mtr_blend_state*>(sraw.data() + 4), reinterpret_cast<const float*>(praw.data() + 1), n, dt,
                                               reinterpret_cast<mtr_anim_layer*>(lraw.data() + 4), nl, reinterpret_cast<mtr_root_step*>(qraw.data() + 4),
                                               reinterpret_cast<float*>(hraw.data() + 1)), MTR_OK);
            CHECK(same(sraw.data() + 4, want_st.data(), (size_t)n * 16) && same(lraw.data() + 4, want_ly.data(), ly.size() * 16));
            CHECK(same(qraw.data() + 4, want_sp.data(), sp.size() * 16) && same(hraw.data() + 1, want_sh.data(), sh.size() * 4) && same(praw.data() + 1, pr.data(), pr.size() * 4));
        }
        advanced += 3;
        // ---- every invalid call: nothing is launched, nothing changes ----
        const uint64_t launches = g_launches;
        memcpy(st_dev, st.data(), (size_t)n * 16);
        memcpy(sp_dev, sp.data(), sp.size() * 16);
        auto odd = [](auto* p, int by) { return reinterpret_cast<decltype(p)>(reinterpret_cast<char*>(p) + by); };
        EXPECT(mtr_anim_blend_advance_device(nullptr, st_dev, pr_dev, n, dt, ly_dev, nl, sp_dev, sh_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_device(bl, nullptr, pr_dev, n, dt, ly_dev, nl, sp_dev, sh_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_device(bl, st_dev, nullptr, n, dt, ly_dev, nl, sp_dev, sh_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_device(bl, st_dev, pr_dev, 0, dt, ly_dev, nl, sp_dev, sh_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_device(bl, st_dev, pr_dev, (size_t)maxn + 1, dt, ly_dev, nl, sp_dev, sh_dev, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_device(bl, st_dev, pr_dev, n, dt, ly_dev, 2, sp_dev, sh_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_device(bl, st_dev, pr_dev, n, dt, ly_dev, 9, sp_dev, sh_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_device(bl, odd(st_dev, 8), pr_dev, n, dt, ly_dev, nl, sp_dev, sh_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_device(bl, st_dev, odd(pr_dev, 2), n, dt, ly_dev, nl, sp_dev, sh_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_device(bl, st_dev, pr_dev, n, dt, odd(ly_dev, 4), nl, sp_dev, sh_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_device(bl, st_dev, pr_dev, n, dt, ly_dev, nl, odd(sp_dev, 8), sh_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_device(bl, st_dev, pr_dev, n, dt, ly_dev, nl, sp_dev, odd(sh_dev, 1), caller), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_host(nullptr, st.data(), pr.data(), n, dt, ly.data(), nl, sp.data(), sh.data()), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_host(bl, nullptr, pr.data(), n, dt, ly.data(), nl, sp.data(), sh.data()), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_host(bl, st.data(), nullptr, n, dt, ly.data(), nl, sp.data(), sh.data()), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_host(bl, st.data(), pr.data(), 0, dt, ly.data(), nl, sp.data(), sh.data()), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_host(bl, st.data(), pr.data(), (size_t)maxn + 1, dt, ly.data(), nl, sp.data(), sh.data()), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_host(bl, st.data(), pr.data(), n, dt, ly.data(), 2, sp.data(), sh.data()), MTR_E_INVALID);
        EXPECT(mtr_anim_blend_advance_host(bl, st.data(), pr.data(), n, dt, ly.data(), 9, sp.data(), sh.data()), MTR_E_INVALID);
        rejected += 19;
        CHECK(launches == g_launches && same(st_dev, st.data(), (size_t)n * 16) && same(ly_dev, ly.data(), ly.size() * 16) && same(sp_dev, sp.data(), sp.size() * 16));
        CHECK(same(sh_dev, sh.data(), sh.size() * 4) && same(pr_dev, pr.data(), pr.size() * 4) && sh[0] == 7.0f);
        // ---- sets created and destroyed with calls queued; a frame collects the garbage ----
        for (int k = 0; k < 3; k++) {
            mtr_anim_blend* tmp = nullptr;
            EXPECT(mtr_anim_blend_create(dev, C, nk.data(), fl.data(), rt.data(), sm.data(), K, tp, T, NP, px, py, damp, maxn, &tmp), MTR_OK);
            for (int q = 0; q < k; q++) {
                EXPECT(mtr_anim_blend_advance_device(tmp, st_dev, pr_dev, n, dt, q ? ly_dev : nullptr, nl, sp_dev, q ? nullptr : sh_dev, q ? caller : caller2), MTR_OK);
                advanced++;
            }
            mtr_anim_blend_destroy(tmp);  // straight after the call: the kernel is queued (k == 0: never used)
            mtr_frame* f = nullptr;
            EXPECT(mtr_frame_begin(dev, 64, 48, clear, 1.0f, &f), MTR_OK);
            EXPECT(mtr_frame_submit(f), MTR_OK);
            EXPECT(mtr_frame_wait(f), MTR_OK);
            mtr_frame_destroy(f);
        }
        mtr_anim_blend_destroy(bl);
        mtr_anim_blend_destroy(nullptr);
        free(st_dev); free(pr_dev); free(ly_dev); free(sp_dev); free(sh_dev);
    }
    hipStreamDestroy(caller);
    hipStreamDestroy(caller2);
    mtr_device_destroy(dev);
    printf("advanced=%ld rejected=%ld launches=%llu failed=%d\n", advanced, rejected, (unsigned long long)g_launches, g_failed);
    return g_failed ? 1 : 0;
}
