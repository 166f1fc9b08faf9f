// AddressSanitizer / UBSan run of the HOST side of controllers (csrc/host_ctrl.cpp: mtr_anim_ctrl_create / _destroy,
// mtr_anim_ctrl_step_device, mtr_anim_ctrl_step_host) over the stand-in HIP runtime (tests/cpp/hip_stub: device memory = host
// heap), a stand-alone program.  The k_ctrl launcher here does what the kernel does, with csrc/ctrl_math.h on exactly the
// words CtrlParams hands it: one ctrl_step per instance, command slot i, one count per fire.  A wrong size, offset or stride
// on the host side is an ASan report, and the results are compared with a second run of the rule on the caller's copies.
// Every rejected creation and step of include/mtr.h's table is made and must launch nothing and leave states, parameters,
// commands and counts as they were, the error naming the node or transition; controllers are created and destroyed with
// steps queued.
//   usage: ctrl_host_asan <iterations>
#define MTR_RND_SEED 0x13198A2E03707344ull
#include "harness.h"
#include "../../mt_renderer_amd/csrc/ctrl_math.h"

static uint64_t g_launches = 0;
static const void* g_last_stream = nullptr;

static mtr::CtrlTables tables_of(const CtrlParams& p) {
    mtr::CtrlTables tb;
    tb.nodes = reinterpret_cast<const mtr::CtrlWord*>(p.nodes);
    tb.trans = reinterpret_cast<const mtr::CtrlWord*>(p.trans);
    tb.clips = reinterpret_cast<const mtr::PlayClip*>(p.clips);
    tb.nnodes = p.nnodes; tb.nany = p.nany; tb.nclips = p.nclips; tb.nparams = p.nparams;
    return tb;
}

void mtr_launch_ctrl(const CtrlParams& p, hipStream_t s) {
    if (!p.nodes || !p.trans || !p.clips || !p.states || !p.play || !p.cmds || !p.n || !p.nnodes || !p.nclips) abort();
    if (((uintptr_t)p.nodes & 15u) || ((uintptr_t)p.trans & 15u) || ((uintptr_t)p.clips & 15u) || ((uintptr_t)p.states & 15u) || ((uintptr_t)p.play & 15u) ||
        ((uintptr_t)p.cmds & 15u) || ((uintptr_t)p.params & 3u) || ((uintptr_t)p.counts & 3u) || (p.nparams && !p.params))
        abort();
    g_launches++;
    g_last_stream = s;
    const mtr::CtrlTables tb = tables_of(p);
    for (uint32_t inst = 0; inst < p.n; inst++) {
        mtr::CtrlState st;
        mtr::PlayState pl;
        memcpy(&st, p.states + (size_t)inst * 4, 16);
        memcpy(&pl, p.play + (size_t)inst * 8, 32);
        const mtr::CtrlStep r = mtr::ctrl_step(st, pl, p.params ? p.params + (size_t)inst * p.nparams : nullptr, inst, p.dt, tb);
        memcpy(p.states + (size_t)inst * 4, &st, 16);
        memcpy(p.cmds + (size_t)inst * 4, &r.cmd, 16);
        if (p.counts && r.fired != MTR_CTRL_NONE) p.counts[r.fired] += 1u;
    }
}

static float edge() {
    static const float e[] = {0.0f, -0.0f, 0.3f, 1.5f, 29.8f, -1e-7f, 1e30f, NAN, INFINITY, -1.0f, 0.05f, 1e-41f, 0.5f, 1.0f};
    return e[rnd() % (sizeof e / sizeof e[0])];
}
static uint16_t some_param(uint32_t NP) {
    static const uint16_t b[] = {MTR_CTRL_TIME, MTR_CTRL_POS, MTR_CTRL_PHASE, MTR_CTRL_ENDED, MTR_CTRL_FADING};
    return NP && (rnd() & 1) ? (uint16_t)pick(0, NP - 1) : b[rnd() % 5];
}

int main(int argc, char** argv) {
    const long iters = argc > 1 ? strtol(argv[1], nullptr, 10) : 40;
    mtr_device* dev = nullptr;
    if (mtr_device_create(0, &dev)) return 3;
    hipStream_t caller = nullptr, caller2 = nullptr;
    if (hipStreamCreateWithFlags(&caller, hipStreamNonBlocking) || hipStreamCreateWithFlags(&caller2, hipStreamNonBlocking)) return 3;
    const float clear[4] = {1, 1, 1, 1};
    long stepped = 0, rejected = 0;
    for (long it = 0; it < iters; it++) {
        const uint32_t C = pick(1, 5), S = pick(1, 6), nany = it % 3 ? pick(0, 2) : 0, NP = it % 4 == 0 ? 0 : it % 4 == 1 ? 16 : pick(1, 15), n = pick(1, 70);
        std::vector<uint32_t> nk(C), fl(C);
        for (uint32_t c = 0; c < C; c++) { nk[c] = rnd() % 4 ? pick(1, 40) : (1u << 24); fl[c] = (uint32_t)(rnd() & 1); }
        std::vector<mtr_ctrl_node> nodes(S);
        std::vector<mtr_ctrl_trans> trans(nany);
        for (uint32_t s = 0; s < S; s++) {
            const uint32_t cnt = it % 5 == 4 ? 0 : pick(0, 4);
            nodes[s] = {pick(0, C - 1), (uint32_t)trans.size(), cnt, (uint32_t)rnd()};
            trans.resize(trans.size() + cnt);
        }
        const uint32_t T = (uint32_t)trans.size();
        for (auto& t : trans) {
            t.target = pick(0, S - 1); t.flags = pick(0, 15); t.seconds = edge(); t.x = edge(); t.ncond = pick(0, 3); t.pad = (uint32_t)rnd();
            for (uint32_t k = 0; k < 3; k++) {
                if (k < t.ncond) t.cond[k] = {some_param(NP), (uint16_t)pick(0, 5), edge()};
                else t.cond[k] = {(uint16_t)rnd(), (uint16_t)rnd(), edge()};  // unused: junk that nobody validates or reads
            }
        }
        const mtr_ctrl_trans* tp = T ? trans.data() : nullptr;
        // ---- every invalid creation ----
        mtr_anim_ctrl* none = (mtr_anim_ctrl*)1;
        auto create = [&](size_t nclips, const uint32_t* k, const uint32_t* f, const mtr_ctrl_node* nd, size_t ns, const mtr_ctrl_trans* tr, size_t nt, size_t na,
                          size_t np) { return mtr_anim_ctrl_create(dev, nclips, k, f, nd, ns, tr, nt, na, np, &none); };
        EXPECT(mtr_anim_ctrl_create(nullptr, C, nk.data(), fl.data(), nodes.data(), S, tp, T, nany, NP, &none), MTR_E_INVALID);
        EXPECT(mtr_anim_ctrl_create(dev, C, nk.data(), fl.data(), nodes.data(), S, tp, T, nany, NP, nullptr), MTR_E_INVALID);
        EXPECT(create(0, nk.data(), fl.data(), nodes.data(), S, tp, T, nany, NP), MTR_E_INVALID);
        EXPECT(create(((size_t)1 << 24) + 1, nk.data(), fl.data(), nodes.data(), S, tp, T, nany, NP), MTR_E_INVALID);
        EXPECT(create(C, nullptr, fl.data(), nodes.data(), S, tp, T, nany, NP), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), nullptr, S, tp, T, nany, NP), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), nodes.data(), 0, tp, T, nany, NP), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), nodes.data(), 65536, tp, T, nany, NP), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), nodes.data(), S, nullptr, T + 1, nany, NP), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), nodes.data(), S, tp, ((size_t)1 << 20) + 1, nany, NP), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), nodes.data(), S, tp, T, T + 1, NP), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), nodes.data(), S, tp, T, nany, 17), MTR_E_INVALID);
        rejected += 12;
        {
            const uint32_t c = pick(0, C - 1);
            char want[32];
            snprintf(want, sizeof want, "clip %u ", c);
            std::vector<uint32_t> bad_n = nk, bad_f = fl;
            bad_n[c] = rnd() & 1 ? 0u : (1u << 24) + 1u;
            bad_f[c] |= 2u << pick(0, 29);
            EXPECT(create(C, bad_n.data(), fl.data(), nodes.data(), S, tp, T, nany, NP), MTR_E_INVALID); NAMES(want);
            EXPECT(create(C, nk.data(), bad_f.data(), nodes.data(), S, tp, T, nany, NP), MTR_E_INVALID); NAMES(want);
            rejected += 2;
        }
        {
            const uint32_t s = pick(0, S - 1);
            char want[32];
            snprintf(want, sizeof want, "node %u ", s);
            std::vector<mtr_ctrl_node> b;
            b = nodes; b[s].clip = rnd() & 1 ? C : 0xFFFFFFFFu;
            EXPECT(create(C, nk.data(), fl.data(), b.data(), S, tp, T, nany, NP), MTR_E_INVALID); NAMES(want);
            b = nodes; b[s].first = T + 1;
            EXPECT(create(C, nk.data(), fl.data(), b.data(), S, tp, T, nany, NP), MTR_E_INVALID); NAMES(want);
            b = nodes; b[s].count = T - b[s].first + 1;
            EXPECT(create(C, nk.data(), fl.data(), b.data(), S, tp, T, nany, NP), MTR_E_INVALID); NAMES(want);
            b = nodes; b[s].first = T ? 1u : 0u; b[s].count = 0xFFFFFFFFu;  // first + count wraps to first - 1
            EXPECT(create(C, nk.data(), fl.data(), b.data(), S, tp, T, nany, NP), MTR_E_INVALID); NAMES(want);
            rejected += 4;
            if (nany) {  // a range that reaches into the any-state transitions
                b = nodes; b[s].first = nany - 1; b[s].count = 1;
                EXPECT(create(C, nk.data(), fl.data(), b.data(), S, tp, T, nany, NP), MTR_E_INVALID); NAMES(want);
                rejected++;
            }
        }
        if (T) {
            const uint32_t t = pick(0, T - 1);
            char want[32];
            snprintf(want, sizeof want, "transition %u ", t);
            std::vector<mtr_ctrl_trans> b;
            b = trans; b[t].target = rnd() & 1 ? S : 0xFFFFFFFFu;
            EXPECT(create(C, nk.data(), fl.data(), nodes.data(), S, b.data(), T, nany, NP), MTR_E_INVALID); NAMES(want);
            b = trans; b[t].flags |= 16u << pick(0, 27);
            EXPECT(create(C, nk.data(), fl.data(), nodes.data(), S, b.data(), T, nany, NP), MTR_E_INVALID); NAMES(want);
            b = trans; b[t].ncond = rnd() & 1 ? 4u : 0xFFFFFFFFu;
            EXPECT(create(C, nk.data(), fl.data(), nodes.data(), S, b.data(), T, nany, NP), MTR_E_INVALID); NAMES(want);
            b = trans; b[t].ncond = 3; for (auto& c : b[t].cond) c = {MTR_CTRL_TIME, 0, 0.0f};
            b[t].cond[pick(0, 2)].op = 6;
            EXPECT(create(C, nk.data(), fl.data(), nodes.data(), S, b.data(), T, nany, NP), MTR_E_INVALID); NAMES(want);
            b[t].cond[0].op = b[t].cond[1].op = b[t].cond[2].op = 5;
            b[t].cond[pick(0, 2)].param = rnd() & 1 ? (uint16_t)NP : (uint16_t)(MTR_CTRL_FADING - 1);
            EXPECT(create(C, nk.data(), fl.data(), nodes.data(), S, b.data(), T, nany, NP), MTR_E_INVALID); NAMES(want);
            rejected += 5;
        }
        if (none) { fprintf(stderr, "a failed create must clear *out\n"); return 1; }
        mtr_anim_ctrl *ct = nullptr, *ct0 = nullptr;
        EXPECT(mtr_anim_ctrl_create(dev, C, nk.data(), fl.data(), nodes.data(), S, tp, T, nany, NP, &ct), MTR_OK);
        EXPECT(mtr_anim_ctrl_create(dev, C, nk.data(), nullptr, nodes.data(), S, tp, T, nany, NP, &ct0), MTR_OK);  // NULL flags: all 0
        for (uint32_t c = 0; c < C; c++) {  // the image: the clips (period, flags, 0, key count), the nodes, the transitions
            float P;
            memcpy(&P, ct->d + c * 4, 4);
            CHECK(P == (float)(fl[c] ? nk[c] : nk[c] - 1) && ct->d[c * 4 + 1] == fl[c] && ct->d[c * 4 + 2] == 0 && ct->d[c * 4 + 3] == nk[c] && ct0->d[c * 4 + 1] == 0);
        }
        CHECK(same(ct->d + C * 4, nodes.data(), S * 16) && (T == 0 || same(ct->d + C * 4 + S * 4, trans.data(), (size_t)T * 48)));
        // ---- inputs, exactly sized: one record too many read or written is a report ----
        std::vector<mtr_ctrl_state> st(n);
        for (auto& s : st) { s.node = rnd() % 5 ? pick(0, S - 1) : (uint32_t)rnd(); s.t = edge(); s.fired = (uint32_t)rnd(); s.user = (uint32_t)rnd(); }
        std::vector<mtr_play_state> pl(n);
        for (auto& s : pl) { s.clip_a = rnd() % 5 ? pick(0, C - 1) : (uint32_t)rnd(); s.clip_b = rnd() % 5 ? pick(0, C - 1) : (uint32_t)rnd(); s.x_a = edge(); s.x_b = edge(); s.w = edge(); s.fade = rnd() & 1 ? 0.0f : edge(); s.speed = edge(); s.flags = (uint32_t)rnd(); }
        std::vector<float> pr((size_t)n * NP);
        for (auto& v : pr) v = edge();
        std::vector<uint32_t> cnt(T);
        for (auto& v : cnt) v = pick(0, 9);
        const float dt = it % 7 == 3 ? 0.0f : it % 7 == 5 ? -1.0f / 30 : 1.0f / 30;
        // what the rule makes of them, on copies
        std::vector<mtr_ctrl_state> want = st;
        std::vector<float> want_pr = pr;
        std::vector<mtr_play_cmd> want_cm(n);
        std::vector<uint32_t> want_cnt = cnt;
        {
            CtrlParams p{};
            p.clips = ct->d; p.nodes = ct->d + C * 4; p.trans = p.nodes + S * 4; p.nnodes = S; p.nany = nany; p.nclips = C; p.nparams = NP;
            const mtr::CtrlTables tb = tables_of(p);
            for (uint32_t i = 0; i < n; i++) {
                mtr::CtrlState s; mtr::PlayState q;
                memcpy(&s, &want[i], 16);
                memcpy(&q, &pl[i], 32);
                const mtr::CtrlStep r = mtr::ctrl_step(s, q, NP ? want_pr.data() + (size_t)i * NP : nullptr, i, dt, tb);
                memcpy(&want[i], &s, 16);
                memcpy(&want_cm[i], &r.cmd, 16);
                if (r.fired != MTR_CTRL_NONE) { if (r.fired >= T) return 1; want_cnt[r.fired]++; }
            }
        }
        mtr_ctrl_state* st_dev = dev_copy(st);
        mtr_play_state* pl_dev = dev_copy(pl);
        float* pr_dev = dev_copy(pr);
        uint32_t* cnt_dev = dev_copy(cnt);
        std::vector<mtr_play_cmd> cm(n);
        memset(cm.data(), 0x5A, cm.size() * 16);
        mtr_play_cmd* cm_dev = dev_copy(cm);
        // ---- the valid calls ----
        EXPECT(mtr_anim_ctrl_step_device(ct, st_dev, pl_dev, NP ? pr_dev : nullptr, n, dt, cm_dev, T ? cnt_dev : nullptr, caller), MTR_OK);
        CHECK(g_last_stream == caller && ct->recorded && ct->last_stream == caller);
        CHECK(same(st_dev, want.data(), (size_t)n * 16) && same(cm_dev, want_cm.data(), (size_t)n * 16));
        CHECK(same(pr_dev, want_pr.data(), pr.size() * 4) && same(cnt_dev, want_cnt.data(), (size_t)T * 4));
        CHECK(same(pl_dev, pl.data(), (size_t)n * 32));  // the play states are read only
        // another stream (a second one, or the device's own), counts NULL: the counts stay, and the stream first waits for
        // the controller's event, so that the one event covers the step before too when the destroy parks the tables
        memcpy(st_dev, st.data(), (size_t)n * 16);
        if (NP) memcpy(pr_dev, pr.data(), pr.size() * 4);
        const hipStream_t other = it & 1 ? caller2 : dev->stream;
        g_ops.clear();
        hipStubTrace() = trace;
        EXPECT(mtr_anim_ctrl_step_device(ct, st_dev, pl_dev, NP ? pr_dev : nullptr, n, dt, cm_dev, nullptr, it & 1 ? caller2 : nullptr), MTR_OK);
        hipStubTrace() = nullptr;
        {
            bool waited = false;
            for (const Op& o : g_ops) waited |= o.op == "hipStreamWaitEvent" && o.what == ct->last && o.stream == other;
            CHECK(waited && g_last_stream == other && ct->last_stream == other);
        }
        CHECK(same(st_dev, want.data(), (size_t)n * 16) && same(cnt_dev, want_cnt.data(), (size_t)T * 4));
        // the host hook: everything in host memory, unaligned on purpose; states, parameters and counts come back
        {
            std::vector<uint8_t> raw((size_t)n * 16 + 4), praw((size_t)n * 32 + 4), craw((size_t)n * 16 + 4, 0x5A), fraw(pr.size() * 4 + 5), nraw((size_t)T * 4 + 5);
            memcpy(raw.data() + 4, st.data(), (size_t)n * 16);
            memcpy(praw.data() + 4, pl.data(), (size_t)n * 32);
            if (NP) memcpy(fraw.data() + 1, pr.data(), pr.size() * 4);
            if (T) memcpy(nraw.data() + 1, cnt.data(), (size_t)T * 4);
            EXPECT(mtr_anim_ctrl_step_host(ct, reinterpret_cast<mtr_ctrl_state*>(raw.data() + 4), reinterpret_cast<const mtr_play_state*>(praw.data() + 4),
                                           NP ? reinterpret_cast<float*>(fraw.data() + 1) : nullptr, n, dt, reinterpret_cast<mtr_play_cmd*>(craw.data() + 4),
                                           T ? reinterpret_cast<uint32_t*>(nraw.data() + 1) : nullptr), MTR_OK);
            CHECK(same(raw.data() + 4, want.data(), (size_t)n * 16) && same(craw.data() + 4, want_cm.data(), (size_t)n * 16));
            CHECK(same(fraw.data() + 1, want_pr.data(), pr.size() * 4) && same(nraw.data() + 1, want_cnt.data(), (size_t)T * 4));
        }
        stepped += 3;
        // ---- every invalid call: nothing is launched, nothing changes ----
        const uint64_t launches = g_launches;
        memcpy(st_dev, st.data(), (size_t)n * 16);
        if (NP) memcpy(pr_dev, pr.data(), pr.size() * 4);
        memset(cm_dev, 0x5A, (size_t)n * 16);
        auto odd = [](auto* p, int by) { return reinterpret_cast<decltype(p)>(reinterpret_cast<char*>(p) + by); };
        float* prp = NP ? pr_dev : nullptr;
        EXPECT(mtr_anim_ctrl_step_device(nullptr, st_dev, pl_dev, prp, n, dt, cm_dev, cnt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_ctrl_step_device(ct, nullptr, pl_dev, prp, n, dt, cm_dev, cnt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_ctrl_step_device(ct, st_dev, nullptr, prp, n, dt, cm_dev, cnt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_ctrl_step_device(ct, st_dev, pl_dev, prp, n, dt, nullptr, cnt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_ctrl_step_device(ct, st_dev, pl_dev, prp, 0, dt, cm_dev, cnt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_ctrl_step_device(ct, st_dev, pl_dev, prp, ((size_t)1 << 27) + 1, dt, cm_dev, cnt_dev, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_ctrl_step_device(ct, odd(st_dev, 8), pl_dev, prp, n, dt, cm_dev, cnt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_ctrl_step_device(ct, st_dev, odd(pl_dev, 8), prp, n, dt, cm_dev, cnt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_ctrl_step_device(ct, st_dev, pl_dev, prp, n, dt, odd(cm_dev, 4), cnt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_ctrl_step_device(ct, st_dev, pl_dev, odd(pr_dev, 2), n, dt, cm_dev, cnt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_ctrl_step_device(ct, st_dev, pl_dev, prp, n, dt, cm_dev, odd(cnt_dev, 1), caller), MTR_E_INVALID);
        EXPECT(mtr_anim_ctrl_step_host(nullptr, st.data(), pl.data(), pr.data(), n, dt, cm.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_ctrl_step_host(ct, nullptr, pl.data(), pr.data(), n, dt, cm.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_ctrl_step_host(ct, st.data(), nullptr, pr.data(), n, dt, cm.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_ctrl_step_host(ct, st.data(), pl.data(), pr.data(), n, dt, nullptr, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_ctrl_step_host(ct, st.data(), pl.data(), pr.data(), 0, dt, cm.data(), nullptr), MTR_E_INVALID);
        rejected += 16;
        if (NP) {
            EXPECT(mtr_anim_ctrl_step_device(ct, st_dev, pl_dev, nullptr, n, dt, cm_dev, cnt_dev, caller), MTR_E_INVALID);
            EXPECT(mtr_anim_ctrl_step_host(ct, st.data(), pl.data(), nullptr, n, dt, cm.data(), nullptr), MTR_E_INVALID);
            rejected += 2;
        }
        CHECK(launches == g_launches && same(st_dev, st.data(), (size_t)n * 16) && same(pr_dev, pr.data(), pr.size() * 4));
        CHECK(same(cnt_dev, want_cnt.data(), (size_t)T * 4));
        for (size_t i = 0; i < (size_t)n * 16; i++) CHECK(reinterpret_cast<uint8_t*>(cm_dev)[i] == 0x5A);
        // ---- controllers created and destroyed with steps queued; a frame collects the garbage ----
        for (int k = 0; k < 3; k++) {
            mtr_anim_ctrl* tmp = nullptr;
            EXPECT(mtr_anim_ctrl_create(dev, C, nk.data(), fl.data(), nodes.data(), S, tp, T, nany, NP, &tmp), MTR_OK);
            for (int q = 0; q < k; q++) {
                EXPECT(mtr_anim_ctrl_step_device(tmp, st_dev, pl_dev, prp, n, dt, cm_dev, T && q ? cnt_dev : nullptr, q ? caller : caller2), MTR_OK);
                stepped++;
            }
            mtr_anim_ctrl_destroy(tmp);  // straight after the call: the kernel is queued (k == 0: never stepped)
            mtr_frame* f = nullptr;
            EXPECT(mtr_frame_begin(dev, 64, 48, clear, 1.0f, &f), MTR_OK);
            EXPECT(mtr_frame_submit(f), MTR_OK);
            EXPECT(mtr_frame_wait(f), MTR_OK);
            mtr_frame_destroy(f);
        }
        mtr_anim_ctrl_destroy(ct);
        mtr_anim_ctrl_destroy(ct0);
        mtr_anim_ctrl_destroy(nullptr);
        free(st_dev); free(pl_dev); free(pr_dev); free(cnt_dev); free(cm_dev);
    }
    hipStreamDestroy(caller);
    hipStreamDestroy(caller2);
    mtr_device_destroy(dev);
    printf("stepped=%ld rejected=%ld launches=%llu failed=%d\n", stepped, rejected, (unsigned long long)g_launches, g_failed);
    return g_failed ? 1 : 0;
}
