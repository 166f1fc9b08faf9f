// AddressSanitizer / UBSan run of the HOST side of players (csrc/host_player.cpp: mtr_anim_player_create / _destroy,
// mtr_anim_player_advance_device(_cmds), mtr_anim_player_advance_host) over the stand-in HIP runtime (tests/cpp/hip_stub:
// device memory = host heap), a stand-alone program.  The k_play launcher here does what the two kernels do, with
// csrc/play_math.h on exactly the words PlayParams hands it: the largest command index + 1 per instance into the scratch
// array, then one play_advance per instance and the records of the frame.  A wrong size, offset or stride on the host side is
// an ASan report, and the results are compared with a second run of the rule on the caller's copies.  Every rejected call of
// include/mtr.h's table is made and must launch nothing and leave the states as they were; players are created and destroyed
// with advances queued; host commands are staged in the player's own buffer before the call returns; the scratch array is
// the player's, zero between calls, and freed once (a second free is an ASan report when the devices are destroyed).
//   usage: player_host_asan <iterations>
#define MTR_RND_SEED 0x243F6A8885A308D3ull
#include "harness.h"
#include "../../mt_renderer_amd/csrc/play_math.h"

static uint64_t g_launches = 0, g_cmd_launches = 0;
static const void* g_last_cmds = nullptr;
static const void* g_last_stream = nullptr;

static void frame_out(const PlayParams& p, uint32_t inst, const mtr::PlayFrame& f) {
    auto fb = [](float v) { uint32_t u; memcpy(&u, &v, 4); return u; };
    if (p.out_states) {
        uint32_t* o = p.out_states + (size_t)inst * 6;
        o[0] = f.clip_a; o[1] = f.clip_b; o[2] = fb(f.x_a); o[3] = fb(f.x_b); o[4] = fb(f.w); o[5] = 0;
    }
    if (p.out_layers) {
        uint32_t* o = p.out_layers + (size_t)inst * p.nlayers * 4;
        o[0] = f.clip_a; o[1] = fb(f.x_a); o[2] = 0; o[3] = 0;
        o[4] = f.clip_b; o[5] = fb(f.x_b); o[6] = fb(f.w); o[7] = 0;
    }
    if (p.out_steps) {
        uint32_t* o = p.out_steps + (size_t)inst * 8;
        o[0] = f.clip_a; o[1] = fb(f.x0_a); o[2] = fb(f.dx_a); o[3] = 0;
        o[4] = f.clip_b; o[5] = fb(f.x0_b); o[6] = fb(f.dx_b); o[7] = fb(f.w);
    }
}

void mtr_launch_play(const PlayParams& p, hipStream_t s) {
    if (!p.table || !p.states || !p.scratch || !p.n || !p.nclips || ((uintptr_t)p.states & 15u) || ((uintptr_t)p.table & 15u)) abort();
    if ((p.ncmds && (!p.cmds || ((uintptr_t)p.cmds & 15u))) || ((uintptr_t)p.out_layers & 15u) || ((uintptr_t)p.out_steps & 15u) || ((uintptr_t)p.out_states & 7u)) abort();
    if (p.out_layers && (p.nlayers < 2 || p.nlayers > 8)) abort();
    g_launches++;
    g_cmd_launches += p.ncmds != 0;
    g_last_cmds = p.cmds;
    g_last_stream = s;
    for (uint32_t i = 0; i < p.ncmds; i++) {
        const uint32_t inst = p.cmds[(size_t)i * 4];
        if (inst < p.n && p.scratch[inst] < i + 1) p.scratch[inst] = i + 1;
    }
    for (uint32_t inst = 0; inst < p.n; inst++) {
        uint32_t slot = 0;
        if (p.ncmds) { slot = p.scratch[inst]; p.scratch[inst] = 0; }
        if (slot > p.ncmds) abort();
        mtr::PlayState st;
        mtr::PlayCmd cmd;
        memcpy(&st, p.states + (size_t)inst * 8, 32);
        if (slot) memcpy(&cmd, p.cmds + (size_t)(slot - 1) * 4, 16);
        const mtr::PlayFrame f = mtr::play_advance(st, slot ? &cmd : nullptr, p.dt, reinterpret_cast<const mtr::PlayClip*>(p.table), p.nclips);
        memcpy(p.states + (size_t)inst * 8, &st, 32);
        frame_out(p, inst, f);
    }
}

static float edge() {
    static const float e[] = {0.0f, -0.0f, 0.3f, 1.5f, 29.8f, -1e-7f, 1e30f, NAN, INFINITY, -1.0f, 0.05f, 1e-41f};
    return e[rnd() % (sizeof e / sizeof e[0])];
}
static bool scratch_clean(const mtr_anim_player* pl) {
    const uint32_t* s = pl->d + (size_t)pl->nclips * 4;
    for (uint32_t i = 0; i < pl->max_instances; i++)
        if (s[i]) return false;
    return true;
}

int main(int argc, char** argv) {
    const long iters = argc > 1 ? strtol(argv[1], nullptr, 10) : 40;
    mtr_device *dev = nullptr, *dev2 = nullptr;
    if (mtr_device_create(0, &dev) || mtr_device_create(0, &dev2)) return 3;
    hipStream_t caller = nullptr, caller2 = nullptr;
    if (hipStreamCreateWithFlags(&caller, hipStreamNonBlocking) || hipStreamCreateWithFlags(&caller2, hipStreamNonBlocking)) return 3;
    const float clear[4] = {1, 1, 1, 1};
    long advanced = 0, rejected = 0;
    for (long it = 0; it < iters; it++) {
        const uint32_t C = pick(1, 5), n = pick(1, 70), cap = n + pick(0, 3), m = it % 4 == 0 ? 0 : pick(1, 90), nl = it % 3 ? pick(2, 8) : 2;
        std::vector<uint32_t> nk(C), fl(C);
        std::vector<float> rates(C);
        for (uint32_t c = 0; c < C; c++) { nk[c] = rnd() % 4 ? pick(1, 40) : (1u << 24); fl[c] = (uint32_t)(rnd() & 1); rates[c] = (float)pick(1, 60) * (rnd() & 1 ? 1.0f : -0.5f); }
        // ---- every invalid creation ----
        mtr_anim_player* none = (mtr_anim_player*)1;
        EXPECT(mtr_anim_player_create(nullptr, C, nk.data(), fl.data(), rates.data(), cap, &none), MTR_E_INVALID);
        EXPECT(mtr_anim_player_create(dev, C, nk.data(), fl.data(), rates.data(), cap, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_player_create(dev, 0, nk.data(), fl.data(), rates.data(), cap, &none), MTR_E_INVALID);
        EXPECT(mtr_anim_player_create(dev, C, nullptr, fl.data(), rates.data(), cap, &none), MTR_E_INVALID);
        EXPECT(mtr_anim_player_create(dev, C, nk.data(), fl.data(), nullptr, cap, &none), MTR_E_INVALID);
        EXPECT(mtr_anim_player_create(dev, C, nk.data(), fl.data(), rates.data(), 0, &none), MTR_E_INVALID);
        EXPECT(mtr_anim_player_create(dev, C, nk.data(), fl.data(), rates.data(), ((size_t)1 << 27) + 1, &none), MTR_E_INVALID);
        {
            const uint32_t c = pick(0, C - 1);
            char want[32];
            snprintf(want, sizeof want, "clip %u ", c);
            std::vector<uint32_t> bad_n = nk, bad_f = fl;
            std::vector<float> bad_r = rates;
            bad_n[c] = rnd() & 1 ? 0u : (1u << 24) + 1u;
            bad_f[c] |= 2u << pick(0, 29);
            bad_r[c] = rnd() % 3 == 0 ? NAN : rnd() & 1 ? INFINITY : -INFINITY;
            EXPECT(mtr_anim_player_create(dev, C, bad_n.data(), fl.data(), rates.data(), cap, &none), MTR_E_INVALID); NAMES(want);
            EXPECT(mtr_anim_player_create(dev, C, nk.data(), bad_f.data(), rates.data(), cap, &none), MTR_E_INVALID); NAMES(want);
            EXPECT(mtr_anim_player_create(dev, C, nk.data(), fl.data(), bad_r.data(), cap, &none), MTR_E_INVALID); NAMES(want);
        }
        if (none) { fprintf(stderr, "a failed create must clear *out\n"); return 1; }
        rejected += 10;
        mtr_anim_player *pl = nullptr, *pl0 = nullptr;
        EXPECT(mtr_anim_player_create(dev, C, nk.data(), fl.data(), rates.data(), cap, &pl), MTR_OK);
        EXPECT(mtr_anim_player_create(dev2, C, nk.data(), nullptr, rates.data(), cap, &pl0), MTR_OK);  // NULL flags: all 0
        CHECK(scratch_clean(pl) && scratch_clean(pl0));
        for (uint32_t c = 0; c < C; c++) {  // the table: period, flags, rate, key count
            float P;
            memcpy(&P, pl->d + c * 4, 4);
            CHECK(P == (float)(fl[c] ? nk[c] : nk[c] - 1) && pl->d[c * 4 + 1] == fl[c] && pl->d[c * 4 + 3] == nk[c] && pl0->d[c * 4 + 1] == 0);
        }
        // ---- inputs, exactly sized: one record too many read or written is a report ----
        std::vector<mtr_play_state> st(n);
        for (auto& s : st) { s.clip_a = rnd() % 5 ? pick(0, C - 1) : (uint32_t)rnd(); s.clip_b = rnd() % 5 ? pick(0, C - 1) : (uint32_t)rnd(); s.x_a = edge(); s.x_b = edge(); s.w = edge(); s.fade = edge(); s.speed = edge(); s.flags = (uint32_t)rnd(); }
        std::vector<mtr_play_cmd> cm(m);
        for (auto& c : cm) { c.instance = rnd() % 6 ? pick(0, n - 1) : n + pick(0, 5); c.clip = rnd() % 5 ? pick(0, C - 1) : (uint32_t)rnd(); c.x = edge(); c.seconds = edge(); }
        const float dt = it % 7 == 3 ? 0.0f : it % 7 == 5 ? -1.0f / 30 : 1.0f / 30;
        // what the rule makes of them, on copies
        std::vector<mtr_play_state> want = st;
        std::vector<mtr::PlayFrame> wf(n);
        {
            std::vector<uint32_t> sel(n, 0);
            for (uint32_t i = 0; i < m; i++) if (cm[i].instance < n) sel[cm[i].instance] = i + 1;
            for (uint32_t i = 0; i < n; i++) {
                mtr::PlayState s; mtr::PlayCmd c;
                memcpy(&s, &want[i], 32);
                if (sel[i]) memcpy(&c, &cm[sel[i] - 1], 16);
                wf[i] = mtr::play_advance(s, sel[i] ? &c : nullptr, dt, reinterpret_cast<const mtr::PlayClip*>(pl->d), C);
                memcpy(&want[i], &s, 32);
            }
        }
        mtr_play_state* st_dev = dev_copy(st);
        mtr_play_cmd* cm_dev = dev_copy(cm);
        std::vector<mtr_anim_state> oa(n);
        std::vector<mtr_anim_layer> ol((size_t)n * nl);
        std::vector<mtr_root_step> os_((size_t)n * 2);
        memset(ol.data(), 0x5A, ol.size() * sizeof(mtr_anim_layer));
        mtr_anim_state* oa_dev = dev_copy(oa);
        mtr_anim_layer* ol_dev = dev_copy(ol);
        mtr_root_step* os_dev = dev_copy(os_);
        // ---- the valid calls ----
        // host commands: staged in the player's buffer by a copy issued before the call returns, the launch reads that buffer
        g_ops.clear();
        hipStubTrace() = trace;
        EXPECT(mtr_anim_player_advance_device(pl, st_dev, n, dt, m ? cm.data() : nullptr, m, oa_dev, ol_dev, nl, os_dev, caller), MTR_OK);
        hipStubTrace() = nullptr;
        if (m) {
            bool staged = false;
            for (const Op& o : g_ops) staged |= o.op == "hipMemcpyAsync" && o.bytes == (size_t)m * 16 && o.what == pl->cmds && o.stream == caller;
            CHECK(staged && g_last_cmds == pl->cmds && pl->cmd_cap >= m && g_last_cmds != cm.data());
            for (auto& c : cm) c.instance ^= 1u;  // the caller's list is free again: the next comparison still holds
            for (auto& c : cm) c.instance ^= 1u;
        }
        CHECK(g_last_stream == caller && pl->recorded && pl->last_stream == caller);
        CHECK(memcmp(st_dev, want.data(), (size_t)n * 32) == 0 && scratch_clean(pl));
        for (uint32_t i = 0; i < n; i++) {
            CHECK(oa_dev[i].clip_a == wf[i].clip_a && oa_dev[i].clip_b == wf[i].clip_b && oa_dev[i].pad == 0 && memcmp(&oa_dev[i].x_a, &wf[i].x_a, 12) == 0);
            CHECK(ol_dev[(size_t)i * nl].clip == wf[i].clip_a && ol_dev[(size_t)i * nl + 1].clip == wf[i].clip_b && ol_dev[(size_t)i * nl + 1].mode == 0);
            for (uint32_t l = 2; l < nl; l++) CHECK(ol_dev[(size_t)i * nl + l].clip == 0x5A5A5A5Au && ol_dev[(size_t)i * nl + l].mask == 0x5A5A);
            CHECK(os_dev[i * 2].clip == wf[i].clip_a && memcmp(&os_dev[i * 2].x, &wf[i].x0_a, 4) == 0 && memcmp(&os_dev[i * 2 + 1].dx, &wf[i].dx_b, 4) == 0);
        }
        // device commands, the other stream (ordered behind the call before by the player's event), outputs NULL in turn
        memcpy(st_dev, st.data(), (size_t)n * 32);
        g_ops.clear();
        hipStubTrace() = trace;
        EXPECT(mtr_anim_player_advance_device_cmds(pl, st_dev, n, dt, m ? cm_dev : nullptr, m, it % 3 == 0 ? nullptr : oa_dev, it % 3 == 1 ? nullptr : ol_dev, nl,
                                                   it % 3 == 2 ? nullptr : os_dev, caller2), MTR_OK);
        hipStubTrace() = nullptr;
        {
            bool waited = false;
            for (const Op& o : g_ops) waited |= o.op == "hipStreamWaitEvent" && o.what == pl->last && o.stream == caller2;
            CHECK(waited && (m == 0 || g_last_cmds == cm_dev) && pl->last_stream == caller2);
        }
        CHECK(memcmp(st_dev, want.data(), (size_t)n * 32) == 0 && scratch_clean(pl));
        // the host hook: everything in host memory, unaligned on purpose; the states and layers 2.. come back
        {
            std::vector<uint8_t> raw((size_t)n * 32 + 4), lraw((size_t)n * nl * 16 + 4, 0x5A);
            memcpy(raw.data() + 4, st.data(), (size_t)n * 32);
            std::vector<mtr_root_step> hs((size_t)n * 2);
            EXPECT(mtr_anim_player_advance_host(pl, reinterpret_cast<mtr_play_state*>(raw.data() + 4), n, dt, m ? cm.data() : nullptr, m, oa.data(),
                                                reinterpret_cast<mtr_anim_layer*>(lraw.data() + 4), nl, hs.data()), MTR_OK);
            CHECK(memcmp(raw.data() + 4, want.data(), (size_t)n * 32) == 0 && scratch_clean(pl));
            CHECK(memcmp(hs.data(), os_dev, hs.size() * 16) == 0);  // the same inputs: the same steps as the device calls wrote
            for (uint32_t i = 0; i < n; i++)
                for (uint32_t l = 2; l < nl; l++) CHECK(lraw[4 + ((size_t)i * nl + l) * 16] == 0x5A && lraw[4 + ((size_t)i * nl + l) * 16 + 15] == 0x5A);
            EXPECT(mtr_anim_player_advance_host(pl0, reinterpret_cast<mtr_play_state*>(raw.data() + 4), n, dt, nullptr, 0, nullptr, nullptr, 0, nullptr), MTR_OK);
        }
        advanced += 4;
        // ---- every invalid call: nothing is launched, nothing changes ----
        const uint64_t launches = g_launches;
        std::vector<mtr_play_state> keep(st_dev, st_dev + n);
        auto odd = [](auto* p) { return reinterpret_cast<decltype(p)>(reinterpret_cast<char*>(p) + 8); };
        mtr_play_cmd one{0, 0, 1.0f, 0.0f};
        for (int devcmds = 0; devcmds < 2; devcmds++) {
            auto fn = devcmds ? mtr_anim_player_advance_device_cmds : mtr_anim_player_advance_device;
            const mtr_play_cmd* c1 = devcmds ? cm_dev : &one;
            const size_t m1 = devcmds ? m : 1;
            EXPECT(fn(nullptr, st_dev, n, dt, c1, m1, oa_dev, ol_dev, nl, os_dev, caller), MTR_E_INVALID);
            EXPECT(fn(pl, nullptr, n, dt, c1, m1, oa_dev, ol_dev, nl, os_dev, caller), MTR_E_INVALID);
            EXPECT(fn(pl, st_dev, 0, dt, c1, m1, oa_dev, ol_dev, nl, os_dev, caller), MTR_E_INVALID);
            EXPECT(fn(pl, st_dev, cap + 1, dt, c1, m1, oa_dev, ol_dev, nl, os_dev, caller), MTR_E_INVALID);
            EXPECT(fn(pl, st_dev, n, dt, c1, m1, oa_dev, ol_dev, 1, os_dev, caller), MTR_E_INVALID);
            EXPECT(fn(pl, st_dev, n, dt, c1, m1, oa_dev, ol_dev, 9, os_dev, nullptr), MTR_E_INVALID);
            EXPECT(fn(pl, odd(st_dev), n, dt, c1, m1, oa_dev, ol_dev, nl, os_dev, caller), MTR_E_INVALID);
            EXPECT(fn(pl, st_dev, n, dt, c1, m1, reinterpret_cast<mtr_anim_state*>(reinterpret_cast<char*>(oa_dev) + 4), ol_dev, nl, os_dev, caller), MTR_E_INVALID);
            EXPECT(fn(pl, st_dev, n, dt, c1, m1, oa_dev, odd(ol_dev), nl, os_dev, caller), MTR_E_INVALID);
            EXPECT(fn(pl, st_dev, n, dt, c1, m1, oa_dev, ol_dev, nl, odd(os_dev), caller), MTR_E_INVALID);
            EXPECT(fn(pl, st_dev, n, dt, nullptr, 3, oa_dev, ol_dev, nl, os_dev, caller), MTR_E_INVALID);
            EXPECT(fn(pl, st_dev, n, dt, c1, (size_t)1 << 31, oa_dev, ol_dev, nl, os_dev, caller), MTR_E_INVALID);
            rejected += 12;
        }
        EXPECT(mtr_anim_player_advance_device_cmds(pl, st_dev, n, dt, odd(cm_dev), 1, oa_dev, ol_dev, nl, os_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_player_advance_host(nullptr, st.data(), n, dt, nullptr, 0, nullptr, nullptr, 0, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_player_advance_host(pl, nullptr, n, dt, nullptr, 0, nullptr, nullptr, 0, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_player_advance_host(pl, st.data(), 0, dt, nullptr, 0, nullptr, nullptr, 0, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_player_advance_host(pl, st.data(), cap + 1, dt, nullptr, 0, nullptr, nullptr, 0, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_player_advance_host(pl, st.data(), n, dt, nullptr, 2, nullptr, nullptr, 0, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_player_advance_host(pl, st.data(), n, dt, nullptr, 0, nullptr, ol.data(), 1, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_player_advance_host(pl, st.data(), n, dt, nullptr, 0, nullptr, ol.data(), 9, nullptr), MTR_E_INVALID);
        rejected += 8;
        CHECK(launches == g_launches && memcmp(keep.data(), st_dev, (size_t)n * 32) == 0 && scratch_clean(pl));
        // ---- players created and destroyed with advances queued, the command buffer growing; a frame collects the garbage ----
        for (int k = 0; k < 3; k++) {
            mtr_anim_player* tmp = nullptr;
            EXPECT(mtr_anim_player_create(dev, C, nk.data(), fl.data(), rates.data(), cap, &tmp), MTR_OK);
            for (uint32_t grow = 1; grow <= 3 && m; grow++) {  // 1, 2, 3 thirds of the list: the buffer is outgrown twice
                const size_t part = std::max<size_t>(1, (size_t)m * grow / 3);
                EXPECT(mtr_anim_player_advance_device(tmp, st_dev, n, dt, cm.data(), part, nullptr, nullptr, 0, k ? os_dev : nullptr, k == 1 ? caller : nullptr), MTR_OK);
                advanced++;
            }
            EXPECT(mtr_anim_player_advance_device_cmds(tmp, st_dev, n, dt, nullptr, 0, oa_dev, nullptr, 0, nullptr, caller2), MTR_OK);
            advanced++;
            CHECK(scratch_clean(tmp));
            mtr_anim_player_destroy(tmp);  // straight after the call: the kernel is queued
            mtr_frame* f = nullptr;
            EXPECT(mtr_frame_begin(dev, 64, 48, clear, 1.0f, &f), MTR_OK);
            EXPECT(mtr_frame_submit(f), MTR_OK);
            EXPECT(mtr_frame_wait(f), MTR_OK);
            mtr_frame_destroy(f);
        }
        mtr_anim_player_destroy(pl);
        mtr_anim_player_destroy(pl0);
        mtr_anim_player_destroy(nullptr);
        free(st_dev); free(cm_dev); free(oa_dev); free(ol_dev); free(os_dev);
    }
    hipStreamDestroy(caller);
    hipStreamDestroy(caller2);
    mtr_device_destroy(dev2);
    mtr_device_destroy(dev);
    printf("advanced=%ld rejected=%ld launches=%llu cmd_launches=%llu failed=%d\n", advanced, rejected, (unsigned long long)g_launches,
           (unsigned long long)g_cmd_launches, g_failed);
    return g_failed ? 1 : 0;
}
