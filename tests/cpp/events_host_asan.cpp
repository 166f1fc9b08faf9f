// AddressSanitizer / UBSan run of the HOST side of animation events (csrc/host_events.cpp: mtr_anim_events_create / _destroy,
// mtr_anim_events_collect_device, mtr_anim_events_collect_host) over the stand-in HIP runtime (tests/cpp/hip_stub: device memory
// = host heap), a stand-alone program.  The k_events launcher here does what the three kernels do, with csrc/event_math.h on
// exactly the words EventParams hands it: a count per instance, the block sums in the set's scratch, their exclusive scan, the
// fill.  A wrong size, offset or stride on the host side is an ASan report, and the results are compared with a second run of
// the rule on the caller's copies.  Every rejected creation and call of include/mtr.h's table is made and must launch nothing
// and leave the list, the count and the bits as they were, the error naming the clip and the marker; sets are created and
// destroyed with calls queued.
//   usage: events_host_asan <iterations>
#define MTR_RND_SEED 0x243F6A8885A308D3ull
#include "harness.h"
#include "../../mt_renderer_amd/csrc/event_math.h"

static uint64_t g_launches = 0;
static const void* g_last_stream = nullptr;

// the rule on the words of p; sums may be nullptr (the second run on the caller's copies keeps its own)
static void run_rule(const EventParams& p, uint32_t* sums) {
    mtr::EventTables t;
    t.clips = reinterpret_cast<const mtr::PlayClip*>(p.clips);
    t.ranges = p.ranges;
    t.markers = reinterpret_cast<const mtr::EventMarker*>(p.markers);
    t.nclips = p.nclips;
    const mtr::EventStepIn* steps = reinterpret_cast<const mtr::EventStepIn*>(p.steps);
    const uint32_t nb = (p.n + 255u) / 256u;
    std::vector<uint32_t> own(nb, 0u), counts(p.n);
    if (!sums) sums = own.data();
    for (uint32_t b = 0; b < nb; b++) sums[b] = 0;
    for (uint32_t i = 0; i < p.n; i++) {
        counts[i] = mtr::event_count(steps + (size_t)i * p.nsteps, p.nsteps, p.min_weight, t);
        sums[i / 256u] += counts[i];
    }
    uint32_t carry = 0;
    for (uint32_t b = 0; b < nb; b++) { const uint32_t v = sums[b]; sums[b] = carry; carry += v; }
    p.count[0] = carry;
    p.count[1] = carry < p.capacity ? carry : p.capacity;
    for (uint32_t i = 0; i < p.n; i++) {
        uint32_t idx = sums[i / 256u], mask = 0;
        for (uint32_t j = i / 256u * 256u; j < i; j++) idx += counts[j];
        mtr::event_walk(steps + (size_t)i * p.nsteps, p.nsteps, p.min_weight, t, [&](const mtr::EventMarker& m, uint32_t where, float w) {
            if (idx < p.capacity) {
                const mtr::EventRecord r{i, m.id, where, w};
                memcpy(p.out + (size_t)idx * 4, &r, 16);
            }
            idx++;
            mask |= 1u << (m.id & 31u);
        });
        if (p.bits) p.bits[i] = mask;
    }
}

void mtr_launch_events(const EventParams& p, hipStream_t s) {
    if (!p.clips || !p.ranges || !p.markers || !p.sums || !p.steps || !p.count || !p.n || !p.nclips || !p.nsteps || p.nsteps > 8) abort();
    if (((uintptr_t)p.clips & 15u) || ((uintptr_t)p.ranges & 7u) || ((uintptr_t)p.markers & 7u) || ((uintptr_t)p.sums & 3u) || ((uintptr_t)p.steps & 15u) ||
        ((uintptr_t)p.out & 15u) || ((uintptr_t)p.count & 3u) || ((uintptr_t)p.bits & 3u) || (p.capacity && !p.out) || (!p.capacity && p.out))
        abort();
    g_launches++;
    g_last_stream = s;
    run_rule(p, p.sums);
}

static float edge() {
    static const float e[] = {0.0f, -0.0f, 0.3f, 1.5f, 29.8f, -1e-7f, 1e30f, NAN, INFINITY, -INFINITY, -1.0f, 0.05f, 1e-41f, -1e-41f, 0.5f, 1.0f, -0.37f, 7.0f};
    return e[rnd() % (sizeof e / sizeof e[0])];
}

int main(int argc, char** argv) {
    const long iters = argc > 1 ? strtol(argv[1], nullptr, 10) : 40;
    mtr_device* dev = nullptr;
    if (mtr_device_create(0, &dev)) return 3;
    hipStream_t caller = nullptr, caller2 = nullptr;
    if (hipStreamCreateWithFlags(&caller, hipStreamNonBlocking) || hipStreamCreateWithFlags(&caller2, hipStreamNonBlocking)) return 3;
    const float clear[4] = {1, 1, 1, 1};
    long collected = 0, rejected = 0;
    for (long it = 0; it < iters; it++) {
        const uint32_t C = pick(1, 5), S = it % 3 == 0 ? 1 : it % 3 == 1 ? 2 : pick(3, 8), n = it % 4 == 3 ? pick(257, 600) : pick(1, 70), maxn = n + pick(0, 300);
        std::vector<uint32_t> nk(C), fl(C), cnt(C);
        std::vector<mtr_event_marker> mk;
        for (uint32_t c = 0; c < C; c++) {
            nk[c] = rnd() % 4 ? pick(2, 40) : (1u << 24);
            fl[c] = (uint32_t)(rnd() & 1);
            cnt[c] = it % 5 == 4 ? 0 : rnd() % 3 ? pick(0, 6) : 65;
            const float P = fl[c] ? (float)nk[c] : (float)(nk[c] - 1u);
            float x = 0.0f;
            for (uint32_t k = 0; k < cnt[c]; k++) {  // non-decreasing with ties, inside the clip
                if (rnd() % 3) x = std::min(x + P * 0.01f * (float)pick(0, 9), fl[c] ? std::nextafterf(P, 0.0f) : P);
                mk.push_back({x, (uint32_t)rnd()});
            }
        }
        const uint32_t M = (uint32_t)mk.size();
        uint32_t max_count = 0;
        for (uint32_t c = 0; c < C; c++) max_count = std::max(max_count, cnt[c]);
        const mtr_event_marker* mp = M ? mk.data() : nullptr;
        // ---- every invalid creation ----
        mtr_anim_events* none = (mtr_anim_events*)1;
        auto create = [&](size_t nclips, const uint32_t* k, const uint32_t* f, const uint32_t* cn, const mtr_event_marker* m, size_t mi) {
            return mtr_anim_events_create(dev, nclips, k, f, cn, m, mi, &none);
        };
        EXPECT(mtr_anim_events_create(nullptr, C, nk.data(), fl.data(), cnt.data(), mp, maxn, &none), MTR_E_INVALID);
        EXPECT(mtr_anim_events_create(dev, C, nk.data(), fl.data(), cnt.data(), mp, maxn, nullptr), MTR_E_INVALID);
        EXPECT(create(0, nk.data(), fl.data(), cnt.data(), mp, maxn), MTR_E_INVALID);
        EXPECT(create(((size_t)1 << 24) + 1, nk.data(), fl.data(), nullptr, nullptr, maxn), MTR_E_INVALID);
        EXPECT(create(C, nullptr, fl.data(), cnt.data(), mp, maxn), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), cnt.data(), mp, 0), MTR_E_INVALID);
        EXPECT(create(C, nk.data(), fl.data(), cnt.data(), mp, ((size_t)1 << 27) + 1), MTR_E_INVALID);
        rejected += 7;
        {
            std::vector<uint32_t> big = cnt;
            big[pick(0, C - 1)] = (1u << 24) + 1u;  // more than 2^24 markers in all: rejected before a marker is read
            EXPECT(create(C, nk.data(), fl.data(), big.data(), mp, maxn), MTR_E_INVALID);
            rejected++;
            if (M) { EXPECT(create(C, nk.data(), fl.data(), cnt.data(), nullptr, maxn), MTR_E_INVALID); rejected++; }
        }
        {
            const uint32_t c = pick(0, C - 1);
            char want[32];
            snprintf(want, sizeof want, "clip %u ", c);
            std::vector<uint32_t> bad_n = nk, bad_f = fl;
            bad_n[c] = rnd() & 1 ? 0u : (1u << 24) + 1u;
            bad_f[c] |= 2u << pick(0, 29);
            EXPECT(create(C, bad_n.data(), fl.data(), cnt.data(), mp, maxn), MTR_E_INVALID); NAMES(want);
            EXPECT(create(C, nk.data(), bad_f.data(), cnt.data(), mp, maxn), MTR_E_INVALID); NAMES(want);
            rejected += 2;
        }
        if (M) {  // a marker that is not finite, negative, past the clip, or ahead of the one before it
            uint32_t c = pick(0, C - 1);
            while (cnt[c] == 0) c = (c + 1) % C;
            uint32_t first = 0;
            for (uint32_t j = 0; j < c; j++) first += cnt[j];
            const uint32_t k = pick(0, cnt[c] - 1);
            const float P = fl[c] ? (float)nk[c] : (float)(nk[c] - 1u);
            char wc[32], wm[32];
            snprintf(wc, sizeof wc, "clip %u ", c);
            snprintf(wm, sizeof wm, "marker %u ", k);
            const float bads[] = {NAN, INFINITY, -INFINITY, -1e-7f, fl[c] ? P : std::nextafterf(P, INFINITY)};
            for (float b : bads) {
                std::vector<mtr_event_marker> bm = mk;
                bm[first + k].x = b;
                EXPECT(create(C, nk.data(), fl.data(), cnt.data(), bm.data(), maxn), MTR_E_INVALID); NAMES(wc); NAMES(wm);
                rejected++;
            }
            if (cnt[c] >= 2) {
                std::vector<mtr_event_marker> bm = mk;
                bm[first].x = P * 0.5f; bm[first + 1].x = P * 0.25f;  // marker 1 lies before marker 0
                for (uint32_t j = 2; j < cnt[c]; j++) bm[first + j].x = P * 0.5f;
                EXPECT(create(C, nk.data(), fl.data(), cnt.data(), bm.data(), maxn), MTR_E_INVALID); NAMES(wc); NAMES("marker 1 ");
                rejected++;
            }
        }
        if (none) { fprintf(stderr, "a failed create must clear *out\n"); return 1; }
        mtr_anim_events *ev = nullptr, *ev0 = nullptr;
        EXPECT(mtr_anim_events_create(dev, C, nk.data(), fl.data(), cnt.data(), mp, maxn, &ev), MTR_OK);
        EXPECT(mtr_anim_events_create(dev, C, nk.data(), nullptr, nullptr, nullptr, maxn, &ev0), MTR_OK);  // NULL flags and counts: all 0
        {   // the image: the clips (period, flags, 0, key count), the ranges, the markers
            uint32_t first = 0;
            for (uint32_t c = 0; c < C; c++) {
                float P;
                memcpy(&P, ev->d + c * 4, 4);
                CHECK(P == (float)(fl[c] ? nk[c] : nk[c] - 1) && ev->d[c * 4 + 1] == fl[c] && ev->d[c * 4 + 2] == 0 && ev->d[c * 4 + 3] == nk[c] && ev0->d[c * 4 + 1] == 0);
                CHECK(ev->d[C * 4 + c * 2] == first && ev->d[C * 4 + c * 2 + 1] == cnt[c] && ev0->d[C * 4 + c * 2 + 1] == 0);
                first += cnt[c];
            }
            CHECK(ev->w_ranges % 4 == 0 && ev->w_markers % 4 == 0 && ev->max_count == max_count && ev->nmarkers == M);
            CHECK(same(ev->d + C * 4 + ev->w_ranges, mk.data(), (size_t)M * 8));
        }
        // ---- inputs, exactly sized: one record too many read or written is a report ----
        std::vector<mtr_root_step> st((size_t)n * S);
        for (auto& s : st) {
            s.clip = rnd() % 5 ? pick(0, C - 1) : (uint32_t)rnd();
            s.x = rnd() & 1 ? edge() : (float)pick(0, 40);
            s.dx = rnd() & 1 ? edge() : (float)pick(1, 50) * (rnd() & 1 ? 0.4f : -0.4f);
            s.w = edge();
        }
        const float mw = it % 4 == 0 ? 0.0f : it % 4 == 1 ? 0.5f : it % 4 == 2 ? NAN : 0.0f;
        // what the rule makes of them, on copies: first with no list, for the total
        uint32_t total = 0;
        {
            uint32_t cnt2[2];
            EventParams p{};
            p.clips = ev->d; p.ranges = ev->d + C * 4; p.markers = p.ranges + ev->w_ranges; p.steps = reinterpret_cast<const uint32_t*>(st.data());
            p.count = cnt2; p.nclips = C; p.nsteps = S; p.n = n; p.capacity = 0; p.min_weight = mw;
            run_rule(p, nullptr);
            total = cnt2[0];
        }
        const uint32_t cap = it % 3 == 0 ? 0 : it % 3 == 1 ? (total ? total - 1 : 0) : total + 5;
        std::vector<mtr_anim_event> list(cap);
        if (cap) memset(list.data(), 0x5A, (size_t)cap * 16);
        std::vector<uint32_t> bits(n, 0xA5A5A5A5u), count(2, 0x77777777u);
        std::vector<mtr_anim_event> want = list;
        std::vector<uint32_t> want_bits = bits, want_count = count;
        {
            EventParams p{};
            p.clips = ev->d; p.ranges = ev->d + C * 4; p.markers = p.ranges + ev->w_ranges; p.steps = reinterpret_cast<const uint32_t*>(st.data());
            p.out = cap ? reinterpret_cast<uint32_t*>(want.data()) : nullptr; p.count = want_count.data(); p.bits = want_bits.data();
            p.nclips = C; p.nsteps = S; p.n = n; p.capacity = cap; p.min_weight = mw;
            run_rule(p, nullptr);
            CHECK(want_count[0] == total && want_count[1] == std::min(total, cap));
        }
        mtr_root_step* st_dev = dev_copy(st);
        mtr_anim_event* ls_dev = dev_copy(list);
        uint32_t* bt_dev = dev_copy(bits);
        uint32_t* ct_dev = dev_copy(count);
        mtr_anim_event* lsp = cap ? ls_dev : nullptr;
        // ---- the valid calls ----
        EXPECT(mtr_anim_events_collect_device(ev, st_dev, S, n, mw, lsp, cap, ct_dev, bt_dev, caller), MTR_OK);
        CHECK(g_last_stream == caller && ev->recorded && ev->last_stream == caller);
        CHECK(same(ls_dev, want.data(), (size_t)cap * 16) && same(ct_dev, want_count.data(), 8) && same(bt_dev, want_bits.data(), (size_t)n * 4));
        CHECK(same(st_dev, st.data(), st.size() * 16));  // the steps are read only
        // another stream (a second one, or the device's own), bits NULL: the bits stay, and the stream first waits for the set's
        // event, so that the calls on one set are ordered among themselves and the destroy can park the set behind it
        if (cap) memcpy(ls_dev, list.data(), (size_t)cap * 16);
        memcpy(bt_dev, bits.data(), (size_t)n * 4);
        memcpy(ct_dev, count.data(), 8);
        const hipStream_t other = it & 1 ? caller2 : dev->stream;
        g_ops.clear();
        hipStubTrace() = trace;
        EXPECT(mtr_anim_events_collect_device(ev, st_dev, S, n, mw, lsp, cap, ct_dev, nullptr, it & 1 ? caller2 : nullptr), MTR_OK);
        hipStubTrace() = nullptr;
        {
            bool waited = false;
            for (const Op& o : g_ops) waited |= o.op == "hipStreamWaitEvent" && o.what == ev->last && o.stream == other;
            CHECK(waited && g_last_stream == other && ev->last_stream == other);
        }
        CHECK(same(ls_dev, want.data(), (size_t)cap * 16) && same(ct_dev, want_count.data(), 8) && same(bt_dev, bits.data(), (size_t)n * 4));
        // the host hook: everything in host memory, unaligned on purpose; the list's tail comes back as it went in
        {
            std::vector<uint8_t> sraw(st.size() * 16 + 4), lraw((size_t)cap * 16 + 4, 0x5A), braw((size_t)n * 4 + 5), craw(8 + 5, 0x77);
            memcpy(sraw.data() + 4, st.data(), st.size() * 16);
            memcpy(braw.data() + 1, bits.data(), (size_t)n * 4);
            EXPECT(mtr_anim_events_collect_host(ev, reinterpret_cast<const mtr_root_step*>(sraw.data() + 4), S, n, mw,
                                                cap ? reinterpret_cast<mtr_anim_event*>(lraw.data() + 4) : nullptr, cap, reinterpret_cast<uint32_t*>(craw.data() + 1),
                                                reinterpret_cast<uint32_t*>(braw.data() + 1)), MTR_OK);
            CHECK(same(lraw.data() + 4, want.data(), (size_t)cap * 16) && same(craw.data() + 1, want_count.data(), 8));
            CHECK(same(braw.data() + 1, want_bits.data(), (size_t)n * 4));
        }
        collected += 3;
        // ---- every invalid call: nothing is launched, nothing changes ----
        const uint64_t launches = g_launches;
        if (cap) memcpy(ls_dev, list.data(), (size_t)cap * 16);
        memcpy(bt_dev, bits.data(), (size_t)n * 4);
        memcpy(ct_dev, count.data(), 8);
        auto odd = [](auto* p, int by) { return reinterpret_cast<decltype(p)>(reinterpret_cast<char*>(p) + by); };
        EXPECT(mtr_anim_events_collect_device(nullptr, st_dev, S, n, mw, lsp, cap, ct_dev, bt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_device(ev, nullptr, S, n, mw, lsp, cap, ct_dev, bt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_device(ev, st_dev, S, n, mw, lsp, cap, nullptr, bt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_device(ev, st_dev, 0, n, mw, lsp, cap, ct_dev, bt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_device(ev, st_dev, 9, n, mw, lsp, cap, ct_dev, bt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_device(ev, st_dev, S, 0, mw, lsp, cap, ct_dev, bt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_device(ev, st_dev, S, (size_t)maxn + 1, mw, lsp, cap, ct_dev, bt_dev, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_device(ev, st_dev, S, n, mw, nullptr, cap + 1, ct_dev, bt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_device(ev, odd(st_dev, 8), S, n, mw, lsp, cap, ct_dev, bt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_device(ev, st_dev, S, n, mw, odd(ls_dev, 4), cap + 1, ct_dev, bt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_device(ev, st_dev, S, n, mw, lsp, cap, odd(ct_dev, 2), bt_dev, caller), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_device(ev, st_dev, S, n, mw, lsp, cap, ct_dev, odd(bt_dev, 1), caller), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_host(nullptr, st.data(), S, n, mw, list.data(), cap, count.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_host(ev, nullptr, S, n, mw, list.data(), cap, count.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_host(ev, st.data(), S, n, mw, list.data(), cap, nullptr, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_host(ev, st.data(), 9, n, mw, list.data(), cap, count.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_host(ev, st.data(), S, 0, mw, list.data(), cap, count.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_host(ev, st.data(), S, n, mw, nullptr, cap + 1, count.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_events_collect_host(ev, st.data(), S, n, mw, list.data(), (size_t)1 << 32, count.data(), nullptr), MTR_E_INVALID);
        rejected += 19;
        CHECK(launches == g_launches && same(ls_dev, list.data(), (size_t)cap * 16) && same(bt_dev, bits.data(), (size_t)n * 4) && same(ct_dev, count.data(), 8));
        CHECK(count[0] == 0x77777777u && count[1] == 0x77777777u);
        // ---- sets created and destroyed with calls queued; a frame collects the garbage ----
        for (int k = 0; k < 3; k++) {
            mtr_anim_events* tmp = nullptr;
            EXPECT(mtr_anim_events_create(dev, C, nk.data(), fl.data(), cnt.data(), mp, maxn, &tmp), MTR_OK);
            for (int q = 0; q < k; q++) {
                EXPECT(mtr_anim_events_collect_device(tmp, st_dev, S, n, mw, lsp, cap, ct_dev, q ? bt_dev : nullptr, q ? caller : caller2), MTR_OK);
                collected++;
            }
            mtr_anim_events_destroy(tmp);  // straight after the call: the kernels are queued (k == 0: never used)
            mtr_frame* f = nullptr;
            EXPECT(mtr_frame_begin(dev, 64, 48, clear, 1.0f, &f), MTR_OK);
            EXPECT(mtr_frame_submit(f), MTR_OK);
            EXPECT(mtr_frame_wait(f), MTR_OK);
            mtr_frame_destroy(f);
        }
        mtr_anim_events_destroy(ev);
        mtr_anim_events_destroy(ev0);
        mtr_anim_events_destroy(nullptr);
        free(st_dev); free(ls_dev); free(bt_dev); free(ct_dev);
    }
    // the one rejection that needs a large set: n * nsteps * the largest marker count of a clip above 2^32 - 1.  Nothing is read.
    {
        const uint32_t nk1 = 1u << 24, fl1 = 1u, cn1 = 1u << 12;
        std::vector<mtr_event_marker> mk(cn1);
        for (uint32_t k = 0; k < cn1; k++) mk[k] = {(float)k, k};
        mtr_anim_events* big = nullptr;
        EXPECT(mtr_anim_events_create(dev, 1, &nk1, &fl1, &cn1, mk.data(), (size_t)1 << 27, &big), MTR_OK);
        const uint64_t launches = g_launches;
        uint32_t two[2] = {5, 6};
        alignas(16) static mtr_root_step one[8];
        EXPECT(mtr_anim_events_collect_device(big, one, 8, (size_t)1 << 17, 0.0f, nullptr, 0, two, nullptr, caller), MTR_E_INVALID);  // 2^17 * 8 * 2^12 = 2^32
        CHECK(launches == g_launches && two[0] == 5 && two[1] == 6);
        rejected++;
        mtr_anim_events_destroy(big);
    }
    hipStreamDestroy(caller);
    hipStreamDestroy(caller2);
    mtr_device_destroy(dev);
    printf("collected=%ld rejected=%ld launches=%llu failed=%d\n", collected, rejected, (unsigned long long)g_launches, g_failed);
    return g_failed ? 1 : 0;
}
