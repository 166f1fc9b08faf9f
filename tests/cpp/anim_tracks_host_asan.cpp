// AddressSanitizer / UBSan run of the HOST side of animation tracks (csrc/host_anim.cpp, csrc/host_batch.cpp: mtr_anim_create_tracks and the
// section-14 entry points on a track set) over the stand-in HIP runtime (tests/cpp/hip_stub: device memory = host heap).
// The k_anim launcher here is a reader: for every instance it touches its state and, of every clip the state names
// (clamped), the first and last key of the uniform set, or the first and last descriptor of the track set and the first
// and last time and value those descriptors own, and it writes the last word of the output.  A wrong size or offset on
// the host side is an ASan report.   usage: anim_tracks_host_asan <iterations>
#define MTR_RND_SEED 0x243F6A8885A308D3ull
#include "harness.h"
#include "../../mt_renderer_amd/csrc/mtr_files.cpp"

static uint64_t g_key_reads = 0, g_track_reads = 0;
static void touch_uniform(const AnimParams& p, uint32_t ninst) {
    if (!p.keys || p.tracks || p.values || p.times) abort();
    float acc = 0.0f;
    const uint32_t J = p.pose.njoints;
    for (uint32_t i = 0; i < ninst; i++) {
        const uint32_t* st = p.states + (size_t)i * 6;
        for (int k = 0; k < 2; k++) {
            const uint32_t c = st[k] < p.nclips ? st[k] : p.nclips - 1u;
            const uint32_t first = p.clips[c * 4], n = p.clips[c * 4 + 1];
            if (n == 0 || p.clips[c * 4 + 3] != 0) abort();
            acc += p.keys[(size_t)first * J * 12] + p.keys[((size_t)(first + n) * J) * 12 - 1];
            g_key_reads += 2;
        }
        acc += (float)(st[2] + st[3] + st[4] + st[5]);
    }
    p.pose.out[(size_t)ninst * J * 16 - 1] = acc;
}
static void touch_tracks(const AnimParams& p, uint32_t ninst) {
    if (p.keys || !p.tracks || !p.values || !p.times) abort();
    if (((uintptr_t)p.tracks & 15u) || ((uintptr_t)p.values & 7u) || ((uintptr_t)p.times & 1u)) abort();  // what the kernel's loads assume
    uint32_t acc = 0;
    const uint32_t J = p.pose.njoints;
    for (uint32_t i = 0; i < ninst; i++) {
        const uint32_t* st = p.states + (size_t)i * 6;
        for (int k = 0; k < 2; k++) {
            const uint32_t c = st[k] < p.nclips ? st[k] : p.nclips - 1u;
            const uint32_t ticks = p.clips[c * 4 + 1];
            if (ticks == 0 || ticks > 65536u || p.clips[c * 4 + 3] != 0) abort();
            const uint32_t* ends[2] = {p.tracks + (size_t)c * J * 3 * 8, p.tracks + ((size_t)(c + 1) * J * 3 - 1) * 8};
            for (const uint32_t* d : ends) {
                const uint32_t first = d[0], count = d[1];
                if (count == 0) abort();
                acc += d[7];  // the descriptor's last word
                if (p.times[first] != 0 || p.times[first + count - 1] >= ticks) abort();
                acc += p.values[(size_t)first * 2] + p.values[(size_t)(first + count) * 2 - 1];
                g_track_reads += 4;
            }
        }
        acc += st[2] + st[3] + st[4] + st[5];
    }
    p.pose.out[(size_t)ninst * J * 16 - 1] = (float)acc;
}
static void check_skeleton(const AnimParams& p) { if (p.pose.imats[(size_t)p.pose.njoints * 16 - 1] != 1.0f) abort(); }
void mtr_launch_anim(const AnimParams& p, bool tracks, bool fold, uint32_t ninst, hipStream_t) {
    if (fold) check_skeleton(p);
    if (tracks) touch_tracks(p, ninst); else touch_uniform(p, ninst);
}

// a valid random track set: exactly sized arrays, so that one key too many read by the library is an ASan report
struct Set {
    uint32_t J = 0;
    std::vector<uint32_t> nticks, flags;
    std::vector<mtr_anim_track> tracks;
    std::vector<uint16_t> times, values;
    int32_t create(mtr_device* dev, mtr_anim** out, bool with_flags = true) const {
        return mtr_anim_create_tracks(dev, J, nticks.size(), nticks.data(), with_flags ? flags.data() : nullptr, tracks.data(), times.data(),
                                      values.data(), times.size(), out);
    }
};
static Set make_set(uint32_t J, uint32_t nclips) {
    Set s;
    s.J = J;
    for (uint32_t c = 0; c < nclips; c++) {
        const uint32_t ticks = c == 0 ? 65536u : (rnd() % 4 ? pick(4, 300) : 1u);
        s.nticks.push_back(ticks);
        s.flags.push_back((uint32_t)rnd() & 3u);
        for (uint32_t t = 0; t < J * 3; t++) {
            uint32_t count = std::min(ticks, rnd() % 3 ? pick(1, 5) : pick(1, 70));
            mtr_anim_track d{};
            d.first = (uint32_t)s.times.size(); d.count = count;
            d.step[0] = d.step[1] = d.step[2] = 0.001f;
            uint32_t tick = 0;
            for (uint32_t k = 0; k < count; k++) {
                s.times.push_back((uint16_t)tick);
                for (int w = 0; w < 4; w++) s.values.push_back((uint16_t)rnd());
                const uint32_t room = ticks - 1u - tick - (count - 1u - k);  // ticks left beyond what the remaining keys need
                tick += 1u + (room && k + 1 < count ? (uint32_t)(rnd() % std::min(room, 600u)) : 0u);
            }
            s.tracks.push_back(d);
        }
    }
    return s;
}

int main(int argc, char** argv) {
    const long iters = argc > 1 ? strtol(argv[1], nullptr, 10) : 100;
    static const float verts[24] = {1, 1, -1, 1, -1, -1, 1, 1, 1, 1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1};
    static const uint16_t idx[36] = {4, 2, 0, 2, 7, 3, 6, 5, 7, 1, 7, 5, 0, 3, 1, 4, 1, 5, 4, 6, 2, 2, 6, 7, 6, 4, 5, 1, 3, 7, 0, 2, 3, 4, 0, 1};
    mtr_device *dev = nullptr, *dev2 = nullptr;
    if (mtr_device_create(0, &dev) || mtr_device_create(0, &dev2)) return 3;
    mtr_primitive p{};
    p.w[0] = 8u << 16;
    p.w[2] = (12u << 16) | (3u << 24);
    p.w[7] = 36;
    mtr_layout l{};
    l.num_elements = 1;
    l.elements[0].semantic = MTR_SEM_POSITION; l.elements[0].format = MTR_IEF_F32; l.elements[0].count = 3;
    const int32_t p2t = -1;
    const uint32_t dbg = 3;
    const float clear[4] = {1, 1, 1, 1};
    const float vp[16] = {0.25f, 0.1f, 0.05f, 0, -0.1f, 0.25f, 0.05f, 0, 0.05f, -0.05f, 0.1f, 0, 0, 0, 0.5f, 1};
    long animated = 0, rejected = 0;
    for (long it = 0; it < iters; it++) {
        mtr_model* model = nullptr;
        EXPECT(mtr_model_create(dev, verts, sizeof verts, idx, 36, &p, 1, &l, &p2t, nullptr, 0, &dbg, &model), MTR_OK);
        const uint32_t J = it % 9 == 0 ? 256 : pick(1, 70), n = pick(1, 40);
        std::vector<uint8_t> parents(J);
        for (uint32_t j = 0; j < J; j++) parents[j] = j ? (uint8_t)(rnd() % j) : 255;
        std::vector<float> imats((size_t)J * 16, 1.0f), mats((size_t)n * 16, 0.0f);
        EXPECT(mtr_model_set_skeleton(model, parents.data(), imats.data(), J), MTR_OK);
        mtr_batch* batch = nullptr;
        EXPECT(mtr_batch_create(dev, model, n, mats.data(), nullptr, 0, nullptr, &batch), MTR_OK);
        const uint32_t nclips = pick(1, 4);
        const Set good = make_set(J, nclips);
        // ---- every invalid creation, one violation at a time ----
        mtr_anim* none = (mtr_anim*)1;
        auto bad = [&](const Set& s) { return s.create(dev, &none); };
        { Set s = good; s.J = 0; EXPECT(bad(s), MTR_E_INVALID); }
        { Set s = good; s.J = 257; EXPECT(bad(s), MTR_E_INVALID); }
        EXPECT(mtr_anim_create_tracks(dev, J, 0, good.nticks.data(), nullptr, good.tracks.data(), good.times.data(), good.values.data(), good.times.size(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_create_tracks(dev, J, nclips, nullptr, nullptr, good.tracks.data(), good.times.data(), good.values.data(), good.times.size(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_create_tracks(dev, J, nclips, good.nticks.data(), nullptr, nullptr, good.times.data(), good.values.data(), good.times.size(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_create_tracks(dev, J, nclips, good.nticks.data(), nullptr, good.tracks.data(), nullptr, good.values.data(), good.times.size(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_create_tracks(dev, J, nclips, good.nticks.data(), nullptr, good.tracks.data(), good.times.data(), nullptr, good.times.size(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_create_tracks(dev, J, nclips, good.nticks.data(), nullptr, good.tracks.data(), good.times.data(), good.values.data(), 0, &none), MTR_E_INVALID);
        EXPECT(mtr_anim_create_tracks(dev, J, nclips, good.nticks.data(), nullptr, good.tracks.data(), good.times.data(), good.values.data(), (size_t)1 << 31, &none), MTR_E_INVALID);
        EXPECT(mtr_anim_create_tracks(nullptr, J, nclips, good.nticks.data(), nullptr, good.tracks.data(), good.times.data(), good.values.data(), good.times.size(), &none), MTR_E_INVALID);
        { Set s = good; s.nticks[rnd() % nclips] = 0; EXPECT(bad(s), MTR_E_INVALID); }
        { Set s = good; s.nticks[rnd() % nclips] = 65537; EXPECT(bad(s), MTR_E_INVALID); }
        const size_t ti = rnd() % good.tracks.size();
        { Set s = good; s.tracks[ti].count = 0; EXPECT(bad(s), MTR_E_INVALID); }
        { Set s = good; s.tracks[ti].first = (uint32_t)s.times.size() - s.tracks[ti].count + 1u; EXPECT(bad(s), MTR_E_INVALID); }
        { Set s = good; s.tracks[ti].first = 0xFFFFFFFFu; EXPECT(bad(s), MTR_E_INVALID); }                       // first + count wraps
        { Set s = good; s.tracks[ti].count = 0xFFFFFFFFu; EXPECT(bad(s), MTR_E_INVALID); }
        { Set s = good; s.times[s.tracks[ti].first] = 1; EXPECT(bad(s), MTR_E_INVALID); }
        {
            // a track with at least two keys: equal times, falling times, a last time at the clip's length
            size_t tj = ti;
            while (good.tracks[tj].count < 2 && tj + 1 < good.tracks.size()) tj++;
            while (good.tracks[tj].count < 2 && tj > 0) tj--;
            const mtr_anim_track& t = good.tracks[tj];
            if (t.count >= 2) {
                const uint32_t ticks = good.nticks[tj / (J * 3)];
                { Set s = good; s.times[t.first + t.count - 1] = s.times[t.first + t.count - 2]; EXPECT(bad(s), MTR_E_INVALID); }
                { Set s = good; s.times[t.first + 1] = 0; EXPECT(bad(s), MTR_E_INVALID); }
                if (ticks < 65536u) { Set s = good; s.times[t.first + t.count - 1] = (uint16_t)ticks; EXPECT(bad(s), MTR_E_INVALID); rejected++; }
                if (!strstr(mtr_last_error(dev), "clip ") || !strstr(mtr_last_error(dev), "joint ") || !strstr(mtr_last_error(dev), "channel ")) {
                    fprintf(stderr, "the error must name clip, joint and channel: %s\n", mtr_last_error(dev));
                    return 1;
                }
                rejected += 2;
            }
        }
        if (none) { fprintf(stderr, "a failed create must clear *out\n"); return 1; }
        rejected += 17;
        // ---- sets of both kinds ----
        mtr_anim *tracks = nullptr, *other = nullptr, *foreign = nullptr, *uniform = nullptr;
        EXPECT(good.create(dev, &tracks, rnd() % 2), MTR_OK);
        EXPECT(good.create(dev2, &foreign), MTR_OK);
        const Set small = make_set(J == 256 ? 255 : J + 1, 1);
        EXPECT(small.create(dev, &other), MTR_OK);
        const uint32_t nk[2] = {pick(1, 30), pick(1, 30)};
        std::vector<mtr_anim_key> keys((size_t)(nk[0] + nk[1]) * J);
        for (auto& k : keys) { k = mtr_anim_key{}; k.q[3] = 1.0f; }
        EXPECT(mtr_anim_create(dev, J, 2, nk, nullptr, keys.data(), &uniform), MTR_OK);
        std::vector<mtr_anim_state> st(n);
        for (auto& s : st) {
            s.clip_a = rnd() % 4 ? pick(0, nclips - 1) : (uint32_t)rnd();
            s.clip_b = rnd() % 4 ? pick(0, nclips - 1) : 0xFFFFFFFFu;
            s.x_a = (float)(rnd() % 100000) * 0.37f - 100.0f;
            s.x_b = rnd() % 5 ? (float)(rnd() % 1000) : NAN;
            s.w = rnd() % 3 ? (float)(rnd() % 100) * 0.01f : 0.0f;
            s.pad = (uint32_t)rnd();
        }
        EXPECT(mtr_batch_animate(batch, tracks, st.data()), MTR_OK);
        EXPECT(mtr_batch_animate_device(batch, tracks, st.data(), nullptr), MTR_OK);  // stub runtime: device memory is host memory
        EXPECT(mtr_model_animate(model, tracks, &st[0]), MTR_OK);
        animated += 3;
        EXPECT(mtr_batch_animate(batch, other, st.data()), MTR_E_INVALID);
        EXPECT(mtr_batch_animate(batch, foreign, st.data()), MTR_E_INVALID);
        EXPECT(mtr_batch_animate(batch, tracks, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_device(batch, tracks, (const mtr_anim_state*)((const char*)st.data() + 4), nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_device(batch, foreign, st.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_model_animate(model, other, &st[0]), MTR_E_INVALID);
        EXPECT(mtr_model_animate(model, tracks, nullptr), MTR_E_INVALID);
        rejected += 7;
        std::vector<float> locals((size_t)n * J * 16);
        EXPECT(mtr_anim_sample(tracks, st.data(), n, locals.data(), locals.size()), MTR_OK);
        EXPECT(mtr_anim_sample(tracks, st.data(), n, locals.data(), locals.size() - 1), MTR_E_INVALID);
        EXPECT(mtr_anim_sample(tracks, st.data(), 0, nullptr, 0), MTR_OK);
        // ---- one batch animated alternately from the uniform and the track set, frames in flight, sets coming and going ----
        mtr_frame* frames[4] = {};
        int k = 0;
        for (auto& f : frames) {
            EXPECT(mtr_batch_animate(batch, k % 2 ? uniform : tracks, st.data()), MTR_OK);
            EXPECT(mtr_model_animate(model, k % 2 ? tracks : uniform, &st[0]), MTR_OK);
            animated += 2;
            EXPECT(mtr_frame_begin(dev, 64, 48, clear, 1.0f, &f), MTR_OK);
            EXPECT(mtr_frame_draw_batch(f, batch, vp), MTR_OK);
            EXPECT(mtr_frame_draw_model(f, model, vp), MTR_OK);
            EXPECT(mtr_frame_submit(f), MTR_OK);
            if (k == 1) {  // a set of each kind created and destroyed while frames are in flight
                mtr_anim* tmp = nullptr;
                EXPECT(good.create(dev, &tmp), MTR_OK);
                EXPECT(mtr_batch_animate(batch, tmp, st.data()), MTR_OK);
                mtr_anim_destroy(tmp);
                EXPECT(mtr_anim_create(dev, J, 2, nk, nullptr, keys.data(), &tmp), MTR_OK);
                EXPECT(mtr_batch_animate(batch, tmp, st.data()), MTR_OK);
                mtr_anim_destroy(tmp);
                animated += 2;
            }
            k++;
        }
        mtr_anim_destroy(tracks);  // straight after a submit
        mtr_anim_destroy(uniform);
        mtr_anim_destroy(other);
        mtr_anim_destroy(foreign);
        for (auto& f : frames) { EXPECT(mtr_frame_wait(f), MTR_OK); mtr_frame_destroy(f); }
        mtr_batch_destroy(batch);
        mtr_model_destroy(model);
    }
    mtr_device_destroy(dev2);
    mtr_device_destroy(dev);
    printf("animated=%ld rejected=%ld key_reads=%llu track_reads=%llu\n", animated, rejected, (unsigned long long)g_key_reads, (unsigned long long)g_track_reads);
    return 0;
}
