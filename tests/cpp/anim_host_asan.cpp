// AddressSanitizer / UBSan run of the HOST side of the animation entry points (csrc/host_anim.cpp, csrc/host_batch.cpp: mtr_anim_*, mtr_*_animate*)
// over the stand-in HIP runtime (tests/cpp/hip_stub: device memory = host heap).  The k_anim launcher here is a reader: it
// touches, for every instance, its state and the first and last word of the keys its (clamped) clips own, and the last word of
// what it would write, so a wrong size or offset on the host side is an ASan report.   usage: anim_host_asan <iterations>
#define MTR_RND_SEED 0x13198A2E03707344ull
#include "harness.h"
#include "../../mt_renderer_amd/csrc/mtr_files.cpp"

static uint64_t g_reads = 0;
static float touch(const AnimParams& p, uint32_t ninst) {
    float acc = 0.0f;
    const uint32_t J = p.pose.njoints;
    for (uint32_t i = 0; i < ninst; i++) {
        const uint32_t* st = p.states + (size_t)i * 6;
        for (int k = 0; k < 2; k++) {
            const uint32_t c = st[k] < p.nclips ? st[k] : p.nclips - 1u;
            const uint32_t first = p.clips[c * 4], n = p.clips[c * 4 + 1];
            if (n == 0 || p.clips[c * 4 + 3] != 0) abort();
            acc += p.keys[(size_t)first * J * 12] + p.keys[((size_t)(first + n) * J) * 12 - 1];
            g_reads += 2;
        }
        acc += (float)(st[2] + st[3] + st[4] + st[5]);
    }
    p.pose.out[(size_t)ninst * J * 16 - 1] = acc;
    return acc;
}
void mtr_launch_anim(const AnimParams& p, bool tracks, bool fold, uint32_t ninst, hipStream_t) {
    if (tracks) abort();  // uniform sets only here
    if (fold && p.pose.imats[(size_t)p.pose.njoints * 16 - 1] != 1.0f) abort();  // the skeleton's last inverse bind element
    touch(p, ninst);
}

int main(int argc, char** argv) {
    const long iters = argc > 1 ? strtol(argv[1], nullptr, 10) : 200;
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
        mtr_model *model = nullptr, *bare = nullptr;
        EXPECT(mtr_model_create(dev, verts, sizeof verts, idx, 36, &p, 1, &l, &p2t, nullptr, 0, &dbg, &model), MTR_OK);
        EXPECT(mtr_model_create(dev, verts, sizeof verts, idx, 36, &p, 1, &l, &p2t, nullptr, 0, &dbg, &bare), MTR_OK);
        const uint32_t J = it % 7 == 0 ? 256 : pick(1, 70), n = pick(1, 40);
        std::vector<uint8_t> parents(J);
        for (uint32_t j = 0; j < J; j++) parents[j] = j ? (uint8_t)(rnd() % j) : 255;
        std::vector<float> imats((size_t)J * 16, 1.0f), mats((size_t)n * 16, 0.0f);
        EXPECT(mtr_model_set_skeleton(model, parents.data(), imats.data(), J), MTR_OK);
        mtr_batch *batch = nullptr, *bare_batch = nullptr;
        EXPECT(mtr_batch_create(dev, model, n, mats.data(), nullptr, 0, nullptr, &batch), MTR_OK);
        EXPECT(mtr_batch_create(dev, bare, n, mats.data(), nullptr, 0, nullptr, &bare_batch), MTR_OK);
        // ---- creation: valid and invalid shapes ----
        const uint32_t nclips = pick(1, 5);
        std::vector<uint32_t> nkeys(nclips), flags(nclips);
        size_t total = 0;
        for (uint32_t c = 0; c < nclips; c++) { nkeys[c] = pick(1, 40); flags[c] = (uint32_t)rnd() & 3u; total += nkeys[c]; }
        std::vector<mtr_anim_key> keys(total * J);
        for (auto& k : keys) { k = mtr_anim_key{}; k.q[3] = 1.0f; k.s[0] = k.s[1] = k.s[2] = 1.0f; }
        mtr_anim *anim = nullptr, *other = nullptr, *foreign = nullptr, *none = (mtr_anim*)1;
        EXPECT(mtr_anim_create(dev, 0, nclips, nkeys.data(), flags.data(), keys.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_create(dev, 257, nclips, nkeys.data(), flags.data(), keys.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_create(dev, J, 0, nkeys.data(), flags.data(), keys.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_create(dev, J, nclips, nullptr, flags.data(), keys.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_create(dev, J, nclips, nkeys.data(), flags.data(), nullptr, &none), MTR_E_INVALID);
        EXPECT(mtr_anim_create(nullptr, J, nclips, nkeys.data(), flags.data(), keys.data(), &none), MTR_E_INVALID);
        {
            std::vector<uint32_t> zero = nkeys;
            zero[rnd() % nclips] = 0;
            EXPECT(mtr_anim_create(dev, J, nclips, zero.data(), flags.data(), keys.data(), &none), MTR_E_INVALID);
            zero[rnd() % nclips] = 0xFFFFFFFFu;
            EXPECT(mtr_anim_create(dev, J, nclips, zero.data(), flags.data(), keys.data(), &none), MTR_E_INVALID);
        }
        if (none) { fprintf(stderr, "a failed create must clear *out\n"); return 1; }
        rejected += 8;
        EXPECT(mtr_anim_create(dev, J, nclips, nkeys.data(), rnd() % 2 ? flags.data() : nullptr, keys.data(), &anim), MTR_OK);
        const uint32_t J2 = J == 256 ? 255 : J + 1;
        std::vector<mtr_anim_key> keys2((size_t)J2);
        const uint32_t one = 1;
        EXPECT(mtr_anim_create(dev, J2, 1, &one, nullptr, keys2.data(), &other), MTR_OK);
        EXPECT(mtr_anim_create(dev2, J, nclips, nkeys.data(), flags.data(), keys.data(), &foreign), MTR_OK);
        // ---- states: mostly sane, sometimes hostile ----
        std::vector<mtr_anim_state> st(n);
        for (auto& s : st) {
            s.clip_a = rnd() % 4 ? pick(0, nclips - 1) : (uint32_t)rnd();
            s.clip_b = rnd() % 4 ? pick(0, nclips - 1) : 0xFFFFFFFFu;
            s.x_a = (float)(rnd() % 1000) * 0.37f - 100.0f;
            s.x_b = rnd() % 5 ? (float)(rnd() % 1000) : NAN;
            s.w = rnd() % 3 ? (float)(rnd() % 100) * 0.01f : 0.0f;
            s.pad = (uint32_t)rnd();
        }
        EXPECT(mtr_batch_animate(batch, anim, st.data()), MTR_OK);
        EXPECT(mtr_batch_animate_device(batch, anim, st.data(), nullptr), MTR_OK);  // stub runtime: device memory is host memory
        EXPECT(mtr_model_animate(model, anim, &st[0]), MTR_OK);
        animated += 3;
        EXPECT(mtr_batch_animate(nullptr, anim, st.data()), MTR_E_INVALID);
        EXPECT(mtr_batch_animate(batch, nullptr, st.data()), MTR_E_INVALID);
        EXPECT(mtr_batch_animate(batch, anim, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate(batch, other, st.data()), MTR_E_INVALID);
        EXPECT(mtr_batch_animate(batch, foreign, st.data()), MTR_E_INVALID);
        EXPECT(mtr_batch_animate(bare_batch, anim, st.data()), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_device(batch, anim, (const mtr_anim_state*)((const char*)st.data() + 4), nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_device(batch, anim, nullptr, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_device(batch, foreign, st.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_model_animate(bare, anim, &st[0]), MTR_E_INVALID);
        EXPECT(mtr_model_animate(model, other, &st[0]), MTR_E_INVALID);
        EXPECT(mtr_model_animate(model, anim, nullptr), MTR_E_INVALID);
        EXPECT(mtr_model_animate(nullptr, anim, &st[0]), MTR_E_INVALID);
        rejected += 13;
        std::vector<float> locals((size_t)n * J * 16);
        EXPECT(mtr_anim_sample(anim, st.data(), n, locals.data(), locals.size()), MTR_OK);
        EXPECT(mtr_anim_sample(anim, st.data(), n, locals.data(), locals.size() - 1), MTR_E_INVALID);
        EXPECT(mtr_anim_sample(anim, nullptr, n, locals.data(), locals.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_sample(anim, st.data(), 0, nullptr, 0), MTR_OK);
        EXPECT(mtr_anim_sample(nullptr, st.data(), n, locals.data(), locals.size()), MTR_E_INVALID);
        std::vector<float> pal((size_t)n * J * 16);
        EXPECT(mtr_batch_read_palettes(batch, pal.data(), pal.size()), MTR_OK);  // npal = njoints after animate
        // ---- frames in flight around animate calls and an early destroy ----
        mtr_frame* frames[3] = {};
        for (auto& f : frames) {
            EXPECT(mtr_batch_animate(batch, anim, st.data()), MTR_OK);
            EXPECT(mtr_frame_begin(dev, 64, 48, clear, 1.0f, &f), MTR_OK);
            EXPECT(mtr_frame_draw_batch(f, batch, vp), MTR_OK);
            EXPECT(mtr_frame_draw_model(f, model, vp), MTR_OK);
            EXPECT(mtr_frame_submit(f), MTR_OK);
        }
        mtr_anim_destroy(anim);  // straight after a submit
        mtr_anim_destroy(other);
        mtr_anim_destroy(foreign);
        mtr_anim_destroy(nullptr);
        for (auto& f : frames) { EXPECT(mtr_frame_wait(f), MTR_OK); mtr_frame_destroy(f); }
        mtr_batch_destroy(batch);
        mtr_batch_destroy(bare_batch);
        mtr_model_destroy(model);
        mtr_model_destroy(bare);
    }
    mtr_device_destroy(dev2);
    mtr_device_destroy(dev);
    printf("animated=%ld rejected=%ld key_reads=%llu\n", animated, rejected, (unsigned long long)g_reads);
    return 0;
}
