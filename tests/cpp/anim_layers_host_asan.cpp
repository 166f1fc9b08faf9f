// AddressSanitizer / UBSan run of the HOST side of animation layers (csrc/host_anim.cpp, csrc/host_batch.cpp: mtr_anim_masks_create / _destroy,
// mtr_model_animate_layers, mtr_batch_animate_layers, mtr_batch_animate_layers_device, mtr_anim_sample_layers) over the
// stand-in HIP runtime (tests/cpp/hip_stub: device memory = host heap).  The k_anim_layers launcher here is a reader:
// for every instance it touches its first and last layer and, of every layer, the first and last weight of the mask it
// names (clamped) and the clip table entry with the first and last key (or descriptor) of the clip it names (clamped), and
// it writes the last word of the output.  A wrong size or offset on the host side is an ASan report.
//   usage: anim_layers_host_asan <iterations>
#define MTR_RND_SEED 0x13198A2E03707344ull
#include "harness.h"
#include "../../mt_renderer_amd/csrc/mtr_files.cpp"

// the section-14 launchers: the plain animate calls are made here too, between the layered ones
void mtr_launch_anim(const AnimParams& p, bool, bool fold, uint32_t ninst, hipStream_t) {
    if (!fold) abort();  // no plain sample call is made here
    p.pose.out[(size_t)ninst * p.pose.njoints * 16 - 1] = (float)p.states[(size_t)ninst * 6 - 1];
}

static uint64_t g_layer_reads = 0, g_mask_reads = 0, g_clip_reads = 0;
static void touch_layers(const AnimLayerParams& p, uint32_t ninst, bool tracks) {
    const AnimParams& a = p.anim;
    if (a.states || !p.layers || ((uintptr_t)p.layers & 15u) || p.nlayers < 1 || p.nlayers > MTR_ANIM_MAX_LAYERS) abort();
    if ((p.nmasks != 0) != (p.masks != nullptr)) abort();
    if (tracks ? (a.keys || !a.tracks || !a.values || !a.times) : (!a.keys || a.tracks)) abort();
    const uint32_t J = a.pose.njoints;
    float acc = 0.0f;
    for (uint32_t i = 0; i < ninst; i++)
        for (uint32_t l = 0; l < p.nlayers; l++) {
            const uint32_t* rec = p.layers + ((size_t)i * p.nlayers + l) * 4;  // the first and the last layer of the call among them
            g_layer_reads++;
            uint32_t mask = rec[3] & 0xFFFFu;
            mask = mask < p.nmasks ? mask : p.nmasks;
            if (mask) {
                const float m0 = p.masks[(size_t)(mask - 1u) * J], m1 = p.masks[(size_t)mask * J - 1];
                if (!(m0 >= 0.0f && m0 <= 1.0f && m1 >= 0.0f && m1 <= 1.0f)) abort();
                acc += m0 + m1;
                g_mask_reads += 2;
            }
            const uint32_t c = rec[0] < a.nclips ? rec[0] : a.nclips - 1u;
            const uint32_t* ct = a.clips + (size_t)c * 4;
            if (ct[1] == 0 || ct[3] != 0) abort();
            if (tracks) {
                const uint32_t* ends[2] = {a.tracks + (size_t)c * J * 3 * 8, a.tracks + ((size_t)(c + 1) * J * 3 - 1) * 8};
                for (const uint32_t* d : ends) {
                    if (d[1] == 0 || a.times[d[0]] != 0) abort();
                    acc += (float)(a.values[(size_t)d[0] * 2] + a.values[(size_t)(d[0] + d[1]) * 2 - 1]);
                }
            } else {
                acc += a.keys[(size_t)ct[0] * J * 12] + a.keys[((size_t)(ct[0] + ct[1]) * J) * 12 - 1];
            }
            g_clip_reads += 2;
        }
    a.pose.out[(size_t)ninst * J * 16 - 1] = acc;
}
static void check_skeleton(const AnimLayerParams& p) { if (p.anim.pose.imats[(size_t)p.anim.pose.njoints * 16 - 1] != 1.0f) abort(); }
void mtr_launch_anim_layers(const AnimLayerParams& p, bool tracks, bool fold, uint32_t ninst, hipStream_t) {
    if (fold) check_skeleton(p);
    touch_layers(p, ninst, tracks);
}

// a one-clip-per-entry track set with one key per track: exactly sized arrays
static int32_t make_tracks(mtr_device* dev, uint32_t J, uint32_t nclips, mtr_anim** out) {
    std::vector<uint32_t> nticks(nclips, 16u);
    std::vector<mtr_anim_track> tr((size_t)nclips * J * 3);
    std::vector<uint16_t> times(tr.size(), 0), values(tr.size() * 4, 7);
    for (size_t t = 0; t < tr.size(); t++) { tr[t] = mtr_anim_track{}; tr[t].first = (uint32_t)t; tr[t].count = 1; }
    return mtr_anim_create_tracks(dev, J, nclips, nticks.data(), nullptr, tr.data(), times.data(), values.data(), times.size(), out);
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
        mtr_model *model = nullptr, *bare = nullptr;
        EXPECT(mtr_model_create(dev, verts, sizeof verts, idx, 36, &p, 1, &l, &p2t, nullptr, 0, &dbg, &model), MTR_OK);
        EXPECT(mtr_model_create(dev, verts, sizeof verts, idx, 36, &p, 1, &l, &p2t, nullptr, 0, &dbg, &bare), MTR_OK);  // no skeleton
        const uint32_t J = it % 9 == 0 ? 256 : pick(1, 70), n = pick(1, 40), L = it % 7 == 0 ? 8 : pick(1, 8);
        std::vector<uint8_t> parents(J);
        for (uint32_t j = 0; j < J; j++) parents[j] = j ? (uint8_t)(rnd() % j) : 255;
        std::vector<float> imats((size_t)J * 16, 1.0f), mats((size_t)n * 16, 0.0f);
        EXPECT(mtr_model_set_skeleton(model, parents.data(), imats.data(), J), MTR_OK);
        mtr_batch* batch = nullptr;
        EXPECT(mtr_batch_create(dev, model, n, mats.data(), nullptr, 0, nullptr, &batch), MTR_OK);
        // ---- mask sets: every invalid creation, one violation at a time; exactly sized weights ----
        const uint32_t M = pick(1, 5);
        std::vector<float> weights((size_t)M * J);
        for (auto& w : weights) w = rnd() % 3 == 0 ? 0.0f : (rnd() % 4 == 0 ? 1.0f : (float)(rnd() % 1000) * 0.001f);
        mtr_anim_masks* none = (mtr_anim_masks*)1;
        EXPECT(mtr_anim_masks_create(nullptr, J, M, weights.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_masks_create(dev, J, M, weights.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_masks_create(dev, 0, M, weights.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_masks_create(dev, 257, M, weights.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_masks_create(dev, J, 0, weights.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_masks_create(dev, J, M, nullptr, &none), MTR_E_INVALID);
        const size_t wi = rnd() % weights.size();
        const float bad_w[4] = {NAN, -0.001f, 1.0001f, INFINITY};
        for (float bw : bad_w) {
            std::vector<float> w2 = weights;
            w2[wi] = bw;
            EXPECT(mtr_anim_masks_create(dev, J, M, w2.data(), &none), MTR_E_INVALID);
            char want[64];
            snprintf(want, sizeof want, "mask %zu, joint %zu ", wi / J + 1, wi % J);
            if (!strstr(mtr_last_error(dev), want)) { fprintf(stderr, "the error must name the mask and the joint (%s): %s\n", want, mtr_last_error(dev)); return 1; }
        }
        if (none) { fprintf(stderr, "a failed create must clear *out\n"); return 1; }
        rejected += 10;
        mtr_anim_masks *masks = nullptr, *masks_other = nullptr, *masks_foreign = nullptr;
        EXPECT(mtr_anim_masks_create(dev, J, M, weights.data(), &masks), MTR_OK);
        EXPECT(mtr_anim_masks_create(dev2, J, M, weights.data(), &masks_foreign), MTR_OK);
        std::vector<float> w_other((size_t)(J == 256 ? 255 : J + 1), 0.5f);
        EXPECT(mtr_anim_masks_create(dev, w_other.size(), 1, w_other.data(), &masks_other), MTR_OK);
        // ---- animation sets of both kinds, one of another joint count, one of another device ----
        const uint32_t nclips = pick(1, 4);
        std::vector<uint32_t> nk(nclips);
        size_t total = 0;
        for (auto& k : nk) { k = pick(1, 20); total += k; }
        std::vector<mtr_anim_key> keys(total * J);
        for (auto& k : keys) { k = mtr_anim_key{}; k.q[3] = 1.0f; }
        mtr_anim *uniform = nullptr, *tracks = nullptr, *other = nullptr, *foreign = nullptr;
        EXPECT(mtr_anim_create(dev, J, nclips, nk.data(), nullptr, keys.data(), &uniform), MTR_OK);
        EXPECT(mtr_anim_create(dev2, J, nclips, nk.data(), nullptr, keys.data(), &foreign), MTR_OK);
        EXPECT(make_tracks(dev, J, nclips, &tracks), MTR_OK);
        EXPECT(make_tracks(dev, J == 256 ? 255 : J + 1, 1, &other), MTR_OK);
        std::vector<mtr_anim_layer> ly((size_t)n * L);  // exactly sized: one layer too many read is a report
        for (auto& r : ly) {
            r.clip = rnd() % 4 ? pick(0, nclips - 1) : (uint32_t)rnd();
            r.x = rnd() % 5 ? (float)(rnd() % 1000) * 0.37f - 50.0f : NAN;
            r.w = rnd() % 3 ? (float)(rnd() % 140) * 0.01f - 0.2f : 0.0f;
            r.mask = rnd() % 4 ? (uint16_t)pick(0, M) : (uint16_t)rnd();
            r.mode = (uint16_t)rnd();
        }
        std::vector<mtr_anim_state> st(n, mtr_anim_state{});
        // ---- the valid calls: both kinds of set, with and without masks, host and "device" layers (stub: host memory) ----
        EXPECT(mtr_batch_animate_layers(batch, uniform, masks, ly.data(), L), MTR_OK);
        EXPECT(mtr_batch_animate_layers(batch, tracks, nullptr, ly.data(), L), MTR_OK);
        EXPECT(mtr_batch_animate_layers_device(batch, tracks, masks, ly.data(), L, nullptr), MTR_OK);
        EXPECT(mtr_batch_animate_layers_device(batch, uniform, nullptr, ly.data(), L, nullptr), MTR_OK);
        EXPECT(mtr_model_animate_layers(model, uniform, masks, ly.data(), L), MTR_OK);
        EXPECT(mtr_model_animate_layers(model, tracks, nullptr, ly.data() + (size_t)(n - 1) * L, L), MTR_OK);
        animated += 6;
        std::vector<float> locals((size_t)n * J * 16);
        EXPECT(mtr_anim_sample_layers(uniform, masks, ly.data(), L, n, locals.data(), locals.size()), MTR_OK);
        EXPECT(mtr_anim_sample_layers(tracks, nullptr, ly.data(), L, n, locals.data(), locals.size()), MTR_OK);
        EXPECT(mtr_anim_sample_layers(tracks, masks, ly.data(), L, 0, nullptr, 0), MTR_OK);
        // ---- every invalid call ----
        EXPECT(mtr_batch_animate_layers(nullptr, uniform, masks, ly.data(), L), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_layers(batch, nullptr, masks, ly.data(), L), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_layers(batch, uniform, masks, nullptr, L), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_layers(batch, uniform, masks, ly.data(), 0), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_layers(batch, uniform, masks, ly.data(), 9), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_layers(batch, uniform, masks_other, ly.data(), L), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_layers(batch, uniform, masks_foreign, ly.data(), L), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_layers(batch, other, masks, ly.data(), L), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_layers(batch, foreign, masks, ly.data(), L), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_layers_device(nullptr, uniform, masks, ly.data(), L, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_layers_device(batch, uniform, masks, nullptr, L, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_layers_device(batch, uniform, masks, (const mtr_anim_layer*)((const char*)ly.data() + 8), L, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_layers_device(batch, uniform, masks, ly.data(), 9, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_layers_device(batch, tracks, masks_other, ly.data(), L, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_layers_device(batch, foreign, nullptr, ly.data(), L, nullptr), MTR_E_INVALID);
        EXPECT(mtr_model_animate_layers(nullptr, uniform, masks, ly.data(), L), MTR_E_INVALID);
        EXPECT(mtr_model_animate_layers(model, nullptr, masks, ly.data(), L), MTR_E_INVALID);
        EXPECT(mtr_model_animate_layers(model, uniform, masks, nullptr, L), MTR_E_INVALID);
        EXPECT(mtr_model_animate_layers(model, uniform, masks, ly.data(), 0), MTR_E_INVALID);
        EXPECT(mtr_model_animate_layers(model, uniform, masks_foreign, ly.data(), L), MTR_E_INVALID);
        EXPECT(mtr_model_animate_layers(model, other, nullptr, ly.data(), L), MTR_E_INVALID);
        EXPECT(mtr_model_animate_layers(bare, uniform, nullptr, ly.data(), L), MTR_E_INVALID);
        EXPECT(mtr_anim_sample_layers(nullptr, masks, ly.data(), L, n, locals.data(), locals.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_sample_layers(uniform, masks, ly.data(), 0, n, locals.data(), locals.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_sample_layers(uniform, masks, ly.data(), 9, n, locals.data(), locals.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_sample_layers(uniform, masks_other, ly.data(), L, n, locals.data(), locals.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_sample_layers(uniform, masks, nullptr, L, n, locals.data(), locals.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_sample_layers(uniform, masks, ly.data(), L, n, locals.data(), locals.size() - 1), MTR_E_INVALID);
        rejected += 28;
        // ---- one batch animated by the three kinds of call with frames in flight, mask and clip sets coming and going ----
        mtr_frame* frames[4] = {};
        int k = 0;
        for (auto& f : frames) {
            if (k % 2) EXPECT(mtr_batch_animate(batch, k == 1 ? uniform : tracks, st.data()), MTR_OK);
            else EXPECT(mtr_batch_animate_layers(batch, k == 0 ? uniform : tracks, masks, ly.data(), L), MTR_OK);
            EXPECT(mtr_model_animate_layers(model, k % 2 ? tracks : uniform, k == 3 ? nullptr : masks, ly.data(), L), MTR_OK);
            animated += 2;
            mtr_anim_masks* tmp = nullptr;
            if (k == 1) {  // a mask set created, used and destroyed straight after the submit
                EXPECT(mtr_anim_masks_create(dev, J, M, weights.data(), &tmp), MTR_OK);
                EXPECT(mtr_batch_animate_layers(batch, uniform, tmp, ly.data(), L), MTR_OK);
                animated++;
            }
            EXPECT(mtr_frame_begin(dev, 64, 48, clear, 1.0f, &f), MTR_OK);
            EXPECT(mtr_frame_draw_batch(f, batch, vp), MTR_OK);
            EXPECT(mtr_frame_draw_model(f, model, vp), MTR_OK);
            EXPECT(mtr_frame_submit(f), MTR_OK);
            mtr_anim_masks_destroy(tmp);
            k++;
        }
        mtr_anim_masks_destroy(masks);  // straight after a submit
        mtr_anim_masks_destroy(masks_other);
        mtr_anim_masks_destroy(masks_foreign);
        mtr_anim_masks_destroy(nullptr);
        mtr_anim_destroy(uniform);
        mtr_anim_destroy(tracks);
        mtr_anim_destroy(other);
        mtr_anim_destroy(foreign);
        for (auto& f : frames) { EXPECT(mtr_frame_wait(f), MTR_OK); mtr_frame_destroy(f); }
        mtr_batch_destroy(batch);
        mtr_model_destroy(model);
        mtr_model_destroy(bare);
    }
    mtr_device_destroy(dev2);
    mtr_device_destroy(dev);
    printf("animated=%ld rejected=%ld layer_reads=%llu mask_reads=%llu clip_reads=%llu\n", animated, rejected, (unsigned long long)g_layer_reads,
           (unsigned long long)g_mask_reads, (unsigned long long)g_clip_reads);
    return 0;
}
