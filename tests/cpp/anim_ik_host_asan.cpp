// AddressSanitizer / UBSan run of the HOST side of inverse kinematics (csrc/host_anim.cpp, csrc/host_batch.cpp: mtr_anim_ik_create / _destroy,
// mtr_model_animate_ik, mtr_batch_animate_ik, mtr_batch_animate_ik_device, mtr_anim_sample_ik) over the stand-in HIP runtime
// (tests/cpp/hip_stub: device memory = host heap).  The k_anim_ik launcher here is a reader: for every instance it
// touches its first and last layer and its first and last target, every chain of the set, the path table entry of every
// chain's joint a with the first and last byte of that path, and it writes the last word of the output.  A wrong size or
// offset on the host side is an ASan report.
//   usage: anim_ik_host_asan <iterations>
#define MTR_RND_SEED 0x243F6A8885A308D3ull
#include "harness.h"
#include "../../mt_renderer_amd/csrc/mtr_files.cpp"

// the other pose sources: the plain, layered and posed calls are made here too, between the IK ones
void mtr_launch_pose(const PoseParams& p, uint32_t ninst, hipStream_t) { p.out[(size_t)ninst * p.njoints * 16 - 1] = p.locals[(size_t)ninst * p.njoints * 16 - 1]; }
void mtr_launch_anim(const AnimParams& p, bool, bool fold, uint32_t ninst, hipStream_t) {
    if (!fold) abort();  // no plain or layered sample call is made here
    p.pose.out[(size_t)ninst * p.pose.njoints * 16 - 1] = (float)p.states[(size_t)ninst * 6 - 1];
}
void mtr_launch_anim_layers(const AnimLayerParams& p, bool, bool fold, uint32_t ninst, hipStream_t) {
    if (!fold) abort();
    p.anim.pose.out[(size_t)ninst * p.anim.pose.njoints * 16 - 1] = (float)p.layers[(size_t)ninst * p.nlayers * 4 - 1];
}

static uint64_t g_target_reads = 0, g_chain_reads = 0, g_path_reads = 0;
static void touch_ik(const AnimIkParams& p, uint32_t ninst, bool tracks, bool fold) {
    const AnimLayerParams& lp = p.layers;
    const AnimParams& a = lp.anim;
    const uint32_t J = a.pose.njoints;
    if (a.states || !lp.layers || ((uintptr_t)lp.layers & 15u) || lp.nlayers < 1 || lp.nlayers > MTR_ANIM_MAX_LAYERS) abort();
    if (!p.targets || ((uintptr_t)p.targets & 15u) || !p.chains || p.nchains < 1 || p.nchains > MTR_ANIM_MAX_IK) abort();
    if (!p.paths || !p.path_words || p.path_bytes == 0 || p.path_bytes > MTR_POSE_MAX_PATH_BYTES) abort();
    if (tracks ? (a.keys || !a.tracks) : (!a.keys || a.tracks)) abort();
    if (fold) {  // the model's own path table, and its inverse bind matrices
        if (p.paths != a.pose.paths || p.path_words != a.pose.path_words || p.path_bytes != a.pose.path_bytes) abort();
        if (a.pose.imats[(size_t)J * 16 - 1] != 1.0f) abort();
    }
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(p.path_words);
    uint32_t acc = bytes[p.path_bytes - 1];
    for (uint32_t k = 0; k < p.nchains; k++) {
        const uint32_t* ch = p.chains + (size_t)k * 8;
        g_chain_reads++;
        if (ch[0] > 1u || ch[1] >= J || (ch[7] & ~1u)) abort();
        if (ch[0] == 0u && (ch[2] >= J || ch[3] >= J)) abort();
        const uint32_t w = p.paths[ch[1]], ofs = w & 0xFFFFu, len = w >> 16;
        if (len == 0 || ofs + len > p.path_bytes || bytes[ofs + len - 1] != ch[1] || bytes[ofs] >= J) abort();
        acc += p.paths[J - 1];
        g_path_reads += 3;
    }
    for (uint32_t i = 0; i < ninst; i++) {
        acc += lp.layers[(size_t)i * lp.nlayers * 4] + lp.layers[(size_t)(i + 1) * lp.nlayers * 4 - 1];
        acc += p.targets[(size_t)i * p.nchains * 8] + p.targets[(size_t)(i + 1) * p.nchains * 8 - 1];  // the first and last target
        g_target_reads += 2;
    }
    a.pose.out[(size_t)ninst * J * 16 - 1] = (float)acc;
}
void mtr_launch_anim_ik(const AnimIkParams& p, bool tracks, bool fold, uint32_t ninst, hipStream_t) { touch_ik(p, ninst, tracks, fold); }

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
        // a skeleton of at least 4 joints whose last three are a chain: (J-3, J-2, J-1); the rest random; a root as 255 or itself
        const uint32_t J = it % 9 == 0 ? 256 : pick(4, 70), n = pick(1, 40), L = pick(1, 8), K = it % 5 == 0 ? 4 : pick(1, 4);
        std::vector<uint8_t> parents(J);
        for (uint32_t j = 0; j < J; j++) parents[j] = j ? (uint8_t)(j >= J - 2 ? j - 1 : rnd() % j) : (it % 2 ? 255 : 0);
        std::vector<float> imats((size_t)J * 16, 1.0f), mats((size_t)n * 16, 0.0f);
        EXPECT(mtr_model_set_skeleton(model, parents.data(), imats.data(), J), MTR_OK);
        mtr_batch* batch = nullptr;
        EXPECT(mtr_batch_create(dev, model, n, mats.data(), nullptr, 0, nullptr, &batch), MTR_OK);
        std::vector<mtr_ik_chain> chains(K);  // exactly sized
        for (uint32_t k = 0; k < K; k++) {
            mtr_ik_chain& c = chains[k];
            c = mtr_ik_chain{};
            if (k % 2 == 0) { c.kind = MTR_IK_TWO_BONE; c.joint[0] = J - 3; c.joint[1] = J - 2; c.joint[2] = J - 1; c.flags = k ? 0u : MTR_IK_POLE; }
            else { c.kind = MTR_IK_AIM; c.joint[0] = pick(0, J - 1); c.joint[1] = (uint32_t)rnd(); c.joint[2] = (uint32_t)rnd(); c.axis[1] = 1.0f; c.flags = k == 1 ? MTR_IK_POLE : 0u; }
        }
        // ---- IK sets: every invalid creation, one violation at a time ----
        mtr_anim_ik* none = (mtr_anim_ik*)1;
        EXPECT(mtr_anim_ik_create(nullptr, J, parents.data(), K, chains.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_ik_create(dev, J, parents.data(), K, chains.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_ik_create(dev, 0, parents.data(), K, chains.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_ik_create(dev, 257, parents.data(), K, chains.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_ik_create(dev, J, nullptr, K, chains.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_ik_create(dev, J, parents.data(), 0, chains.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_ik_create(dev, J, parents.data(), 5, chains.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_ik_create(dev, J, parents.data(), K, nullptr, &none), MTR_E_INVALID);
        {
            std::vector<uint8_t> cyc = parents;
            cyc[0] = (uint8_t)(J - 2);  // J-2 -> J-3 -> .. -> 0 -> J-2 (never 255, the root's mark)
            EXPECT(mtr_anim_ik_create(dev, J, cyc.data(), K, chains.data(), &none), MTR_E_INVALID);
            cyc = parents;
            cyc[1] = (uint8_t)(J < 255 ? J : 254);  // out of range (J = 256: 254 is a valid parent, a cycle or not -- skip the count)
            if (J < 255) EXPECT(mtr_anim_ik_create(dev, J, cyc.data(), K, chains.data(), &none), MTR_E_INVALID);
        }
        rejected += 9;
        const uint32_t kk = pick(0, K - 1);
        char want[32];
        snprintf(want, sizeof want, "chain %u ", kk);
        auto bad_chain = [&](auto&& change) {
            std::vector<mtr_ik_chain> c2 = chains;
            change(c2[kk]);
            return mtr_anim_ik_create(dev, J, parents.data(), K, c2.data(), &none);
        };
        EXPECT(bad_chain([](mtr_ik_chain& c) { c.kind = 2; }), MTR_E_INVALID); NAMES(want);
        EXPECT(bad_chain([](mtr_ik_chain& c) { c.flags |= 4u; }), MTR_E_INVALID); NAMES(want);
        EXPECT(bad_chain([&](mtr_ik_chain& c) { c.joint[0] = J; }), MTR_E_INVALID); NAMES(want);
        EXPECT(bad_chain([&](mtr_ik_chain& c) { c.kind = MTR_IK_TWO_BONE; c.joint[0] = J - 3; c.joint[1] = J - 2; c.joint[2] = J; }), MTR_E_INVALID); NAMES(want);
        EXPECT(bad_chain([&](mtr_ik_chain& c) { c.kind = MTR_IK_TWO_BONE; c.joint[0] = J - 3; c.joint[1] = J; c.joint[2] = J - 1; }), MTR_E_INVALID); NAMES(want);
        EXPECT(bad_chain([&](mtr_ik_chain& c) { c.kind = MTR_IK_TWO_BONE; c.joint[0] = J - 3; c.joint[1] = J - 2; c.joint[2] = J - 2; }), MTR_E_INVALID); NAMES(want);
        EXPECT(bad_chain([&](mtr_ik_chain& c) { c.kind = MTR_IK_TWO_BONE; c.joint[0] = J - 2; c.joint[1] = J - 2; c.joint[2] = J - 1; }), MTR_E_INVALID); NAMES(want);
        EXPECT(bad_chain([&](mtr_ik_chain& c) { c.kind = MTR_IK_TWO_BONE; c.joint[0] = J - 1; c.joint[1] = J - 2; c.joint[2] = J - 3; }), MTR_E_INVALID); NAMES(want);
        EXPECT(bad_chain([&](mtr_ik_chain& c) { c.kind = MTR_IK_TWO_BONE; c.joint[0] = J - 4; c.joint[1] = J - 2; c.joint[2] = J - 1; }), MTR_E_INVALID); NAMES(want);
        EXPECT(bad_chain([&](mtr_ik_chain& c) { c.kind = MTR_IK_TWO_BONE; c.joint[0] = 1; c.joint[1] = 0; c.joint[2] = J - 1; }), MTR_E_INVALID); NAMES(want);  // b a root
        EXPECT(bad_chain([](mtr_ik_chain& c) { c.kind = MTR_IK_AIM; c.axis[0] = c.axis[1] = c.axis[2] = 0.0f; }), MTR_E_INVALID); NAMES(want);
        EXPECT(bad_chain([](mtr_ik_chain& c) { c.kind = MTR_IK_AIM; c.axis[0] = -0.0f; c.axis[1] = 0.0f; c.axis[2] = 0.0f; }), MTR_E_INVALID); NAMES(want);
        EXPECT(bad_chain([](mtr_ik_chain& c) { c.kind = MTR_IK_AIM; c.axis[2] = NAN; }), MTR_E_INVALID); NAMES(want);
        EXPECT(bad_chain([](mtr_ik_chain& c) { c.kind = MTR_IK_AIM; c.axis[0] = INFINITY; }), MTR_E_INVALID); NAMES(want);
        if (none) { fprintf(stderr, "a failed create must clear *out\n"); return 1; }
        rejected += 14;
        // ---- the sets: the skeleton's, one of another joint count, one of other parents, one of another device ----
        mtr_anim_ik *ik = nullptr, *ik_other = nullptr, *ik_tree = nullptr, *ik_foreign = nullptr;
        EXPECT(mtr_anim_ik_create(dev, J, parents.data(), K, chains.data(), &ik), MTR_OK);
        EXPECT(mtr_anim_ik_create(dev2, J, parents.data(), K, chains.data(), &ik_foreign), MTR_OK);
        std::vector<uint8_t> tree = parents;
        const uint32_t moved = 1 + (J > 5 ? pick(0, J - 5) : 0);  // a joint below the chain, hung onto another valid parent (or made a root)
        tree[moved] = tree[moved] == 0 ? 255 : 0;
        EXPECT(mtr_anim_ik_create(dev, J, tree.data(), K, chains.data(), &ik_tree), MTR_OK);
        {
            const uint32_t J2 = J == 256 ? 255 : J + 1;
            std::vector<uint8_t> par2(J2);
            for (uint32_t j = 0; j < J2; j++) par2[j] = j ? (uint8_t)(j - 1) : 255;
            mtr_ik_chain c = mtr_ik_chain{};
            c.kind = MTR_IK_AIM; c.axis[0] = 1.0f;
            std::vector<mtr_ik_chain> cs(K, c);
            EXPECT(mtr_anim_ik_create(dev, J2, par2.data(), K, cs.data(), &ik_other), MTR_OK);
        }
        const uint32_t M = pick(1, 3);
        std::vector<float> weights((size_t)M * J, 0.5f);
        mtr_anim_masks* masks = nullptr;
        EXPECT(mtr_anim_masks_create(dev, J, M, weights.data(), &masks), MTR_OK);
        const uint32_t nclips = pick(1, 4);
        std::vector<uint32_t> nk(nclips);
        size_t total = 0;
        for (auto& k : nk) { k = pick(1, 20); total += k; }
        std::vector<mtr_anim_key> keys(total * J);
        for (auto& k : keys) { k = mtr_anim_key{}; k.q[3] = 1.0f; }
        mtr_anim *uniform = nullptr, *tracks = nullptr, *other = nullptr;
        EXPECT(mtr_anim_create(dev, J, nclips, nk.data(), nullptr, keys.data(), &uniform), MTR_OK);
        EXPECT(make_tracks(dev, J, nclips, &tracks), MTR_OK);
        EXPECT(make_tracks(dev, J == 256 ? 255 : J + 1, 1, &other), MTR_OK);
        std::vector<mtr_anim_layer> ly((size_t)n * L);     // exactly sized: one record too many read is a report
        std::vector<mtr_ik_target> tg((size_t)n * K);
        for (auto& r : ly) { r.clip = (uint32_t)rnd(); r.x = (float)(rnd() % 1000) * 0.37f; r.w = 0.5f; r.mask = (uint16_t)rnd(); r.mode = (uint16_t)rnd(); }
        for (auto& t : tg) { t = mtr_ik_target{}; t.pos[0] = rnd() % 7 ? (float)(rnd() % 100) : NAN; t.w = rnd() % 4 ? 1.0f : NAN; t.pole[2] = INFINITY; t.pad = (uint32_t)rnd(); }
        std::vector<mtr_anim_state> st(n, mtr_anim_state{});
        std::vector<float> locals((size_t)n * J * 16, 0.0f);
        // ---- the valid calls: both kinds of set, with and without masks, host and "device" records (stub: host memory) ----
        EXPECT(mtr_batch_animate_ik(batch, uniform, masks, ly.data(), L, ik, tg.data()), MTR_OK);
        EXPECT(mtr_batch_animate_ik(batch, tracks, nullptr, ly.data(), L, ik, tg.data()), MTR_OK);
        EXPECT(mtr_batch_animate_ik_device(batch, tracks, masks, ly.data(), L, ik, tg.data(), nullptr), MTR_OK);
        EXPECT(mtr_batch_animate_ik_device(batch, uniform, nullptr, ly.data(), L, ik, tg.data(), nullptr), MTR_OK);
        EXPECT(mtr_model_animate_ik(model, uniform, masks, ly.data(), L, ik, tg.data()), MTR_OK);
        EXPECT(mtr_model_animate_ik(model, tracks, nullptr, ly.data() + (size_t)(n - 1) * L, L, ik, tg.data() + (size_t)(n - 1) * K), MTR_OK);
        EXPECT(mtr_anim_sample_ik(uniform, masks, ik, ly.data(), L, tg.data(), n, locals.data(), locals.size()), MTR_OK);
        EXPECT(mtr_anim_sample_ik(tracks, nullptr, ik_tree, ly.data(), L, tg.data(), n, locals.data(), locals.size()), MTR_OK);  // its own skeleton
        EXPECT(mtr_anim_sample_ik(tracks, masks, ik, ly.data(), L, tg.data(), 0, nullptr, 0), MTR_OK);
        animated += 8;
        // ---- every invalid call ----
        EXPECT(mtr_batch_animate_ik(nullptr, uniform, masks, ly.data(), L, ik, tg.data()), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik(batch, nullptr, masks, ly.data(), L, ik, tg.data()), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik(batch, uniform, masks, nullptr, L, ik, tg.data()), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik(batch, uniform, masks, ly.data(), 0, ik, tg.data()), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik(batch, uniform, masks, ly.data(), 9, ik, tg.data()), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik(batch, other, masks, ly.data(), L, ik, tg.data()), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik(batch, uniform, masks, ly.data(), L, nullptr, tg.data()), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik(batch, uniform, masks, ly.data(), L, ik, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik(batch, uniform, masks, ly.data(), L, ik_other, tg.data()), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik(batch, uniform, masks, ly.data(), L, ik_foreign, tg.data()), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik(batch, uniform, masks, ly.data(), L, ik_tree, tg.data()), MTR_E_INVALID);
        snprintf(want, sizeof want, "joint %u ", moved);
        NAMES(want);
        EXPECT(mtr_batch_animate_ik_device(nullptr, uniform, masks, ly.data(), L, ik, tg.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik_device(batch, uniform, masks, nullptr, L, ik, tg.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik_device(batch, uniform, masks, ly.data(), L, ik, nullptr, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik_device(batch, uniform, masks, ly.data(), L, ik, (const mtr_ik_target*)((const char*)tg.data() + 8), nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik_device(batch, uniform, masks, (const mtr_anim_layer*)((const char*)ly.data() + 8), L, ik, tg.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik_device(batch, uniform, masks, ly.data(), L, nullptr, tg.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik_device(batch, tracks, masks, ly.data(), L, ik_tree, tg.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_animate_ik_device(batch, tracks, nullptr, ly.data(), L, ik_foreign, tg.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_model_animate_ik(nullptr, uniform, masks, ly.data(), L, ik, tg.data()), MTR_E_INVALID);
        EXPECT(mtr_model_animate_ik(model, uniform, masks, nullptr, L, ik, tg.data()), MTR_E_INVALID);
        EXPECT(mtr_model_animate_ik(model, uniform, masks, ly.data(), L, nullptr, tg.data()), MTR_E_INVALID);
        EXPECT(mtr_model_animate_ik(model, uniform, masks, ly.data(), L, ik, nullptr), MTR_E_INVALID);
        EXPECT(mtr_model_animate_ik(model, uniform, masks, ly.data(), L, ik_other, tg.data()), MTR_E_INVALID);
        EXPECT(mtr_model_animate_ik(model, uniform, masks, ly.data(), L, ik_tree, tg.data()), MTR_E_INVALID);
        EXPECT(mtr_model_animate_ik(bare, uniform, nullptr, ly.data(), L, ik, tg.data()), MTR_E_INVALID);
        EXPECT(mtr_anim_sample_ik(nullptr, masks, ik, ly.data(), L, tg.data(), n, locals.data(), locals.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_sample_ik(uniform, masks, nullptr, ly.data(), L, tg.data(), n, locals.data(), locals.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_sample_ik(uniform, masks, ik_other, ly.data(), L, tg.data(), n, locals.data(), locals.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_sample_ik(uniform, masks, ik_foreign, ly.data(), L, tg.data(), n, locals.data(), locals.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_sample_ik(uniform, masks, ik, ly.data(), 9, tg.data(), n, locals.data(), locals.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_sample_ik(uniform, masks, ik, ly.data(), L, nullptr, n, locals.data(), locals.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_sample_ik(uniform, masks, ik, ly.data(), L, tg.data(), n, locals.data(), locals.size() - 1), MTR_E_INVALID);
        rejected += 34;
        // ---- one batch animated by every kind of call with frames in flight, IK sets created and destroyed between them ----
        mtr_frame* frames[4] = {};
        int k = 0;
        for (auto& f : frames) {
            if (k == 1) EXPECT(mtr_batch_animate(batch, uniform, st.data()), MTR_OK);
            else if (k == 2) EXPECT(mtr_batch_animate_layers(batch, uniform, masks, ly.data(), L), MTR_OK);
            else if (k == 3) EXPECT(mtr_batch_set_poses(batch, locals.data(), J), MTR_OK);
            else EXPECT(mtr_batch_animate_ik(batch, tracks, masks, ly.data(), L, ik, tg.data()), MTR_OK);
            EXPECT(mtr_model_animate_ik(model, k % 2 ? tracks : uniform, k == 3 ? nullptr : masks, ly.data(), L, ik, tg.data()), MTR_OK);
            animated += 2;
            mtr_anim_ik* tmp = nullptr;
            if (k >= 1) {  // an IK set created, used (host or "device" targets) and destroyed straight after the submit
                EXPECT(mtr_anim_ik_create(dev, J, parents.data(), K, chains.data(), &tmp), MTR_OK);
                if (k == 2) EXPECT(mtr_batch_animate_ik_device(batch, uniform, masks, ly.data(), L, tmp, tg.data(), nullptr), MTR_OK);
                else EXPECT(mtr_batch_animate_ik(batch, uniform, nullptr, ly.data(), L, tmp, tg.data()), MTR_OK);
                animated++;
            }
            EXPECT(mtr_frame_begin(dev, 64, 48, clear, 1.0f, &f), MTR_OK);
            EXPECT(mtr_frame_draw_batch(f, batch, vp), MTR_OK);
            EXPECT(mtr_frame_draw_model(f, model, vp), MTR_OK);
            EXPECT(mtr_frame_submit(f), MTR_OK);
            mtr_anim_ik_destroy(tmp);
            k++;
        }
        mtr_anim_ik_destroy(ik);  // straight after a submit
        mtr_anim_ik_destroy(ik_other);
        mtr_anim_ik_destroy(ik_tree);
        mtr_anim_ik_destroy(ik_foreign);
        mtr_anim_ik_destroy(nullptr);
        mtr_anim_masks_destroy(masks);
        mtr_anim_destroy(uniform);
        mtr_anim_destroy(tracks);
        mtr_anim_destroy(other);
        for (auto& f : frames) { EXPECT(mtr_frame_wait(f), MTR_OK); mtr_frame_destroy(f); }
        mtr_batch_destroy(batch);
        mtr_model_destroy(model);
        mtr_model_destroy(bare);
    }
    mtr_device_destroy(dev2);
    mtr_device_destroy(dev);
    printf("animated=%ld rejected=%ld target_reads=%llu chain_reads=%llu path_reads=%llu\n", animated, rejected, (unsigned long long)g_target_reads,
           (unsigned long long)g_chain_reads, (unsigned long long)g_path_reads);
    return 0;
}
