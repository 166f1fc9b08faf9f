// AddressSanitizer / UBSan run of the HOST side of spring bones (csrc/host_spring.cpp, csrc/host_anim.cpp, csrc/host_batch.cpp:
// mtr_anim_spring_create / _destroy, mtr_batch_animate_spring_device, mtr_anim_sample_spring) over the stand-in HIP runtime
// (tests/cpp/hip_stub: device memory = host heap, everything runs at once).  The k_anim_spring launcher here checks the
// set's image (the joint table against the springs, the path of every spring joint), touch the first and last layer, target
// and motion matrix of every instance, and run the rule of csrc/spring_math.h on the state words they are handed, each
// spring at a position made of its index and the instance's: a wrong size or offset on the host side is an ASan report, and
// the states after a call are compared with a second run of the rule.
//   usage: spring_host_asan <iterations>
#define MTR_RND_SEED 0x13198A2E03707344ull
#include "harness.h"
#include "../../mt_renderer_amd/csrc/mtr_files.cpp"

struct float4 {
    float x, y, z, w;
};
static inline float4 make_float4(float x, float y, float z, float w) {
    float4 r = {x, y, z, w};
    return r;
}
#include "../../mt_renderer_amd/csrc/spring_math.h"

// a spring call makes the checks of the kinds it nests over, so their kernels count as built; the layered call is made
// here too, between the spring ones
void mtr_launch_anim(const AnimParams&, bool, bool, uint32_t, hipStream_t) { abort(); }
void mtr_launch_anim_layers(const AnimLayerParams& p, bool, bool fold, uint32_t ninst, hipStream_t) {
    if (!fold) abort();
    p.anim.pose.out[(size_t)ninst * p.anim.pose.njoints * 16 - 1] = (float)p.layers[(size_t)ninst * p.nlayers * 4 - 1];
}
void mtr_launch_anim_ik(const AnimIkParams&, bool, bool, uint32_t, hipStream_t) { abort(); }

static float f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t u32(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// the rule on one state record of instance i and spring k, as the launcher and the harness's second run both apply it
static void rule(const uint32_t* sp, uint32_t* st, uint32_t i, uint32_t k, float dt, const float* motion) {
    using namespace mtr;
    SpringMotion D = {};
    if (motion) {
        const float* m = motion + (size_t)i * 16;
        D.c0 = ik_vec3(m[0], m[1], m[2]); D.c1 = ik_vec3(m[4], m[5], m[6]); D.c2 = ik_vec3(m[8], m[9], m[10]); D.t = ik_vec3(m[12], m[13], m[14]);
    }
    SpringState s;
    s.cur = ik_vec3(f32(st[0]), f32(st[1]), f32(st[2]));
    s.live = st[3];
    s.prev = ik_vec3(f32(st[4]), f32(st[5]), f32(st[6]));
    AnimVec qa = anim_vec(0.0f, 0.0f, 0.0f, 1.0f);
    spring_step(ik_vec3((float)k, (float)i, 0.5f), anim_vec(0.0f, 0.0f, 0.0f, 1.0f), qa, ik_vec3(f32(sp[4]), f32(sp[5]), f32(sp[6])),
                ik_vec3(f32(sp[8]), f32(sp[9]), f32(sp[10])), f32(sp[2]), f32(sp[3]), dt, motion != nullptr, D, s);
    st[0] = u32(s.cur.x); st[1] = u32(s.cur.y); st[2] = u32(s.cur.z); st[3] = s.live;
    st[4] = u32(s.prev.x); st[5] = u32(s.prev.y); st[6] = u32(s.prev.z); st[7] = 0u;
}

static uint64_t g_launches = 0, g_state_steps = 0, g_path_reads = 0;
static void run_springs(const AnimSpringParams& p, uint32_t ninst, bool tracks, bool fold) {
    const AnimIkParams& ip = p.ik;
    const AnimLayerParams& lp = ip.layers;
    const AnimParams& a = lp.anim;
    const uint32_t J = a.pose.njoints;
    g_launches++;
    if (a.states || !lp.layers || ((uintptr_t)lp.layers & 15u) || lp.nlayers < 1 || lp.nlayers > MTR_ANIM_MAX_LAYERS) abort();
    if (ip.nchains > MTR_ANIM_MAX_IK || (ip.nchains ? (!ip.chains || !ip.targets || ((uintptr_t)ip.targets & 15u)) : (ip.chains || ip.targets))) abort();
    if (!ip.paths || !ip.path_words || ip.path_bytes == 0 || ip.path_bytes > MTR_POSE_MAX_PATH_BYTES) abort();
    if (!p.springs || !p.joint_tab || !p.states || ((uintptr_t)p.states & 15u) || ((uintptr_t)p.motion & 15u)) abort();
    if (p.nsprings < 1 || p.nsprings > MTR_ANIM_MAX_SPRINGS || p.nrounds < 1 || p.nrounds > p.nsprings) abort();
    if (tracks ? (a.keys || !a.tracks) : (!a.keys || a.tracks)) abort();
    if (fold) {  // the model's own path table, and its inverse bind matrices
        if (ip.paths != a.pose.paths || ip.path_words != a.pose.path_words || ip.path_bytes != a.pose.path_bytes) abort();
        if (a.pose.imats[(size_t)J * 16 - 1] != 1.0f) abort();
    }
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(ip.path_words);
    uint32_t acc = bytes[ip.path_bytes - 1], seen = 0, top = 0;
    for (uint32_t j = 0; j < J; j++) {  // the joint table against the springs and the paths
        const uint32_t tab = p.joint_tab[j];
        if (tab == MTR_SPRING_NONE) continue;
        const uint32_t k = tab & 0xFFu, rd = tab >> 8;
        if (k >= p.nsprings || rd >= p.nrounds || p.springs[(size_t)k * 12] != j || p.springs[(size_t)k * 12 + 1] != 0u) abort();
        const uint32_t w = ip.paths[j], ofs = w & 0xFFFFu, len = w >> 16;
        if (len == 0 || ofs + len > ip.path_bytes || bytes[ofs + len - 1] != j) abort();
        uint32_t above = 0;  // the round is the number of spring joints on the path above j
        for (uint32_t s = 0; s + 1 < len; s++) above += p.joint_tab[bytes[ofs + s]] != MTR_SPRING_NONE;
        if (above != rd) abort();
        top = std::max(top, rd + 1);
        seen++;
        g_path_reads += len;
    }
    if (seen != p.nsprings || top != p.nrounds) abort();
    for (uint32_t i = 0; i < ninst; i++) {
        acc += lp.layers[(size_t)i * lp.nlayers * 4] + lp.layers[(size_t)(i + 1) * lp.nlayers * 4 - 1];
        if (ip.nchains) acc += ip.targets[(size_t)i * ip.nchains * 8] + ip.targets[(size_t)(i + 1) * ip.nchains * 8 - 1];
        for (uint32_t k = 0; k < p.nsprings; k++) {
            rule(p.springs + (size_t)k * 12, p.states + ((size_t)i * p.nsprings + k) * 8, i, k, p.dt, p.motion);
            g_state_steps++;
        }
    }
    a.pose.out[(size_t)ninst * J * 16 - 1] = (float)acc;
}
void mtr_launch_anim_spring(const AnimSpringParams& p, bool tracks, bool fold, uint32_t ninst, hipStream_t) { run_springs(p, ninst, tracks, fold); }

static float unit() { return (float)(rnd() % 2001) / 1000.0f - 1.0f; }

// a rejected call: the code, no launch, the states as they were
#define REJECT(call) do { const uint64_t l_ = g_launches; EXPECT(call, MTR_E_INVALID); if (g_launches != l_ || memcmp(st.data(), st_before.data(), st.size() * sizeof st[0])) { fprintf(stderr, "line %d: a rejected call launched or changed the states\n", __LINE__); return 1; } rejected++; } while (0)

static int32_t make_tracks(mtr_device* dev, uint32_t J, uint32_t nclips, mtr_anim** out) {
    std::vector<uint32_t> nticks(nclips, 16u);
    std::vector<mtr_anim_track> tr((size_t)nclips * J * 3);
    std::vector<uint16_t> times(tr.size(), 0), values(tr.size() * 4, 7);
    for (size_t t = 0; t < tr.size(); t++) { tr[t] = mtr_anim_track{}; tr[t].first = (uint32_t)t; tr[t].count = 1; }
    return mtr_anim_create_tracks(dev, J, nclips, nticks.data(), nullptr, tr.data(), times.data(), values.data(), times.size(), out);
}

// 16-byte aligned storage for the records the device call takes (std::vector's is, for these sizes, but say so)
template <class T>
struct Aligned {
    std::vector<unsigned char> raw;
    size_t n;
    explicit Aligned(size_t count) : raw(count * sizeof(T) + 16), n(count) {}
    T* data() { return reinterpret_cast<T*>(raw.data() + (16 - ((uintptr_t)raw.data() & 15u)) % 16); }
    size_t size() const { return n; }
    T& operator[](size_t i) { return data()[i]; }
};

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
    hipStream_t s1 = nullptr, s2 = nullptr;
    if (hipStreamCreateWithFlags(&s1, 0) || hipStreamCreateWithFlags(&s2, 0)) return 3;
    long animated = 0, rejected = 0;
    for (long it = 0; it < iters; it++) {
        mtr_model *model = nullptr, *bare = nullptr;
        EXPECT(mtr_model_create(dev, verts, sizeof verts, idx, 36, &p, 1, &l, &p2t, nullptr, 0, &dbg, &model), MTR_OK);
        EXPECT(mtr_model_create(dev, verts, sizeof verts, idx, 36, &p, 1, &l, &p2t, nullptr, 0, &dbg, &bare), MTR_OK);  // no skeleton
        const uint32_t J = it % 9 == 0 ? 256 : pick(4, 70), n = pick(1, 40), L = pick(1, 8), K = it % 5 == 0 ? 16 : pick(1, std::min(16u, J));
        std::vector<uint8_t> parents(J);
        for (uint32_t j = 0; j < J; j++) parents[j] = j ? (uint8_t)(rnd() % j) : (it % 2 ? 255 : 0);
        std::vector<float> imats((size_t)J * 16, 1.0f), mats((size_t)n * 16, 0.0f);
        EXPECT(mtr_model_set_skeleton(model, parents.data(), imats.data(), J), MTR_OK);
        mtr_batch* batch = nullptr;
        EXPECT(mtr_batch_create(dev, model, n, mats.data(), nullptr, 0, nullptr, &batch), MTR_OK);
        std::vector<mtr_spring> springs(K);  // exactly sized; K distinct joints in random order
        {
            std::vector<uint32_t> js(J);
            for (uint32_t j = 0; j < J; j++) js[j] = j;
            for (uint32_t k = 0; k < K; k++) std::swap(js[k], js[k + rnd() % (J - k)]);
            for (uint32_t k = 0; k < K; k++) {
                mtr_spring& s = springs[k];
                s = mtr_spring{};
                s.joint = js[k]; s.stiffness = (float)(rnd() % 100); s.drag = (float)(rnd() % 11) / 10.0f;
                s.tail[0] = unit(); s.tail[1] = 1.0f + unit(); s.tail[2] = unit(); s.tail[k % 3] += 0.25f;
                s.gravity[1] = -9.8f * unit();
                s.pad0 = NAN; s.pad1 = INFINITY;  // not read
            }
        }
        // ---- spring sets: every invalid creation, one violation at a time ----
        mtr_anim_spring* none = (mtr_anim_spring*)1;
        std::vector<mtr_spring_state> st(1), st_before(1);  // nothing to compare at creation
        EXPECT(mtr_anim_spring_create(nullptr, J, parents.data(), K, springs.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_spring_create(dev, J, parents.data(), K, springs.data(), nullptr), MTR_E_INVALID);
        REJECT(mtr_anim_spring_create(dev, 0, parents.data(), K, springs.data(), &none));
        REJECT(mtr_anim_spring_create(dev, 257, parents.data(), K, springs.data(), &none));
        REJECT(mtr_anim_spring_create(dev, J, nullptr, K, springs.data(), &none));
        REJECT(mtr_anim_spring_create(dev, J, parents.data(), 0, springs.data(), &none));
        REJECT(mtr_anim_spring_create(dev, J, parents.data(), 17, springs.data(), &none));
        REJECT(mtr_anim_spring_create(dev, J, parents.data(), K, nullptr, &none));
        {
            std::vector<uint8_t> cyc = parents;
            cyc[1] = 2; cyc[2] = 3; cyc[3] = 1;  // 1 -> 2 -> 3 -> 1
            REJECT(mtr_anim_spring_create(dev, J, cyc.data(), K, springs.data(), &none));
            cyc = parents;
            cyc[1] = (uint8_t)(J < 255 ? J : 254);  // out of range (J = 256: 254 is a valid parent)
            if (J < 255) REJECT(mtr_anim_spring_create(dev, J, cyc.data(), K, springs.data(), &none));
            else rejected++;
        }
        const uint32_t kk = pick(0, K - 1);
        char want[32];
        snprintf(want, sizeof want, "spring %u ", kk);
        auto bad_spring = [&](auto&& change) {
            std::vector<mtr_spring> s2v = springs;
            change(s2v[kk]);
            return mtr_anim_spring_create(dev, J, parents.data(), K, s2v.data(), &none);
        };
        REJECT(bad_spring([&](mtr_spring& s) { s.joint = J; })); NAMES(want);
        REJECT(bad_spring([](mtr_spring& s) { s.flags = 1u; })); NAMES(want);
        REJECT(bad_spring([](mtr_spring& s) { s.flags = 0x80000000u; })); NAMES(want);
        REJECT(bad_spring([](mtr_spring& s) { s.tail[0] = s.tail[1] = s.tail[2] = 0.0f; })); NAMES(want);
        REJECT(bad_spring([](mtr_spring& s) { s.tail[0] = -0.0f; s.tail[1] = s.tail[2] = 0.0f; })); NAMES(want);
        REJECT(bad_spring([](mtr_spring& s) { s.tail[1] = NAN; })); NAMES(want);
        REJECT(bad_spring([](mtr_spring& s) { s.tail[2] = -INFINITY; })); NAMES(want);
        REJECT(bad_spring([](mtr_spring& s) { s.stiffness = -1.0f; })); NAMES(want);
        REJECT(bad_spring([](mtr_spring& s) { s.stiffness = NAN; })); NAMES(want);
        REJECT(bad_spring([](mtr_spring& s) { s.stiffness = INFINITY; })); NAMES(want);
        REJECT(bad_spring([](mtr_spring& s) { s.drag = -0.01f; })); NAMES(want);
        REJECT(bad_spring([](mtr_spring& s) { s.drag = 1.01f; })); NAMES(want);
        REJECT(bad_spring([](mtr_spring& s) { s.drag = NAN; })); NAMES(want);
        REJECT(bad_spring([](mtr_spring& s) { s.gravity[0] = NAN; })); NAMES(want);
        REJECT(bad_spring([](mtr_spring& s) { s.gravity[2] = INFINITY; })); NAMES(want);
        if (K > 1) {  // a joint named twice: the later spring is the one named
            std::vector<mtr_spring> s2v = springs;
            const uint32_t first = kk ? pick(0, kk - 1) : 0, second = kk ? kk : 1;
            s2v[second].joint = s2v[first].joint;
            snprintf(want, sizeof want, "spring %u ", second);
            REJECT(mtr_anim_spring_create(dev, J, parents.data(), K, s2v.data(), &none)); NAMES(want);
        } else rejected++;
        if (none) { fprintf(stderr, "a failed create must clear *out\n"); return 1; }
        // ---- the sets: the skeleton's, one of another joint count, one of other parents, one of another device ----
        mtr_anim_spring *sp = nullptr, *sp_other = nullptr, *sp_tree = nullptr, *sp_foreign = nullptr;
        EXPECT(mtr_anim_spring_create(dev, J, parents.data(), K, springs.data(), &sp), MTR_OK);
        EXPECT(mtr_anim_spring_create(dev2, J, parents.data(), K, springs.data(), &sp_foreign), MTR_OK);
        std::vector<uint8_t> tree = parents;
        const uint32_t moved = pick(1, J - 1);  // hung onto another valid parent, or made a root
        tree[moved] = tree[moved] == 0 ? 255 : 0;
        EXPECT(mtr_anim_spring_create(dev, J, tree.data(), K, springs.data(), &sp_tree), MTR_OK);
        const uint32_t J2 = J == 256 ? 255 : J + 1;
        std::vector<uint8_t> par2(J2);
        for (uint32_t j = 0; j < J2; j++) par2[j] = j ? (uint8_t)(j - 1) : 255;
        {
            std::vector<mtr_spring> s2v(springs.begin(), springs.begin() + std::min(K, J2));
            for (auto& s : s2v) s.joint %= J2;
            EXPECT(mtr_anim_spring_create(dev, J2, par2.data(), 1, s2v.data(), &sp_other), MTR_OK);
        }
        // IK sets: the skeleton's (AIM chains only: any joint will do), one of other parents
        const uint32_t KC = pick(1, 4);
        std::vector<mtr_ik_chain> chains(KC);
        for (auto& c : chains) { c = mtr_ik_chain{}; c.kind = MTR_IK_AIM; c.joint[0] = pick(0, J - 1); c.axis[1] = 1.0f; }
        mtr_anim_ik *ik = nullptr, *ik_tree = nullptr;
        EXPECT(mtr_anim_ik_create(dev, J, parents.data(), KC, chains.data(), &ik), MTR_OK);
        EXPECT(mtr_anim_ik_create(dev, J, tree.data(), KC, chains.data(), &ik_tree), MTR_OK);
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
        EXPECT(make_tracks(dev, J2, 1, &other), MTR_OK);
        // the records the "device" call takes, exactly sized and 16-byte aligned
        Aligned<mtr_anim_layer> ly((size_t)n * L);
        Aligned<mtr_ik_target> tg((size_t)n * KC);
        Aligned<mtr_spring_state> dst((size_t)n * K);
        Aligned<float> mo((size_t)n * 16);
        for (size_t i = 0; i < ly.size(); i++) { mtr_anim_layer& r = ly[i]; r.clip = (uint32_t)rnd(); r.x = (float)(rnd() % 1000) * 0.37f; r.w = 0.5f; r.mask = (uint16_t)rnd(); r.mode = (uint16_t)rnd(); }
        for (size_t i = 0; i < tg.size(); i++) { mtr_ik_target& t = tg[i]; t = mtr_ik_target{}; t.pos[0] = (float)(rnd() % 100); t.w = 1.0f; t.pad = (uint32_t)rnd(); }
        for (size_t i = 0; i < mo.size(); i++) mo[i] = i % 16 % 5 == 0 ? 1.0f : (i % 16 >= 12 ? unit() : 0.0f);  // the identity and a translation
        st.assign((size_t)n * K, mtr_spring_state{});
        for (size_t i = 0; i < st.size(); i++) {
            mtr_spring_state& s = st[i];
            switch (rnd() % 5) {
            case 0: break;  // not started
            case 1: s.live = 1; s.cur[0] = NAN; break;
            case 2: s.live = (uint32_t)rnd() | 1u; s.prev[2] = INFINITY; break;
            default: s.live = 1; for (int c = 0; c < 3; c++) { s.cur[c] = 3.0f * unit(); s.prev[c] = s.cur[c] + 0.1f * unit(); } s.pad = (uint32_t)rnd();
            }
        }
        const float dts[6] = {1.0f / 60.0f, 1.0f / 30.0f, 0.0f, -1.0f, NAN, INFINITY};
        const float dt = dts[it % 6];
        const uint32_t* img = reinterpret_cast<const uint32_t*>(springs.data());
        auto expect_states = [&](std::vector<mtr_spring_state> from, const float* motion) {  // a second run of the rule
            for (uint32_t i = 0; i < n; i++)
                for (uint32_t k = 0; k < K; k++) rule(img + (size_t)k * 12, reinterpret_cast<uint32_t*>(&from[(size_t)i * K + k]), i, k, dt, motion);
            return from;
        };
        auto same = [](const void* a, const std::vector<mtr_spring_state>& b) { return !memcmp(a, b.data(), b.size() * sizeof b[0]); };
        // ---- the valid device calls, on two streams: with and without IK, motion and masks; each equals a second run of the rule ----
        std::vector<mtr_spring_state> want_st = st;
        memcpy(dst.data(), st.data(), st.size() * sizeof st[0]);
        struct Call { mtr_anim* a; mtr_anim_masks* mk; mtr_anim_ik* ik; bool motion; hipStream_t s; };
        const Call calls[5] = {{uniform, masks, ik, true, s1}, {tracks, nullptr, nullptr, false, s2}, {uniform, nullptr, ik, false, s2},
                               {tracks, masks, nullptr, true, s1}, {uniform, masks, ik, true, nullptr}};
        for (const Call& c : calls) {
            want_st = expect_states(want_st, c.motion ? mo.data() : nullptr);
            EXPECT(mtr_batch_animate_spring_device(batch, c.a, c.mk, ly.data(), L, c.ik, c.ik ? tg.data() : nullptr, sp, dst.data(), c.motion ? mo.data() : nullptr, dt, c.s), MTR_OK);
            if (!same(dst.data(), want_st)) { fprintf(stderr, "iteration %ld: the states after a device call are not the rule's\n", it); return 1; }
            animated++;
        }
        // ---- the host hook on unaligned memory: every array one byte off ----
        {
            std::vector<unsigned char> b_ly(ly.size() * sizeof(mtr_anim_layer) + 1), b_tg(tg.size() * sizeof(mtr_ik_target) + 1), b_st(st.size() * sizeof st[0] + 1),
                b_mo(mo.size() * 4 + 1), b_out((size_t)n * J * 64 + 1);
            memcpy(b_ly.data() + 1, ly.data(), b_ly.size() - 1);
            memcpy(b_tg.data() + 1, tg.data(), b_tg.size() - 1);
            memcpy(b_st.data() + 1, st.data(), b_st.size() - 1);
            memcpy(b_mo.data() + 1, mo.data(), b_mo.size() - 1);
            auto* u_ly = reinterpret_cast<const mtr_anim_layer*>(b_ly.data() + 1);
            auto* u_tg = reinterpret_cast<const mtr_ik_target*>(b_tg.data() + 1);
            auto* u_st = reinterpret_cast<mtr_spring_state*>(b_st.data() + 1);
            auto* u_mo = reinterpret_cast<const float*>(b_mo.data() + 1);
            auto* u_out = reinterpret_cast<float*>(b_out.data() + 1);
            EXPECT(mtr_anim_sample_spring(uniform, masks, ik, sp, u_ly, L, u_tg, u_st, u_mo, dt, n, u_out, (size_t)n * J * 16), MTR_OK);
            if (!same(u_st, expect_states(st, mo.data()))) { fprintf(stderr, "iteration %ld: the states after the host hook are not the rule's\n", it); return 1; }
            memcpy(b_st.data() + 1, st.data(), b_st.size() - 1);
            EXPECT(mtr_anim_sample_spring(tracks, nullptr, nullptr, sp_tree, u_ly, L, nullptr, u_st, nullptr, dt, n, u_out, (size_t)n * J * 16), MTR_OK);  // its own skeleton
            if (!same(u_st, expect_states(st, nullptr))) { fprintf(stderr, "iteration %ld: the host hook without motion\n", it); return 1; }
            EXPECT(mtr_anim_sample_spring(tracks, masks, ik, sp, u_ly, L, u_tg, nullptr, nullptr, dt, 0, nullptr, 0), MTR_OK);
            animated += 2;
        }
        // ---- every invalid call: no launch, the states untouched ----
        memcpy(st.data(), dst.data(), st.size() * sizeof st[0]);
        st_before = st;
        mtr_spring_state* S = st.data();
        std::vector<float> locals((size_t)n * J * 16, 0.0f);
#define DEV(b, a, mk, lyp, nl, ikp, tgp, spp, stp, mop) mtr_batch_animate_spring_device(b, a, mk, lyp, nl, ikp, tgp, spp, stp, mop, dt, nullptr)
        if ((uintptr_t)S & 15u) { fprintf(stderr, "the states of the invalid calls must be aligned\n"); return 1; }
        EXPECT(DEV(nullptr, uniform, masks, ly.data(), L, ik, tg.data(), sp, S, mo.data()), MTR_E_INVALID);
        REJECT(DEV(batch, nullptr, masks, ly.data(), L, ik, tg.data(), sp, S, mo.data()));
        REJECT(DEV(batch, other, masks, ly.data(), L, ik, tg.data(), sp, S, mo.data()));
        REJECT(DEV(batch, uniform, masks, nullptr, L, ik, tg.data(), sp, S, mo.data()));
        REJECT(DEV(batch, uniform, masks, (const mtr_anim_layer*)((const char*)ly.data() + 8), L, ik, tg.data(), sp, S, mo.data()));
        REJECT(DEV(batch, uniform, masks, ly.data(), 0, ik, tg.data(), sp, S, mo.data()));
        REJECT(DEV(batch, uniform, masks, ly.data(), 9, ik, tg.data(), sp, S, mo.data()));
        REJECT(DEV(batch, uniform, masks, ly.data(), L, ik, nullptr, sp, S, mo.data()));       // an IK set without targets
        REJECT(DEV(batch, uniform, masks, ly.data(), L, nullptr, tg.data(), sp, S, mo.data()));  // targets without an IK set
        REJECT(DEV(batch, uniform, masks, ly.data(), L, ik, (const mtr_ik_target*)((const char*)tg.data() + 8), sp, S, mo.data()));
        REJECT(DEV(batch, uniform, masks, ly.data(), L, ik_tree, tg.data(), sp, S, mo.data()));
        REJECT(DEV(batch, uniform, masks, ly.data(), L, ik, tg.data(), nullptr, S, mo.data()));
        REJECT(DEV(batch, uniform, masks, ly.data(), L, ik, tg.data(), sp_other, S, mo.data()));
        REJECT(DEV(batch, uniform, masks, ly.data(), L, ik, tg.data(), sp_foreign, S, mo.data()));
        REJECT(DEV(batch, uniform, masks, ly.data(), L, ik, tg.data(), sp_tree, S, mo.data()));
        snprintf(want, sizeof want, "joint %u ", moved);
        NAMES(want);
        REJECT(DEV(batch, uniform, masks, ly.data(), L, ik, tg.data(), sp, nullptr, mo.data()));
        REJECT(DEV(batch, uniform, masks, ly.data(), L, ik, tg.data(), sp, (mtr_spring_state*)((char*)S + 8), mo.data()));
        REJECT(DEV(batch, uniform, masks, ly.data(), L, ik, tg.data(), sp, S, (const float*)((const char*)mo.data() + 4)));
        {
            mtr_batch* plain = nullptr;  // a batch whose model has no skeleton
            EXPECT(mtr_batch_create(dev, bare, n, mats.data(), nullptr, 0, nullptr, &plain), MTR_OK);
            REJECT(DEV(plain, uniform, masks, ly.data(), L, ik, tg.data(), sp, S, mo.data()));
            mtr_batch_destroy(plain);
        }
#define HOOK(a, mk, ikp, spp, lyp, nl, tgp, stp, nn, outp, cnt) mtr_anim_sample_spring(a, mk, ikp, spp, lyp, nl, tgp, stp, mo.data(), dt, nn, outp, cnt)
        EXPECT(HOOK(nullptr, masks, ik, sp, ly.data(), L, tg.data(), S, n, locals.data(), locals.size()), MTR_E_INVALID);
        REJECT(HOOK(uniform, masks, ik, nullptr, ly.data(), L, tg.data(), S, n, locals.data(), locals.size()));
        REJECT(HOOK(uniform, masks, ik, sp_other, ly.data(), L, tg.data(), S, n, locals.data(), locals.size()));
        REJECT(HOOK(uniform, masks, ik, sp_foreign, ly.data(), L, tg.data(), S, n, locals.data(), locals.size()));
        REJECT(HOOK(uniform, masks, ik_tree, sp, ly.data(), L, tg.data(), S, n, locals.data(), locals.size()));  // the two sets disagree
        REJECT(HOOK(uniform, masks, ik, sp, ly.data(), 9, tg.data(), S, n, locals.data(), locals.size()));
        REJECT(HOOK(uniform, masks, ik, sp, nullptr, L, tg.data(), S, n, locals.data(), locals.size()));
        REJECT(HOOK(uniform, masks, ik, sp, ly.data(), L, nullptr, S, n, locals.data(), locals.size()));
        REJECT(HOOK(uniform, masks, nullptr, sp, ly.data(), L, tg.data(), S, n, locals.data(), locals.size()));
        REJECT(HOOK(uniform, masks, ik, sp, ly.data(), L, tg.data(), nullptr, n, locals.data(), locals.size()));
        REJECT(HOOK(uniform, masks, ik, sp, ly.data(), L, tg.data(), S, n, locals.data(), locals.size() - 1));
        REJECT(HOOK(uniform, masks, ik, sp, ly.data(), L, tg.data(), S, n, nullptr, locals.size()));
        // ---- one batch animated with frames in flight, spring sets created, used and destroyed with their calls queued ----
        mtr_frame* frames[3] = {};
        int k = 0;
        for (auto& f : frames) {
            if (k == 1) EXPECT(mtr_batch_animate_layers_device(batch, uniform, masks, ly.data(), L, nullptr), MTR_OK);
            else EXPECT(mtr_batch_animate_spring_device(batch, tracks, masks, ly.data(), L, ik, tg.data(), sp, dst.data(), nullptr, dt, k ? s1 : s2), MTR_OK);
            mtr_anim_spring* tmp = nullptr;
            EXPECT(mtr_anim_spring_create(dev, J, parents.data(), K, springs.data(), &tmp), MTR_OK);
            EXPECT(mtr_batch_animate_spring_device(batch, uniform, nullptr, ly.data(), L, nullptr, nullptr, tmp, dst.data(), mo.data(), dt, k % 2 ? s2 : s1), MTR_OK);
            mtr_anim_spring_destroy(tmp);  // its call is queued
            animated += 2;
            EXPECT(mtr_frame_begin(dev, 64, 48, clear, 1.0f, &f), MTR_OK);
            EXPECT(mtr_frame_draw_batch(f, batch, vp), MTR_OK);
            EXPECT(mtr_frame_submit(f), MTR_OK);
            k++;
        }
        mtr_anim_spring_destroy(sp);  // straight after a submit
        mtr_anim_spring_destroy(sp_other);
        mtr_anim_spring_destroy(sp_tree);
        mtr_anim_spring_destroy(sp_foreign);
        mtr_anim_spring_destroy(nullptr);
        mtr_anim_ik_destroy(ik);
        mtr_anim_ik_destroy(ik_tree);
        mtr_anim_masks_destroy(masks);
        mtr_anim_destroy(uniform);
        mtr_anim_destroy(tracks);
        mtr_anim_destroy(other);
        for (auto& f : frames) { EXPECT(mtr_frame_wait(f), MTR_OK); mtr_frame_destroy(f); }
        mtr_batch_destroy(batch);
        mtr_model_destroy(model);
        mtr_model_destroy(bare);
    }
    (void)hipStreamDestroy(s1);
    (void)hipStreamDestroy(s2);
    mtr_device_destroy(dev2);
    mtr_device_destroy(dev);
    printf("animated=%ld rejected=%ld launches=%llu state_steps=%llu path_reads=%llu\n", animated, rejected, (unsigned long long)g_launches,
           (unsigned long long)g_state_steps, (unsigned long long)g_path_reads);
    return 0;
}
