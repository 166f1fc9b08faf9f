// AddressSanitizer / UBSan run of the HOST side of root motion (csrc/host_anim.cpp, csrc/host_batch.cpp: mtr_anim_root_create / _destroy,
// mtr_batch_root_motion(_device), mtr_anim_root_deltas(_device)) over the stand-in HIP runtime (tests/cpp/hip_stub: device
// memory = host heap), a stand-alone program.  The two k_root launchers here are readers: they touch the first and last
// step, the first and last word of the clip table, of the root flags and of the keys (or descriptors, values and times),
// the first and last input matrix, and write the first and last output element.  A wrong size or offset on the host side
// is an ASan report.  Every rejected call of include/mtr.h's table is made and must leave the batch's version ring as it
// was; root sets are created and destroyed with calls queued and frames in flight; and a trace hook pins the event order of
// a root-motion call between an animate call and an attach call on the same batch.
//   usage: root_host_asan <iterations>
#define MTR_RND_SEED 0x13198A2E03707344ull
#include "harness.h"

static uint64_t g_root_launches = 0, g_delta_launches = 0, g_step_reads = 0;
static float g_sink = 0.0f;
static size_t g_key_words = 0;  // what the trajectory set of the next launch holds behind its clip table (uniform keys)

static void touch_root(const RootParams& p, bool apply, hipStream_t s) {
    const AnimParams& a = p.anim;
    if (!p.steps || ((uintptr_t)p.steps & 15u) || p.nsteps < 1 || p.nsteps > MTR_ROOT_MAX_STEPS || !p.n || !p.root_flags || !a.clips || !a.nclips) abort();
    if (p.joint >= a.pose.njoints || !p.out || (apply && !p.mats_in)) abort();
    if (a.tracks ? (a.keys || !a.values || !a.times) : (!a.keys || a.values || a.times)) abort();
    uint32_t acc = p.steps[0] + p.steps[(size_t)p.n * p.nsteps * 4 - 1];
    g_step_reads += 2;
    acc += a.clips[0] + a.clips[(size_t)a.nclips * 4 - 1] + p.root_flags[0] + p.root_flags[a.nclips - 1];
    if (p.root_flags[a.nclips - 1] & ~1u) abort();
    if (a.tracks) {
        const uint32_t* last = a.tracks + ((size_t)a.nclips * a.pose.njoints * 3 - 1) * 8;
        acc += a.tracks[0] + last[7] + a.values[0] + a.values[((size_t)last[0] + last[1]) * 2 - 1] + a.times[(size_t)last[0] + last[1] - 1];
    } else {
        g_sink += a.keys[0] + a.keys[g_key_words - 1];
    }
    if (apply) g_sink += p.mats_in[0] + p.mats_in[(size_t)p.n * 16 - 1];
    p.out[0] = (float)acc;
    p.out[(size_t)p.n * 16 - 1] = 1.0f;
    g_ops.push_back({apply ? "root" : "root_deltas", 0, p.out, s});
}
void mtr_launch_root(const RootParams& p, hipStream_t s) { g_root_launches++; touch_root(p, true, s); }
void mtr_launch_root_deltas(const RootParams& p, hipStream_t s) { g_delta_launches++; touch_root(p, false, s); }
void mtr_launch_attach(const AttachParams& p, hipStream_t s) {
    g_sink += (float)p.recs[0] + p.src_mats[0] + p.src_mats[(size_t)p.n_src * 16 - 1];
    p.out[0] = 1.0f;
    p.out[(size_t)p.n * 16 - 1] = 1.0f;
    g_ops.push_back({"attach", 0, p.out, s});
}
void mtr_launch_anim(const AnimParams& p, bool, bool fold, uint32_t ninst, hipStream_t s) {
    if (!fold) abort();  // no sample call is made here
    p.pose.out[(size_t)ninst * p.pose.njoints * 16 - 1] = (float)p.states[(size_t)ninst * 6 - 1];
    g_ops.push_back({"anim", 0, p.pose.out, s});
}

static int32_t make_tracks(mtr_device* dev, uint32_t J, uint32_t nclips, const uint32_t* flags, mtr_anim** out) {
    std::vector<uint32_t> nticks(nclips, 16u);
    std::vector<mtr_anim_track> tr((size_t)nclips * J * 3);
    std::vector<uint16_t> times(tr.size(), 0), values(tr.size() * 4, 7);
    for (size_t t = 0; t < tr.size(); t++) { tr[t] = mtr_anim_track{}; tr[t].first = (uint32_t)t; tr[t].count = 1; }
    return mtr_anim_create_tracks(dev, J, nclips, nticks.data(), flags, tr.data(), times.data(), values.data(), times.size(), out);
}

struct Ring {
    int cur;
    std::vector<mtr_batch::Ver> vers;
    bool operator==(const Ring& o) const {
        if (cur != o.cur || vers.size() != o.vers.size()) return false;
        for (size_t i = 0; i < vers.size(); i++) {
            const mtr_batch::Ver &a = vers[i], &b = o.vers[i];
            if (a.d != b.d || a.ready != b.ready || a.read != b.read || a.read_pending != b.read_pending || a.pinned != b.pinned || a.npal != b.npal) return false;
        }
        return true;
    }
};
static Ring ring(const mtr_batch* b) { return Ring{b->cur, b->vers}; }

// ---- the event order of animate, root motion, attach on one batch ----
static mtr_device* g_dev = nullptr;
static hipStream_t g_caller = nullptr;
static std::string name_of(const mtr_batch* b, const mtr_anim* traj, const mtr_anim_root* root, const mtr_anim* anim, const void* w) {
    if (!w) return "";
    for (size_t i = 0; i < b->vers.size(); i++) {
        const mtr_batch::Ver& v = b->vers[i];
        const std::string base = " v" + std::to_string(i);
        if (w == v.ready) return base + ".ready";
        if (w == v.read) return base + ".read";
        if (w == v.d) return base;
        if (v.d && w == v.d + (size_t)b->n * 16) return base + ".pals";
    }
    if (w == traj->last) return " traj.last";
    if (w == root->last) return " root.last";
    if (w == anim->last) return " anim.last";
    if (w == g_dev->pose_stage) return " stage";
    return " elsewhere";
}
static std::string stream_name(const void* s) { return s == g_dev->s_copy ? "copy" : s == g_dev->stream ? "public" : s == g_caller ? "caller" : "?"; }
static long find(const std::vector<std::string>& l, const std::string& line) {
    for (long i = 0; i < (long)l.size(); i++)
        if (l[(size_t)i] == line) return i;
    return -1;
}
#define ORDER(l, a, b) do { const long ia_ = find(l, a), ib_ = find(l, b); if (ia_ < 0 || ib_ < 0 || ia_ >= ib_) { \
    fprintf(stderr, "line %d: '%s' (%ld) does not come before '%s' (%ld)\n", __LINE__, std::string(a).c_str(), ia_, std::string(b).c_str(), ib_); \
    for (const std::string& s_ : l) fprintf(stderr, "    %s\n", s_.c_str()); g_failed++; } } while (0)

static int event_order(mtr_device* dev, mtr_model* model, uint32_t J) {
    const uint32_t n = 5, S = 2;
    std::vector<float> mats((size_t)n * 16, 0.0f);
    mtr_batch* b = nullptr;
    EXPECT(mtr_batch_create(dev, model, n, mats.data(), nullptr, 0, nullptr, &b), MTR_OK);
    const uint32_t nk = 4;
    std::vector<mtr_anim_key> keys((size_t)nk * J), tkeys(nk);
    mtr_anim *anim = nullptr, *traj = nullptr;
    mtr_anim_root* root = nullptr;
    EXPECT(mtr_anim_create(dev, J, 1, &nk, nullptr, keys.data(), &anim), MTR_OK);
    EXPECT(mtr_anim_create(dev, 1, 1, &nk, nullptr, tkeys.data(), &traj), MTR_OK);
    const uint32_t cyc = MTR_ROOT_CYCLIC;
    EXPECT(mtr_anim_root_create(dev, 1, 1, 0, &cyc, &root), MTR_OK);
    std::vector<mtr_anim_state> st(n, mtr_anim_state{});
    std::vector<mtr_root_step> steps((size_t)n * S, mtr_root_step{0, 1.0f, 0.5f, 0.5f});
    mtr_attach* recs = static_cast<mtr_attach*>(aligned_alloc(16, n * sizeof(mtr_attach)));
    memset(recs, 0, n * sizeof(mtr_attach));
    {   // the staging buffer at its steady size: growing it is the one host wait of a host-record call
        std::vector<float> z((size_t)n * J * 16, 0.0f);
        EXPECT(stage_pose(dev, z.data(), z.size()), MTR_OK);
    }
    g_key_words = (size_t)nk * 12;
    hipStubTrace() = trace;
    g_ops.clear();
    EXPECT(mtr_batch_animate(b, anim, st.data()), MTR_OK);                       // writes version A on the copy stream
    const int va = b->cur;
    const size_t mark1 = g_ops.size();
    EXPECT(mtr_batch_root_motion(b, traj, root, steps.data(), S), MTR_OK);        // reads A, writes version B on the copy stream
    const int vb = b->cur;
    const size_t mark2 = g_ops.size();
    EXPECT(mtr_batch_attach_device(b, b, recs, g_caller), MTR_OK);                // reads B, writes version C on the caller's stream
    const int vc = b->cur;
    hipStubTrace() = nullptr;
    CHECK(va != vb && vb != vc);  // a call never writes the version it reads; C may be A again, which nothing draws
    CHECK(b->vers[(size_t)vb].npal == J && b->vers[(size_t)vc].npal == J);        // the palettes are kept
    std::vector<std::string> l1, l2, l3;
    for (size_t i = 0; i < g_ops.size(); i++)
        (i < mark1 ? l1 : i < mark2 ? l2 : l3).push_back(g_ops[i].op + name_of(b, traj, root, anim, g_ops[i].what) + " " + stream_name(g_ops[i].stream));
    const std::string A = " v" + std::to_string(va), B = " v" + std::to_string(vb), Cv = " v" + std::to_string(vc);
    ORDER(l1, "anim" + A + ".pals copy", "hipEventRecord" + A + ".ready copy");
    // the root-motion call: its steps staged, then behind A's write; the kernel; then the events of everything it read and wrote
    ORDER(l2, "hipMemcpyAsync stage copy", "hipStreamWaitEvent" + A + ".ready copy");
    ORDER(l2, "hipStreamWaitEvent" + A + ".ready copy", "root" + B + " copy");
    ORDER(l2, "root" + B + " copy", "hipEventRecord traj.last copy");
    ORDER(l2, "root" + B + " copy", "hipEventRecord root.last copy");
    ORDER(l2, "root" + B + " copy", "hipEventRecord" + A + ".read copy");
    ORDER(l2, "root" + B + " copy", "hipMemcpyAsync" + B + ".pals copy");         // the palettes, device to device
    ORDER(l2, "hipMemcpyAsync" + B + ".pals copy", "hipEventRecord" + B + ".ready copy");
    CHECK(find(l2, "hipStreamSynchronize copy") < 0 && find(l2, "hipStreamSynchronize public") < 0);  // no host wait
    // the attach call on another stream waits for the root-motion write before k_attach reads it
    ORDER(l3, "hipStreamWaitEvent" + B + ".ready caller", "attach" + Cv + " caller");
    ORDER(l3, "attach" + Cv + " caller", "hipEventRecord" + B + ".read caller");
    ORDER(l3, "attach" + Cv + " caller", "hipEventRecord" + Cv + ".ready caller");
    if (vc == va) {  // the write into the version k_root read waits for that reader, and clears its mark
        ORDER(l3, "hipStreamWaitEvent" + A + ".read caller", "attach" + Cv + " caller");
        CHECK(!b->vers[(size_t)va].read_pending);
    } else {
        CHECK(b->vers[(size_t)va].read_pending);
    }
    CHECK(b->vers[(size_t)vb].read_pending && traj->recorded && root->recorded && traj->last_stream == dev->s_copy && root->last_stream == dev->s_copy);
    // a second root-motion call on the caller's stream waits for the trajectory set's and the root set's last reader
    g_ops.clear();
    hipStubTrace() = trace;
    EXPECT(mtr_batch_root_motion_device(b, traj, root, steps.data(), S, g_caller), MTR_OK);
    hipStubTrace() = nullptr;
    std::vector<std::string> l4;
    for (const Op& o : g_ops) l4.push_back(o.op + name_of(b, traj, root, anim, o.what) + " " + stream_name(o.stream));
    const std::string D = " v" + std::to_string(b->cur);
    ORDER(l4, "hipStreamWaitEvent traj.last caller", "root" + D + " caller");
    ORDER(l4, "hipStreamWaitEvent root.last caller", "root" + D + " caller");
    ORDER(l4, "hipStreamWaitEvent" + Cv + ".ready caller", "root" + D + " caller");
    mtr_anim_root_destroy(root);  // with the call queued: parked, not freed
    mtr_anim_destroy(traj);
    mtr_anim_destroy(anim);
    mtr_batch_destroy(b);
    free(recs);
    return 0;
}

int main(int argc, char** argv) {
    const long iters = argc > 1 ? strtol(argv[1], nullptr, 10) : 40;
    static const float verts[24] = {1, 1, -1, 1, -1, -1, 1, 1, 1, 1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1};
    static const uint16_t idx[36] = {4, 2, 0, 2, 7, 3, 6, 5, 7, 1, 7, 5, 0, 3, 1, 4, 1, 5, 4, 6, 2, 2, 6, 7, 6, 4, 5, 1, 3, 7, 0, 2, 3, 4, 0, 1};
    mtr_device *dev = nullptr, *dev2 = nullptr;
    if (mtr_device_create(0, &dev) || mtr_device_create(0, &dev2)) return 3;
    g_dev = dev;
    if (hipStreamCreateWithFlags(&g_caller, hipStreamNonBlocking)) return 3;
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
    long moved = 0, rejected = 0;
    {   // the event order, on a model with a skeleton (the animate call needs one; root motion does not)
        mtr_model* model = nullptr;
        EXPECT(mtr_model_create(dev, verts, sizeof verts, idx, 36, &p, 1, &l, &p2t, nullptr, 0, &dbg, &model), MTR_OK);
        const uint32_t J = 6;
        std::vector<uint8_t> parents(J);
        for (uint32_t j = 0; j < J; j++) parents[j] = j ? (uint8_t)(j - 1) : 255;
        std::vector<float> imats((size_t)J * 16, 1.0f);
        EXPECT(mtr_model_set_skeleton(model, parents.data(), imats.data(), J), MTR_OK);
        if (event_order(dev, model, J)) return 1;
        mtr_model_destroy(model);
    }
    for (long it = 0; it < iters; it++) {
        mtr_model* bare = nullptr;  // no skeleton
        EXPECT(mtr_model_create(dev, verts, sizeof verts, idx, 36, &p, 1, &l, &p2t, nullptr, 0, &dbg, &bare), MTR_OK);
        const uint32_t J = it % 7 == 0 ? 256 : pick(1, 9), C = pick(1, 5), n = pick(1, 40), S = it % 5 == 0 ? 8 : pick(1, 8), joint = pick(0, J - 1);
        const uint32_t npal = it % 3 ? 0 : pick(1, 4);
        std::vector<float> mats((size_t)n * 16, 0.0f), pals((size_t)n * npal * 16, 0.5f);
        mtr_batch* batch = nullptr;
        EXPECT(mtr_batch_create(dev, bare, n, mats.data(), npal ? pals.data() : nullptr, npal, nullptr, &batch), MTR_OK);
        std::vector<uint32_t> nk(C), rflags(C), loopf(C, 0u);
        size_t total = 0;
        for (uint32_t c = 0; c < C; c++) { nk[c] = pick(1, 20); total += nk[c]; rflags[c] = (uint32_t)(rnd() & 1); }
        loopf[pick(0, C - 1)] = MTR_CLIP_LOOP;
        std::vector<mtr_anim_key> keys(total * J);  // exactly sized
        for (auto& k : keys) { k = mtr_anim_key{}; k.q[3] = 1.0f; }
        mtr_anim *uniform = nullptr, *tracks = nullptr, *looped = nullptr, *looped_tracks = nullptr, *other_j = nullptr, *other_c = nullptr, *foreign = nullptr;
        EXPECT(mtr_anim_create(dev, J, C, nk.data(), nullptr, keys.data(), &uniform), MTR_OK);
        EXPECT(make_tracks(dev, J, C, nullptr, &tracks), MTR_OK);
        EXPECT(mtr_anim_create(dev, J, C, nk.data(), loopf.data(), keys.data(), &looped), MTR_OK);
        EXPECT(make_tracks(dev, J, C, loopf.data(), &looped_tracks), MTR_OK);
        EXPECT(make_tracks(dev, J == 256 ? 255 : J + 1, C, nullptr, &other_j), MTR_OK);
        EXPECT(make_tracks(dev, J, C + 1, nullptr, &other_c), MTR_OK);
        EXPECT(make_tracks(dev2, J, C, nullptr, &foreign), MTR_OK);
        g_key_words = total * J * 12;
        // ---- root sets: every invalid creation ----
        mtr_anim_root* none = (mtr_anim_root*)1;
        EXPECT(mtr_anim_root_create(nullptr, J, C, joint, rflags.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_root_create(dev, J, C, joint, rflags.data(), nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_root_create(dev, 0, C, 0, rflags.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_root_create(dev, 257, C, joint, rflags.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_root_create(dev, J, 0, joint, rflags.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_root_create(dev, J, C, J, rflags.data(), &none), MTR_E_INVALID);
        EXPECT(mtr_anim_root_create(dev, J, C, 0xFFFFFFFFu, rflags.data(), &none), MTR_E_INVALID);
        {
            std::vector<uint32_t> bad = rflags;
            const uint32_t c = pick(0, C - 1);
            bad[c] |= 2u << pick(0, 29);
            char want[32];
            snprintf(want, sizeof want, "clip %u ", c);
            EXPECT(mtr_anim_root_create(dev, J, C, joint, bad.data(), &none), MTR_E_INVALID); NAMES(want);
        }
        if (none) { fprintf(stderr, "a failed create must clear *out\n"); return 1; }
        rejected += 8;
        mtr_anim_root *root = nullptr, *root0 = nullptr, *root_j = nullptr, *root_c = nullptr, *root_foreign = nullptr;
        EXPECT(mtr_anim_root_create(dev, J, C, joint, rflags.data(), &root), MTR_OK);
        EXPECT(mtr_anim_root_create(dev, J, C, joint, nullptr, &root0), MTR_OK);  // NULL flags: all 0
        EXPECT(mtr_anim_root_create(dev, J == 256 ? 255 : J + 1, C, 0, nullptr, &root_j), MTR_OK);
        EXPECT(mtr_anim_root_create(dev, J, C + 1, joint, nullptr, &root_c), MTR_OK);
        EXPECT(mtr_anim_root_create(dev2, J, C, joint, rflags.data(), &root_foreign), MTR_OK);
        std::vector<mtr_root_step> steps((size_t)n * S);  // exactly sized: one record too many read is a report
        for (auto& s : steps) { s.clip = (uint32_t)rnd(); s.x = rnd() % 5 ? (float)(rnd() % 1000) * 0.37f : NAN; s.dx = rnd() % 6 ? 0.37f : INFINITY; s.w = rnd() % 4 ? 0.5f : NAN; }
        mtr_root_step* steps_dev = static_cast<mtr_root_step*>(aligned_alloc(16, steps.size() * sizeof(mtr_root_step)));
        memcpy(steps_dev, steps.data(), steps.size() * sizeof(mtr_root_step));
        std::vector<float> out((size_t)n * 16, 0.0f);
        float* out_dev = static_cast<float*>(aligned_alloc(16, out.size() * 4));
        // ---- the valid calls: both kinds of set, host and "device" steps (stub: host memory) ----
        EXPECT(mtr_batch_root_motion(batch, uniform, root, steps.data(), S), MTR_OK);
        EXPECT(mtr_batch_root_motion(batch, tracks, root0, steps.data(), S), MTR_OK);
        EXPECT(mtr_batch_root_motion_device(batch, tracks, root, steps_dev, S, nullptr), MTR_OK);
        EXPECT(mtr_batch_root_motion_device(batch, uniform, root, steps_dev, S, g_caller), MTR_OK);
        EXPECT(mtr_anim_root_deltas(uniform, root, steps.data(), S, n, out.data(), out.size()), MTR_OK);
        EXPECT(mtr_anim_root_deltas(tracks, root, steps.data(), S, n, out.data(), out.size() + 3), MTR_OK);
        EXPECT(mtr_anim_root_deltas_device(tracks, root0, steps_dev, S, n, out_dev, nullptr), MTR_OK);
        EXPECT(mtr_anim_root_deltas_device(uniform, root, steps_dev, S, n, out_dev, g_caller), MTR_OK);
        CHECK(out[n * 16 - 1] == 1.0f && out_dev[n * 16 - 1] == 1.0f);
        moved += 8;
        {
            mtr_batch::Ver v = batch->vers[(size_t)batch->cur];
            CHECK(v.npal == npal);  // npal is kept
        }
        // ---- every invalid call: nothing changes ----
        const Ring before = ring(batch);
        const mtr_root_step* odd = (const mtr_root_step*)((const char*)steps_dev + 8);
        EXPECT(mtr_batch_root_motion(nullptr, uniform, root, steps.data(), S), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion(batch, nullptr, root, steps.data(), S), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion(batch, uniform, nullptr, steps.data(), S), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion(batch, uniform, root, nullptr, S), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion(batch, uniform, root, steps.data(), 0), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion(batch, uniform, root, steps.data(), 9), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion(batch, looped, root, steps.data(), S), MTR_E_INVALID); NAMES("LOOP");
        EXPECT(mtr_batch_root_motion(batch, looped_tracks, root, steps.data(), S), MTR_E_INVALID); NAMES("LOOP");
        EXPECT(mtr_batch_root_motion(batch, other_j, root, steps.data(), S), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion(batch, other_c, root, steps.data(), S), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion(batch, uniform, root_j, steps.data(), S), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion(batch, uniform, root_c, steps.data(), S), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion(batch, uniform, root_foreign, steps.data(), S), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion(batch, foreign, root_foreign, steps.data(), S), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion_device(nullptr, uniform, root, steps_dev, S, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion_device(batch, nullptr, root, steps_dev, S, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion_device(batch, uniform, nullptr, steps_dev, S, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion_device(batch, uniform, root, nullptr, S, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion_device(batch, uniform, root, odd, S, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion_device(batch, uniform, root, steps_dev, 0, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion_device(batch, uniform, root, steps_dev, 9, g_caller), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion_device(batch, looped, root, steps_dev, S, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion_device(batch, tracks, root_c, steps_dev, S, nullptr), MTR_E_INVALID);
        EXPECT(mtr_batch_root_motion_device(batch, tracks, root_foreign, steps_dev, S, nullptr), MTR_E_INVALID);
        CHECK(ring(batch) == before);
        const uint64_t launches = g_root_launches + g_delta_launches;
        EXPECT(mtr_anim_root_deltas(nullptr, root, steps.data(), S, n, out.data(), out.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas(uniform, nullptr, steps.data(), S, n, out.data(), out.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas(uniform, root, nullptr, S, n, out.data(), out.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas(uniform, root, steps.data(), S, n, nullptr, out.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas(uniform, root, steps.data(), 0, n, out.data(), out.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas(uniform, root, steps.data(), 9, n, out.data(), out.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas(uniform, root, steps.data(), S, 0, out.data(), out.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas(uniform, root, steps.data(), S, ((size_t)1 << 27) + 1, out.data(), (size_t)1 << 40), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas(uniform, root, steps.data(), S, n, out.data(), out.size() - 1), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas(looped, root, steps.data(), S, n, out.data(), out.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas(other_j, root, steps.data(), S, n, out.data(), out.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas(uniform, root_foreign, steps.data(), S, n, out.data(), out.size()), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas_device(nullptr, root, steps_dev, S, n, out_dev, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas_device(uniform, nullptr, steps_dev, S, n, out_dev, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas_device(uniform, root, nullptr, S, n, out_dev, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas_device(uniform, root, odd, S, n, out_dev, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas_device(uniform, root, steps_dev, S, n, nullptr, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas_device(uniform, root, steps_dev, S, n, out_dev + 1, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas_device(uniform, root, steps_dev, S, 0, out_dev, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas_device(uniform, root, steps_dev, S, ((size_t)1 << 27) + 1, out_dev, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas_device(uniform, root, steps_dev, 9, n, out_dev, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas_device(looped_tracks, root, steps_dev, S, n, out_dev, nullptr), MTR_E_INVALID);
        EXPECT(mtr_anim_root_deltas_device(uniform, root_c, steps_dev, S, n, out_dev, nullptr), MTR_E_INVALID);
        CHECK(launches == g_root_launches + g_delta_launches);
        rejected += 24 + 23;
        // ---- frames in flight, root sets created and destroyed with calls queued ----
        mtr_frame* frames[3] = {};
        int k = 0;
        for (auto& f : frames) {
            mtr_anim_root* tmp = nullptr;
            EXPECT(mtr_anim_root_create(dev, J, C, joint, rflags.data(), &tmp), MTR_OK);
            if (k == 1) EXPECT(mtr_batch_root_motion_device(batch, uniform, tmp, steps_dev, S, g_caller), MTR_OK);
            else EXPECT(mtr_batch_root_motion(batch, k ? tracks : uniform, tmp, steps.data(), S), MTR_OK);
            moved++;
            mtr_anim_root_destroy(tmp);  // straight after the call: the kernel is queued
            EXPECT(mtr_frame_begin(dev, 64, 48, clear, 1.0f, &f), MTR_OK);
            EXPECT(mtr_frame_draw_batch(f, batch, vp), MTR_OK);
            EXPECT(mtr_frame_submit(f), MTR_OK);
            k++;
        }
        mtr_anim_root_destroy(root);
        mtr_anim_root_destroy(root0);
        mtr_anim_root_destroy(root_j);
        mtr_anim_root_destroy(root_c);
        mtr_anim_root_destroy(root_foreign);
        mtr_anim_root_destroy(nullptr);
        for (mtr_anim* a : {uniform, tracks, looped, looped_tracks, other_j, other_c, foreign}) mtr_anim_destroy(a);
        for (auto& f : frames) { EXPECT(mtr_frame_wait(f), MTR_OK); mtr_frame_destroy(f); }
        mtr_batch_destroy(batch);
        mtr_model_destroy(bare);
        free(steps_dev);
        free(out_dev);
    }
    hipStreamDestroy(g_caller);
    mtr_device_destroy(dev2);
    mtr_device_destroy(dev);
    printf("moved=%ld rejected=%ld root_launches=%llu delta_launches=%llu step_reads=%llu failed=%d sink=%s\n", moved, rejected, (unsigned long long)g_root_launches,
           (unsigned long long)g_delta_launches, (unsigned long long)g_step_reads, g_failed, g_sink == g_sink ? "ok" : "nan");
    return g_failed ? 1 : 0;
}
