// The stream traffic of every animation entry point (SPEC.md sections 13 to 20), pinned on the CPU: the host side of the
// library (csrc/host_*.cpp) over the stand-in HIP runtime of tests/cpp/hip_stub, compiled with AddressSanitizer and UBSan.
// The program makes each call once at the smallest shapes that reach every branch (a 3-joint chain, 2 instances, a uniform
// set and a track set of 2 clips, 1 and 2 layers with and without masks, 1 IK chain, root motion of 1 and 2 steps, a player
// with and without host commands), the device variants on the device's own stream and on a caller's stream in turn, so that
// every set is read on a second stream after a first; then each set's destroy with a kernel queued, and one rejected call
// per entry point.  It prints what reaches the runtime: operation, byte count, and streams (S), events (E) and buffers (B)
// numbered by first appearance; every launcher prints its name, its instance count and where its parameters point, as byte
// offsets from the base of the image they lie in.  tests/test_anim_call_trace.py compares the text with
// tests/golden/anim_call_trace.txt.  A rejected call must print no operation.  What it does not see: the stand-in's
// synchronous hipMemcpy is not traced and the clip, track, mask, IK and root sets are created with the trace off, so the
// sizes and the order of the parts a create uploads are pinned only through the launchers' offsets here, by the ASan
// harnesses of each feature (whose launchers read the first and last word of every part) and by the GPU tests.
#include "host_all.h"
using namespace mtr_host;

#define MUST(x) do { if ((x) != MTR_OK) { fprintf(stderr, "line %d: %s failed\n", __LINE__, #x); exit(4); } } while (0)

// ---- names by first appearance ----
static std::vector<const void*> g_streams, g_events, g_bufs;
static std::string named(std::vector<const void*>& v, const void* p, char tag) {
    if (!p) return "-";
    size_t i = 0;
    while (i < v.size() && v[i] != p) i++;
    if (i == v.size()) v.push_back(p);
    return tag + std::to_string(i);
}
static std::string S(const void* p) { return named(g_streams, p, 'S'); }
static std::string E(const void* p) { return named(g_events, p, 'E'); }
static std::string B(const void* p) { return named(g_bufs, p, 'B'); }
static std::string off(const void* p, const void* base) {
    return p ? "+" + std::to_string(static_cast<const char*>(p) - static_cast<const char*>(base)) : std::string("-");
}
static std::string num(uint64_t v) { return std::to_string(v); }

static long g_ops = 0;
static void trace(const char* name, size_t bytes, const void* what, const void* stream) {
    const bool ev = !strcmp(name, "hipStreamWaitEvent") || !strcmp(name, "hipEventRecord");
    const std::string w = ev ? E(what) : B(what), s = S(stream);
    printf("    %s %zu %s %s\n", name, bytes, w.c_str(), s.c_str());
    g_ops++;
}
static void launched(const char* name, uint64_t n, hipStream_t s, const std::string& params) {
    const std::string sn = S(s);
    printf("    launch %s ninst=%llu %s%s\n", name, (unsigned long long)n, sn.c_str(), params.c_str());
    g_ops++;
}

// ---- the launchers ----
static std::string pose_str(const PoseParams& p) {
    std::string s = " njoints=" + num(p.njoints) + " path_bytes=" + num(p.path_bytes);
    s += " locals=" + B(p.locals);
    s += " imats=" + B(p.imats) + " paths=" + off(p.paths, p.imats) + " path_words=" + off(p.path_words, p.imats);
    s += " out=" + B(p.out);
    return s;
}
static std::string anim_str(const AnimParams& a) {
    std::string s = " nclips=" + num(a.nclips) + " clips=" + B(a.clips) + " keys=" + off(a.keys, a.clips) + " tracks=" + off(a.tracks, a.clips) +
                    " values=" + off(a.values, a.clips) + " times=" + off(a.times, a.clips);
    s += " states=" + B(a.states);
    return s + pose_str(a.pose);
}
static std::string layers_str(const AnimLayerParams& l) {
    std::string s = " nlayers=" + num(l.nlayers) + " nmasks=" + num(l.nmasks) + " layers=" + B(l.layers);
    s += " masks=" + B(l.masks);
    return s + anim_str(l.anim);
}
static std::string ik_str(const AnimIkParams& k) {
    std::string s = " nchains=" + num(k.nchains) + " ik_path_bytes=" + num(k.path_bytes) + " chains=" + B(k.chains);
    s += " targets=" + B(k.targets);
    const bool own = k.paths == k.layers.anim.pose.paths;  // the model's table, or the IK set's copy behind its chains
    s += own ? std::string(" ik_paths=pose") : " ik_paths=" + off(k.paths, k.chains) + " ik_path_words=" + off(k.path_words, k.chains);
    return s + layers_str(k.layers);
}
void mtr_launch_pose(const PoseParams& p, uint32_t n, hipStream_t s) { launched("pose", n, s, pose_str(p)); }
void mtr_launch_anim(const AnimParams& p, uint32_t n, hipStream_t s) { launched("anim", n, s, anim_str(p)); }
void mtr_launch_anim_sample(const AnimParams& p, uint32_t n, hipStream_t s) { launched("anim_sample", n, s, anim_str(p)); }
void mtr_launch_anim_tracks(const AnimParams& p, uint32_t n, hipStream_t s) { launched("anim_tracks", n, s, anim_str(p)); }
void mtr_launch_anim_tracks_sample(const AnimParams& p, uint32_t n, hipStream_t s) { launched("anim_tracks_sample", n, s, anim_str(p)); }
void mtr_launch_anim_layers(const AnimLayerParams& p, uint32_t n, hipStream_t s) { launched("anim_layers", n, s, layers_str(p)); }
void mtr_launch_anim_layers_sample(const AnimLayerParams& p, uint32_t n, hipStream_t s) { launched("anim_layers_sample", n, s, layers_str(p)); }
void mtr_launch_anim_layers_tracks(const AnimLayerParams& p, uint32_t n, hipStream_t s) { launched("anim_layers_tracks", n, s, layers_str(p)); }
void mtr_launch_anim_layers_tracks_sample(const AnimLayerParams& p, uint32_t n, hipStream_t s) { launched("anim_layers_tracks_sample", n, s, layers_str(p)); }
void mtr_launch_anim_ik(const AnimIkParams& p, uint32_t n, hipStream_t s) { launched("anim_ik", n, s, ik_str(p)); }
void mtr_launch_anim_ik_sample(const AnimIkParams& p, uint32_t n, hipStream_t s) { launched("anim_ik_sample", n, s, ik_str(p)); }
void mtr_launch_anim_ik_tracks(const AnimIkParams& p, uint32_t n, hipStream_t s) { launched("anim_ik_tracks", n, s, ik_str(p)); }
void mtr_launch_anim_ik_tracks_sample(const AnimIkParams& p, uint32_t n, hipStream_t s) { launched("anim_ik_tracks_sample", n, s, ik_str(p)); }
void mtr_launch_attach(const AttachParams& p, hipStream_t s) {
    std::string t = " n_src=" + num(p.n_src) + " npal=" + num(p.npal) + " recs=" + B(p.recs);
    t += " src_mats=" + B(p.src_mats) + " src_pals=" + off(p.src_pals, p.src_mats);
    launched("attach", p.n, s, t + " out=" + B(p.out));
}
static std::string root_str(const RootParams& p) {
    std::string t = " joint=" + num(p.joint) + " nsteps=" + num(p.nsteps) + " root_flags=" + B(p.root_flags);
    t += " steps=" + B(p.steps);
    t += " mats_in=" + B(p.mats_in);
    t += " out=" + B(p.out);
    return t + anim_str(p.anim);
}
void mtr_launch_root(const RootParams& p, hipStream_t s) { launched("root", p.n, s, root_str(p)); }
void mtr_launch_root_deltas(const RootParams& p, hipStream_t s) { launched("root_deltas", p.n, s, root_str(p)); }
void mtr_launch_play(const PlayParams& p, hipStream_t s) {
    std::string t = " ncmds=" + num(p.ncmds) + " nclips=" + num(p.nclips) + " nlayers=" + num(p.nlayers) + " table=" + B(p.table) + " scratch=" + off(p.scratch, p.table);
    t += " states=" + B(p.states);
    t += " cmds=" + B(p.cmds);
    t += " out_states=" + B(p.out_states);
    t += " out_layers=" + B(p.out_layers);
    t += " out_steps=" + B(p.out_steps);
    launched("play", p.n, s, t);
}
void mtr_launch_geom(const GeomParams&, hipStream_t) {}
void mtr_launch_scan(const FrameBuffers&, hipStream_t) {}
void mtr_launch_fill(const FrameBuffers&, uint32_t, hipStream_t) {}
void mtr_launch_tile(const TileParams& p, bool, hipStream_t) { if (p.host_status) __atomic_store_n(p.host_status, 0x80000000u, __ATOMIC_RELEASE); }
void mtr_launch_tile_vis(const TileParams& p, bool, hipStream_t) { if (p.host_status) __atomic_store_n(p.host_status, 0x80000000u, __ATOMIC_RELEASE); }
void mtr_launch_alpha_min(const uint8_t*, size_t, uint32_t* out_min, hipStream_t) { *out_min = 255; }
void mtr_launch_vertex_stage(const GeomParams&, uint32_t, float*, float*, hipStream_t) {}
void mtr_launch_bc1_decode(const uint8_t*, uint8_t*, uint32_t, uint32_t, hipStream_t) {}
void mtr_launch_bc7_decode(const uint8_t*, uint8_t*, uint32_t, uint32_t, hipStream_t) {}
void mtr_launch_pack_shard(const uint8_t*, uint8_t*, uint32_t, uint32_t, const uint32_t*, uint32_t, uint32_t, hipStream_t) {}
void mtr_launch_unpack_shards(const uint8_t*, uint8_t*, uint32_t, uint32_t, const uint32_t*, hipStream_t) {}
void mtr_launch_cull_instances(const CullParams&, hipStream_t) {}
void mtr_launch_cull_chunks(const ChunkCullParams&, hipStream_t) {}

// ---- calls ----
static mtr_device* g_dev = nullptr;
static int g_failed = 0;
static long g_rejected = 0;

#define CALL(x) do { printf("%s\n", #x); hipStubTrace() = trace; const int32_t rc_ = (x); hipStubTrace() = nullptr; \
    if (rc_ != MTR_OK) { printf("    FAILED %d: %s\n", rc_, mtr_last_error(g_dev)); g_failed++; } } while (0)
// a rejected call: its code and message, and no operation
#define REJECT(x) do { const long ops_ = g_ops; hipStubTrace() = trace; const int32_t rc_ = (x); hipStubTrace() = nullptr; \
    printf("%s\n    = %d: %s\n", #x, rc_, rc_ ? mtr_last_error(g_dev) : ""); g_rejected++; \
    if (rc_ == MTR_OK || g_ops != ops_) { printf("    NOT REJECTED CLEANLY\n"); g_failed++; } } while (0)
// a destroy with a kernel queued: nothing reaches a stream; what it parks is printed
#define DESTROY(x) do { printf("%s\n", #x); const size_t g0_ = g_dev->garbage.size(); hipStubTrace() = trace; x; hipStubTrace() = nullptr; \
    for (size_t i_ = g0_; i_ < g_dev->garbage.size(); i_++) { const std::string b_ = B(g_dev->garbage[i_].p), e_ = E(g_dev->garbage[i_].ev); \
        printf("    parked %s behind %s\n", b_.c_str(), e_.c_str()); } } while (0)

template <class T>
static T* dev_copy(const std::vector<T>& v) {  // "device" memory: the stub's is the heap; 16-byte aligned like hipMalloc's
    const size_t bytes = (v.size() * sizeof(T) + 15) / 16 * 16;
    T* p = static_cast<T*>(aligned_alloc(16, bytes ? bytes : 16));
    memset(p, 0, bytes ? bytes : 16);
    if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}
template <class T>
static T* odd(T* p) { return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + 4); }  // misaligned

static mtr_anim* make_uniform(mtr_device* d, uint32_t J, const uint32_t* flags) {
    const uint32_t nk[2] = {2, 3};
    std::vector<mtr_anim_key> keys((size_t)5 * J);
    for (auto& k : keys) { k = mtr_anim_key{}; k.q[3] = 1.0f; k.s[0] = k.s[1] = k.s[2] = 1.0f; }
    mtr_anim* a = nullptr;
    MUST(mtr_anim_create(d, J, 2, nk, flags, keys.data(), &a));
    return a;
}
static mtr_anim* make_tracks(mtr_device* d, uint32_t J) {
    const uint32_t nticks[2] = {16, 8};
    std::vector<mtr_anim_track> tr((size_t)2 * J * 3);
    std::vector<uint16_t> times(tr.size() + 1, 0), values((tr.size() + 1) * 4, 7);  // an odd key total: the times end in half a word
    for (size_t t = 0; t < tr.size(); t++) { tr[t] = mtr_anim_track{}; tr[t].first = (uint32_t)t; tr[t].count = 1; }
    tr.back().count = 2; times.back() = 5;
    mtr_anim* a = nullptr;
    MUST(mtr_anim_create_tracks(d, J, 2, nticks, nullptr, tr.data(), times.data(), values.data(), times.size(), &a));
    return a;
}

int main() {
    setenv("MTR_NSLOTS", "1", 1);
    mtr_device *d = nullptr, *d2 = nullptr;
    MUST(mtr_device_create(0, &d));
    MUST(mtr_device_create(0, &d2));
    g_dev = d;
    hipStream_t caller = nullptr;
    MUST((int32_t)hipStreamCreateWithFlags(&caller, hipStreamNonBlocking));
    // the streams in a fixed order of appearance
    { const std::string a = S(d->s_copy), b = S(d->stream), c = S(caller); printf("streams: copy=%s public=%s caller=%s\n", a.c_str(), b.c_str(), c.c_str()); }

    const uint32_t J = 3, N = 2;
    const float verts[9] = {-0.5f, -0.5f, 0.5f, 0.5f, -0.5f, 0.5f, 0.0f, 0.5f, 0.5f};
    const uint16_t idx[3] = {0, 1, 2};
    mtr_primitive pr;
    memset(&pr, 0, sizeof pr);
    pr.w[0] = 3u << 16; pr.w[2] = 1 | (12u << 16) | (3u << 24); pr.w[7] = 3;
    mtr_layout lay;
    memset(&lay, 0, sizeof lay);
    lay.elements[lay.num_elements++] = mtr_element{MTR_SEM_POSITION, MTR_IEF_F32, 3, 0, 0, 0};
    mtr_model *m = nullptr, *bare = nullptr;
    MUST(mtr_model_create(d, verts, sizeof verts, idx, 3, &pr, 1, &lay, nullptr, nullptr, 0, nullptr, &m));
    MUST(mtr_model_create(d, verts, sizeof verts, idx, 3, &pr, 1, &lay, nullptr, nullptr, 0, nullptr, &bare));  // no skeleton
    const uint8_t parents[J] = {255, 0, 1};
    std::vector<float> imats((size_t)J * 16, 0.0f), mats((size_t)N * 16, 0.0f);
    for (uint32_t j = 0; j < J; j++) imats[j * 16] = imats[j * 16 + 5] = imats[j * 16 + 10] = imats[j * 16 + 15] = 1.0f;
    MUST(mtr_model_set_skeleton(m, parents, imats.data(), J));
    mtr_batch *b = nullptr, *src = nullptr, *plain = nullptr;
    MUST(mtr_batch_create(d, m, N, mats.data(), nullptr, 0, nullptr, &b));
    MUST(mtr_batch_create(d, m, 1, mats.data(), nullptr, 0, nullptr, &src));
    MUST(mtr_batch_create(d, bare, N, mats.data(), nullptr, 0, nullptr, &plain));

    // ---- the sets ----
    const uint32_t loop[2] = {MTR_CLIP_LOOP, 0};
    mtr_anim* sets[2] = {make_uniform(d, J, nullptr), make_tracks(d, J)};
    mtr_anim *looped = make_uniform(d, J, loop), *wide = make_uniform(d, J + 1, nullptr), *foreign = make_uniform(d2, J, nullptr);
    std::vector<float> weights((size_t)J, 0.5f);
    mtr_anim_masks* mk = nullptr;
    MUST(mtr_anim_masks_create(d, J, 1, weights.data(), &mk));
    mtr_ik_chain chain = mtr_ik_chain{};
    chain.kind = MTR_IK_TWO_BONE; chain.joint[0] = 0; chain.joint[1] = 1; chain.joint[2] = 2; chain.flags = MTR_IK_POLE;
    mtr_anim_ik* ik = nullptr;
    MUST(mtr_anim_ik_create(d, J, parents, 1, &chain, &ik));
    const uint32_t cyc[2] = {MTR_ROOT_CYCLIC, 0};
    mtr_anim_root* root = nullptr;
    MUST(mtr_anim_root_create(d, J, 2, 1, cyc, &root));
    const uint32_t pnk[2] = {2, 3};
    const float rates[2] = {30.0f, 24.0f};
    mtr_anim_player* pl = nullptr;
    printf("mtr_anim_player_create\n");
    hipStubTrace() = trace;
    MUST(mtr_anim_player_create(d, 2, pnk, loop, rates, N + 1, &pl));
    hipStubTrace() = nullptr;

    // ---- the records, on the host and in "device" memory ----
    std::vector<mtr_anim_state> st(N, mtr_anim_state{0, 1, 0.5f, 1.5f, 0.25f, 0});
    std::vector<mtr_anim_layer> ly1(N, mtr_anim_layer{1, 0.5f, 1.0f, 0, 0}), ly2((size_t)N * 2, mtr_anim_layer{0, 0.5f, 0.5f, 1, 0});
    std::vector<mtr_ik_target> tg(N, mtr_ik_target{});
    std::vector<mtr_root_step> steps1(N, mtr_root_step{0, 0.0f, 0.5f, 1.0f}), steps2((size_t)N * 2, mtr_root_step{1, 1.0f, 0.5f, 0.5f});
    std::vector<mtr_attach> recs(N, mtr_attach{});
    std::vector<float> locals((size_t)N * J * 16, 0.0f), out16((size_t)N * 16, 0.0f);
    std::vector<mtr_play_state> ps(N, mtr_play_state{0, 1, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0});
    std::vector<mtr_play_cmd> cmds(3, mtr_play_cmd{1, 1, 0.0f, 0.5f});
    mtr_anim_state* st_dev = dev_copy(st);
    mtr_anim_layer *ly1_dev = dev_copy(ly1), *ly2_dev = dev_copy(ly2);
    mtr_ik_target* tg_dev = dev_copy(tg);
    mtr_root_step *steps1_dev = dev_copy(steps1), *steps2_dev = dev_copy(steps2);
    mtr_attach* recs_dev = dev_copy(recs);
    float *locals_dev = dev_copy(locals), *out_dev = dev_copy(out16);
    mtr_play_state* ps_dev = dev_copy(ps);
    mtr_play_cmd* cmds_dev = dev_copy(cmds);
    mtr_anim_state* oa_dev = dev_copy(st);
    mtr_anim_layer* ol_dev = dev_copy(ly2);
    mtr_root_step* os_dev = dev_copy(steps2);

    // ---- poses and plain updates: the same version writer ----
    printf("==== poses ====\n");
    CALL(mtr_batch_update(b, mats.data(), nullptr, 0));
    CALL(mtr_batch_set_poses(b, locals.data(), J));
    CALL(mtr_batch_set_poses_device(b, locals_dev, J, nullptr));
    CALL(mtr_batch_set_poses_device(b, locals_dev, J, caller));
    CALL(mtr_batch_update(b, nullptr, locals.data(), J));

    for (int k = 0; k < 2; k++) {
        mtr_anim* a = sets[k];
        printf("==== %s set ====\n", k ? "track" : "uniform");
        CALL(mtr_model_animate(m, a, st.data()));
        CALL(mtr_batch_animate(b, a, st.data()));
        CALL(mtr_batch_animate_device(b, a, st_dev, nullptr));
        CALL(mtr_batch_animate_device(b, a, st_dev, caller));
        CALL(mtr_anim_sample(a, st.data(), N, locals.data(), locals.size()));
        CALL(mtr_model_animate_layers(m, a, nullptr, ly1.data(), 1));
        CALL(mtr_model_animate_layers(m, a, mk, ly2.data(), 2));
        CALL(mtr_batch_animate_layers(b, a, nullptr, ly1.data(), 1));
        CALL(mtr_batch_animate_layers(b, a, mk, ly2.data(), 2));
        CALL(mtr_batch_animate_layers_device(b, a, mk, ly2_dev, 2, nullptr));
        CALL(mtr_batch_animate_layers_device(b, a, mk, ly1_dev, 1, caller));
        CALL(mtr_batch_animate_layers_device(b, a, nullptr, ly2_dev, 2, caller));
        CALL(mtr_anim_sample_layers(a, nullptr, ly1.data(), 1, N, locals.data(), locals.size()));
        CALL(mtr_anim_sample_layers(a, mk, ly2.data(), 2, N, locals.data(), locals.size()));
        CALL(mtr_model_animate_ik(m, a, nullptr, ly1.data(), 1, ik, tg.data()));
        CALL(mtr_model_animate_ik(m, a, mk, ly2.data(), 2, ik, tg.data()));
        CALL(mtr_batch_animate_ik(b, a, nullptr, ly1.data(), 1, ik, tg.data()));
        CALL(mtr_batch_animate_ik(b, a, mk, ly2.data(), 2, ik, tg.data()));
        CALL(mtr_batch_animate_ik_device(b, a, mk, ly2_dev, 2, ik, tg_dev, nullptr));
        CALL(mtr_batch_animate_ik_device(b, a, nullptr, ly1_dev, 1, ik, tg_dev, caller));
        CALL(mtr_anim_sample_ik(a, nullptr, ik, ly1.data(), 1, tg.data(), N, locals.data(), locals.size()));
        CALL(mtr_anim_sample_ik(a, mk, ik, ly2.data(), 2, tg.data(), N, locals.data(), locals.size()));
        // root motion over the same set as the trajectory
        CALL(mtr_batch_root_motion(b, a, root, steps1.data(), 1));
        CALL(mtr_batch_root_motion(b, a, root, steps2.data(), 2));
        CALL(mtr_batch_root_motion_device(b, a, root, steps2_dev, 2, nullptr));
        CALL(mtr_batch_root_motion_device(b, a, root, steps1_dev, 1, caller));
        CALL(mtr_anim_root_deltas(a, root, steps1.data(), 1, N, out16.data(), out16.size()));
        CALL(mtr_anim_root_deltas(a, root, steps2.data(), 2, N, out16.data(), out16.size()));
        CALL(mtr_anim_root_deltas_device(a, root, steps2_dev, 2, N, out_dev, nullptr));
        CALL(mtr_anim_root_deltas_device(a, root, steps1_dev, 1, N, out_dev, caller));
    }

    printf("==== attachments ====\n");
    CALL(mtr_batch_attach(b, src, recs.data()));
    CALL(mtr_batch_attach_device(b, src, recs_dev, nullptr));
    CALL(mtr_batch_attach_device(b, b, recs_dev, caller));
    CALL(mtr_batch_sockets(b, recs.data(), N, out16.data(), out16.size()));
    CALL(mtr_batch_sockets_device(b, recs_dev, N, out_dev, nullptr));
    CALL(mtr_batch_sockets_device(b, recs_dev, N, out_dev, caller));
    CALL(mtr_batch_read_model_mats(b, out16.data(), out16.size()));
    CALL(mtr_batch_read_palettes(b, locals.data(), locals.size()));

    printf("==== player ====\n");
    CALL(mtr_anim_player_advance_device(pl, ps_dev, N, 0.5f, nullptr, 0, oa_dev, nullptr, 0, nullptr, nullptr));
    CALL(mtr_anim_player_advance_device(pl, ps_dev, N, 0.5f, cmds.data(), 1, oa_dev, ol_dev, 2, os_dev, nullptr));
    CALL(mtr_anim_player_advance_device(pl, ps_dev, N, 0.5f, cmds.data(), 3, nullptr, ol_dev, 2, nullptr, caller));  // outgrows the staged commands
    CALL(mtr_anim_player_advance_device(pl, ps_dev, N, 0.5f, cmds.data(), 2, nullptr, nullptr, 0, os_dev, caller));
    CALL(mtr_anim_player_advance_device_cmds(pl, ps_dev, N, 0.5f, cmds_dev, 3, oa_dev, ol_dev, 2, os_dev, nullptr));
    CALL(mtr_anim_player_advance_device_cmds(pl, ps_dev, N, 0.5f, nullptr, 0, nullptr, nullptr, 0, nullptr, caller));
    CALL(mtr_anim_player_advance_host(pl, ps.data(), N, 0.5f, nullptr, 0, nullptr, nullptr, 0, nullptr));
    CALL(mtr_anim_player_advance_host(pl, ps.data(), N, 0.5f, cmds.data(), 3, st.data(), ly2.data(), 2, steps2.data()));

    // ---- one rejected call per entry point ----
    printf("==== rejected ====\n");
    mtr_anim* none = nullptr;
    const uint32_t nk0[2] = {2, 0};
    std::vector<mtr_anim_key> keys((size_t)5 * J);
    REJECT(mtr_anim_create(d, J, 2, nk0, nullptr, keys.data(), &none));
    REJECT(mtr_anim_create_tracks(d, J, 2, nk0, nullptr, nullptr, nullptr, nullptr, 1, &none));
    mtr_anim_masks* no_mk = nullptr;
    const float heavy[J] = {0.0f, 2.0f, 1.0f};
    REJECT(mtr_anim_masks_create(d, J, 1, heavy, &no_mk));
    mtr_anim_ik* no_ik = nullptr;
    mtr_ik_chain twice = chain;
    twice.joint[2] = 1;
    REJECT(mtr_anim_ik_create(d, J, parents, 1, &twice, &no_ik));
    mtr_anim_root* no_root = nullptr;
    REJECT(mtr_anim_root_create(d, J, 2, J, nullptr, &no_root));
    mtr_anim_player* no_pl = nullptr;
    REJECT(mtr_anim_player_create(d, 2, pnk, loop, rates, 0, &no_pl));
    REJECT(mtr_batch_update(b, nullptr, locals.data(), 257));
    REJECT(mtr_batch_set_poses(b, locals.data(), J + 1));
    REJECT(mtr_batch_set_poses_device(plain, locals_dev, J, caller));
    REJECT(mtr_model_animate(bare, sets[0], st.data()));
    REJECT(mtr_batch_animate(b, wide, st.data()));
    REJECT(mtr_batch_animate_device(b, sets[1], odd(st_dev), caller));
    REJECT(mtr_anim_sample(sets[0], st.data(), N, locals.data(), locals.size() - 1));
    REJECT(mtr_model_animate_layers(m, sets[0], mk, ly2.data(), 9));
    REJECT(mtr_batch_animate_layers(b, foreign, mk, ly2.data(), 2));
    REJECT(mtr_batch_animate_layers_device(b, sets[1], mk, odd(ly2_dev), 2, nullptr));
    REJECT(mtr_anim_sample_layers(sets[1], mk, ly2.data(), 0, N, locals.data(), locals.size()));
    REJECT(mtr_model_animate_ik(m, sets[0], mk, ly2.data(), 2, nullptr, tg.data()));
    REJECT(mtr_batch_animate_ik(plain, sets[0], mk, ly2.data(), 2, ik, tg.data()));
    REJECT(mtr_batch_animate_ik_device(b, sets[1], mk, ly2_dev, 2, ik, odd(tg_dev), caller));
    REJECT(mtr_anim_sample_ik(wide, mk, ik, ly2.data(), 2, tg.data(), N, locals.data(), locals.size()));
    REJECT(mtr_batch_attach(b, nullptr, recs.data()));
    REJECT(mtr_batch_attach_device(b, src, odd(recs_dev), caller));
    REJECT(mtr_batch_sockets(b, recs.data(), N, out16.data(), out16.size() - 1));
    REJECT(mtr_batch_sockets_device(b, recs_dev, 0, out_dev, caller));
    REJECT(mtr_batch_root_motion(b, looped, root, steps1.data(), 1));
    REJECT(mtr_batch_root_motion_device(b, sets[0], root, steps2_dev, 9, caller));
    REJECT(mtr_anim_root_deltas(sets[1], nullptr, steps1.data(), 1, N, out16.data(), out16.size()));
    REJECT(mtr_anim_root_deltas_device(wide, root, steps1_dev, 1, N, out_dev, caller));
    REJECT(mtr_anim_player_advance_device(pl, ps_dev, N + 2, 0.5f, nullptr, 0, oa_dev, nullptr, 0, nullptr, caller));
    REJECT(mtr_anim_player_advance_device_cmds(pl, ps_dev, N, 0.5f, odd(cmds_dev), 1, oa_dev, nullptr, 0, nullptr, caller));
    REJECT(mtr_anim_player_advance_host(pl, ps.data(), N, 0.5f, nullptr, 0, nullptr, ly2.data(), 1, nullptr));
    REJECT(mtr_batch_read_model_mats(b, out16.data(), out16.size() - 1));
    REJECT(mtr_batch_read_palettes(b, locals.data(), 1));

    // ---- every set destroyed with a kernel queued ----
    printf("==== destroyed ====\n");
    CALL(mtr_batch_animate_ik_device(b, sets[0], mk, ly2_dev, 2, ik, tg_dev, caller));
    CALL(mtr_batch_root_motion_device(b, sets[1], root, steps1_dev, 1, caller));
    CALL(mtr_anim_player_advance_device(pl, ps_dev, N, 0.5f, cmds.data(), 1, nullptr, nullptr, 0, nullptr, caller));
    DESTROY(mtr_anim_destroy(sets[0]));
    DESTROY(mtr_anim_destroy(sets[1]));
    DESTROY(mtr_anim_masks_destroy(mk));
    DESTROY(mtr_anim_ik_destroy(ik));
    DESTROY(mtr_anim_root_destroy(root));
    DESTROY(mtr_anim_player_destroy(pl));
    DESTROY(mtr_anim_destroy(looped));  // never read: parked all the same
    mtr_anim_destroy(wide);
    mtr_anim_destroy(foreign);
    mtr_anim_destroy(nullptr);

    for (void* p : {(void*)st_dev, (void*)ly1_dev, (void*)ly2_dev, (void*)tg_dev, (void*)steps1_dev, (void*)steps2_dev, (void*)recs_dev, (void*)locals_dev,
                    (void*)out_dev, (void*)ps_dev, (void*)cmds_dev, (void*)oa_dev, (void*)ol_dev, (void*)os_dev}) free(p);
    for (mtr_batch* x : {b, src, plain}) mtr_batch_destroy(x);
    mtr_model_destroy(m);
    mtr_model_destroy(bare);
    (void)hipStreamDestroy(caller);
    mtr_device_destroy(d2);
    mtr_device_destroy(d);
    printf("anim_call_trace: ops=%ld rejected=%ld failed=%d\n", g_ops, g_rejected, g_failed);
    return g_failed ? 1 : 0;
}
