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
// Appended behind that first recording, whose lines stay as they are (its closing line with its counts included): the other
// clock sets (SPEC.md sections 21 to 23: controllers, event sets, blend sets) and the spring set (section 24), at 3
// instances; their creates and destroys traced, every optional argument present and absent, a second stream after a first
// for each set, the rejected clips of the four clock-set creates with the order their checks fire in, and a last line with
// the counts of the whole run.
#define MTR_HARNESS_OWN_CULL_INSTANCES
#define MTR_HARNESS_OWN_TRACE
#include "harness.h"

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
// a k_anim launcher's name: the stage, then the set's kind, then fold or sample, as the kernels are named
static std::string anim_name(const char* stage, bool tracks, bool fold) { return std::string(stage) + (tracks ? "_tracks" : "") + (fold ? "" : "_sample"); }
void mtr_launch_anim(const AnimParams& p, bool tracks, bool fold, uint32_t n, hipStream_t s) { launched(anim_name("anim", tracks, fold).c_str(), n, s, anim_str(p)); }
void mtr_launch_anim_layers(const AnimLayerParams& p, bool tracks, bool fold, uint32_t n, hipStream_t s) {
    launched(anim_name("anim_layers", tracks, fold).c_str(), n, s, layers_str(p));
}
void mtr_launch_anim_ik(const AnimIkParams& p, bool tracks, bool fold, uint32_t n, hipStream_t s) { launched(anim_name("anim_ik", tracks, fold).c_str(), n, s, ik_str(p)); }
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
static std::string flt(float v) { return std::to_string(v); }
// a synchronous host hook runs on the copy stream over one scratch block: where its parts lie from the block's first part
static bool host_hook(hipStream_t s);
void mtr_launch_ctrl(const CtrlParams& p, hipStream_t s) {
    std::string t = " nnodes=" + num(p.nnodes) + " nany=" + num(p.nany) + " nclips=" + num(p.nclips) + " nparams=" + num(p.nparams) + " dt=" + flt(p.dt);
    t += " clips=" + B(p.clips) + " nodes=" + off(p.nodes, p.clips) + " trans=" + off(p.trans, p.clips);
    t += " states=" + B(p.states);
    t += " play=" + B(p.play);
    t += " params=" + B(p.params);
    t += " cmds=" + B(p.cmds);
    t += " counts=" + B(p.counts);
    if (host_hook(s)) t += " block: play=" + off(p.play, p.states) + " cmds=" + off(p.cmds, p.states) + " params=" + off(p.params, p.states) + " counts=" + off(p.counts, p.states);
    launched("ctrl", p.n, s, t);
}
void mtr_launch_events(const EventParams& p, hipStream_t s) {
    std::string t = " nclips=" + num(p.nclips) + " nsteps=" + num(p.nsteps) + " capacity=" + num(p.capacity) + " min_weight=" + flt(p.min_weight);
    t += " clips=" + B(p.clips) + " ranges=" + off(p.ranges, p.clips) + " markers=" + off(p.markers, p.clips) + " sums=" + off(p.sums, p.clips);
    t += " steps=" + B(p.steps);
    t += " out=" + B(p.out);
    t += " count=" + B(p.count);
    t += " bits=" + B(p.bits);
    if (host_hook(s)) t += " block: out=" + off(p.out, p.steps) + " bits=" + off(p.bits, p.steps) + " count=" + off(p.count, p.steps);
    launched("events", p.n, s, t);
}
void mtr_launch_blend(const BlendParams& p, hipStream_t s) {
    std::string t = " nclips=" + num(p.nclips) + " nsamples=" + num(p.nsamples) + " ntris=" + num(p.ntris) + " nparams=" + num(p.nparams) +
                    " param_x=" + num(p.param_x) + " param_y=" + num(p.param_y) + " nlayers=" + num(p.nlayers) + " damp=" + flt(p.damp) + " dt=" + flt(p.dt);
    t += " clips=" + B(p.clips) + " samples=" + off(p.samples, p.clips) + " tris=" + off(p.tris, p.clips);
    t += " states=" + B(p.states);
    t += " params=" + B(p.params);
    t += " out_layers=" + B(p.out_layers);
    t += " out_steps=" + B(p.out_steps);
    t += " out_shares=" + B(p.out_shares);
    if (host_hook(s)) t += " block: out_layers=" + off(p.out_layers, p.states) + " out_steps=" + off(p.out_steps, p.states) + " params=" + off(p.params, p.states) +
                           " out_shares=" + off(p.out_shares, p.states);
    launched("blend", p.n, s, t);
}
static std::string spring_str(const AnimSpringParams& p) {
    const AnimIkParams& k = p.ik;
    std::string s = " nsprings=" + num(p.nsprings) + " nrounds=" + num(p.nrounds) + " dt=" + flt(p.dt) + " springs=" + B(p.springs) + " joint_tab=" + off(p.joint_tab, p.springs);
    s += " spring_states=" + B(p.states);
    s += " motion=" + B(p.motion);
    s += " nchains=" + num(k.nchains) + " ik_path_bytes=" + num(k.path_bytes) + " chains=" + B(k.chains);
    s += " targets=" + B(k.targets);
    const bool own = k.paths == k.layers.anim.pose.paths;  // the model's table, or the spring set's copy behind its joint table
    s += own ? std::string(" ik_paths=pose") : " ik_paths=" + off(k.paths, p.springs) + " ik_path_words=" + off(k.path_words, p.springs);
    if (!k.layers.anim.pose.imats) {  // a sample call: the local matrices lead its scratch block
        const void* base = k.layers.anim.pose.out;
        s += " block: layers=" + off(k.layers.layers, base) + " targets=" + off(k.targets, base) + " spring_states=" + off(p.states, base) + " motion=" + off(p.motion, base);
    }
    return s + layers_str(k.layers);
}
void mtr_launch_anim_spring(const AnimSpringParams& p, bool tracks, bool fold, uint32_t n, hipStream_t s) {
    launched(anim_name("anim_spring", tracks, fold).c_str(), n, s, spring_str(p));
}
void mtr_launch_cull_instances(const CullParams&, hipStream_t) {}

// ---- calls ----
static mtr_device* g_dev = nullptr;
static bool host_hook(hipStream_t s) { return s == g_dev->s_copy; }
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

// ---- the clock sets besides the player, and the spring set: 3 instances, 3 clips, a 4-joint chain with 2 springs ----
static void clock_sets(mtr_device* d, hipStream_t caller) {
    const uint32_t N = 3, J = 4;
    const uint32_t nk[3] = {2, 3, 4}, fl[3] = {MTR_CLIP_LOOP, 0, MTR_CLIP_LOOP};
    const float rates[3] = {30.0f, 24.0f, 12.0f};

    printf("==== clock sets: created ====\n");
    // a controller with parameters, transitions and an any-state transition, and one with neither parameters nor transitions
    const mtr_ctrl_node nodes[2] = {{0, 1, 1, 0}, {1, 2, 0, 0}};
    mtr_ctrl_trans trans[2];
    memset(trans, 0, sizeof trans);
    trans[0].target = 0; trans[0].flags = MTR_TR_SELF; trans[0].seconds = 0.25f; trans[0].ncond = 1; trans[0].cond[0] = {1, MTR_OP_GT, 0.5f};
    trans[1].target = 1; trans[1].flags = MTR_TR_CONSUME; trans[1].ncond = 2; trans[1].cond[0] = {0, MTR_OP_GE, 1.0f}; trans[1].cond[1] = {MTR_CTRL_TIME, MTR_OP_GT, 0.0f};
    mtr_anim_ctrl *ctl = nullptr, *ctl0 = nullptr;
    CALL(mtr_anim_ctrl_create(d, 3, nk, fl, nodes, 2, trans, 2, 1, 2, &ctl));
    const mtr_ctrl_node lone[1] = {{2, 0, 0, 0}};
    CALL(mtr_anim_ctrl_create(d, 3, nk, nullptr, lone, 1, nullptr, 0, 0, 0, &ctl0));
    // an event set: two markers on clip 0, none on clip 1, one on clip 2
    const uint32_t counts[3] = {2, 0, 1};
    const mtr_event_marker markers[3] = {{0.5f, 7}, {1.5f, 8}, {1.0f, 9}};
    mtr_anim_events* evs = nullptr;
    CALL(mtr_anim_events_create(d, 3, nk, fl, counts, markers, N, &evs));
    // a 1-D blend set of two samples and a 2-D one of one triangle
    const mtr_blend_sample line[2] = {{0, 0.0f, 0.0f, 0}, {2, 1.0f, 0.0f, 0}};
    const mtr_blend_sample plane[3] = {{0, 0.0f, 0.0f, 0}, {2, 1.0f, 0.0f, 0}, {0, 0.0f, 1.0f, 0}};
    const mtr_blend_tri tri[1] = {{{0, 1, 2}, 0}};
    mtr_anim_blend *bl1 = nullptr, *bl2 = nullptr;
    CALL(mtr_anim_blend_create(d, 3, nk, fl, rates, line, 2, nullptr, 0, 2, 1, 0, 4.0f, N, &bl1));
    CALL(mtr_anim_blend_create(d, 3, nk, fl, rates, plane, 3, tri, 1, 2, 0, 1, 4.0f, N, &bl2));
    // a spring set: the last two joints of a 4-joint chain, two rounds
    const uint8_t parents[J] = {255, 0, 1, 2};
    mtr_spring springs[2];
    memset(springs, 0, sizeof springs);
    for (uint32_t k = 0; k < 2; k++) { springs[k].joint = 2 + k; springs[k].stiffness = 1.0f; springs[k].drag = 0.5f; springs[k].tail[1] = 1.0f; }
    mtr_anim_spring* sp = nullptr;
    CALL(mtr_anim_spring_create(d, J, parents, 2, springs, &sp));

    // what the spring calls need besides: a model of that chain, a batch of 3, a clip set, masks and an IK set over it (trace off)
    const float verts[9] = {-0.5f, -0.5f, 0.5f, 0.5f, -0.5f, 0.5f, 0.0f, 0.5f, 0.5f};
    const uint16_t idx[3] = {0, 1, 2};
    mtr_primitive pr;
    memset(&pr, 0, sizeof pr);
    pr.w[0] = 3u << 16; pr.w[2] = 1 | (12u << 16) | (3u << 24); pr.w[7] = 3;
    mtr_layout lay;
    memset(&lay, 0, sizeof lay);
    lay.elements[lay.num_elements++] = mtr_element{MTR_SEM_POSITION, MTR_IEF_F32, 3, 0, 0, 0};
    mtr_model* m = nullptr;
    MUST(mtr_model_create(d, verts, sizeof verts, idx, 3, &pr, 1, &lay, nullptr, nullptr, 0, nullptr, &m));
    std::vector<float> imats((size_t)J * 16, 0.0f), mats((size_t)N * 16, 0.0f);
    for (uint32_t j = 0; j < J; j++) imats[j * 16] = imats[j * 16 + 5] = imats[j * 16 + 10] = imats[j * 16 + 15] = 1.0f;
    MUST(mtr_model_set_skeleton(m, parents, imats.data(), J));
    mtr_batch* b = nullptr;
    MUST(mtr_batch_create(d, m, N, mats.data(), nullptr, 0, nullptr, &b));
    mtr_anim* a = make_uniform(d, J, nullptr);
    std::vector<float> weights((size_t)J, 0.5f);
    mtr_anim_masks* mk = nullptr;
    MUST(mtr_anim_masks_create(d, J, 1, weights.data(), &mk));
    mtr_ik_chain chain = mtr_ik_chain{};
    chain.kind = MTR_IK_TWO_BONE; chain.joint[0] = 0; chain.joint[1] = 1; chain.joint[2] = 2;
    mtr_anim_ik* ik = nullptr;
    MUST(mtr_anim_ik_create(d, J, parents, 1, &chain, &ik));

    // ---- the records, on the host and in "device" memory ----
    std::vector<mtr_ctrl_state> cs(N, mtr_ctrl_state{0, 0.0f, MTR_CTRL_NONE, 0});
    std::vector<mtr_play_state> ps(N, mtr_play_state{0, 1, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0});
    std::vector<float> prm((size_t)N * 2, 0.75f), shares((size_t)N * 3, 0.0f), motion((size_t)N * 16, 0.0f), locals((size_t)N * J * 16, 0.0f);
    std::vector<mtr_play_cmd> cmds(N, mtr_play_cmd{0, 0, 0.0f, 0.0f});
    std::vector<uint32_t> fired(2, 0u), count(2, 0u), bits(N, 0u);
    std::vector<mtr_root_step> steps2((size_t)N * 2, mtr_root_step{0, 0.25f, 1.0f, 1.0f}), steps3((size_t)N * 3, mtr_root_step{0, 0.0f, 0.0f, 0.0f});
    std::vector<mtr_anim_event> list(4, mtr_anim_event{0, 0, 0, 0.0f});
    std::vector<mtr_blend_state> bs(N, mtr_blend_state{0.0f, 0.5f, 0.25f, 1.0f});
    std::vector<mtr_anim_layer> ly3((size_t)N * 3, mtr_anim_layer{0, 0.5f, 0.5f, 1, 0}), ly4((size_t)N * 4, mtr_anim_layer{1, 0.5f, 0.5f, 0, 0});
    std::vector<mtr_ik_target> tg(N, mtr_ik_target{});
    std::vector<mtr_spring_state> ss((size_t)N * 2, mtr_spring_state{});
    mtr_ctrl_state* cs_dev = dev_copy(cs);
    mtr_play_state* ps_dev = dev_copy(ps);
    float *prm_dev = dev_copy(prm), *shares_dev = dev_copy(shares), *motion_dev = dev_copy(motion);
    mtr_play_cmd* cmds_dev = dev_copy(cmds);
    uint32_t *fired_dev = dev_copy(fired), *count_dev = dev_copy(count), *bits_dev = dev_copy(bits);
    mtr_root_step *steps2_dev = dev_copy(steps2), *steps3_dev = dev_copy(steps3);
    mtr_anim_event* list_dev = dev_copy(list);
    mtr_blend_state* bs_dev = dev_copy(bs);
    mtr_anim_layer *ly3_dev = dev_copy(ly3), *ly4_dev = dev_copy(ly4);
    mtr_ik_target* tg_dev = dev_copy(tg);
    mtr_spring_state* ss_dev = dev_copy(ss);

    // the device variants on the device's own stream and then on the caller's: the second waits for the set's event
    printf("==== controller ====\n");
    CALL(mtr_anim_ctrl_step_device(ctl, cs_dev, ps_dev, prm_dev, N, 0.5f, cmds_dev, fired_dev, nullptr));
    CALL(mtr_anim_ctrl_step_device(ctl, cs_dev, ps_dev, prm_dev, N, 0.5f, cmds_dev, nullptr, caller));
    CALL(mtr_anim_ctrl_step_device(ctl0, cs_dev, ps_dev, nullptr, N, 0.5f, cmds_dev, nullptr, nullptr));
    CALL(mtr_anim_ctrl_step_device(ctl0, cs_dev, ps_dev, nullptr, N, 0.5f, cmds_dev, fired_dev, caller));
    CALL(mtr_anim_ctrl_step_host(ctl, cs.data(), ps.data(), prm.data(), N, 0.5f, cmds.data(), fired.data()));
    CALL(mtr_anim_ctrl_step_host(ctl, cs.data(), ps.data(), prm.data(), N, 0.5f, cmds.data(), nullptr));
    CALL(mtr_anim_ctrl_step_host(ctl0, cs.data(), ps.data(), nullptr, N, 0.5f, cmds.data(), nullptr));
    CALL(mtr_anim_ctrl_step_host(ctl0, cs.data(), ps.data(), nullptr, N, 0.5f, cmds.data(), fired.data()));  // no transitions: no counts to copy

    printf("==== events ====\n");
    CALL(mtr_anim_events_collect_device(evs, steps2_dev, 2, N, 0.0f, list_dev, 4, count_dev, bits_dev, nullptr));
    CALL(mtr_anim_events_collect_device(evs, steps2_dev, 2, N, 0.0f, nullptr, 0, count_dev, nullptr, caller));
    CALL(mtr_anim_events_collect_device(evs, steps2_dev, 2, N, 0.0f, list_dev, 0, count_dev, bits_dev, caller));  // a list and no capacity
    CALL(mtr_anim_events_collect_host(evs, steps2.data(), 2, N, 0.0f, list.data(), 4, count.data(), bits.data()));
    CALL(mtr_anim_events_collect_host(evs, steps2.data(), 2, N, 0.0f, list.data(), 4, count.data(), nullptr));
    CALL(mtr_anim_events_collect_host(evs, steps2.data(), 2, N, 0.0f, nullptr, 0, count.data(), bits.data()));
    CALL(mtr_anim_events_collect_host(evs, steps2.data(), 1, N, 0.0f, nullptr, 0, count.data(), nullptr));

    printf("==== blend ====\n");
    CALL(mtr_anim_blend_advance_device(bl1, bs_dev, prm_dev, N, 0.5f, ly4_dev, 4, steps3_dev, shares_dev, nullptr));
    CALL(mtr_anim_blend_advance_device(bl1, bs_dev, prm_dev, N, 0.5f, nullptr, 0, nullptr, nullptr, caller));
    CALL(mtr_anim_blend_advance_device(bl2, bs_dev, prm_dev, N, 0.5f, ly4_dev, 4, nullptr, shares_dev, nullptr));
    CALL(mtr_anim_blend_advance_device(bl2, bs_dev, prm_dev, N, 0.5f, nullptr, 0, steps3_dev, nullptr, caller));
    CALL(mtr_anim_blend_advance_host(bl1, bs.data(), prm.data(), N, 0.5f, ly4.data(), 4, steps3.data(), shares.data()));
    CALL(mtr_anim_blend_advance_host(bl1, bs.data(), prm.data(), N, 0.5f, nullptr, 0, nullptr, nullptr));
    CALL(mtr_anim_blend_advance_host(bl2, bs.data(), prm.data(), N, 0.5f, ly4.data(), 4, nullptr, nullptr));
    CALL(mtr_anim_blend_advance_host(bl2, bs.data(), prm.data(), N, 0.5f, nullptr, 0, steps3.data(), nullptr));
    CALL(mtr_anim_blend_advance_host(bl2, bs.data(), prm.data(), N, 0.5f, nullptr, 0, nullptr, shares.data()));

    printf("==== spring ====\n");
    CALL(mtr_batch_animate_spring_device(b, a, mk, ly3_dev, 3, ik, tg_dev, sp, ss_dev, motion_dev, 0.5f, nullptr));
    CALL(mtr_batch_animate_spring_device(b, a, nullptr, ly3_dev, 3, nullptr, nullptr, sp, ss_dev, nullptr, 0.5f, caller));
    CALL(mtr_anim_sample_spring(a, mk, ik, sp, ly3.data(), 3, tg.data(), ss.data(), motion.data(), 0.5f, N, locals.data(), locals.size()));
    CALL(mtr_anim_sample_spring(a, nullptr, nullptr, sp, ly3.data(), 3, nullptr, ss.data(), nullptr, 0.5f, N, locals.data(), locals.size()));
    CALL(mtr_anim_sample_spring(a, mk, ik, sp, ly3.data(), 3, tg.data(), ss.data(), nullptr, 0.5f, N, locals.data(), locals.size()));
    CALL(mtr_anim_sample_spring(a, nullptr, nullptr, sp, ly3.data(), 3, nullptr, ss.data(), motion.data(), 0.5f, N, locals.data(), locals.size()));

    // ---- the clip checks of the four creates: each message, and the order the checks fire in ----
    printf("==== clock sets: rejected ====\n");
    mtr_anim_player* no_pl = nullptr;
    mtr_anim_ctrl* no_ctl = nullptr;
    mtr_anim_events* no_ev = nullptr;
    mtr_anim_blend* no_bl = nullptr;
    const uint32_t nk_none[3] = {2, 0, 4}, nk_many[3] = {2, 3, (1u << 24) + 1u}, fl_bad[3] = {MTR_CLIP_LOOP, 2, MTR_CLIP_LOOP};
    const float rates_nan[3] = {30.0f, 24.0f, NAN}, rates_inf[3] = {INFINITY, 24.0f, 12.0f};
    REJECT(mtr_anim_player_create(d, 3, nk_none, fl, rates, N, &no_pl));
    REJECT(mtr_anim_player_create(d, 3, nk_many, fl, rates, N, &no_pl));
    REJECT(mtr_anim_player_create(d, 3, nk, fl_bad, rates, N, &no_pl));
    REJECT(mtr_anim_player_create(d, 3, nk, fl, rates_nan, N, &no_pl));
    REJECT(mtr_anim_player_create(d, 3, nk, nullptr, rates_inf, N, &no_pl));
    REJECT(mtr_anim_ctrl_create(d, 3, nk_none, fl, nodes, 2, trans, 2, 1, 2, &no_ctl));
    REJECT(mtr_anim_ctrl_create(d, 3, nk_many, fl, nodes, 2, trans, 2, 1, 2, &no_ctl));
    REJECT(mtr_anim_ctrl_create(d, 3, nk, fl_bad, nodes, 2, trans, 2, 1, 2, &no_ctl));
    REJECT(mtr_anim_events_create(d, 3, nk_none, fl, counts, markers, N, &no_ev));
    REJECT(mtr_anim_events_create(d, 3, nk_many, fl, counts, markers, N, &no_ev));
    REJECT(mtr_anim_events_create(d, 3, nk, fl_bad, counts, markers, N, &no_ev));
    REJECT(mtr_anim_blend_create(d, 3, nk_none, fl, rates, line, 2, nullptr, 0, 2, 1, 0, 4.0f, N, &no_bl));
    REJECT(mtr_anim_blend_create(d, 3, nk_many, fl, rates, line, 2, nullptr, 0, 2, 1, 0, 4.0f, N, &no_bl));
    REJECT(mtr_anim_blend_create(d, 3, nk, fl_bad, rates, line, 2, nullptr, 0, 2, 1, 0, 4.0f, N, &no_bl));
    REJECT(mtr_anim_blend_create(d, 3, nk, fl, rates_nan, line, 2, nullptr, 0, 2, 1, 0, 4.0f, N, &no_bl));
    REJECT(mtr_anim_blend_create(d, 3, nk, fl, rates_inf, plane, 3, tri, 1, 2, 0, 1, 4.0f, N, &no_bl));
    // a clip's markers are checked before the next clip's flags: the marker of clip 0 is reported, not the flags of clip 1
    const mtr_event_marker markers_out[3] = {{0.5f, 7}, {2.0f, 8}, {1.0f, 9}};
    REJECT(mtr_anim_events_create(d, 3, nk, fl_bad, counts, markers_out, N, &no_ev));
    // two bad clips: the lower index is reported, whichever of its checks comes first in a clip (clip 0: flags, a later
    // check; clip 1: no keys, the first; a not-finite rate of clip 0 against the flags of clip 1 likewise)
    const uint32_t fl_bad0[3] = {4, 0, MTR_CLIP_LOOP}, fl_bad1[3] = {MTR_CLIP_LOOP, 2, MTR_CLIP_LOOP};
    REJECT(mtr_anim_player_create(d, 3, nk_none, fl_bad0, rates, N, &no_pl));
    REJECT(mtr_anim_player_create(d, 3, nk, fl_bad1, rates_inf, N, &no_pl));
    REJECT(mtr_anim_ctrl_create(d, 3, nk_none, fl_bad0, nodes, 2, trans, 2, 1, 2, &no_ctl));
    REJECT(mtr_anim_events_create(d, 3, nk_none, fl_bad0, counts, markers, N, &no_ev));
    REJECT(mtr_anim_blend_create(d, 3, nk_none, fl_bad0, rates, line, 2, nullptr, 0, 2, 1, 0, 4.0f, N, &no_bl));
    REJECT(mtr_anim_blend_create(d, 3, nk, fl_bad1, rates_inf, line, 2, nullptr, 0, 2, 1, 0, 4.0f, N, &no_bl));
    // the table-wide checks stand before the clips'
    REJECT(mtr_anim_player_create(d, 0, nk, fl, rates, N, &no_pl));
    REJECT(mtr_anim_ctrl_create(d, ((size_t)1 << 24) + 1, nk, fl, nodes, 2, trans, 2, 1, 2, &no_ctl));
    REJECT(mtr_anim_events_create(d, 0, nk, fl, counts, markers, N, &no_ev));
    REJECT(mtr_anim_blend_create(d, 0, nk, fl, rates, line, 2, nullptr, 0, 2, 1, 0, 4.0f, N, &no_bl));
    // one rejected call per entry point
    REJECT(mtr_anim_ctrl_step_device(ctl, odd(cs_dev), ps_dev, prm_dev, N, 0.5f, cmds_dev, fired_dev, caller));
    REJECT(mtr_anim_ctrl_step_host(ctl, cs.data(), ps.data(), nullptr, N, 0.5f, cmds.data(), nullptr));
    REJECT(mtr_anim_events_collect_device(evs, odd(steps2_dev), 2, N, 0.0f, list_dev, 4, count_dev, bits_dev, caller));
    REJECT(mtr_anim_events_collect_host(evs, steps2.data(), 2, N, 0.0f, nullptr, 4, count.data(), nullptr));
    REJECT(mtr_anim_blend_advance_device(bl1, bs_dev, prm_dev, N + 1, 0.5f, nullptr, 0, nullptr, nullptr, caller));
    REJECT(mtr_anim_blend_advance_host(bl2, bs.data(), prm.data(), N, 0.5f, ly4.data(), 2, nullptr, nullptr));
    REJECT(mtr_batch_animate_spring_device(b, a, mk, ly3_dev, 3, ik, tg_dev, sp, odd(ss_dev), nullptr, 0.5f, caller));
    REJECT(mtr_anim_sample_spring(a, mk, nullptr, sp, ly3.data(), 3, tg.data(), ss.data(), nullptr, 0.5f, N, locals.data(), locals.size()));
    mtr_anim_spring* no_sp = nullptr;
    REJECT(mtr_anim_spring_create(d, J, parents, 0, springs, &no_sp));

    // ---- each set destroyed with a kernel queued on the caller's stream ----
    printf("==== clock sets: destroyed ====\n");
    CALL(mtr_anim_ctrl_step_device(ctl, cs_dev, ps_dev, prm_dev, N, 0.5f, cmds_dev, nullptr, caller));
    CALL(mtr_anim_events_collect_device(evs, steps2_dev, 2, N, 0.0f, list_dev, 4, count_dev, nullptr, caller));
    CALL(mtr_anim_blend_advance_device(bl2, bs_dev, prm_dev, N, 0.5f, nullptr, 0, nullptr, nullptr, caller));
    CALL(mtr_batch_animate_spring_device(b, a, nullptr, ly3_dev, 3, nullptr, nullptr, sp, ss_dev, nullptr, 0.5f, caller));
    DESTROY(mtr_anim_ctrl_destroy(ctl));
    DESTROY(mtr_anim_ctrl_destroy(ctl0));
    DESTROY(mtr_anim_events_destroy(evs));
    DESTROY(mtr_anim_blend_destroy(bl1));
    DESTROY(mtr_anim_blend_destroy(bl2));
    DESTROY(mtr_anim_spring_destroy(sp));
    mtr_anim_ctrl_destroy(nullptr);
    mtr_anim_events_destroy(nullptr);
    mtr_anim_blend_destroy(nullptr);
    mtr_anim_spring_destroy(nullptr);

    for (void* p : {(void*)cs_dev, (void*)ps_dev, (void*)prm_dev, (void*)shares_dev, (void*)motion_dev, (void*)cmds_dev, (void*)fired_dev, (void*)count_dev,
                    (void*)bits_dev, (void*)steps2_dev, (void*)steps3_dev, (void*)list_dev, (void*)bs_dev, (void*)ly3_dev, (void*)ly4_dev, (void*)tg_dev,
                    (void*)ss_dev}) free(p);
    mtr_anim_destroy(a);
    mtr_anim_masks_destroy(mk);
    mtr_anim_ik_destroy(ik);
    mtr_batch_destroy(b);
    mtr_model_destroy(m);
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
    printf("anim_call_trace: ops=%ld rejected=%ld failed=%d\n", g_ops, g_rejected, g_failed);  // where the first recording ended
    clock_sets(d, caller);

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
