// host_anim.cpp -- the animation sets (clip and track sets, mask sets, IK sets, root sets) and the one path every animate
// call takes to k_anim: what it checks, and how its kernel is queued between the sets' events.  Also what needs no batch:
// the model's animate calls, the sample calls and the root deltas.  Batches call in from host_batch.cpp, players from
// host_player.cpp.
#include "host.h"

// k_anim.hip.  Weak: the host-only builds of this file (tests/cpp, over the HIP stub runtime) link no kernels and define
// the launchers they watch; libmtr.so links k_anim.o.
void mtr_launch_anim(const AnimParams& p, bool tracks, bool fold, uint32_t ninst, hipStream_t s) __attribute__((weak));
void mtr_launch_anim_layers(const AnimLayerParams& p, bool tracks, bool fold, uint32_t ninst, hipStream_t s) __attribute__((weak));
void mtr_launch_anim_ik(const AnimIkParams& p, bool tracks, bool fold, uint32_t ninst, hipStream_t s) __attribute__((weak));
void mtr_launch_anim_spring(const AnimSpringParams& p, bool tracks, bool fold, uint32_t ninst, hipStream_t s) __attribute__((weak));
// k_root.hip, weak for the same reason
void mtr_launch_root(const RootParams& p, hipStream_t s) __attribute__((weak));
void mtr_launch_root_deltas(const RootParams& p, hipStream_t s) __attribute__((weak));

namespace mtr_host {

// ---------------------------------------------------------------------------------------------
// what every set shares
// ---------------------------------------------------------------------------------------------
int32_t set_upload(DeviceSet* s, const char* what, std::initializer_list<Part> parts) {
    mtr_device* d = s->dev;
    size_t bytes = 0;
    for (const Part& p : parts) bytes += p.bytes;
    int32_t rc = dev_alloc(d, &s->d, (bytes + 3) / 4);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    char* at = reinterpret_cast<char*>(s->d);
    for (const Part& p : parts) {
        if (e != hipSuccess) break;
        if (p.p) e = hipMemcpy(at, p.p, p.bytes, hipMemcpyHostToDevice);
        else if ((e = hipMemsetAsync(at, 0, p.bytes, d->s_copy)) == hipSuccess) e = hipStreamSynchronize(d->s_copy);
        at += p.bytes;
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&s->last, hipEventDisableTiming);
    if (e == hipSuccess) return MTR_OK;
    (void)hipFree(s->d);
    s->d = nullptr;
    return fail(d, MTR_E_HIP, std::string(what) + " upload: " + hipGetErrorString(e));
}

int32_t clip_entry(mtr_device* d, const char* who, size_t c, const uint32_t* nkeys, uint32_t flags, const float* rates, uint32_t* out) {
    auto bad = [&](const char* what) { return fail(d, MTR_E_INVALID, std::string(who) + ": clip " + std::to_string(c) + " " + what); };
    if (nkeys[c] == 0 || nkeys[c] > kClipMaxKeys) return bad("has no keys or more than 2^24");
    if (flags & ~MTR_CLIP_LOOP) return bad("has unknown flag bits");
    if (rates && !std::isfinite(rates[c])) return bad("has a rate that is not finite");
    const float period = (flags & MTR_CLIP_LOOP) ? (float)nkeys[c] : (float)(nkeys[c] - 1u);  // exact: at most 2^24
    std::memcpy(&out[0], &period, 4);
    out[1] = flags;
    out[2] = 0u;
    if (rates) std::memcpy(&out[2], &rates[c], 4);
    out[3] = nkeys[c];
    return MTR_OK;
}

int32_t set_before(DeviceSet* s, hipStream_t st) {
    if (s->recorded && s->last_stream != st) HIPCHK(s->dev, hipStreamWaitEvent(st, s->last, 0));
    return MTR_OK;
}

int32_t set_after(DeviceSet* s, hipStream_t st) {
    HIPCHK(s->dev, hipEventRecord(s->last, st));
    s->last_stream = st; s->recorded = true;
    return MTR_OK;
}

void set_park(DeviceSet* s) {
    std::lock_guard<std::mutex> submit_lock(s->dev->submit_mu);
    s->dev->garbage.push_back({s->d, 0, s->last});
}

namespace {

// ---------------------------------------------------------------------------------------------
// the device image of a clip set: the one place that knows it
// ---------------------------------------------------------------------------------------------
constexpr size_t kClipWords = 4;  // a clip table entry

// Words of each part, in device order: the clip table, then the keys (a uniform set), or the descriptors (8 words, a
// joint's three together), the values (2 words a key) and the u16 times (a track set).
struct ClipImage {
    size_t table, tracks, values;
    ClipImage(size_t nclips, size_t njoints, size_t nkeys, bool is_tracks)
        : table(nclips * kClipWords), tracks(is_tracks ? nclips * njoints * 3 * 8 : 0), values(is_tracks ? nkeys * 2 : 0) {}
};

// where a kernel reads the set: the source fields of AnimParams
void anim_source(const mtr_anim* a, AnimParams& ap) {
    const ClipImage im(a->nclips, a->njoints, a->nkeys, a->tracks);
    ap.clips = a->d;
    ap.nclips = a->nclips;
    if (a->tracks) {
        ap.tracks = a->d + im.table;
        ap.values = ap.tracks + im.tracks;
        ap.times = reinterpret_cast<const uint16_t*>(ap.values + im.values);
    } else {
        ap.keys = reinterpret_cast<const float*>(a->d + im.table);
    }
}

// ---------------------------------------------------------------------------------------------
// one animate call
// ---------------------------------------------------------------------------------------------
const char* const kAnimWhat[2][4] = {{"animate", "animate layers", "animate ik", "animate spring"},
                                     {"anim sample", "anim sample layers", "anim sample ik", "anim sample spring"}};
const char* const kAnimKernel[4] = {"k_anim", "k_anim_layers", "k_anim_ik", "k_anim_spring"};

}  // namespace

// A layered call makes the checks of a plain one too, an IK call those of a layered one, a spring call those of an IK call
// where it has an IK set and those of a layered one where it has none: `stage` names the kind a message speaks for.  A
// sample call speaks under its own name throughout.
int32_t anim_check(mtr_device* d, const mtr_model* m, const AnimCall& c, const char* no_room) {
    const bool sample = !m;
    const mtr_anim* a = c.anim;
    const mtr_anim_masks* mk = c.masks;
    const mtr_anim_ik* ik = c.ik;
    const mtr_anim_spring* sp = c.spring;
    const bool springs = c.kind == AnimCall::kSpring;
    auto what = [&](int stage) { return std::string(kAnimWhat[sample][sample ? c.kind : stage]) + ": "; };
    auto bad = [&](int stage, const std::string& msg) { return fail(d, MTR_E_INVALID, what(stage) + msg); };
    auto built = [&](int stage) {
        const bool linked[4] = {mtr_launch_anim != nullptr, mtr_launch_anim_layers != nullptr, mtr_launch_anim_ik != nullptr, mtr_launch_anim_spring != nullptr};
        if (linked[stage]) return (int32_t)MTR_OK;
        return fail(d, MTR_E_UNSUPPORTED, what(stage) + "built without " + kAnimKernel[stage]);
    };
    if (c.kind != AnimCall::kStates) {
        if (c.nlayers < 1 || c.nlayers > MTR_ANIM_MAX_LAYERS) return bad(AnimCall::kLayers, "1 to 8 layers per instance");
        if (sample) {
            if (mk && (mk->dev != d || mk->njoints != a->njoints)) return bad(c.kind, "the mask set is of another device or joint count");
        } else {
            if (mk && mk->dev != d) return bad(AnimCall::kLayers, "the mask set belongs to another device");
            if (mk && mk->njoints != m->skel.njoints) return bad(AnimCall::kLayers, "the mask set's joint count is not the skeleton's");
        }
    }
    int32_t rc;
    if (sample) {
        if ((c.kind == AnimCall::kIk || (springs && ik)) && (!ik || ik->dev != d || ik->njoints != a->njoints))
            return bad(c.kind, "an IK set of this device and joint count");
        if (springs && (!sp || sp->dev != d || sp->njoints != a->njoints)) return bad(c.kind, "a spring set of this device and joint count");
        // the chains walk the spring set's copy of the paths here
        if (springs && ik && ik->parents != sp->parents) return bad(c.kind, "the IK set's parents are not the spring set's");
        if (no_room) return bad(c.kind, no_room);
        return (rc = built(c.kind)) ? rc : set_device(d);
    }
    if (!a) return bad(AnimCall::kStates, "no animation set");
    if (a->dev != d) return bad(AnimCall::kStates, "the animation set belongs to another device");
    if (!m->skel.d) return bad(AnimCall::kStates, "the model has no skeleton");
    if (a->njoints != m->skel.njoints) return bad(AnimCall::kStates, "the animation set's joint count is not the skeleton's");
    if ((rc = built(AnimCall::kStates)) || (rc = set_device(d))) return rc;
    if (c.kind == AnimCall::kStates) return MTR_OK;
    if ((rc = built(AnimCall::kLayers)) || c.kind == AnimCall::kLayers) return rc;
    if (ik || !springs) {
        if (!ik) return bad(AnimCall::kIk, "no IK set");
        if (ik->dev != d) return bad(AnimCall::kIk, "the IK set belongs to another device");
        if (ik->njoints != m->skel.njoints) return bad(AnimCall::kIk, "the IK set's joint count is not the skeleton's");
        for (uint32_t j = 0; j < ik->njoints; j++)
            if (ik->parents[j] != m->skel.parents[j]) return bad(AnimCall::kIk, "the IK set's parent of joint " + std::to_string(j) + " is not the skeleton's");
        if ((rc = built(AnimCall::kIk)) || !springs) return rc;
    }
    if (!sp) return bad(AnimCall::kSpring, "no spring set");
    if (sp->dev != d) return bad(AnimCall::kSpring, "the spring set belongs to another device");
    if (sp->njoints != m->skel.njoints) return bad(AnimCall::kSpring, "the spring set's joint count is not the skeleton's");
    for (uint32_t j = 0; j < sp->njoints; j++)
        if (sp->parents[j] != m->skel.parents[j])
            return bad(AnimCall::kSpring, "the spring set's parent of joint " + std::to_string(j) + " is not the skeleton's");
    return built(AnimCall::kSpring);
}

int32_t anim_enqueue(const AnimCall& c, const mtr_model::Skeleton* sk, float* out, uint32_t ninst, hipStream_t s) {
    mtr_anim* a = c.anim;
    mtr_device* d = a->dev;
    DeviceSet* const sets[4] = {a, c.masks, c.ik, c.spring};
    int32_t rc;
    for (DeviceSet* x : sets)
        if (sk && x && (rc = set_before(x, s))) return rc;
    // the parameters of the four kinds nest: each kernel is handed the part it knows
    AnimSpringParams sp{};
    AnimIkParams& ip = sp.ik;
    AnimLayerParams& lp = ip.layers;
    AnimParams& ap = lp.anim;
    if (sk) ap.pose = pose_params(*sk, nullptr, out);
    else { ap.pose.out = out; ap.pose.njoints = a->njoints; }
    anim_source(a, ap);
    const bool tracks = a->tracks, fold = sk != nullptr;
    if (c.kind == AnimCall::kStates) {
        ap.states = static_cast<const uint32_t*>(c.recs);
        mtr_launch_anim(ap, tracks, fold, ninst, s);
    } else {
        lp.layers = static_cast<const uint32_t*>(c.recs);
        lp.nlayers = (uint32_t)c.nlayers;
        if (c.masks) { lp.masks = c.masks->weights(); lp.nmasks = c.masks->nmasks; }
        if (c.kind == AnimCall::kLayers) {
            mtr_launch_anim_layers(lp, tracks, fold, ninst, s);
        } else {
            // the chain walks read the skeleton's path table as the fold does; a sample call has none and reads the IK set's
            // copy, or the spring set's
            const mtr_anim_ik* ik = c.ik;
            const mtr_anim_spring* ss = c.kind == AnimCall::kSpring ? c.spring : nullptr;
            if (ik) {
                ip.chains = ik->d;
                ip.targets = static_cast<const uint32_t*>(c.targets);
                ip.nchains = ik->nchains;
            }
            if (sk) { ip.paths = ap.pose.paths; ip.path_words = ap.pose.path_words; ip.path_bytes = sk->path_bytes; }
            else if (ss) { ip.paths = ss->d + (size_t)ss->nsprings * 12 + ss->njoints; ip.path_words = ip.paths + ss->njoints; ip.path_bytes = ss->path_bytes; }
            else { ip.paths = ik->d + (size_t)ik->nchains * 8; ip.path_words = ip.paths + ik->njoints; ip.path_bytes = ik->path_bytes; }
            if (ss) {
                sp.springs = ss->d;
                sp.joint_tab = ss->d + (size_t)ss->nsprings * 12;
                sp.states = static_cast<uint32_t*>(c.spring_states);
                sp.motion = c.motion;
                sp.dt = c.dt;
                sp.nsprings = ss->nsprings; sp.nrounds = ss->nrounds;
                mtr_launch_anim_spring(sp, tracks, fold, ninst, s);
            } else {
                mtr_launch_anim_ik(ip, tracks, fold, ninst, s);
            }
        }
    }
    HIPCHK(d, hipGetLastError());
    for (DeviceSet* x : sets)
        if (sk && x && (rc = set_after(x, s))) return rc;
    return MTR_OK;
}

// ---------------------------------------------------------------------------------------------
// root motion: the kernel over a trajectory set and a root set
// ---------------------------------------------------------------------------------------------
int32_t root_check(mtr_device* d, const mtr_anim* traj, const mtr_anim_root* root, size_t nsteps, bool deltas) {
    if (!root) return fail(d, MTR_E_INVALID, "root motion: no root set");
    if (traj->dev != d || root->dev != d) return fail(d, MTR_E_INVALID, "root motion: the trajectory set or the root set belongs to another device");
    if (root->njoints != traj->njoints || root->nclips != traj->nclips)
        return fail(d, MTR_E_INVALID, "root motion: the root set's joint or clip count is not the trajectory set's");
    if (traj->has_loop) return fail(d, MTR_E_INVALID, "root motion: the trajectory set has a MTR_CLIP_LOOP clip (mark it MTR_ROOT_CYCLIC in the root set instead)");
    if (nsteps < 1 || nsteps > MTR_ROOT_MAX_STEPS) return fail(d, MTR_E_INVALID, "root motion: 1 to 8 steps per instance");
    if (!(deltas ? mtr_launch_root_deltas : mtr_launch_root)) return fail(d, MTR_E_UNSUPPORTED, "root motion: built without k_root");
    return set_device(d);
}

int32_t root_enqueue(mtr_anim* traj, mtr_anim_root* root, const void* steps_dev, size_t nsteps, size_t n, const float* mats_in, float* out, hipStream_t s) {
    mtr_device* d = traj->dev;
    int32_t rc;
    if ((rc = set_before(traj, s)) || (rc = set_before(root, s))) return rc;
    RootParams rp{};
    anim_source(traj, rp.anim);
    rp.anim.pose.njoints = traj->njoints;
    rp.root_flags = root->d;
    rp.steps = static_cast<const uint32_t*>(steps_dev);
    rp.mats_in = mats_in; rp.out = out;
    rp.joint = root->joint; rp.nsteps = (uint32_t)nsteps; rp.n = (uint32_t)n;
    (mats_in ? mtr_launch_root : mtr_launch_root_deltas)(rp, s);
    HIPCHK(d, hipGetLastError());
    if ((rc = set_after(traj, s)) || (rc = set_after(root, s))) return rc;
    return MTR_OK;
}

namespace {

// the model's palette from one call of one instance, its records staged: the next buffer of the palette ring, on the copy stream
int32_t model_animate(mtr_model* m, const AnimCall& c) {
    mtr_device* d = m->dev;
    std::lock_guard<std::mutex> submit_lock(d->submit_mu);
    mtr_model::PalBuf* pb = nullptr;
    int32_t rc = next_palette_buffer(m, c.anim->njoints, &pb);
    if (rc || (rc = anim_enqueue(c, &m->skel, pb->d, 1, d->s_copy))) return rc;
    HIPCHK(d, hipEventRecord(pb->ready, d->s_copy));
    return MTR_OK;
}

// The local matrices of n instances to host memory: the records (and the targets) of c lie in host memory here and go
// through scratch behind the matrices, each part a multiple of 16 bytes.
int32_t anim_sample(AnimCall c, size_t rec_words, size_t target_words, size_t n, float* out_locals, const char* no_room) {
    mtr_device* d = c.anim->dev;
    int32_t rc = anim_check(d, nullptr, c, no_room);
    if (rc || !n) return rc;
    StagedBlock blk(d);
    StagedPart &p_locals = blk.part(out_locals, n * c.anim->njoints * 16), &p_recs = blk.part(c.recs, n * rec_words), &p_targets = blk.part(c.targets, n * target_words);
    return blk.run([&]() -> int32_t {
        int32_t r2 = blk.up({&p_recs, &p_targets});
        if (r2) return r2;
        c.recs = p_recs.at; c.targets = p_targets.dev<void>();
        if ((r2 = anim_enqueue(c, nullptr, p_locals.dev<float>(), (uint32_t)n, d->s_copy))) return r2;
        return blk.down({&p_locals});
    });
}

// n instances and room for their local matrices?
bool sample_room(const mtr_anim* a, size_t n, bool records, const float* out_locals, size_t count) {
    return n <= 0xFFFFFFu && (!n || (records && out_locals)) && count >= n * a->njoints * 16;
}

}  // namespace

}  // namespace mtr_host

using namespace mtr_host;

extern "C" {

// ---------------------------------------------------------------------------------------------
// animation clips (SPEC.md section 14)
// ---------------------------------------------------------------------------------------------
int32_t mtr_anim_create(mtr_device* d, size_t njoints, size_t nclips, const uint32_t* nkeys, const uint32_t* flags,
                        const mtr_anim_key* keys, mtr_anim** out) {
    if (!d || !out) return MTR_E_INVALID;
    *out = nullptr;
    if (njoints == 0 || njoints > MTR_POSE_MAX_JOINTS) return fail(d, MTR_E_INVALID, "anim: 1 to 256 joints");
    if (nclips == 0 || nclips > 0xFFFFFFu || !nkeys || !keys) return fail(d, MTR_E_INVALID, "anim: at least one clip, its key counts and keys");
    const ClipImage im(nclips, njoints, 0, false);
    std::vector<uint32_t> table(im.table);
    uint64_t total = 0;
    auto a = std::make_unique<mtr_anim>();
    for (size_t c = 0; c < nclips; c++) {
        // key counts are exact in binary32 (the position arithmetic of section 14)
        if (nkeys[c] == 0 || nkeys[c] > (1u << 24)) return fail(d, MTR_E_INVALID, "anim: a clip has 1 to 16 777 216 keys");
        uint32_t* t = &table[c * kClipWords];
        t[0] = (uint32_t)total;
        t[1] = nkeys[c];
        t[2] = flags ? flags[c] : 0u;
        a->has_loop |= (t[2] & MTR_CLIP_LOOP) != 0;
        total += nkeys[c];
        if (total * njoints > 0x3FFFFFFu) return fail(d, MTR_E_INVALID, "anim: more than 2^26 joint keys");
    }
    int32_t rc = set_device(d);
    if (rc) return rc;
    a->dev = d; a->njoints = (uint32_t)njoints; a->nclips = (uint32_t)nclips;
    if ((rc = set_upload(a.get(), "anim", {{table.data(), im.table * 4}, {keys, (size_t)total * njoints * sizeof(mtr_anim_key)}}))) return rc;
    *out = a.release();
    return MTR_OK;
}

// ---------------------------------------------------------------------------------------------
// animation tracks (SPEC.md section 15): the same mtr_anim, its channel values from tracks
// ---------------------------------------------------------------------------------------------
int32_t mtr_anim_create_tracks(mtr_device* d, size_t njoints, size_t nclips, const uint32_t* nticks, const uint32_t* flags,
                               const mtr_anim_track* tracks, const uint16_t* times, const uint16_t* values, size_t nkeys_total,
                               mtr_anim** out) {
    if (!d || !out) return MTR_E_INVALID;
    *out = nullptr;
    if (njoints == 0 || njoints > MTR_POSE_MAX_JOINTS) return fail(d, MTR_E_INVALID, "anim tracks: 1 to 256 joints");
    if (nclips == 0 || nclips > 0xFFFFFFu || !nticks || !tracks || !times || !values)
        return fail(d, MTR_E_INVALID, "anim tracks: at least one clip, its lengths, track descriptors, key times and key values");
    // first + count of a valid track is at most the key total: 32-bit arithmetic on the device cannot wrap
    if (nkeys_total == 0 || nkeys_total > 0x7FFFFFFFu) return fail(d, MTR_E_INVALID, "anim tracks: 1 to 2^31 - 1 keys");
    static const char* const channel[3] = {"translation", "rotation", "scale"};
    for (size_t c = 0; c < nclips; c++) {
        if (nticks[c] == 0 || nticks[c] > 65536u)
            return fail(d, MTR_E_INVALID, "anim tracks: clip " + std::to_string(c) + " has 1 to 65536 ticks");
        for (size_t j = 0; j < njoints; j++)
            for (size_t ch = 0; ch < 3; ch++) {
                const mtr_anim_track& t = tracks[(c * njoints + j) * 3 + ch];
                const char* what = nullptr;
                if (t.count == 0) what = "has no key";
                else if (t.count > nkeys_total || t.first > nkeys_total - t.count) what = "reaches past the key arrays";
                else if (times[t.first] != 0) what = "does not start at tick 0";
                else if (times[(size_t)t.first + t.count - 1] > nticks[c] - 1u) what = "has a key past the clip's last tick";
                else
                    for (size_t k = (size_t)t.first + 1; k < (size_t)t.first + t.count && !what; k++)
                        if (times[k] <= times[k - 1]) what = "has key times that do not increase";
                if (what)
                    return fail(d, MTR_E_INVALID, "anim tracks: clip " + std::to_string(c) + ", joint " + std::to_string(j) + ", channel " +
                                                      std::to_string(ch) + " (" + channel[ch] + ") " + what);
            }
    }
    int32_t rc = set_device(d);
    if (rc) return rc;
    static_assert(sizeof(mtr_anim_track) == 32, "mtr_anim_track");
    const ClipImage im(nclips, njoints, nkeys_total, true);
    std::vector<uint32_t> table(im.table, 0u);  // per clip: 0, ticks, flags, 0
    auto a = std::make_unique<mtr_anim>();
    a->dev = d; a->njoints = (uint32_t)njoints; a->nclips = (uint32_t)nclips;
    a->tracks = true; a->nkeys = (uint32_t)nkeys_total;
    for (size_t c = 0; c < nclips; c++) {
        uint32_t* t = &table[c * kClipWords];
        t[1] = nticks[c];
        t[2] = flags ? flags[c] : 0u;
        a->has_loop |= (t[2] & MTR_CLIP_LOOP) != 0;
    }
    if ((rc = set_upload(a.get(), "anim", {{table.data(), im.table * 4}, {tracks, im.tracks * 4}, {values, im.values * 4}, {times, nkeys_total * sizeof(uint16_t)}})))
        return rc;
    *out = a.release();
    return MTR_OK;
}

void mtr_anim_destroy(mtr_anim* a) { set_destroy(a); }

int32_t mtr_model_animate(mtr_model* m, mtr_anim* a, const mtr_anim_state* state) {
    if (!m) return MTR_E_INVALID;
    mtr_device* d = m->dev;
    if (!state) return fail(d, MTR_E_INVALID, "animate: no state");
    AnimCall c;
    c.anim = a;
    int32_t rc = anim_check(d, m, c);
    if (rc) return rc;
    if ((rc = stage_pose(d, reinterpret_cast<const float*>(state), sizeof(mtr_anim_state) / sizeof(float)))) return rc;
    c.recs = d->pose_stage;
    return model_animate(m, c);
}

int32_t mtr_anim_sample(mtr_anim* a, const mtr_anim_state* states, size_t n, float* out_locals, size_t count) {
    if (!a) return MTR_E_INVALID;
    AnimCall c;
    c.anim = a; c.recs = states;
    return anim_sample(c, sizeof(mtr_anim_state) / sizeof(float), 0, n, out_locals,
                       sample_room(a, n, states, out_locals, count) ? nullptr : "n states and room for n * njoints * 16 floats");
}

// ---------------------------------------------------------------------------------------------
// animation layers (SPEC.md section 16)
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(mtr_anim_layer) == 16, "mtr_anim_layer");

int32_t mtr_anim_masks_create(mtr_device* d, size_t njoints, size_t nmasks, const float* weights, mtr_anim_masks** out) {
    if (!d || !out) return MTR_E_INVALID;
    *out = nullptr;
    if (njoints == 0 || njoints > MTR_POSE_MAX_JOINTS) return fail(d, MTR_E_INVALID, "anim masks: 1 to 256 joints");
    if (nmasks == 0 || nmasks > 0xFFFFu || !weights) return fail(d, MTR_E_INVALID, "anim masks: 1 to 65535 masks and their weights");
    for (size_t m = 0; m < nmasks; m++)
        for (size_t j = 0; j < njoints; j++) {
            const float w = weights[m * njoints + j];
            if (!(w >= 0.0f && w <= 1.0f))  // NaN fails both
                return fail(d, MTR_E_INVALID, "anim masks: mask " + std::to_string(m + 1) + ", joint " + std::to_string(j) + " has a weight outside [0, 1]");
        }
    int32_t rc = set_device(d);
    if (rc) return rc;
    auto mk = std::make_unique<mtr_anim_masks>();
    mk->dev = d; mk->njoints = (uint32_t)njoints; mk->nmasks = (uint32_t)nmasks;
    if ((rc = set_upload(mk.get(), "anim masks", {{weights, nmasks * njoints * sizeof(float)}}))) return rc;
    *out = mk.release();
    return MTR_OK;
}

void mtr_anim_masks_destroy(mtr_anim_masks* mk) { set_destroy(mk); }

int32_t mtr_model_animate_layers(mtr_model* m, mtr_anim* a, mtr_anim_masks* mk, const mtr_anim_layer* layers, size_t nlayers) {
    if (!m) return MTR_E_INVALID;
    mtr_device* d = m->dev;
    if (!layers) return fail(d, MTR_E_INVALID, "animate layers: no layers");
    AnimCall c;
    c.kind = AnimCall::kLayers; c.anim = a; c.masks = mk; c.nlayers = nlayers;
    int32_t rc = anim_check(d, m, c);
    if (rc) return rc;
    if ((rc = stage_pose(d, reinterpret_cast<const float*>(layers), nlayers * (sizeof(mtr_anim_layer) / sizeof(float))))) return rc;
    c.recs = d->pose_stage;
    return model_animate(m, c);
}

int32_t mtr_anim_sample_layers(mtr_anim* a, mtr_anim_masks* mk, const mtr_anim_layer* layers, size_t nlayers, size_t n, float* out_locals, size_t count) {
    if (!a) return MTR_E_INVALID;
    AnimCall c;
    c.kind = AnimCall::kLayers; c.anim = a; c.masks = mk; c.recs = layers; c.nlayers = nlayers;
    return anim_sample(c, nlayers * 4, 0, n, out_locals,
                       sample_room(a, n, layers, out_locals, count) ? nullptr : "n * nlayers layers and room for n * njoints * 16 floats");
}

// ---------------------------------------------------------------------------------------------
// inverse kinematics (SPEC.md section 17)
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(mtr_ik_chain) == 32 && sizeof(mtr_ik_target) == 32, "mtr_ik_chain, mtr_ik_target");

int32_t mtr_anim_ik_create(mtr_device* d, size_t njoints, const uint8_t* parents, size_t nchains, const mtr_ik_chain* chains, mtr_anim_ik** out) {
    if (!d || !out) return MTR_E_INVALID;
    *out = nullptr;
    if (njoints == 0 || njoints > MTR_POSE_MAX_JOINTS || !parents) return fail(d, MTR_E_INVALID, "anim ik: 1 to 256 joints and their parents");
    if (nchains < 1 || nchains > MTR_ANIM_MAX_IK || !chains) return fail(d, MTR_E_INVALID, "anim ik: 1 to 4 chains");
    std::vector<uint32_t> paths;
    std::vector<uint8_t> bytes;
    if (!pose_paths(parents, njoints, paths, bytes)) return fail(d, MTR_E_INVALID, "anim ik: a parent out of range or a cycle");
    auto root = [&](uint32_t j) { return parents[j] == 255 || parents[j] == j; };
    for (size_t k = 0; k < nchains; k++) {
        const mtr_ik_chain& c = chains[k];
        const char* what = nullptr;
        if (c.kind != MTR_IK_TWO_BONE && c.kind != MTR_IK_AIM) what = "has a kind other than MTR_IK_TWO_BONE and MTR_IK_AIM";
        else if (c.flags & ~MTR_IK_POLE) what = "has unknown flag bits";
        else if (c.joint[0] >= njoints) what = "names a joint past the skeleton's";
        else if (c.kind == MTR_IK_TWO_BONE) {
            const uint32_t a = c.joint[0], b = c.joint[1], cc = c.joint[2];
            if (b >= njoints || cc >= njoints) what = "names a joint past the skeleton's";
            else if (a == b || b == cc || a == cc) what = "names a joint twice";
            else if (root(b) || root(cc)) what = "has a root for its middle or end joint";
            else if (parents[b] != a || parents[cc] != b) what = "is not a joint, its child and that child's child";
        } else {
            const float* ax = c.axis;
            if (!(std::isfinite(ax[0]) && std::isfinite(ax[1]) && std::isfinite(ax[2]))) what = "has an axis that is not finite";
            else if (ax[0] == 0.0f && ax[1] == 0.0f && ax[2] == 0.0f) what = "has a zero axis";
        }
        if (what) return fail(d, MTR_E_INVALID, "anim ik: chain " + std::to_string(k) + " " + what);
    }
    int32_t rc = set_device(d);
    if (rc) return rc;
    auto ik = std::make_unique<mtr_anim_ik>();
    ik->dev = d; ik->njoints = (uint32_t)njoints; ik->nchains = (uint32_t)nchains; ik->path_bytes = (uint32_t)bytes.size();
    ik->parents.assign(parents, parents + njoints);
    for (size_t j = 0; j < njoints; j++)
        if (ik->parents[j] == j) ik->parents[j] = 255;  // a root either way
    std::vector<uint32_t> img(nchains * 8 + njoints + bytes.size() / 4);  // the chains, the path table, the paths
    memcpy(img.data(), chains, nchains * sizeof(mtr_ik_chain));
    memcpy(img.data() + nchains * 8, paths.data(), njoints * 4);
    memcpy(img.data() + nchains * 8 + njoints, bytes.data(), bytes.size());
    if ((rc = set_upload(ik.get(), "anim ik", {{img.data(), img.size() * 4}}))) return rc;
    *out = ik.release();
    return MTR_OK;
}

void mtr_anim_ik_destroy(mtr_anim_ik* ik) { set_destroy(ik); }

int32_t mtr_model_animate_ik(mtr_model* m, mtr_anim* a, mtr_anim_masks* mk, const mtr_anim_layer* layers, size_t nlayers, mtr_anim_ik* ik,
                             const mtr_ik_target* targets) {
    if (!m) return MTR_E_INVALID;
    mtr_device* d = m->dev;
    if (!layers) return fail(d, MTR_E_INVALID, "animate ik: no layers");
    if (!targets) return fail(d, MTR_E_INVALID, "animate ik: no targets");
    AnimCall c;
    c.kind = AnimCall::kIk; c.anim = a; c.masks = mk; c.ik = ik; c.nlayers = nlayers;
    int32_t rc = anim_check(d, m, c);
    if (rc) return rc;
    if ((rc = stage_ik(d, layers, nlayers, targets, ik->nchains, &c.targets))) return rc;
    c.recs = d->pose_stage;
    return model_animate(m, c);
}

int32_t mtr_anim_sample_ik(mtr_anim* a, mtr_anim_masks* mk, mtr_anim_ik* ik, const mtr_anim_layer* layers, size_t nlayers, const mtr_ik_target* targets,
                           size_t n, float* out_locals, size_t count) {
    if (!a) return MTR_E_INVALID;
    AnimCall c;
    c.kind = AnimCall::kIk; c.anim = a; c.masks = mk; c.ik = ik; c.recs = layers; c.nlayers = nlayers; c.targets = targets;
    return anim_sample(c, nlayers * 4, ik ? ik->nchains * 8 : 0, n, out_locals,
                       sample_room(a, n, layers && targets, out_locals, count) ? nullptr
                                                                               : "n * nlayers layers, n * nchains targets and room for n * njoints * 16 floats");
}

// ---------------------------------------------------------------------------------------------
// root motion (SPEC.md section 19): the root set, and the deltas alone
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(mtr_root_step) == 16, "mtr_root_step");

int32_t mtr_anim_root_create(mtr_device* d, size_t njoints, size_t nclips, uint32_t joint, const uint32_t* flags, mtr_anim_root** out) {
    if (!d || !out) return MTR_E_INVALID;
    *out = nullptr;
    if (njoints == 0 || njoints > MTR_POSE_MAX_JOINTS) return fail(d, MTR_E_INVALID, "anim root: 1 to 256 joints");
    if (nclips == 0 || nclips > 0xFFFFFFu) return fail(d, MTR_E_INVALID, "anim root: at least one clip");
    if (joint >= njoints) return fail(d, MTR_E_INVALID, "anim root: the trajectory joint lies past the set's joints");
    std::vector<uint32_t> img(nclips, 0u);
    for (size_t c = 0; c < nclips && flags; c++) {
        if (flags[c] & ~MTR_ROOT_CYCLIC) return fail(d, MTR_E_INVALID, "anim root: clip " + std::to_string(c) + " has unknown flag bits");
        img[c] = flags[c];
    }
    int32_t rc = set_device(d);
    if (rc) return rc;
    auto r = std::make_unique<mtr_anim_root>();
    r->dev = d; r->njoints = (uint32_t)njoints; r->nclips = (uint32_t)nclips; r->joint = joint;
    if ((rc = set_upload(r.get(), "anim root", {{img.data(), img.size() * 4}}))) return rc;
    *out = r.release();
    return MTR_OK;
}

void mtr_anim_root_destroy(mtr_anim_root* r) { set_destroy(r); }

int32_t mtr_anim_root_deltas_device(mtr_anim* traj, mtr_anim_root* root, const mtr_root_step* steps_dev, size_t nsteps, size_t n, float* out_dev,
                                    void* hip_stream) {
    if (!traj) return MTR_E_INVALID;
    mtr_device* d = traj->dev;
    if (!steps_dev || ((uintptr_t)steps_dev & 15u) || !out_dev || ((uintptr_t)out_dev & 15u))
        return fail(d, MTR_E_INVALID, "root deltas: device steps and matrices must be 16-byte aligned");
    if (n == 0 || n > (1u << 27)) return fail(d, MTR_E_INVALID, "root deltas: 1 to 2^27 instances");
    int32_t rc = root_check(d, traj, root, nsteps, true);
    if (rc) return rc;
    return root_enqueue(traj, root, steps_dev, nsteps, n, nullptr, out_dev, caller_stream(d, hip_stream));
}

int32_t mtr_anim_root_deltas(mtr_anim* traj, mtr_anim_root* root, const mtr_root_step* steps, size_t nsteps, size_t n, float* out, size_t count) {
    if (!traj) return MTR_E_INVALID;
    mtr_device* d = traj->dev;
    if (!steps || !out) return fail(d, MTR_E_INVALID, "root deltas: no steps or no room for the matrices");
    if (n == 0 || n > (1u << 27) || count < n * 16) return fail(d, MTR_E_INVALID, "root deltas: 1 to 2^27 instances and room for n * 16 floats");
    int32_t rc = root_check(d, traj, root, nsteps, true);
    if (rc) return rc;
    // the matrices, then the steps (n * 64 bytes in: 16-byte aligned)
    StagedBlock blk(d);
    StagedPart &p_out = blk.part(out, n * 16), &p_steps = blk.part(steps, n * nsteps * 4);
    return blk.run([&]() -> int32_t {
        int32_t r2;
        if ((r2 = blk.up({&p_steps})) || (r2 = root_enqueue(traj, root, p_steps.at, nsteps, n, nullptr, p_out.dev<float>(), d->s_copy))) return r2;
        return blk.down({&p_out});
    });
}

}  // extern "C"
