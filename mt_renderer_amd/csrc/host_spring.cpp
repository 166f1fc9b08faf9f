// host_spring.cpp -- spring bones (SPEC.md section 24): the spring set (its validation, the rounds the host counts, its
// device image) and the two entry points.  The call itself is the fourth kind of animate call: host_anim.cpp checks and
// queues it (anim_check, anim_enqueue), host_batch.cpp writes the batch's version (batch_animate).
#include "host.h"

using namespace mtr_host;

extern "C" {

static_assert(sizeof(mtr_spring) == 48 && sizeof(mtr_spring_state) == 32, "mtr_spring, mtr_spring_state");

int32_t mtr_anim_spring_create(mtr_device* d, size_t njoints, const uint8_t* parents, size_t nsprings, const mtr_spring* springs, mtr_anim_spring** out) {
    if (!d || !out) return MTR_E_INVALID;
    *out = nullptr;
    if (njoints == 0 || njoints > MTR_POSE_MAX_JOINTS || !parents) return fail(d, MTR_E_INVALID, "anim spring: 1 to 256 joints and their parents");
    if (nsprings < 1 || nsprings > MTR_ANIM_MAX_SPRINGS || !springs) return fail(d, MTR_E_INVALID, "anim spring: 1 to 16 springs");
    std::vector<uint32_t> paths;
    std::vector<uint8_t> bytes;
    if (!pose_paths(parents, njoints, paths, bytes)) return fail(d, MTR_E_INVALID, "anim spring: a parent out of range or a cycle");
    auto finite3 = [](const float* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); };
    std::vector<uint32_t> tab(njoints, MTR_SPRING_NONE);  // per joint: its spring (the round is added below)
    for (size_t k = 0; k < nsprings; k++) {
        const mtr_spring& s = springs[k];
        const char* what = nullptr;
        if (s.joint >= njoints) what = "names a joint past the skeleton's";
        else if (tab[s.joint] != MTR_SPRING_NONE) what = "names a joint that an earlier spring names";
        else if (s.flags) what = "has flag bits";
        else if (!finite3(s.tail)) what = "has a tail that is not finite";
        else if (s.tail[0] == 0.0f && s.tail[1] == 0.0f && s.tail[2] == 0.0f) what = "has a zero tail";
        else if (!(std::isfinite(s.stiffness) && s.stiffness >= 0.0f)) what = "has a stiffness that is not finite or negative";
        else if (!(s.drag >= 0.0f && s.drag <= 1.0f)) what = "has a drag outside [0, 1]";  // NaN fails both
        else if (!finite3(s.gravity)) what = "has a gravity that is not finite";
        if (what) return fail(d, MTR_E_INVALID, "anim spring: spring " + std::to_string(k) + " " + what);
        tab[s.joint] = (uint32_t)k;
    }
    // a spring's round: the spring joints among its joint's ancestors.  Springs of one round are not ancestors of one another.
    auto root = [&](uint32_t j) { return parents[j] == 255 || parents[j] == j; };
    uint32_t nrounds = 0;
    std::vector<uint32_t> round(nsprings, 0u);
    for (size_t k = 0; k < nsprings; k++) {
        for (uint32_t j = springs[k].joint; !root(j);) {
            j = parents[j];
            if (tab[j] != MTR_SPRING_NONE) round[k]++;
        }
        nrounds = std::max(nrounds, round[k] + 1u);
    }
    for (size_t k = 0; k < nsprings; k++) tab[springs[k].joint] |= round[k] << 8;
    int32_t rc = set_device(d);
    if (rc) return rc;
    auto sp = std::make_unique<mtr_anim_spring>();
    sp->dev = d; sp->njoints = (uint32_t)njoints; sp->nsprings = (uint32_t)nsprings; sp->nrounds = nrounds; sp->path_bytes = (uint32_t)bytes.size();
    sp->parents.assign(parents, parents + njoints);
    for (size_t j = 0; j < njoints; j++)
        if (sp->parents[j] == j) sp->parents[j] = 255;  // a root either way
    std::vector<uint32_t> img(nsprings * 12 + njoints * 2 + bytes.size() / 4);  // the springs, the joint table, the path table, the paths
    memcpy(img.data(), springs, nsprings * sizeof(mtr_spring));
    for (size_t k = 0; k < nsprings; k++) img[k * 12 + 7] = img[k * 12 + 11] = 0u;  // the pads
    memcpy(img.data() + nsprings * 12, tab.data(), njoints * 4);
    memcpy(img.data() + nsprings * 12 + njoints, paths.data(), njoints * 4);
    memcpy(img.data() + nsprings * 12 + njoints * 2, bytes.data(), bytes.size());
    if ((rc = set_upload(sp.get(), "anim spring", {{img.data(), img.size() * 4}}))) return rc;
    *out = sp.release();
    return MTR_OK;
}

void mtr_anim_spring_destroy(mtr_anim_spring* sp) { set_destroy(sp); }

int32_t mtr_batch_animate_spring_device(mtr_batch* b, mtr_anim* a, mtr_anim_masks* mk, const mtr_anim_layer* layers_dev, size_t nlayers, mtr_anim_ik* ik,
                                        const mtr_ik_target* targets_dev, mtr_anim_spring* sp, mtr_spring_state* states_dev, const float* motion_dev, float dt,
                                        void* hip_stream) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!layers_dev || ((uintptr_t)layers_dev & 15u)) return fail(d, MTR_E_INVALID, "animate spring: device layers must be 16-byte aligned");
    if (ik ? !targets_dev : targets_dev != nullptr) return fail(d, MTR_E_INVALID, "animate spring: targets go with an IK set, and an IK set with targets");
    if ((uintptr_t)targets_dev & 15u) return fail(d, MTR_E_INVALID, "animate spring: device targets must be 16-byte aligned");
    if (!states_dev || ((uintptr_t)states_dev & 15u)) return fail(d, MTR_E_INVALID, "animate spring: device spring states must be 16-byte aligned");
    if ((uintptr_t)motion_dev & 15u) return fail(d, MTR_E_INVALID, "animate spring: device motion must be 16-byte aligned");
    AnimCall c;
    c.kind = AnimCall::kSpring; c.anim = a; c.masks = mk; c.ik = ik; c.recs = layers_dev; c.nlayers = nlayers; c.targets = targets_dev;
    c.spring = sp; c.spring_states = states_dev; c.motion = motion_dev; c.dt = dt;
    int32_t rc = anim_check(d, b->model, c);
    if (rc) return rc;
    return batch_animate(b, c, caller_stream(d, hip_stream));
}

// Everything in host memory: the local matrices, then the layers, the targets, the states and the motion go through scratch,
// each part a multiple of 16 bytes; the states come back behind the kernel.
int32_t mtr_anim_sample_spring(mtr_anim* a, mtr_anim_masks* mk, mtr_anim_ik* ik, mtr_anim_spring* sp, const mtr_anim_layer* layers, size_t nlayers,
                               const mtr_ik_target* targets, mtr_spring_state* states, const float* motion, float dt, size_t n, float* out_locals,
                               size_t count) {
    if (!a) return MTR_E_INVALID;
    mtr_device* d = a->dev;
    AnimCall c;
    c.kind = AnimCall::kSpring; c.anim = a; c.masks = mk; c.ik = ik; c.nlayers = nlayers; c.spring = sp; c.dt = dt;
    const char* no_room = nullptr;
    if (ik ? !targets : targets != nullptr) no_room = "targets go with an IK set, and an IK set with targets";
    else if (n > 0xFFFFFFu || (n && (!layers || !states || !out_locals)) || count < n * a->njoints * 16)
        no_room = "n * nlayers layers, n * nsprings spring states and room for n * njoints * 16 floats";
    int32_t rc = anim_check(d, nullptr, c, no_room);
    if (rc || !n) return rc;
    StagedBlock blk(d);
    StagedPart &p_locals = blk.part(out_locals, n * a->njoints * 16), &p_layers = blk.part(layers, n * nlayers * 4),
               &p_targets = blk.part(targets, ik ? n * ik->nchains * 8 : 0), &p_states = blk.part(states, n * sp->nsprings * 8),
               &p_motion = blk.part(motion, motion ? n * 16 : 0);
    return blk.run([&]() -> int32_t {
        int32_t r2 = blk.up({&p_layers, &p_targets, &p_states, &p_motion});
        if (r2) return r2;
        c.recs = p_layers.at; c.targets = p_targets.dev<void>(); c.spring_states = p_states.at; c.motion = p_motion.dev<float>();
        if ((r2 = anim_enqueue(c, nullptr, p_locals.dev<float>(), (uint32_t)n, d->s_copy))) return r2;
        return blk.down({&p_locals, &p_states});
    });
}

}  // extern "C"
