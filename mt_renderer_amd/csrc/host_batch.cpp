// host_batch.cpp -- instance batches and their versions, pose and animation staging, animation clip sets, mask sets and layers, IK sets,
// attachments, root motion.
#include "host.h"
#include "attach_math.h"

// k_pose.hip.  Weak: the host-only builds of this file (tests/cpp, over the HIP stub runtime) link no kernels and never
// form a pose; libmtr.so links k_pose.o.
void mtr_launch_pose(const PoseParams& p, uint32_t ninst, hipStream_t s) __attribute__((weak));
// k_anim.hip, weak for the same reason
void mtr_launch_anim(const AnimParams& p, uint32_t ninst, hipStream_t s) __attribute__((weak));
void mtr_launch_anim_sample(const AnimParams& p, uint32_t ninst, hipStream_t s) __attribute__((weak));
void mtr_launch_anim_tracks(const AnimParams& p, uint32_t ninst, hipStream_t s) __attribute__((weak));
void mtr_launch_anim_tracks_sample(const AnimParams& p, uint32_t ninst, hipStream_t s) __attribute__((weak));
void mtr_launch_anim_layers(const AnimLayerParams& p, uint32_t ninst, hipStream_t s) __attribute__((weak));
void mtr_launch_anim_layers_sample(const AnimLayerParams& p, uint32_t ninst, hipStream_t s) __attribute__((weak));
void mtr_launch_anim_layers_tracks(const AnimLayerParams& p, uint32_t ninst, hipStream_t s) __attribute__((weak));
void mtr_launch_anim_layers_tracks_sample(const AnimLayerParams& p, uint32_t ninst, hipStream_t s) __attribute__((weak));
void mtr_launch_anim_ik(const AnimIkParams& p, uint32_t ninst, hipStream_t s) __attribute__((weak));
void mtr_launch_anim_ik_sample(const AnimIkParams& p, uint32_t ninst, hipStream_t s) __attribute__((weak));
void mtr_launch_anim_ik_tracks(const AnimIkParams& p, uint32_t ninst, hipStream_t s) __attribute__((weak));
void mtr_launch_anim_ik_tracks_sample(const AnimIkParams& p, uint32_t ninst, hipStream_t s) __attribute__((weak));
// k_attach.hip, weak for the same reason
void mtr_launch_attach(const AttachParams& p, hipStream_t s) __attribute__((weak));
// k_root.hip, weak for the same reason
void mtr_launch_root(const RootParams& p, hipStream_t s) __attribute__((weak));
void mtr_launch_root_deltas(const RootParams& p, hipStream_t s) __attribute__((weak));

namespace mtr_host {

namespace {

// room for count floats in the device's staging buffer (the render thread only)
int32_t stage_reserve(mtr_device* d, size_t count) {
    if (count > d->pose_stage_cap) {
        HIPCHK(d, hipStreamSynchronize(d->s_copy));  // a queued pose kernel may still read the old buffer
        if (d->pose_stage) (void)hipFree(d->pose_stage);
        d->pose_stage = nullptr; d->pose_stage_cap = 0;
        int32_t rc = dev_alloc(d, &d->pose_stage, count);
        if (rc) return rc;
        d->pose_stage_cap = count;
    }
    return MTR_OK;
}

}  // namespace

// host local matrices -> the device's staging buffer, on s_copy (the render thread only)
int32_t stage_pose(mtr_device* d, const float* local_mats, size_t count) {
    int32_t rc = stage_reserve(d, count);
    if (rc) return rc;
    HIPCHK(d, hipMemcpyAsync(d->pose_stage, local_mats, count * sizeof(float), hipMemcpyHostToDevice, d->s_copy));
    return MTR_OK;
}

PoseParams pose_params(const mtr_model::Skeleton& sk, const float* locals, float* out) {
    PoseParams pp{};
    pp.locals = locals; pp.out = out; pp.imats = sk.d;
    pp.paths = reinterpret_cast<const uint32_t*>(sk.d + (size_t)sk.njoints * 16);
    pp.path_words = reinterpret_cast<const uint32_t*>(sk.d + (size_t)sk.njoints * 17);
    pp.njoints = sk.njoints; pp.path_bytes = sk.path_bytes;
    return pp;
}

namespace {

AnimParams anim_params(const mtr_anim* a, const mtr_model::Skeleton& sk, const void* states_dev, float* out) {
    AnimParams ap{};
    ap.pose = pose_params(sk, nullptr, out);
    ap.clips = a->d;
    ap.states = static_cast<const uint32_t*>(states_dev);
    ap.nclips = a->nclips;
    if (a->tracks) {
        ap.tracks = a->d + (size_t)a->nclips * 4;
        ap.values = ap.tracks + (size_t)a->nclips * a->njoints * 3 * 8;
        ap.times = reinterpret_cast<const uint16_t*>(ap.values + (size_t)a->nkeys * 2);
    } else {
        ap.keys = reinterpret_cast<const float*>(a->d + (size_t)a->nclips * 4);
    }
    return ap;
}

// k_anim on the set's kind of source (check_anim has seen the launcher)
void launch_anim(const mtr_anim* a, const AnimParams& ap, uint32_t ninst, hipStream_t s) {
    if (a->tracks) mtr_launch_anim_tracks(ap, ninst, s);
    else mtr_launch_anim(ap, ninst, s);
}

// a layer stack over the set (section 16): layers_dev holds ninst * nlayers records; masks may be nullptr
AnimLayerParams anim_layer_params(const mtr_anim* a, const mtr_anim_masks* mk, const mtr_model::Skeleton& sk, const void* layers_dev,
                                  uint32_t nlayers, float* out) {
    AnimLayerParams lp{};
    lp.anim = anim_params(a, sk, nullptr, out);
    lp.layers = static_cast<const uint32_t*>(layers_dev);
    lp.nlayers = nlayers;
    if (mk) { lp.masks = mk->d; lp.nmasks = mk->nmasks; }
    return lp;
}

void launch_anim_layers(const mtr_anim* a, const AnimLayerParams& lp, uint32_t ninst, hipStream_t s) {
    if (a->tracks) mtr_launch_anim_layers_tracks(lp, ninst, s);
    else mtr_launch_anim_layers(lp, ninst, s);
}

// the layer stacks and the IK targets of one call behind each other in the staging buffer, on s_copy; the layers are a
// multiple of 16 bytes, so the targets (*targets_dev) are 16-byte aligned
int32_t stage_ik(mtr_device* d, const mtr_anim_layer* layers, size_t nl, const mtr_ik_target* targets, size_t nt, const void** targets_dev) {
    const size_t lw = nl * (sizeof(mtr_anim_layer) / sizeof(float)), tw = nt * (sizeof(mtr_ik_target) / sizeof(float));
    int32_t rc = stage_reserve(d, lw + tw);
    if (rc) return rc;
    HIPCHK(d, hipMemcpyAsync(d->pose_stage, layers, lw * sizeof(float), hipMemcpyHostToDevice, d->s_copy));
    HIPCHK(d, hipMemcpyAsync(d->pose_stage + lw, targets, tw * sizeof(float), hipMemcpyHostToDevice, d->s_copy));
    *targets_dev = d->pose_stage + lw;
    return MTR_OK;
}

// the chains of an IK set after a layer stack (section 17): targets_dev holds ninst * nchains records.  sk: the model's
// skeleton, whose path table the chain walks read as the fold does; without one (mtr_anim_sample_ik) the IK set's copy
AnimIkParams anim_ik_params(const mtr_anim* a, const mtr_anim_masks* mk, const mtr_model::Skeleton& sk, const void* layers_dev, uint32_t nlayers,
                            const mtr_anim_ik* ik, const void* targets_dev, float* out) {
    AnimIkParams ip{};
    ip.layers = anim_layer_params(a, mk, sk, layers_dev, nlayers, out);
    ip.chains = ik->d;
    ip.targets = static_cast<const uint32_t*>(targets_dev);
    ip.nchains = ik->nchains;
    if (sk.d) {
        ip.paths = ip.layers.anim.pose.paths; ip.path_words = ip.layers.anim.pose.path_words; ip.path_bytes = sk.path_bytes;
    } else {
        ip.paths = ik->d + (size_t)ik->nchains * 8; ip.path_words = ip.paths + ik->njoints; ip.path_bytes = ik->path_bytes;
    }
    return ip;
}

void launch_anim_ik(const mtr_anim* a, const AnimIkParams& ip, uint32_t ninst, hipStream_t s) {
    if (a->tracks) mtr_launch_anim_ik_tracks(ip, ninst, s);
    else mtr_launch_anim_ik(ip, ninst, s);
}

// around a kernel on `s` that reads the clip set, the mask set or the IK set: see mtr_anim::last
template <class Set>
int32_t anim_before(Set* a, hipStream_t s) {
    if (a->recorded && a->last_stream != s) HIPCHK(a->dev, hipStreamWaitEvent(s, a->last, 0));
    return MTR_OK;
}
template <class Set>
int32_t anim_after(Set* a, hipStream_t s) {
    HIPCHK(a->dev, hipEventRecord(a->last, s));
    a->last_stream = s; a->recorded = true;
    return MTR_OK;
}

// frame `f` has left the GPU (or certainly will have before anything queued after this call runs)
bool frame_done(mtr_device* d, uint64_t f) {
    if (d->frames_submitted >= f + 1 + d->max_inflight) return true;  // frame f + max_inflight waited for it
    hipEvent_t e = d->inflight[f % d->max_inflight];
    const bool done = !e || hipEventQuery(e) == hipSuccess;
    (void)hipGetLastError();  // hipEventQuery reports "not ready" as an error code
    return done;
}

}  // namespace

void release_now(FreeList& fl) {
    for (void* p : fl.bufs) (void)hipFree(p);
    for (hipEvent_t e : fl.events) (void)hipEventDestroy(e);
    fl.bufs.clear();
    fl.events.clear();
}

namespace {

// Retires the buffer of a version nobody will draw again: into `now` (released after the lock) when no frame in flight
// reads it and its last write has completed, otherwise -- or when now is nullptr -- parked in d->garbage with the event of
// that write, collected by a later submit.  A version with an outside reader pending (Ver::read, a k_attach of another
// batch's update) is always parked, behind that reader's event: the reader waited for the write, so its event covers both,
// and nobody asks the host whether it has run.  submit_mu held.
void retire_version(mtr_device* d, mtr_batch::Ver& v, FreeList* now) {
    if (v.d) {
        const bool read_in_flight = v.used && !frame_done(d, v.last_frame);
        bool written = true;
        if (v.ready) { written = hipEventQuery(v.ready) == hipSuccess; (void)hipGetLastError(); }
        if (v.read_pending) {
            d->garbage.push_back({v.d, v.used ? v.last_frame : 0, v.read});
            v.read = nullptr;
            if (v.ready) d->garbage.push_back({nullptr, 0, v.ready});
            v.ready = nullptr;
        } else if (read_in_flight || !written || !now) {
            d->garbage.push_back({v.d, v.used ? v.last_frame : 0, v.ready});
            v.ready = nullptr;
        } else {
            now->bufs.push_back(v.d);
        }
    }
    for (hipEvent_t e : {v.ready, v.read}) {
        if (!e) continue;
        if (now) now->events.push_back(e);
        else d->garbage.push_back({nullptr, 0, e});
    }
    v = mtr_batch::Ver{};
}

// what a root-motion call (section 19) runs in place of k_attach: M * D from the steps (the records) over a trajectory set
struct RootSrc {
    mtr_anim* traj = nullptr;
    mtr_anim_root* root = nullptr;
    uint32_t nsteps = 0;
};

RootParams root_params(const mtr_anim* traj, const mtr_anim_root* root, const void* steps_dev, uint32_t nsteps, size_t n, const float* mats_in, float* out) {
    RootParams rp{};
    rp.anim.clips = traj->d;
    rp.anim.nclips = traj->nclips;
    rp.anim.pose.njoints = traj->njoints;
    if (traj->tracks) {
        rp.anim.tracks = traj->d + (size_t)traj->nclips * 4;
        rp.anim.values = rp.anim.tracks + (size_t)traj->nclips * traj->njoints * 3 * 8;
        rp.anim.times = reinterpret_cast<const uint16_t*>(rp.anim.values + (size_t)traj->nkeys * 2);
    } else {
        rp.anim.keys = reinterpret_cast<const float*>(traj->d + (size_t)traj->nclips * 4);
    }
    rp.root_flags = root->d;
    rp.steps = static_cast<const uint32_t*>(steps_dev);
    rp.mats_in = mats_in; rp.out = out;
    rp.joint = root->joint; rp.nsteps = nsteps; rp.n = (uint32_t)n;
    return rp;
}

// An outside reader of a batch's current version: a k_attach that forms matrices from its instance matrices and palettes
// (SPEC.md section 18) on a stream the batch's own updates need not share.  pin (submit_mu held) takes the current version
// and keeps batch_next_version off it; launch (no lock: only this thread touches a pinned version's events) makes `s` wait
// for the version's write and, when the reader before ran on another stream, for that reader, runs the kernel and records
// Ver::read behind it; unpin (submit_mu held) publishes the event.  The next write into the version waits for it
// (batch_write_version), and a buffer retired meanwhile is parked behind it (retire_version).
struct SrcRead {
    mtr_batch* b = nullptr;
    int vi = -1;
    mtr_batch::Ver v{};
    bool recorded = false;
};

void src_read_pin(mtr_batch* src, SrcRead& r) {
    r.b = src; r.vi = src->cur;
    r.v = src->vers[(size_t)r.vi];
    src->vers[(size_t)r.vi].pinned++;
}

int32_t src_read_launch(SrcRead& r, const void* recs_dev, size_t n, float* out_dev, hipStream_t s, const RootSrc* rt = nullptr) {
    mtr_device* d = r.b->dev;
    if (!r.v.read && hipEventCreateWithFlags(&r.v.read, hipEventDisableTiming) != hipSuccess) return fail(d, MTR_E_HIP, "hipEventCreate failed");
    if (r.v.ready) HIPCHK(d, hipStreamWaitEvent(s, r.v.ready, 0));
    if (r.v.read_pending && r.v.read_stream != s) HIPCHK(d, hipStreamWaitEvent(s, r.v.read, 0));
    if (rt) {  // the version's own matrices times the deltas; the trajectory set and the root set are read like a clip set
        int32_t rc = anim_before(rt->traj, s);
        if (rc || (rc = anim_before(rt->root, s))) return rc;
        mtr_launch_root(root_params(rt->traj, rt->root, recs_dev, rt->nsteps, n, r.v.d, out_dev), s);
        HIPCHK(d, hipGetLastError());
        if ((rc = anim_after(rt->traj, s)) || (rc = anim_after(rt->root, s))) return rc;
    } else {
        AttachParams ap{};
        ap.recs = static_cast<const uint32_t*>(recs_dev);
        ap.src_mats = r.v.d; ap.src_pals = r.v.d + (size_t)r.b->n * 16;
        ap.out = out_dev;
        ap.n = (uint32_t)n; ap.n_src = r.b->n; ap.npal = r.v.npal;
        mtr_launch_attach(ap, s);
        HIPCHK(d, hipGetLastError());
    }
    HIPCHK(d, hipEventRecord(r.v.read, s));
    r.recorded = true;
    return MTR_OK;
}

void src_read_unpin(SrcRead& r, hipStream_t s) {
    mtr_batch::Ver& v = r.b->vers[(size_t)r.vi];
    v.read = r.v.read;
    if (r.recorded) { v.read_pending = true; v.read_stream = s; }
    v.pinned--;
}

}  // namespace

// drops one reference of the batch; the last one retires every version and frees the handle.  submit_mu held.
void batch_unref(mtr_batch* b, FreeList& fl) {
    if (--b->refs) return;
    mtr_device* d = b->dev;
    if (b->hint_slot >= 0) { d->hint_used[b->hint_slot] = false; d->hint_host[2 * b->hint_slot] = d->hint_host[2 * b->hint_slot + 1] = 0u; }
    for (auto& v : b->vers) retire_version(d, v, &fl);
    delete b;
}

namespace {

// A version the next update may write: not the current one, held by no frame that may still (re-)run, and preferably read
// by no frame still on the GPU.  Once the ring has max_inflight + 1 versions the one read longest ago is taken and
// *frame_ev is the completion event of the frame that read it: the writing stream must wait on it.  A version too small
// for npal palettes per instance is emptied (its buffer parked in d->garbage) for the caller to allocate.  No allocation,
// free or host wait here.  submit_mu held.
int32_t batch_next_version(mtr_batch* b, uint32_t npal, int* out, hipEvent_t* frame_ev) {
    mtr_device* d = b->dev;
    int pick = -1, oldest = -1;
    *frame_ev = nullptr;
    for (size_t i = 0; i < b->vers.size() && pick < 0; i++) {
        const mtr_batch::Ver& v = b->vers[i];
        if ((int)i == b->cur || v.pinned) continue;
        if (!v.used || frame_done(d, v.last_frame)) pick = (int)i;
        else if (oldest < 0 || v.last_frame < b->vers[(size_t)oldest].last_frame) oldest = (int)i;
    }
    if (pick < 0 && (oldest < 0 || b->vers.size() < (size_t)d->max_inflight + 1)) {
        if (b->vers.size() >= 4096) return fail(d, MTR_E_NOMEM, "more than 4096 live frames hold a version of this batch");
        b->vers.emplace_back();
        pick = (int)b->vers.size() - 1;
    }
    if (pick < 0) {
        // not done, so its frame is one of the last max_inflight: the ring event still holds that frame's record
        pick = oldest;
        *frame_ev = d->inflight[b->vers[(size_t)pick].last_frame % d->max_inflight];
    }
    mtr_batch::Ver& v = b->vers[(size_t)pick];
    if (v.cap < (size_t)b->n * 16 * (1 + (size_t)npal)) retire_version(d, v, nullptr);
    v.used = false; v.last_frame = 0;
    *out = pick;
    return MTR_OK;
}

// Where the palettes of a pose come from: local matrices (k_pose), animation states over a clip set (k_anim), layer
// stacks over a clip set and an optional mask set (k_anim_layers: nlayers != 0, states holds the layers), or such stacks
// followed by the chains of an IK set (k_anim_ik: ik != nullptr, targets holds the targets); device memory
struct PoseSrc {
    const float* locals = nullptr;
    mtr_anim* anim = nullptr;
    const void* states = nullptr;
    mtr_anim_masks* masks = nullptr;
    uint32_t nlayers = 0;
    mtr_anim_ik* ik = nullptr;
    const void* targets = nullptr;
    explicit operator bool() const { return locals || anim; }
};

// the matrices of an attach call: one record per instance (device memory) against the current version of `src`
// (a root-motion call: src is the batch itself, recs its steps, root what runs instead of k_attach)
struct AttachSrc {
    mtr_batch* src = nullptr;
    const void* recs = nullptr;
    const RootSrc* root = nullptr;
};

// What an update writes into a fresh version.  mats / pals: host arrays, or nullptr = keep the current version's (device
// copy); a pose source replaces the palettes with the pose's; an attach source (at) replaces the matrices with k_attach's.
// Enqueued on `s`, the version made current.
int32_t batch_write_version(mtr_batch* b, const float* mats, const float* pals, uint32_t npal_new, const PoseSrc& src, hipStream_t s,
                            const AttachSrc* at = nullptr) {
    mtr_device* d = b->dev;
    const size_t n = b->n;
    int vi = -1;
    mtr_batch::Ver cur{}, v{};
    SrcRead rd;
    {
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        cur = b->vers[(size_t)b->cur];
        const uint32_t npal = (pals || src) ? npal_new : cur.npal;
        hipEvent_t frame_ev = nullptr;
        int32_t rc = batch_next_version(b, npal, &vi, &frame_ev);
        if (rc) return rc;
        mtr_batch::Ver& nv = b->vers[(size_t)vi];
        nv.npal = npal;
        nv.pinned++;  // nobody else takes it while it is being written
        v = nv;
        if (at) src_read_pin(at->src, rd);  // the source's current version (b's own when batch == src: never the one written)
        // a frame still on the GPU reads it: the write waits for that frame on the device (the enqueue happens under the
        // lock, before any later frame can record the same ring event)
        if (frame_ev) {
            const hipError_t e = hipStreamWaitEvent(s, frame_ev, 0);
            if (e != hipSuccess) { nv.pinned--; if (at) src_read_unpin(rd, s); return fail(d, MTR_E_HIP, std::string("hipStreamWaitEvent: ") + hipGetErrorString(e)); }
        }
    }
    // only this thread touches the version's buffer and event while it is pinned
    int32_t rc = MTR_OK;
    const size_t need = n * 16 * (1 + (size_t)v.npal);
    if (!v.d) {
        if (!(rc = dev_alloc(d, &v.d, need))) v.cap = need;
    }
    if (!rc && !v.ready && hipEventCreateWithFlags(&v.ready, hipEventDisableTiming) != hipSuccess) rc = fail(d, MTR_E_HIP, "hipEventCreate failed");
    auto enqueue = [&]() -> int32_t {
        HIPCHK(d, hipStreamWaitEvent(s, v.ready, 0));    // its previous write (a version may be rewritten before any draw)
        if (v.read_pending) HIPCHK(d, hipStreamWaitEvent(s, v.read, 0));  // and a k_attach of another update that still reads it
        if (cur.ready) HIPCHK(d, hipStreamWaitEvent(s, cur.ready, 0));
        if (at) {
            int32_t arc = src_read_launch(rd, at->recs, n, v.d, s, at->root);
            if (arc) return arc;
        } else if (mats) HIPCHK(d, hipMemcpyAsync(v.d, mats, n * 64, hipMemcpyHostToDevice, s));
        else HIPCHK(d, hipMemcpyAsync(v.d, cur.d, n * 64, hipMemcpyDeviceToDevice, s));
        float* vp = v.d + n * 16;
        if (src.anim) {
            int32_t arc = anim_before(src.anim, s);
            if (arc) return arc;
            if (src.masks && (arc = anim_before(src.masks, s))) return arc;
            if (src.ik && (arc = anim_before(src.ik, s))) return arc;
            if (src.ik)
                launch_anim_ik(src.anim, anim_ik_params(src.anim, src.masks, b->model->skel, src.states, src.nlayers, src.ik, src.targets, vp), (uint32_t)n, s);
            else if (src.nlayers) launch_anim_layers(src.anim, anim_layer_params(src.anim, src.masks, b->model->skel, src.states, src.nlayers, vp), (uint32_t)n, s);
            else launch_anim(src.anim, anim_params(src.anim, b->model->skel, src.states, vp), (uint32_t)n, s);
            HIPCHK(d, hipGetLastError());
            if ((arc = anim_after(src.anim, s))) return arc;
            if (src.masks && (arc = anim_after(src.masks, s))) return arc;
            if (src.ik && (arc = anim_after(src.ik, s))) return arc;
        } else if (src.locals) {
            mtr_launch_pose(pose_params(b->model->skel, src.locals, vp), (uint32_t)n, s);
            HIPCHK(d, hipGetLastError());
        } else if (pals) {
            HIPCHK(d, hipMemcpyAsync(vp, pals, n * v.npal * 64, hipMemcpyHostToDevice, s));
        } else if (v.npal) {
            HIPCHK(d, hipMemcpyAsync(vp, cur.d + n * 16, n * v.npal * 64, hipMemcpyDeviceToDevice, s));
        }
        HIPCHK(d, hipEventRecord(v.ready, s));
        return MTR_OK;
    };
    if (!rc) rc = enqueue();
    std::lock_guard<std::mutex> submit_lock(d->submit_mu);
    mtr_batch::Ver& nv = b->vers[(size_t)vi];
    nv.d = v.d; nv.cap = v.cap; nv.ready = v.ready;
    if (!rc) nv.read_pending = false;  // the write waited for it
    nv.pinned--;
    if (at) src_read_unpin(rd, s);
    if (!rc) b->cur = vi;
    return rc;
}

int32_t check_batch_pose(mtr_batch* b, size_t njoints) {
    mtr_device* d = b->dev;
    if (!b->model->skel.d) return fail(d, MTR_E_INVALID, "pose: the batch's model has no skeleton");
    if (njoints != b->model->skel.njoints) return fail(d, MTR_E_INVALID, "pose: one local matrix per joint of the skeleton");
    if (!mtr_launch_pose) return fail(d, MTR_E_UNSUPPORTED, "pose: built without k_pose");
    return set_device(d);
}

int32_t check_anim(mtr_device* d, const mtr_model* m, const mtr_anim* a) {
    if (!a) return fail(d, MTR_E_INVALID, "animate: no animation set");
    if (a->dev != d) return fail(d, MTR_E_INVALID, "animate: the animation set belongs to another device");
    if (!m->skel.d) return fail(d, MTR_E_INVALID, "animate: the model has no skeleton");
    if (a->njoints != m->skel.njoints) return fail(d, MTR_E_INVALID, "animate: the animation set's joint count is not the skeleton's");
    if (!(a->tracks ? mtr_launch_anim_tracks : mtr_launch_anim)) return fail(d, MTR_E_UNSUPPORTED, "animate: built without k_anim");
    return set_device(d);
}

// what every layered animate call checks besides check_anim
int32_t check_anim_layers(mtr_device* d, const mtr_model* m, const mtr_anim* a, const mtr_anim_masks* mk, size_t nlayers) {
    if (nlayers < 1 || nlayers > MTR_ANIM_MAX_LAYERS) return fail(d, MTR_E_INVALID, "animate layers: 1 to 8 layers per instance");
    if (mk && mk->dev != d) return fail(d, MTR_E_INVALID, "animate layers: the mask set belongs to another device");
    if (mk && mk->njoints != m->skel.njoints) return fail(d, MTR_E_INVALID, "animate layers: the mask set's joint count is not the skeleton's");
    int32_t rc = check_anim(d, m, a);
    if (rc) return rc;
    if (!(a->tracks ? mtr_launch_anim_layers_tracks : mtr_launch_anim_layers)) return fail(d, MTR_E_UNSUPPORTED, "animate layers: built without k_anim_layers");
    return MTR_OK;
}

// what every IK animate call checks besides check_anim_layers
int32_t check_anim_ik(mtr_device* d, const mtr_model* m, const mtr_anim* a, const mtr_anim_masks* mk, size_t nlayers, const mtr_anim_ik* ik) {
    int32_t rc = check_anim_layers(d, m, a, mk, nlayers);
    if (rc) return rc;
    if (!ik) return fail(d, MTR_E_INVALID, "animate ik: no IK set");
    if (ik->dev != d) return fail(d, MTR_E_INVALID, "animate ik: the IK set belongs to another device");
    if (ik->njoints != m->skel.njoints) return fail(d, MTR_E_INVALID, "animate ik: the IK set's joint count is not the skeleton's");
    for (uint32_t j = 0; j < ik->njoints; j++)
        if (ik->parents[j] != m->skel.parents[j])
            return fail(d, MTR_E_INVALID, "animate ik: the IK set's parent of joint " + std::to_string(j) + " is not the skeleton's");
    if (!(a->tracks ? mtr_launch_anim_ik_tracks : mtr_launch_anim_ik)) return fail(d, MTR_E_UNSUPPORTED, "animate ik: built without k_anim_ik");
    return MTR_OK;
}

}  // namespace

}  // namespace mtr_host

using namespace mtr_host;

extern "C" {

// ---------------------------------------------------------------------------------------------
// instance batches
// ---------------------------------------------------------------------------------------------
int32_t mtr_batch_create(mtr_device* d, mtr_model* model, size_t n, const float* model_mats, const float* palettes,
                         size_t npal, const int32_t* texture_override, mtr_batch** out) {
    if (!d || !out) return MTR_E_INVALID;
    *out = nullptr;
    if (!model || model->dev != d || !model_mats || n == 0 || n > 0xFFFFu)
        return fail(d, MTR_E_INVALID, "bad batch arguments");
    if (npal > 256 || (npal && !palettes)) return fail(d, MTR_E_INVALID, "palette: at most 256 matrices");
    auto b = std::unique_ptr<mtr_batch, BatchDeleter>(new mtr_batch());
    b->dev = d; b->model = model; b->n = (uint32_t)n;
    b->vers.emplace_back();
    mtr_batch::Ver& v = b->vers[0];
    v.npal = palettes ? (uint32_t)npal : 0;
    if (texture_override) {
        b->tex_override.assign(texture_override, texture_override + n);
        for (int32_t t : b->tex_override)
            if (t >= (int32_t)model->textures.size()) return fail(d, MTR_E_INVALID, "texture_override out of range");
    }
    int32_t rc = set_device(d);
    if (rc) return rc;
    v.cap = n * 16 * (1 + (size_t)v.npal);
    if ((rc = dev_alloc(d, &v.d, v.cap))) return rc;
    // uploads go through the copy stream and an event: creating a batch does not wait for frames in flight
    HIPCHK(d, hipMemcpyAsync(v.d, model_mats, n * 64, hipMemcpyHostToDevice, d->s_copy));
    if (v.npal) HIPCHK(d, hipMemcpyAsync(v.d + n * 16, palettes, n * npal * 64, hipMemcpyHostToDevice, d->s_copy));
    HIPCHK(d, hipEventCreateWithFlags(&v.ready, hipEventDisableTiming));
    HIPCHK(d, hipEventRecord(v.ready, d->s_copy));
    *out = b.release();
    return MTR_OK;
}

void mtr_batch_destroy(mtr_batch* b) {
    if (!b) return;
    mtr_device* d = b->dev;
    (void)hipSetDevice(d->hip_dev);
    // a frame that drew the batch may still be in flight, or be re-run: the versions its draws recorded stay until those
    // frames are destroyed (their references), then they are parked until that frame has left the GPU (collected at a
    // later submit), as is a version a pose kernel or copy may still be writing.  No stream is drained either way.  The
    // exchange thread destroys the batches its frames own while the render thread submits: submit_mu guards the list.
    FreeList fl;
    {
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        batch_unref(b, fl);
    }
    release_now(fl);
}

int32_t mtr_batch_update(mtr_batch* b, const float* model_mats, const float* palettes, size_t npal) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (palettes && (npal == 0 || npal > 256)) return fail(d, MTR_E_INVALID, "batch update: 1 to 256 palette matrices per instance");
    if (!model_mats && !palettes) return MTR_OK;
    int32_t rc = set_device(d);
    if (rc) return rc;
    return batch_write_version(b, model_mats, palettes, (uint32_t)npal, PoseSrc{}, d->s_copy);
}

int32_t mtr_batch_set_poses(mtr_batch* b, const float* local_mats, size_t njoints) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!local_mats) return fail(d, MTR_E_INVALID, "pose: no local matrices");
    int32_t rc = check_batch_pose(b, njoints);
    if (rc) return rc;
    if ((rc = stage_pose(d, local_mats, (size_t)b->n * njoints * 16))) return rc;
    PoseSrc src;
    src.locals = d->pose_stage;
    return batch_write_version(b, nullptr, nullptr, (uint32_t)njoints, src, d->s_copy);
}

int32_t mtr_batch_set_poses_device(mtr_batch* b, const float* local_mats_dev, size_t njoints, void* hip_stream) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!local_mats_dev || ((uintptr_t)local_mats_dev & 15u)) return fail(d, MTR_E_INVALID, "pose: device matrices must be 16-byte aligned");
    int32_t rc = check_batch_pose(b, njoints);
    if (rc) return rc;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : d->stream;
    PoseSrc src;
    src.locals = local_mats_dev;
    return batch_write_version(b, nullptr, nullptr, (uint32_t)njoints, src, s);
}

// ---------------------------------------------------------------------------------------------
// animation clips (SPEC.md section 14)
// ---------------------------------------------------------------------------------------------
int32_t mtr_anim_create(mtr_device* d, size_t njoints, size_t nclips, const uint32_t* nkeys, const uint32_t* flags,
                        const mtr_anim_key* keys, mtr_anim** out) {
    if (!d || !out) return MTR_E_INVALID;
    *out = nullptr;
    if (njoints == 0 || njoints > MTR_POSE_MAX_JOINTS) return fail(d, MTR_E_INVALID, "anim: 1 to 256 joints");
    if (nclips == 0 || nclips > 0xFFFFFFu || !nkeys || !keys) return fail(d, MTR_E_INVALID, "anim: at least one clip, its key counts and keys");
    std::vector<uint32_t> table(nclips * 4);
    uint64_t total = 0;
    for (size_t c = 0; c < nclips; c++) {
        // key counts are exact in binary32 (the position arithmetic of section 14)
        if (nkeys[c] == 0 || nkeys[c] > (1u << 24)) return fail(d, MTR_E_INVALID, "anim: a clip has 1 to 16 777 216 keys");
        table[c * 4 + 0] = (uint32_t)total;
        table[c * 4 + 1] = nkeys[c];
        table[c * 4 + 2] = flags ? flags[c] : 0u;
        table[c * 4 + 3] = 0u;
        total += nkeys[c];
        if (total * njoints > 0x3FFFFFFu) return fail(d, MTR_E_INVALID, "anim: more than 2^26 joint keys");
    }
    int32_t rc = set_device(d);
    if (rc) return rc;
    auto a = std::make_unique<mtr_anim>();
    a->dev = d; a->njoints = (uint32_t)njoints; a->nclips = (uint32_t)nclips;
    for (size_t c = 0; c < nclips; c++) a->has_loop |= (table[c * 4 + 2] & MTR_CLIP_LOOP) != 0;
    const size_t key_words = (size_t)total * njoints * 12;
    if ((rc = dev_alloc(d, &a->d, table.size() + key_words))) return rc;
    hipError_t e = hipMemcpy(a->d, table.data(), table.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a->d + table.size(), keys, key_words * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&a->last, hipEventDisableTiming);
    if (e != hipSuccess) { (void)hipFree(a->d); return fail(d, MTR_E_HIP, std::string("anim upload: ") + hipGetErrorString(e)); }
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
    // device layout: the clip table (0, ticks, flags, 0), the descriptors (32 bytes, a joint's three together), the
    // values (8 bytes each), the times (dense u16)
    const size_t ntracks = nclips * njoints * 3;
    std::vector<uint32_t> table(nclips * 4, 0u);
    for (size_t c = 0; c < nclips; c++) {
        table[c * 4 + 1] = nticks[c];
        table[c * 4 + 2] = flags ? flags[c] : 0u;
    }
    static_assert(sizeof(mtr_anim_track) == 32, "mtr_anim_track");
    auto a = std::make_unique<mtr_anim>();
    a->dev = d; a->njoints = (uint32_t)njoints; a->nclips = (uint32_t)nclips;
    a->tracks = true; a->nkeys = (uint32_t)nkeys_total;
    for (size_t c = 0; c < nclips; c++) a->has_loop |= (table[c * 4 + 2] & MTR_CLIP_LOOP) != 0;
    const size_t time_words = (nkeys_total + 1) / 2;
    if ((rc = dev_alloc(d, &a->d, table.size() + ntracks * 8 + nkeys_total * 2 + time_words))) return rc;
    uint32_t* p = a->d;
    hipError_t e = hipMemcpy(p, table.data(), table.size() * 4, hipMemcpyHostToDevice);
    p += table.size();
    if (e == hipSuccess) e = hipMemcpy(p, tracks, ntracks * 32, hipMemcpyHostToDevice);
    p += ntracks * 8;
    if (e == hipSuccess) e = hipMemcpy(p, values, nkeys_total * 8, hipMemcpyHostToDevice);
    p += nkeys_total * 2;
    if (e == hipSuccess) e = hipMemcpy(p, times, nkeys_total * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&a->last, hipEventDisableTiming);
    if (e != hipSuccess) { (void)hipFree(a->d); return fail(d, MTR_E_HIP, std::string("anim upload: ") + hipGetErrorString(e)); }
    *out = a.release();
    return MTR_OK;
}

void mtr_anim_destroy(mtr_anim* a) {
    if (!a) return;
    mtr_device* d = a->dev;
    {
        // a kernel may still read the clip set: parked behind the event of the last one, collected by a later submit
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        d->garbage.push_back({a->d, 0, a->last});
    }
    delete a;
}

int32_t mtr_model_animate(mtr_model* m, mtr_anim* a, const mtr_anim_state* state) {
    if (!m) return MTR_E_INVALID;
    mtr_device* d = m->dev;
    if (!state) return fail(d, MTR_E_INVALID, "animate: no state");
    int32_t rc = check_anim(d, m, a);
    if (rc) return rc;
    if ((rc = stage_pose(d, reinterpret_cast<const float*>(state), sizeof(mtr_anim_state) / sizeof(float)))) return rc;
    std::lock_guard<std::mutex> submit_lock(d->submit_mu);
    mtr_model::PalBuf* pb = nullptr;
    if ((rc = next_palette_buffer(m, a->njoints, &pb))) return rc;
    if ((rc = anim_before(a, d->s_copy))) return rc;
    launch_anim(a, anim_params(a, m->skel, d->pose_stage, pb->d), 1, d->s_copy);
    HIPCHK(d, hipGetLastError());
    if ((rc = anim_after(a, d->s_copy))) return rc;
    HIPCHK(d, hipEventRecord(pb->ready, d->s_copy));
    return MTR_OK;
}

int32_t mtr_batch_animate(mtr_batch* b, mtr_anim* a, const mtr_anim_state* states) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!states) return fail(d, MTR_E_INVALID, "animate: no states");
    int32_t rc = check_anim(d, b->model, a);
    if (rc) return rc;
    if ((rc = stage_pose(d, reinterpret_cast<const float*>(states), (size_t)b->n * (sizeof(mtr_anim_state) / sizeof(float))))) return rc;
    PoseSrc src;
    src.anim = a; src.states = d->pose_stage;
    return batch_write_version(b, nullptr, nullptr, a->njoints, src, d->s_copy);
}

int32_t mtr_batch_animate_device(mtr_batch* b, mtr_anim* a, const mtr_anim_state* states_dev, void* hip_stream) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!states_dev || ((uintptr_t)states_dev & 7u)) return fail(d, MTR_E_INVALID, "animate: device states must be 8-byte aligned");
    int32_t rc = check_anim(d, b->model, a);
    if (rc) return rc;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : d->stream;
    PoseSrc src;
    src.anim = a; src.states = states_dev;
    return batch_write_version(b, nullptr, nullptr, a->njoints, src, s);
}

int32_t mtr_anim_sample(mtr_anim* a, const mtr_anim_state* states, size_t n, float* out_locals, size_t count) {
    if (!a) return MTR_E_INVALID;
    mtr_device* d = a->dev;
    const size_t need = n * a->njoints * 16;
    if (n > 0xFFFFFFu || (n && (!states || !out_locals)) || count < need) return fail(d, MTR_E_INVALID, "anim sample: n states and room for n * njoints * 16 floats");
    if (!(a->tracks ? mtr_launch_anim_tracks_sample : mtr_launch_anim_sample)) return fail(d, MTR_E_UNSUPPORTED, "anim sample: built without k_anim");
    int32_t rc = set_device(d);
    if (rc || !n) return rc;
    float* tmp = nullptr;  // the local matrices, then the states
    if ((rc = dev_alloc(d, &tmp, need + n * 6))) return rc;
    auto run = [&]() -> int32_t {
        HIPCHK(d, hipMemcpyAsync(tmp + need, states, n * sizeof(mtr_anim_state), hipMemcpyHostToDevice, d->s_copy));
        AnimParams ap = anim_params(a, mtr_model::Skeleton{}, tmp + need, tmp);
        ap.pose.njoints = a->njoints;
        if (a->tracks) mtr_launch_anim_tracks_sample(ap, (uint32_t)n, d->s_copy);
        else mtr_launch_anim_sample(ap, (uint32_t)n, d->s_copy);
        HIPCHK(d, hipGetLastError());
        HIPCHK(d, hipMemcpyAsync(out_locals, tmp, need * sizeof(float), hipMemcpyDeviceToHost, d->s_copy));
        return MTR_OK;
    };
    rc = run();
    const hipError_t e = hipStreamSynchronize(d->s_copy);  // also when a step failed: the buffer is freed next
    (void)hipFree(tmp);
    if (!rc && e != hipSuccess) rc = fail(d, MTR_E_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    return rc;
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
    if ((rc = dev_alloc(d, &mk->d, nmasks * njoints))) return rc;
    hipError_t e = hipMemcpy(mk->d, weights, nmasks * njoints * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&mk->last, hipEventDisableTiming);
    if (e != hipSuccess) { (void)hipFree(mk->d); return fail(d, MTR_E_HIP, std::string("anim masks upload: ") + hipGetErrorString(e)); }
    *out = mk.release();
    return MTR_OK;
}

void mtr_anim_masks_destroy(mtr_anim_masks* mk) {
    if (!mk) return;
    mtr_device* d = mk->dev;
    {
        // a kernel may still read the weights: parked behind the event of the last one, collected by a later submit
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        d->garbage.push_back({mk->d, 0, mk->last});
    }
    delete mk;
}

int32_t mtr_model_animate_layers(mtr_model* m, mtr_anim* a, mtr_anim_masks* mk, const mtr_anim_layer* layers, size_t nlayers) {
    if (!m) return MTR_E_INVALID;
    mtr_device* d = m->dev;
    if (!layers) return fail(d, MTR_E_INVALID, "animate layers: no layers");
    int32_t rc = check_anim_layers(d, m, a, mk, nlayers);
    if (rc) return rc;
    if ((rc = stage_pose(d, reinterpret_cast<const float*>(layers), nlayers * (sizeof(mtr_anim_layer) / sizeof(float))))) return rc;
    std::lock_guard<std::mutex> submit_lock(d->submit_mu);
    mtr_model::PalBuf* pb = nullptr;
    if ((rc = next_palette_buffer(m, a->njoints, &pb))) return rc;
    if ((rc = anim_before(a, d->s_copy))) return rc;
    if (mk && (rc = anim_before(mk, d->s_copy))) return rc;
    launch_anim_layers(a, anim_layer_params(a, mk, m->skel, d->pose_stage, (uint32_t)nlayers, pb->d), 1, d->s_copy);
    HIPCHK(d, hipGetLastError());
    if ((rc = anim_after(a, d->s_copy))) return rc;
    if (mk && (rc = anim_after(mk, d->s_copy))) return rc;
    HIPCHK(d, hipEventRecord(pb->ready, d->s_copy));
    return MTR_OK;
}

int32_t mtr_batch_animate_layers(mtr_batch* b, mtr_anim* a, mtr_anim_masks* mk, const mtr_anim_layer* layers, size_t nlayers) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!layers) return fail(d, MTR_E_INVALID, "animate layers: no layers");
    int32_t rc = check_anim_layers(d, b->model, a, mk, nlayers);
    if (rc) return rc;
    if ((rc = stage_pose(d, reinterpret_cast<const float*>(layers), (size_t)b->n * nlayers * (sizeof(mtr_anim_layer) / sizeof(float))))) return rc;
    PoseSrc src;
    src.anim = a; src.states = d->pose_stage; src.masks = mk; src.nlayers = (uint32_t)nlayers;
    return batch_write_version(b, nullptr, nullptr, a->njoints, src, d->s_copy);
}

int32_t mtr_batch_animate_layers_device(mtr_batch* b, mtr_anim* a, mtr_anim_masks* mk, const mtr_anim_layer* layers_dev, size_t nlayers, void* hip_stream) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!layers_dev || ((uintptr_t)layers_dev & 15u)) return fail(d, MTR_E_INVALID, "animate layers: device layers must be 16-byte aligned");
    int32_t rc = check_anim_layers(d, b->model, a, mk, nlayers);
    if (rc) return rc;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : d->stream;
    PoseSrc src;
    src.anim = a; src.states = layers_dev; src.masks = mk; src.nlayers = (uint32_t)nlayers;
    return batch_write_version(b, nullptr, nullptr, a->njoints, src, s);
}

int32_t mtr_anim_sample_layers(mtr_anim* a, mtr_anim_masks* mk, const mtr_anim_layer* layers, size_t nlayers, size_t n, float* out_locals, size_t count) {
    if (!a) return MTR_E_INVALID;
    mtr_device* d = a->dev;
    if (nlayers < 1 || nlayers > MTR_ANIM_MAX_LAYERS) return fail(d, MTR_E_INVALID, "anim sample layers: 1 to 8 layers per instance");
    if (mk && (mk->dev != d || mk->njoints != a->njoints)) return fail(d, MTR_E_INVALID, "anim sample layers: the mask set is of another device or joint count");
    const size_t need = n * a->njoints * 16;
    if (n > 0xFFFFFFu || (n && (!layers || !out_locals)) || count < need)
        return fail(d, MTR_E_INVALID, "anim sample layers: n * nlayers layers and room for n * njoints * 16 floats");
    if (!(a->tracks ? mtr_launch_anim_layers_tracks_sample : mtr_launch_anim_layers_sample)) return fail(d, MTR_E_UNSUPPORTED, "anim sample layers: built without k_anim_layers");
    int32_t rc = set_device(d);
    if (rc || !n) return rc;
    float* tmp = nullptr;  // the local matrices, then the layers (need is a multiple of 16 floats: 16-byte aligned)
    if ((rc = dev_alloc(d, &tmp, need + n * nlayers * 4))) return rc;
    auto run = [&]() -> int32_t {
        HIPCHK(d, hipMemcpyAsync(tmp + need, layers, n * nlayers * sizeof(mtr_anim_layer), hipMemcpyHostToDevice, d->s_copy));
        AnimLayerParams lp = anim_layer_params(a, mk, mtr_model::Skeleton{}, tmp + need, (uint32_t)nlayers, tmp);
        lp.anim.pose.njoints = a->njoints;
        if (a->tracks) mtr_launch_anim_layers_tracks_sample(lp, (uint32_t)n, d->s_copy);
        else mtr_launch_anim_layers_sample(lp, (uint32_t)n, d->s_copy);
        HIPCHK(d, hipGetLastError());
        HIPCHK(d, hipMemcpyAsync(out_locals, tmp, need * sizeof(float), hipMemcpyDeviceToHost, d->s_copy));
        return MTR_OK;
    };
    rc = run();
    const hipError_t e = hipStreamSynchronize(d->s_copy);  // also when a step failed: the buffer is freed next
    (void)hipFree(tmp);
    if (!rc && e != hipSuccess) rc = fail(d, MTR_E_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    return rc;
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
    if ((rc = dev_alloc(d, &ik->d, img.size()))) return rc;
    hipError_t e = hipMemcpy(ik->d, img.data(), img.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ik->last, hipEventDisableTiming);
    if (e != hipSuccess) { (void)hipFree(ik->d); return fail(d, MTR_E_HIP, std::string("anim ik upload: ") + hipGetErrorString(e)); }
    *out = ik.release();
    return MTR_OK;
}

void mtr_anim_ik_destroy(mtr_anim_ik* ik) {
    if (!ik) return;
    mtr_device* d = ik->dev;
    {
        // a kernel may still read the chains: parked behind the event of the last one, collected by a later submit
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        d->garbage.push_back({ik->d, 0, ik->last});
    }
    delete ik;
}

int32_t mtr_model_animate_ik(mtr_model* m, mtr_anim* a, mtr_anim_masks* mk, const mtr_anim_layer* layers, size_t nlayers, mtr_anim_ik* ik,
                             const mtr_ik_target* targets) {
    if (!m) return MTR_E_INVALID;
    mtr_device* d = m->dev;
    if (!layers) return fail(d, MTR_E_INVALID, "animate ik: no layers");
    if (!targets) return fail(d, MTR_E_INVALID, "animate ik: no targets");
    int32_t rc = check_anim_ik(d, m, a, mk, nlayers, ik);
    if (rc) return rc;
    const void* tg = nullptr;
    if ((rc = stage_ik(d, layers, nlayers, targets, ik->nchains, &tg))) return rc;
    std::lock_guard<std::mutex> submit_lock(d->submit_mu);
    mtr_model::PalBuf* pb = nullptr;
    if ((rc = next_palette_buffer(m, a->njoints, &pb))) return rc;
    if ((rc = anim_before(a, d->s_copy))) return rc;
    if (mk && (rc = anim_before(mk, d->s_copy))) return rc;
    if ((rc = anim_before(ik, d->s_copy))) return rc;
    launch_anim_ik(a, anim_ik_params(a, mk, m->skel, d->pose_stage, (uint32_t)nlayers, ik, tg, pb->d), 1, d->s_copy);
    HIPCHK(d, hipGetLastError());
    if ((rc = anim_after(a, d->s_copy))) return rc;
    if (mk && (rc = anim_after(mk, d->s_copy))) return rc;
    if ((rc = anim_after(ik, d->s_copy))) return rc;
    HIPCHK(d, hipEventRecord(pb->ready, d->s_copy));
    return MTR_OK;
}

int32_t mtr_batch_animate_ik(mtr_batch* b, mtr_anim* a, mtr_anim_masks* mk, const mtr_anim_layer* layers, size_t nlayers, mtr_anim_ik* ik,
                             const mtr_ik_target* targets) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!layers) return fail(d, MTR_E_INVALID, "animate ik: no layers");
    if (!targets) return fail(d, MTR_E_INVALID, "animate ik: no targets");
    int32_t rc = check_anim_ik(d, b->model, a, mk, nlayers, ik);
    if (rc) return rc;
    PoseSrc src;
    if ((rc = stage_ik(d, layers, (size_t)b->n * nlayers, targets, (size_t)b->n * ik->nchains, &src.targets))) return rc;
    src.anim = a; src.states = d->pose_stage; src.masks = mk; src.nlayers = (uint32_t)nlayers; src.ik = ik;
    return batch_write_version(b, nullptr, nullptr, a->njoints, src, d->s_copy);
}

int32_t mtr_batch_animate_ik_device(mtr_batch* b, mtr_anim* a, mtr_anim_masks* mk, const mtr_anim_layer* layers_dev, size_t nlayers, mtr_anim_ik* ik,
                                    const mtr_ik_target* targets_dev, void* hip_stream) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!layers_dev || ((uintptr_t)layers_dev & 15u)) return fail(d, MTR_E_INVALID, "animate ik: device layers must be 16-byte aligned");
    if (!targets_dev || ((uintptr_t)targets_dev & 15u)) return fail(d, MTR_E_INVALID, "animate ik: device targets must be 16-byte aligned");
    int32_t rc = check_anim_ik(d, b->model, a, mk, nlayers, ik);
    if (rc) return rc;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : d->stream;
    PoseSrc src;
    src.anim = a; src.states = layers_dev; src.masks = mk; src.nlayers = (uint32_t)nlayers; src.ik = ik; src.targets = targets_dev;
    return batch_write_version(b, nullptr, nullptr, a->njoints, src, s);
}

int32_t mtr_anim_sample_ik(mtr_anim* a, mtr_anim_masks* mk, mtr_anim_ik* ik, const mtr_anim_layer* layers, size_t nlayers, const mtr_ik_target* targets,
                           size_t n, float* out_locals, size_t count) {
    if (!a) return MTR_E_INVALID;
    mtr_device* d = a->dev;
    if (nlayers < 1 || nlayers > MTR_ANIM_MAX_LAYERS) return fail(d, MTR_E_INVALID, "anim sample ik: 1 to 8 layers per instance");
    if (mk && (mk->dev != d || mk->njoints != a->njoints)) return fail(d, MTR_E_INVALID, "anim sample ik: the mask set is of another device or joint count");
    if (!ik || ik->dev != d || ik->njoints != a->njoints) return fail(d, MTR_E_INVALID, "anim sample ik: an IK set of this device and joint count");
    const size_t need = n * a->njoints * 16;
    if (n > 0xFFFFFFu || (n && (!layers || !targets || !out_locals)) || count < need)
        return fail(d, MTR_E_INVALID, "anim sample ik: n * nlayers layers, n * nchains targets and room for n * njoints * 16 floats");
    if (!(a->tracks ? mtr_launch_anim_ik_tracks_sample : mtr_launch_anim_ik_sample)) return fail(d, MTR_E_UNSUPPORTED, "anim sample ik: built without k_anim_ik");
    int32_t rc = set_device(d);
    if (rc || !n) return rc;
    float* tmp = nullptr;  // the local matrices, the layers, the targets (each a multiple of 16 bytes)
    const size_t lw = n * nlayers * 4, tw = n * ik->nchains * 8;
    if ((rc = dev_alloc(d, &tmp, need + lw + tw))) return rc;
    auto run = [&]() -> int32_t {
        HIPCHK(d, hipMemcpyAsync(tmp + need, layers, lw * sizeof(float), hipMemcpyHostToDevice, d->s_copy));
        HIPCHK(d, hipMemcpyAsync(tmp + need + lw, targets, tw * sizeof(float), hipMemcpyHostToDevice, d->s_copy));
        AnimIkParams ip = anim_ik_params(a, mk, mtr_model::Skeleton{}, tmp + need, (uint32_t)nlayers, ik, tmp + need + lw, tmp);
        ip.layers.anim.pose.njoints = a->njoints;
        if (a->tracks) mtr_launch_anim_ik_tracks_sample(ip, (uint32_t)n, d->s_copy);
        else mtr_launch_anim_ik_sample(ip, (uint32_t)n, d->s_copy);
        HIPCHK(d, hipGetLastError());
        HIPCHK(d, hipMemcpyAsync(out_locals, tmp, need * sizeof(float), hipMemcpyDeviceToHost, d->s_copy));
        return MTR_OK;
    };
    rc = run();
    const hipError_t e = hipStreamSynchronize(d->s_copy);  // also when a step failed: the buffer is freed next
    (void)hipFree(tmp);
    if (!rc && e != hipSuccess) rc = fail(d, MTR_E_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    return rc;
}

// ---------------------------------------------------------------------------------------------
// attachments (SPEC.md section 18)
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(mtr_attach) == 80 && sizeof(mtr_attach) == MTR_ATTACH_WORDS * 4, "mtr_attach");

int32_t mtr_batch_attach(mtr_batch* b, mtr_batch* src, const mtr_attach* recs) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!src || !recs) return fail(d, MTR_E_INVALID, "attach: no source batch or no records");
    if (src->dev != d) return fail(d, MTR_E_INVALID, "attach: the source batch belongs to another device");
    if (!mtr_launch_attach) return fail(d, MTR_E_UNSUPPORTED, "attach: built without k_attach");
    int32_t rc = set_device(d);
    if (rc) return rc;
    if ((rc = stage_pose(d, reinterpret_cast<const float*>(recs), (size_t)b->n * MTR_ATTACH_WORDS))) return rc;
    const AttachSrc at{src, d->pose_stage};
    return batch_write_version(b, nullptr, nullptr, 0, PoseSrc{}, d->s_copy, &at);
}

int32_t mtr_batch_attach_device(mtr_batch* b, mtr_batch* src, const mtr_attach* recs_dev, void* hip_stream) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!src) return fail(d, MTR_E_INVALID, "attach: no source batch");
    if (!recs_dev || ((uintptr_t)recs_dev & 15u)) return fail(d, MTR_E_INVALID, "attach: device records must be 16-byte aligned");
    if (src->dev != d) return fail(d, MTR_E_INVALID, "attach: the source batch belongs to another device");
    if (!mtr_launch_attach) return fail(d, MTR_E_UNSUPPORTED, "attach: built without k_attach");
    int32_t rc = set_device(d);
    if (rc) return rc;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : d->stream;
    const AttachSrc at{src, recs_dev};
    return batch_write_version(b, nullptr, nullptr, 0, PoseSrc{}, s, &at);
}

int32_t mtr_batch_sockets_device(mtr_batch* src, const mtr_attach* recs_dev, size_t n, float* out_dev, void* hip_stream) {
    if (!src) return MTR_E_INVALID;
    mtr_device* d = src->dev;
    if (!recs_dev || ((uintptr_t)recs_dev & 15u) || !out_dev || ((uintptr_t)out_dev & 15u))
        return fail(d, MTR_E_INVALID, "sockets: device records and matrices must be 16-byte aligned");
    if (n == 0 || n > (1u << 27)) return fail(d, MTR_E_INVALID, "sockets: 1 to 2^27 records");
    if (!mtr_launch_attach) return fail(d, MTR_E_UNSUPPORTED, "sockets: built without k_attach");
    int32_t rc = set_device(d);
    if (rc) return rc;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : d->stream;
    SrcRead rd;
    {
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        src_read_pin(src, rd);
    }
    rc = src_read_launch(rd, recs_dev, n, out_dev, s);
    std::lock_guard<std::mutex> submit_lock(d->submit_mu);
    src_read_unpin(rd, s);
    return rc;
}

int32_t mtr_batch_sockets(mtr_batch* src, const mtr_attach* recs, size_t n, float* out, size_t count) {
    if (!src) return MTR_E_INVALID;
    mtr_device* d = src->dev;
    if (!recs || !out) return fail(d, MTR_E_INVALID, "sockets: no records or no room for the matrices");
    if (n == 0 || n > (1u << 27) || count < n * 16) return fail(d, MTR_E_INVALID, "sockets: 1 to 2^27 records and room for n * 16 floats");
    if (!mtr_launch_attach) return fail(d, MTR_E_UNSUPPORTED, "sockets: built without k_attach");
    int32_t rc = set_device(d);
    if (rc) return rc;
    float* tmp = nullptr;  // the matrices, then the records (n * 64 bytes in: 16-byte aligned)
    if ((rc = dev_alloc(d, &tmp, n * 16 + n * MTR_ATTACH_WORDS))) return rc;
    SrcRead rd;
    {
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        src_read_pin(src, rd);
    }
    auto run = [&]() -> int32_t {
        HIPCHK(d, hipMemcpyAsync(tmp + n * 16, recs, n * sizeof(mtr_attach), hipMemcpyHostToDevice, d->s_copy));
        int32_t r2 = src_read_launch(rd, tmp + n * 16, n, tmp, d->s_copy);
        if (r2) return r2;
        HIPCHK(d, hipMemcpyAsync(out, tmp, n * 64, hipMemcpyDeviceToHost, d->s_copy));
        return MTR_OK;
    };
    rc = run();
    const hipError_t e = hipStreamSynchronize(d->s_copy);  // also when a step failed: the buffer is freed next
    (void)hipFree(tmp);
    {
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        src_read_unpin(rd, d->s_copy);
    }
    if (!rc && e != hipSuccess) rc = fail(d, MTR_E_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    return rc;
}

// ---------------------------------------------------------------------------------------------
// root motion (SPEC.md section 19)
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
    if ((rc = dev_alloc(d, &r->d, img.size()))) return rc;
    hipError_t e = hipMemcpy(r->d, img.data(), img.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->last, hipEventDisableTiming);
    if (e != hipSuccess) { (void)hipFree(r->d); return fail(d, MTR_E_HIP, std::string("anim root upload: ") + hipGetErrorString(e)); }
    *out = r.release();
    return MTR_OK;
}

void mtr_anim_root_destroy(mtr_anim_root* r) {
    if (!r) return;
    mtr_device* d = r->dev;
    {
        // a kernel may still read the flags: parked behind the event of the last one, collected by a later submit
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        d->garbage.push_back({r->d, 0, r->last});
    }
    delete r;
}

// what every root-motion call checks of its trajectory set, root set and step count
static int32_t check_root(mtr_device* d, const mtr_anim* traj, const mtr_anim_root* root, size_t nsteps, bool deltas) {
    if (!root) return fail(d, MTR_E_INVALID, "root motion: no root set");
    if (traj->dev != d || root->dev != d) return fail(d, MTR_E_INVALID, "root motion: the trajectory set or the root set belongs to another device");
    if (root->njoints != traj->njoints || root->nclips != traj->nclips)
        return fail(d, MTR_E_INVALID, "root motion: the root set's joint or clip count is not the trajectory set's");
    if (traj->has_loop) return fail(d, MTR_E_INVALID, "root motion: the trajectory set has a MTR_CLIP_LOOP clip (mark it MTR_ROOT_CYCLIC in the root set instead)");
    if (nsteps < 1 || nsteps > MTR_ROOT_MAX_STEPS) return fail(d, MTR_E_INVALID, "root motion: 1 to 8 steps per instance");
    if (!(deltas ? mtr_launch_root_deltas : mtr_launch_root)) return fail(d, MTR_E_UNSUPPORTED, "root motion: built without k_root");
    return set_device(d);
}

int32_t mtr_batch_root_motion(mtr_batch* b, mtr_anim* traj, mtr_anim_root* root, const mtr_root_step* steps, size_t nsteps) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!traj || !steps) return fail(d, MTR_E_INVALID, "root motion: no trajectory set or no steps");
    int32_t rc = check_root(d, traj, root, nsteps, false);
    if (rc) return rc;
    if ((rc = stage_pose(d, reinterpret_cast<const float*>(steps), (size_t)b->n * nsteps * 4))) return rc;
    const RootSrc rs{traj, root, (uint32_t)nsteps};
    const AttachSrc at{b, d->pose_stage, &rs};
    return batch_write_version(b, nullptr, nullptr, 0, PoseSrc{}, d->s_copy, &at);
}

int32_t mtr_batch_root_motion_device(mtr_batch* b, mtr_anim* traj, mtr_anim_root* root, const mtr_root_step* steps_dev, size_t nsteps, void* hip_stream) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!traj) return fail(d, MTR_E_INVALID, "root motion: no trajectory set");
    if (!steps_dev || ((uintptr_t)steps_dev & 15u)) return fail(d, MTR_E_INVALID, "root motion: device steps must be 16-byte aligned");
    int32_t rc = check_root(d, traj, root, nsteps, false);
    if (rc) return rc;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : d->stream;
    const RootSrc rs{traj, root, (uint32_t)nsteps};
    const AttachSrc at{b, steps_dev, &rs};
    return batch_write_version(b, nullptr, nullptr, 0, PoseSrc{}, s, &at);
}

int32_t mtr_anim_root_deltas_device(mtr_anim* traj, mtr_anim_root* root, const mtr_root_step* steps_dev, size_t nsteps, size_t n, float* out_dev,
                                    void* hip_stream) {
    if (!traj) return MTR_E_INVALID;
    mtr_device* d = traj->dev;
    if (!steps_dev || ((uintptr_t)steps_dev & 15u) || !out_dev || ((uintptr_t)out_dev & 15u))
        return fail(d, MTR_E_INVALID, "root deltas: device steps and matrices must be 16-byte aligned");
    if (n == 0 || n > (1u << 27)) return fail(d, MTR_E_INVALID, "root deltas: 1 to 2^27 instances");
    int32_t rc = check_root(d, traj, root, nsteps, true);
    if (rc) return rc;
    hipStream_t s = hip_stream ? static_cast<hipStream_t>(hip_stream) : d->stream;
    if ((rc = anim_before(traj, s)) || (rc = anim_before(root, s))) return rc;
    mtr_launch_root_deltas(root_params(traj, root, steps_dev, (uint32_t)nsteps, n, nullptr, out_dev), s);
    HIPCHK(d, hipGetLastError());
    if ((rc = anim_after(traj, s)) || (rc = anim_after(root, s))) return rc;
    return MTR_OK;
}

int32_t mtr_anim_root_deltas(mtr_anim* traj, mtr_anim_root* root, const mtr_root_step* steps, size_t nsteps, size_t n, float* out, size_t count) {
    if (!traj) return MTR_E_INVALID;
    mtr_device* d = traj->dev;
    if (!steps || !out) return fail(d, MTR_E_INVALID, "root deltas: no steps or no room for the matrices");
    if (n == 0 || n > (1u << 27) || count < n * 16) return fail(d, MTR_E_INVALID, "root deltas: 1 to 2^27 instances and room for n * 16 floats");
    int32_t rc = check_root(d, traj, root, nsteps, true);
    if (rc) return rc;
    float* tmp = nullptr;  // the matrices, then the steps (n * 64 bytes in: 16-byte aligned)
    if ((rc = dev_alloc(d, &tmp, n * 16 + n * nsteps * 4))) return rc;
    auto run = [&]() -> int32_t {
        HIPCHK(d, hipMemcpyAsync(tmp + n * 16, steps, n * nsteps * sizeof(mtr_root_step), hipMemcpyHostToDevice, d->s_copy));
        int32_t r2 = anim_before(traj, d->s_copy);
        if (r2 || (r2 = anim_before(root, d->s_copy))) return r2;
        mtr_launch_root_deltas(root_params(traj, root, tmp + n * 16, (uint32_t)nsteps, n, nullptr, tmp), d->s_copy);
        HIPCHK(d, hipGetLastError());
        if ((r2 = anim_after(traj, d->s_copy)) || (r2 = anim_after(root, d->s_copy))) return r2;
        HIPCHK(d, hipMemcpyAsync(out, tmp, n * 64, hipMemcpyDeviceToHost, d->s_copy));
        return MTR_OK;
    };
    rc = run();
    const hipError_t e = hipStreamSynchronize(d->s_copy);  // also when a step failed: the buffer is freed next
    (void)hipFree(tmp);
    if (!rc && e != hipSuccess) rc = fail(d, MTR_E_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    return rc;
}

int32_t mtr_batch_read_model_mats(mtr_batch* b, float* out, size_t count) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    const size_t need = (size_t)b->n * 16;
    if (!out || count < need) return fail(d, MTR_E_INVALID, "read_model_mats: room for n * 16 floats needed");
    mtr_batch::Ver v{};
    {
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        v = b->vers[(size_t)b->cur];
    }
    int32_t rc = set_device(d);
    if (rc) return rc;
    HIPCHK(d, hipStreamWaitEvent(d->s_copy, v.ready, 0));
    HIPCHK(d, hipMemcpyAsync(out, v.d, need * sizeof(float), hipMemcpyDeviceToHost, d->s_copy));
    HIPCHK(d, hipStreamSynchronize(d->s_copy));
    return MTR_OK;
}

int32_t mtr_batch_read_palettes(mtr_batch* b, float* out, size_t count) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    mtr_batch::Ver v{};
    {
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        v = b->vers[(size_t)b->cur];
    }
    const size_t need = (size_t)b->n * v.npal * 16;
    if ((!out && need) || count < need) return fail(d, MTR_E_INVALID, "read_palettes: room for n * npal * 16 floats needed");
    int32_t rc = set_device(d);
    if (rc || !need) return rc;
    HIPCHK(d, hipStreamWaitEvent(d->s_copy, v.ready, 0));
    HIPCHK(d, hipMemcpyAsync(out, v.d + (size_t)b->n * 16, need * sizeof(float), hipMemcpyDeviceToHost, d->s_copy));
    HIPCHK(d, hipStreamSynchronize(d->s_copy));
    return MTR_OK;
}

}  // extern "C"
