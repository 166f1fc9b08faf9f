// host_batch.cpp -- instance batches and their versions: what an update writes into a fresh version (matrices and palettes
// from host arrays, poses, animate calls, attachments, root motion), the staging of host records, sockets and read-backs.
#include "host.h"
#include "attach_math.h"

// k_pose.hip.  Weak: the host-only builds of this file (tests/cpp, over the HIP stub runtime) link no kernels and never
// form a pose; libmtr.so links k_pose.o.
void mtr_launch_pose(const PoseParams& p, uint32_t ninst, hipStream_t s) __attribute__((weak));
// k_attach.hip, weak for the same reason
void mtr_launch_attach(const AttachParams& p, hipStream_t s) __attribute__((weak));

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

PoseParams pose_params(const mtr_model::Skeleton& sk, const float* locals, float* out) {
    PoseParams pp{};
    pp.locals = locals; pp.out = out; pp.imats = sk.d;
    pp.paths = reinterpret_cast<const uint32_t*>(sk.d + (size_t)sk.njoints * 16);
    pp.path_words = reinterpret_cast<const uint32_t*>(sk.d + (size_t)sk.njoints * 17);
    pp.njoints = sk.njoints; pp.path_bytes = sk.path_bytes;
    return pp;
}

namespace {

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

// An outside reader of a batch's current version: a kernel that forms matrices from its instance matrices and palettes --
// k_attach (SPEC.md section 18), or k_root over the batch's own matrices (section 19) -- on a stream the batch's own updates
// need not share.  pin (submit_mu held) takes the current version and keeps batch_next_version off it; launch (no lock: only
// this thread touches a pinned version's events) makes `s` wait for the version's write and, when the reader before ran on
// another stream, for that reader, runs the kernel and records Ver::read behind it; unpin (submit_mu held) publishes the
// event.  The next write into the version waits for it (batch_write_version), and a buffer retired meanwhile is parked
// behind it (retire_version).
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

// kernel(v): queues the reader of version v on s
template <class K>
int32_t src_read_launch(SrcRead& r, hipStream_t s, K&& kernel) {
    mtr_device* d = r.b->dev;
    if (!r.v.read && hipEventCreateWithFlags(&r.v.read, hipEventDisableTiming) != hipSuccess) return fail(d, MTR_E_HIP, "hipEventCreate failed");
    if (r.v.ready) HIPCHK(d, hipStreamWaitEvent(s, r.v.ready, 0));
    if (r.v.read_pending && r.v.read_stream != s) HIPCHK(d, hipStreamWaitEvent(s, r.v.read, 0));
    int32_t rc = kernel(r.v);
    if (rc) return rc;
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

// k_attach: n records (device memory) against version v of src, n matrices out
int32_t attach_launch(const mtr_batch* src, const mtr_batch::Ver& v, const void* recs_dev, size_t n, float* out_dev, hipStream_t s) {
    AttachParams ap{};
    ap.recs = static_cast<const uint32_t*>(recs_dev);
    ap.src_mats = v.d; ap.src_pals = v.d + (size_t)src->n * 16;
    ap.out = out_dev;
    ap.n = (uint32_t)n; ap.n_src = src->n; ap.npal = v.npal;
    mtr_launch_attach(ap, s);
    HIPCHK(src->dev, hipGetLastError());
    return MTR_OK;
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

// Where the instance matrices of a fresh version come from: the current version's (a device copy), a host array, k_attach
// over the current version of `src` with one record per instance (device memory), or k_root over the batch's own current
// matrices with nsteps steps per instance (device memory) -- both outside readers of the version they read (SrcRead)
struct MatSrc {
    enum { kKeep, kHost, kAttach, kRoot } from = kKeep;
    const float* host = nullptr;
    mtr_batch* src = nullptr;
    const void* recs = nullptr;
    mtr_anim* traj = nullptr;
    mtr_anim_root* root = nullptr;
    size_t nsteps = 0;
};

// Where its palettes come from: the current version's (a device copy), a host array of npal per instance, local matrices
// in device memory (k_pose), or an animate call (k_anim*)
struct PalSrc {
    enum { kKeep, kHost, kLocals, kAnim } from = kKeep;
    const float* mats = nullptr;  // the host palettes, or the local matrices
    uint32_t npal = 0;
    AnimCall anim;
};

// What an update writes into a fresh version, enqueued on `s`; the version is made current.
int32_t batch_write_version(mtr_batch* b, const MatSrc& ms, const PalSrc& ps, hipStream_t s) {
    mtr_device* d = b->dev;
    const size_t n = b->n;
    const bool reads = ms.from == MatSrc::kAttach || ms.from == MatSrc::kRoot;
    int vi = -1;
    mtr_batch::Ver cur{}, v{};
    SrcRead rd;
    {
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        cur = b->vers[(size_t)b->cur];
        const uint32_t npal = ps.from == PalSrc::kKeep ? cur.npal : ps.npal;
        hipEvent_t frame_ev = nullptr;
        int32_t rc = batch_next_version(b, npal, &vi, &frame_ev);
        if (rc) return rc;
        mtr_batch::Ver& nv = b->vers[(size_t)vi];
        nv.npal = npal;
        nv.pinned++;  // nobody else takes it while it is being written
        v = nv;
        if (reads) src_read_pin(ms.src, rd);  // the source's current version (b's own when batch == src: never the one written)
        // a frame still on the GPU reads it: the write waits for that frame on the device (the enqueue happens under the
        // lock, before any later frame can record the same ring event)
        if (frame_ev) {
            const hipError_t e = hipStreamWaitEvent(s, frame_ev, 0);
            if (e != hipSuccess) { nv.pinned--; if (reads) src_read_unpin(rd, s); return fail(d, MTR_E_HIP, std::string("hipStreamWaitEvent: ") + hipGetErrorString(e)); }
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
        int32_t erc = MTR_OK;
        switch (ms.from) {
        case MatSrc::kAttach: erc = src_read_launch(rd, s, [&](const mtr_batch::Ver& sv) { return attach_launch(ms.src, sv, ms.recs, n, v.d, s); }); break;
        case MatSrc::kRoot: erc = src_read_launch(rd, s, [&](const mtr_batch::Ver& sv) { return root_enqueue(ms.traj, ms.root, ms.recs, ms.nsteps, n, sv.d, v.d, s); }); break;
        case MatSrc::kHost: HIPCHK(d, hipMemcpyAsync(v.d, ms.host, n * 64, hipMemcpyHostToDevice, s)); break;
        case MatSrc::kKeep: HIPCHK(d, hipMemcpyAsync(v.d, cur.d, n * 64, hipMemcpyDeviceToDevice, s)); break;
        }
        if (erc) return erc;
        float* vp = v.d + n * 16;
        switch (ps.from) {
        case PalSrc::kAnim: erc = anim_enqueue(ps.anim, &b->model->skel, vp, (uint32_t)n, s); break;
        case PalSrc::kLocals:
            mtr_launch_pose(pose_params(b->model->skel, ps.mats, vp), (uint32_t)n, s);
            HIPCHK(d, hipGetLastError());
            break;
        case PalSrc::kHost: HIPCHK(d, hipMemcpyAsync(vp, ps.mats, n * v.npal * 64, hipMemcpyHostToDevice, s)); break;
        case PalSrc::kKeep:
            if (v.npal) HIPCHK(d, hipMemcpyAsync(vp, cur.d + n * 16, n * v.npal * 64, hipMemcpyDeviceToDevice, s));
            break;
        }
        if (erc) return erc;
        HIPCHK(d, hipEventRecord(v.ready, s));
        return MTR_OK;
    };
    if (!rc) rc = enqueue();
    std::lock_guard<std::mutex> submit_lock(d->submit_mu);
    mtr_batch::Ver& nv = b->vers[(size_t)vi];
    nv.d = v.d; nv.cap = v.cap; nv.ready = v.ready;
    if (!rc) nv.read_pending = false;  // the write waited for it
    nv.pinned--;
    if (reads) src_read_unpin(rd, s);
    if (!rc) b->cur = vi;
    return rc;
}

// the palettes of a pose: local matrices in device memory
int32_t batch_pose(mtr_batch* b, const float* locals_dev, size_t njoints, hipStream_t s) {
    PalSrc ps;
    ps.from = PalSrc::kLocals; ps.mats = locals_dev; ps.npal = (uint32_t)njoints;
    return batch_write_version(b, MatSrc{}, ps, s);
}

}  // namespace

// the palettes of an animate call, its records in device memory (host_spring.cpp calls in too)
int32_t batch_animate(mtr_batch* b, const AnimCall& c, hipStream_t s) {
    PalSrc ps;
    ps.from = PalSrc::kAnim; ps.npal = c.anim->njoints; ps.anim = c;
    return batch_write_version(b, MatSrc{}, ps, s);
}

namespace {

// the matrices of an attach call: one record per instance (device memory) against the current version of src
int32_t batch_attach(mtr_batch* b, mtr_batch* src, const void* recs_dev, hipStream_t s) {
    MatSrc ms;
    ms.from = MatSrc::kAttach; ms.src = src; ms.recs = recs_dev;
    return batch_write_version(b, ms, PalSrc{}, s);
}

// the matrices of a root-motion call: the batch's own current ones times the deltas of nsteps steps per instance (device memory)
int32_t batch_root_motion(mtr_batch* b, mtr_anim* traj, mtr_anim_root* root, const void* steps_dev, size_t nsteps, hipStream_t s) {
    MatSrc ms;
    ms.from = MatSrc::kRoot; ms.src = b; ms.recs = steps_dev; ms.traj = traj; ms.root = root; ms.nsteps = nsteps;
    return batch_write_version(b, ms, PalSrc{}, s);
}

// the current version of src, pinned for a socket call (its own lock: no update is in progress here)
void sockets_pin(mtr_batch* src, SrcRead& rd) {
    std::lock_guard<std::mutex> submit_lock(src->dev->submit_mu);
    src_read_pin(src, rd);
}
void sockets_unpin(SrcRead& rd, hipStream_t s) {
    std::lock_guard<std::mutex> submit_lock(rd.b->dev->submit_mu);
    src_read_unpin(rd, s);
}

int32_t check_batch_pose(mtr_batch* b, size_t njoints) {
    mtr_device* d = b->dev;
    if (!b->model->skel.d) return fail(d, MTR_E_INVALID, "pose: the batch's model has no skeleton");
    if (njoints != b->model->skel.njoints) return fail(d, MTR_E_INVALID, "pose: one local matrix per joint of the skeleton");
    if (!mtr_launch_pose) return fail(d, MTR_E_UNSUPPORTED, "pose: built without k_pose");
    return set_device(d);
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
    MatSrc ms;
    PalSrc ps;
    if (model_mats) { ms.from = MatSrc::kHost; ms.host = model_mats; }
    if (palettes) { ps.from = PalSrc::kHost; ps.mats = palettes; ps.npal = (uint32_t)npal; }
    return batch_write_version(b, ms, ps, d->s_copy);
}

int32_t mtr_batch_set_poses(mtr_batch* b, const float* local_mats, size_t njoints) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!local_mats) return fail(d, MTR_E_INVALID, "pose: no local matrices");
    int32_t rc = check_batch_pose(b, njoints);
    if (rc) return rc;
    if ((rc = stage_pose(d, local_mats, (size_t)b->n * njoints * 16))) return rc;
    return batch_pose(b, d->pose_stage, njoints, d->s_copy);
}

int32_t mtr_batch_set_poses_device(mtr_batch* b, const float* local_mats_dev, size_t njoints, void* hip_stream) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!local_mats_dev || ((uintptr_t)local_mats_dev & 15u)) return fail(d, MTR_E_INVALID, "pose: device matrices must be 16-byte aligned");
    int32_t rc = check_batch_pose(b, njoints);
    if (rc) return rc;
    return batch_pose(b, local_mats_dev, njoints, caller_stream(d, hip_stream));
}

// ---------------------------------------------------------------------------------------------
// animate calls (SPEC.md sections 14 to 17): the sets and the kernels are host_anim.cpp's
// ---------------------------------------------------------------------------------------------
int32_t mtr_batch_animate(mtr_batch* b, mtr_anim* a, const mtr_anim_state* states) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!states) return fail(d, MTR_E_INVALID, "animate: no states");
    AnimCall c;
    c.anim = a;
    int32_t rc = anim_check(d, b->model, c);
    if (rc) return rc;
    if ((rc = stage_pose(d, reinterpret_cast<const float*>(states), (size_t)b->n * (sizeof(mtr_anim_state) / sizeof(float))))) return rc;
    c.recs = d->pose_stage;
    return batch_animate(b, c, d->s_copy);
}

int32_t mtr_batch_animate_device(mtr_batch* b, mtr_anim* a, const mtr_anim_state* states_dev, void* hip_stream) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!states_dev || ((uintptr_t)states_dev & 7u)) return fail(d, MTR_E_INVALID, "animate: device states must be 8-byte aligned");
    AnimCall c;
    c.anim = a; c.recs = states_dev;
    int32_t rc = anim_check(d, b->model, c);
    if (rc) return rc;
    return batch_animate(b, c, caller_stream(d, hip_stream));
}

int32_t mtr_batch_animate_layers(mtr_batch* b, mtr_anim* a, mtr_anim_masks* mk, const mtr_anim_layer* layers, size_t nlayers) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!layers) return fail(d, MTR_E_INVALID, "animate layers: no layers");
    AnimCall c;
    c.kind = AnimCall::kLayers; c.anim = a; c.masks = mk; c.nlayers = nlayers;
    int32_t rc = anim_check(d, b->model, c);
    if (rc) return rc;
    if ((rc = stage_pose(d, reinterpret_cast<const float*>(layers), (size_t)b->n * nlayers * (sizeof(mtr_anim_layer) / sizeof(float))))) return rc;
    c.recs = d->pose_stage;
    return batch_animate(b, c, d->s_copy);
}

int32_t mtr_batch_animate_layers_device(mtr_batch* b, mtr_anim* a, mtr_anim_masks* mk, const mtr_anim_layer* layers_dev, size_t nlayers, void* hip_stream) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!layers_dev || ((uintptr_t)layers_dev & 15u)) return fail(d, MTR_E_INVALID, "animate layers: device layers must be 16-byte aligned");
    AnimCall c;
    c.kind = AnimCall::kLayers; c.anim = a; c.masks = mk; c.recs = layers_dev; c.nlayers = nlayers;
    int32_t rc = anim_check(d, b->model, c);
    if (rc) return rc;
    return batch_animate(b, c, caller_stream(d, hip_stream));
}

int32_t mtr_batch_animate_ik(mtr_batch* b, mtr_anim* a, mtr_anim_masks* mk, const mtr_anim_layer* layers, size_t nlayers, mtr_anim_ik* ik,
                             const mtr_ik_target* targets) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!layers) return fail(d, MTR_E_INVALID, "animate ik: no layers");
    if (!targets) return fail(d, MTR_E_INVALID, "animate ik: no targets");
    AnimCall c;
    c.kind = AnimCall::kIk; c.anim = a; c.masks = mk; c.ik = ik; c.nlayers = nlayers;
    int32_t rc = anim_check(d, b->model, c);
    if (rc) return rc;
    if ((rc = stage_ik(d, layers, (size_t)b->n * nlayers, targets, (size_t)b->n * ik->nchains, &c.targets))) return rc;
    c.recs = d->pose_stage;
    return batch_animate(b, c, d->s_copy);
}

int32_t mtr_batch_animate_ik_device(mtr_batch* b, mtr_anim* a, mtr_anim_masks* mk, const mtr_anim_layer* layers_dev, size_t nlayers, mtr_anim_ik* ik,
                                    const mtr_ik_target* targets_dev, void* hip_stream) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!layers_dev || ((uintptr_t)layers_dev & 15u)) return fail(d, MTR_E_INVALID, "animate ik: device layers must be 16-byte aligned");
    if (!targets_dev || ((uintptr_t)targets_dev & 15u)) return fail(d, MTR_E_INVALID, "animate ik: device targets must be 16-byte aligned");
    AnimCall c;
    c.kind = AnimCall::kIk; c.anim = a; c.masks = mk; c.ik = ik; c.recs = layers_dev; c.nlayers = nlayers; c.targets = targets_dev;
    int32_t rc = anim_check(d, b->model, c);
    if (rc) return rc;
    return batch_animate(b, c, caller_stream(d, hip_stream));
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
    return batch_attach(b, src, d->pose_stage, d->s_copy);
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
    return batch_attach(b, src, recs_dev, caller_stream(d, hip_stream));
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
    hipStream_t s = caller_stream(d, hip_stream);
    SrcRead rd;
    sockets_pin(src, rd);
    rc = src_read_launch(rd, s, [&](const mtr_batch::Ver& sv) { return attach_launch(src, sv, recs_dev, n, out_dev, s); });
    sockets_unpin(rd, s);
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
    hipStream_t s = d->s_copy;
    // the matrices, then the records (n * 64 bytes in: 16-byte aligned).  The version is pinned once the scratch is there
    // and stays pinned until the stream has drained.
    SrcRead rd;
    StagedBlock blk(d);
    StagedPart &p_out = blk.part(out, n * 16), &p_recs = blk.part(recs, n * MTR_ATTACH_WORDS);
    rc = blk.run([&]() -> int32_t {
        sockets_pin(src, rd);
        int32_t r2;
        if ((r2 = blk.up({&p_recs})) ||
            (r2 = src_read_launch(rd, s, [&](const mtr_batch::Ver& sv) { return attach_launch(src, sv, p_recs.at, n, p_out.dev<float>(), s); })))
            return r2;
        return blk.down({&p_out});
    });
    if (rd.b) sockets_unpin(rd, s);  // not pinned only where the scratch could not be allocated
    return rc;
}

// ---------------------------------------------------------------------------------------------
// root motion (SPEC.md section 19): the batch's own matrices times the deltas
// ---------------------------------------------------------------------------------------------
int32_t mtr_batch_root_motion(mtr_batch* b, mtr_anim* traj, mtr_anim_root* root, const mtr_root_step* steps, size_t nsteps) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!traj || !steps) return fail(d, MTR_E_INVALID, "root motion: no trajectory set or no steps");
    int32_t rc = root_check(d, traj, root, nsteps, false);
    if (rc) return rc;
    if ((rc = stage_pose(d, reinterpret_cast<const float*>(steps), (size_t)b->n * nsteps * 4))) return rc;
    return batch_root_motion(b, traj, root, d->pose_stage, nsteps, d->s_copy);
}

int32_t mtr_batch_root_motion_device(mtr_batch* b, mtr_anim* traj, mtr_anim_root* root, const mtr_root_step* steps_dev, size_t nsteps, void* hip_stream) {
    if (!b) return MTR_E_INVALID;
    mtr_device* d = b->dev;
    if (!traj) return fail(d, MTR_E_INVALID, "root motion: no trajectory set");
    if (!steps_dev || ((uintptr_t)steps_dev & 15u)) return fail(d, MTR_E_INVALID, "root motion: device steps must be 16-byte aligned");
    int32_t rc = root_check(d, traj, root, nsteps, false);
    if (rc) return rc;
    return batch_root_motion(b, traj, root, steps_dev, nsteps, caller_stream(d, hip_stream));
}

// ---------------------------------------------------------------------------------------------
// read-backs
// ---------------------------------------------------------------------------------------------
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
