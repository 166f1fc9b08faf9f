// host_device.cpp -- the device handle: error state, status words and the sticky overflow error, create / destroy /
// synchronize and the mtr_device_set_* switches.
#include "host.h"

namespace mtr_host {

namespace {

thread_local std::string g_create_error = "";

}  // namespace

std::mutex g_err_mu;

int32_t fail(mtr_device* d, int32_t code, const std::string& msg) {
    std::lock_guard<std::mutex> g(g_err_mu);
    if (d) d->err = msg; else g_create_error = msg;
    return code;
}

int32_t set_device(mtr_device* d) {
    HIPCHK(d, hipSetDevice(d->hip_dev));
    return MTR_OK;
}

// Waits for everything the library has queued: the public stream and every slot stream (frames handed to the exchange
// thread are not waited for by the public stream).  Used before freeing or overwriting what a frame in flight may read.
int32_t drain_all(mtr_device* d) {
    HIPCHK(d, hipStreamSynchronize(d->stream));
    for (uint32_t i = 0; i < d->nslots; i++)
        if (d->slots[i].stream) HIPCHK(d, hipStreamSynchronize(d->slots[i].stream));
    return MTR_OK;
}

// bounded per-bin queues overflowed: later frames get twice the bound (up to 16384 entries per bin, then exact two-pass)
void grow_direct_queues(mtr_device* d) {
    if (d->qcap < 16384) { d->qcap *= 2; d->scap *= 2; }
    else d->direct_enabled = false;
}

namespace {

// A frame nobody waited for raised an overflow flag: its pixels are missing triangles and it is gone.  Latch an error
// for the next API call that can report one, and raise the bounds so the frames that follow fit.  submit_mu held.
void latch_overflow(mtr_device* d, uint32_t flags, uint64_t frame_index) {
    if (flags & 4u) grow_direct_queues(d);
    if (flags & 2u) d->queue_scale = std::min<uint32_t>(d->queue_scale * 2, 1024);
    if (d->sticky_err == MTR_OK) {
        d->sticky_err = MTR_E_OVERFLOW;
        d->sticky_msg = "frame " + std::to_string(frame_index) + " overflowed its bin queues (flags " + std::to_string(flags) +
                        ") and was never waited for: it is missing triangles; queue bounds raised for later frames";
    }
}

}  // namespace

// Looks at status word i if nobody has.  force: the word's frame is known to have left the GPU (a word that is still
// invalid then belongs to a frame without a tile workgroup).  submit_mu held.
void examine_status(mtr_device* d, int i, bool force) {
    if (d->status_checked[i]) return;
    const uint32_t v = status_load(d, i);
    if (!(v & 0x80000000u) && !force) return;
    d->status_checked[i] = true;
    d->status_released[i] = false;
    if (v & 0x7fffffffu) latch_overflow(d, v & 0x7fffffffu, d->status_owner[i]);
}

void poll_released(mtr_device* d) {
    for (uint32_t i = 0; i < d->max_inflight; i++)
        if (d->status_released[i]) examine_status(d, (int)i, false);
}

int32_t report_sticky(mtr_device* d) {
    if (d->sticky_err == MTR_OK) return MTR_OK;
    const int32_t rc = d->sticky_err;
    const std::string msg = d->sticky_msg;
    d->sticky_err = MTR_OK;
    d->sticky_msg.clear();
    return fail(d, rc, msg);
}

}  // namespace mtr_host

using namespace mtr_host;

extern "C" {

int32_t mtr_abi_version(void) { return MTR_ABI_VERSION; }

const char* mtr_last_error(const mtr_device* dev) { return dev ? dev->err.c_str() : g_create_error.c_str(); }

int32_t mtr_device_create_on_stream(int32_t hip_device, void* hip_stream, mtr_device** out) {
    if (!out) return fail(nullptr, MTR_E_INVALID, "out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, MTR_E_HIP, std::string("no HIP device: ") + hipGetErrorString(e));
    if (hip_device < 0 || hip_device >= n) return fail(nullptr, MTR_E_INVALID, "hip_device out of range");
    auto d = std::make_unique<mtr_device>();
    d->hip_dev = hip_device;
    HIPCHK(nullptr, hipSetDevice(hip_device));
    if (hip_stream) {
        d->stream = reinterpret_cast<hipStream_t>(hip_stream);
    } else {
        HIPCHK(nullptr, hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking));
        d->own_stream = true;
    }
    if (const char* e = getenv("MTR_NSLOTS")) {
        const long v = strtol(e, nullptr, 10);
        if (v >= 1 && v <= MTR_MAX_SLOTS) d->nslots = (uint32_t)v;
    }
    for (uint32_t i = 0; i < d->nslots; i++) HIPCHK(nullptr, hipStreamCreateWithFlags(&d->slots[i].stream, hipStreamNonBlocking));
    HIPCHK(nullptr, hipStreamCreateWithFlags(&d->s_copy, hipStreamNonBlocking));
    HIPCHK(nullptr, hipHostMalloc(reinterpret_cast<void**>(&d->status_host), mtr_device::kMaxInflight * sizeof(uint32_t),
                                  hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(nullptr, hipHostGetDevicePointer(reinterpret_cast<void**>(&d->status_dev), d->status_host, 0));
    for (uint32_t i = 0; i < mtr_device::kMaxInflight; i++) { d->status_host[i] = 0x80000000u; d->status_checked[i] = true; }
    HIPCHK(nullptr, hipHostMalloc(reinterpret_cast<void**>(&d->hint_host), mtr_device::kHintSlots * 2 * sizeof(uint32_t),
                                  hipHostMallocMapped | hipHostMallocCoherent));
    HIPCHK(nullptr, hipHostGetDevicePointer(reinterpret_cast<void**>(&d->hint_dev), d->hint_host, 0));
    memset(d->hint_host, 0, mtr_device::kHintSlots * 2 * sizeof(uint32_t));
    if (const char* e = getenv("MTR_VIS_WAVES")) {
        const long v = strtol(e, nullptr, 10);
        if (v == 2 || v == 4 || v == 8) d->vis_waves = (uint32_t)v;
    }
    if (const char* e = getenv("MTR_TILE_RUN")) {
        const long v = strtol(e, nullptr, 10);
        if (v >= 0 && v <= 65536) d->xcd_run = (uint32_t)v;
    }
    if (const char* e = getenv("MTR_CULL_DEBUG")) {
        const long v = strtol(e, nullptr, 10);
        if (v == 0 || v == 1 || v == 3 || v == 4 || v == 5) d->cull_debug = (uint32_t)v;
    }
    if (const char* e = getenv("MTR_GEOM_SLOTS")) {
        const long v = strtol(e, nullptr, 10);
        if (v >= 1 && v <= 0xFFFF) d->geom_slots = (uint32_t)v;
    }
    if (const char* e = getenv("MTR_MAX_INFLIGHT")) {
        const long v = strtol(e, nullptr, 10);
        if (v >= 1 && v <= (long)mtr_device::kMaxInflight) d->max_inflight = (uint32_t)v;
    }
    *out = d.release();
    return MTR_OK;
}

int32_t mtr_device_create(int32_t hip_device, mtr_device** out) {
    return mtr_device_create_on_stream(hip_device, nullptr, out);
}

void mtr_device_destroy(mtr_device* d) {
    if (!d) return;
    (void)mtr_device_exchange_stop(d);
    (void)hipSetDevice(d->hip_dev);
    (void)hipStreamSynchronize(d->stream);
    for (Slot& sl : d->slots)
        if (sl.stream) (void)hipStreamSynchronize(sl.stream);
    for (hipEvent_t e : d->inflight)
        if (e) (void)hipEventDestroy(e);
    for (auto& g : d->garbage) {
        if (g.ev) { (void)hipEventSynchronize(g.ev); (void)hipEventDestroy(g.ev); }
        if (g.p) (void)hipFree(g.p);
    }
    if (d->s_copy) (void)hipStreamSynchronize(d->s_copy);
    if (d->pose_stage) (void)hipFree(d->pose_stage);
    if (d->s_copy) (void)hipStreamDestroy(d->s_copy);
    if (d->cube) mtr_model_destroy(d->cube);
    for (auto& t : d->own_tables) {
        if (t->d_lists) (void)hipFree(t->d_lists);
        if (t->d_src_of_bin) (void)hipFree(t->d_src_of_bin);
    }
    for (auto& f : d->free_fb) {
        (void)hipFree(f.color);
        (void)hipFree(f.depth);
        (void)hipFree(f.counters);
        if (f.done) (void)hipEventDestroy(f.done);
    }
    for (Slot& sl : d->slots) {
        void* ptrs[] = {sl.rec_hdr, sl.rec_a, sl.rec_l, sl.rec_b, sl.chunk_info, sl.defer_list, sl.bin_count, sl.bin_fill,
                        sl.bin_start, sl.seg_start, sl.entries, sl.segs, sl.mats, sl.bin_flag, sl.inst_list, sl.inst_count, sl.work_mask, sl.comp};
        for (void* p : ptrs)
            if (p) (void)hipFree(p);
        if (sl.stream) (void)hipStreamDestroy(sl.stream);
    }
    if (d->own_stream) (void)hipStreamDestroy(d->stream);
    if (d->status_host) (void)hipHostFree(d->status_host);
    if (d->hint_host) (void)hipHostFree(d->hint_host);
    delete d;
}

int32_t mtr_device_synchronize(mtr_device* d) {
    if (!d) return MTR_E_INVALID;
    int32_t rc = set_device(d);
    if (rc) return rc;
    if ((rc = mtr_device_exchange_drain(d))) return rc;
    if ((rc = drain_all(d))) return rc;
    std::lock_guard<std::mutex> submit_lock(d->submit_mu);
    for (uint32_t i = 0; i < d->max_inflight; i++) examine_status(d, (int)i, true);  // every frame has left the GPU
    return report_sticky(d);
}

int32_t mtr_device_set_tile_mode(mtr_device* d, int32_t mode) {
    if (!d) return MTR_E_INVALID;
    if (mode != MTR_TILE_AUTO && mode != MTR_TILE_ORDERED && mode != MTR_TILE_VISIBILITY)
        return fail(d, MTR_E_INVALID, "unknown tile mode");
    d->tile_mode = mode;
    return MTR_OK;
}

int32_t mtr_device_set_binning(mtr_device* d, int32_t single_pass, uint32_t queue_capacity) {
    if (!d) return MTR_E_INVALID;
    if (queue_capacity && (queue_capacity < 64 || queue_capacity > 65536)) return fail(d, MTR_E_INVALID, "queue capacity out of range");
    std::lock_guard<std::mutex> g(d->submit_mu);  // the exchange thread grows the bound when it re-runs an overflowed frame
    d->direct_enabled = single_pass != 0;
    if (queue_capacity) { d->qcap = queue_capacity; d->scap = std::max<uint32_t>(16, queue_capacity / 8); }
    return MTR_OK;
}

int32_t mtr_device_set_profiling(mtr_device* d, int32_t enable) {
    if (!d) return MTR_E_INVALID;
    d->profiling = enable != 0;
    return MTR_OK;
}

int32_t mtr_device_set_texture_residency(mtr_device* d, uint32_t mode) {
    if (!d) return MTR_E_INVALID;
    if (mode != MTR_TEXRES_DECODED && mode != MTR_TEXRES_BLOCKS) return fail(d, MTR_E_INVALID, "unknown texture residency mode");
    d->texture_residency = mode;
    return MTR_OK;
}

int32_t mtr_device_set_culling(mtr_device* d, int32_t mode) {
    if (!d) return MTR_E_INVALID;
    if (mode < MTR_GEOM_CULL_OFF || mode > MTR_GEOM_CULL_ALL_FRAMES) return fail(d, MTR_E_INVALID, "unknown culling mode");
    std::lock_guard<std::mutex> g(d->submit_mu);
    d->cull_enabled = mode != MTR_GEOM_CULL_OFF;
    d->cull_unsharded = mode == MTR_GEOM_CULL_ALL_FRAMES;
    return MTR_OK;
}

uint32_t mtr_crc32(const uint8_t* bytes, size_t len, uint32_t init) {
    // src/util/crc.rs:36-50: reflected 0xEDB88320 table, no final xor, stops at the first NUL
    struct Table {
        uint32_t t[256];
        constexpr Table() : t() {
            for (uint32_t i = 0; i < 256; i++) {
                uint32_t c = i;
                for (int k = 0; k < 8; k++) c = (c & 1) ? (0xEDB88320u ^ (c >> 1)) : (c >> 1);
                t[i] = c;
            }
        }
    };
    static constexpr Table kTable{};  // constant-initialised: no lazy set-up for two threads to race on
    const uint32_t* table = kTable.t;
    uint32_t v = init;
    for (size_t i = 0; i < len && bytes[i] != 0; i++) v = table[(bytes[i] ^ v) & 0xff] ^ (v >> 8);
    return v;
}

}  // extern "C"
