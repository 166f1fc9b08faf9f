// host_events.cpp -- animation events (SPEC.md section 22): the event set, its validated markers, and the collect calls that
// run k_events on step records in device memory.
#include "host.h"

// k_events.hip.  Weak: the host-only builds of this file (tests/cpp, over the HIP stub runtime) link no kernels; libmtr.so
// links k_events.o.
void mtr_launch_events(const EventParams& p, hipStream_t s) __attribute__((weak));

namespace mtr_host {

namespace {

constexpr size_t kEvMaxInstances = (size_t)1 << 27, kEvMaxMarkers = (size_t)1 << 24;

// what every collect call checks before it touches anything; device: the pointers are device memory and must be aligned
int32_t events_check(const mtr_anim_events* ev, const void* steps, size_t nsteps, size_t n, const void* out, size_t capacity, const void* count,
                     const void* bits, bool device) {
    mtr_device* d = ev->dev;
    if (!steps || !count) return fail(d, MTR_E_INVALID, "events collect: no steps or no count");
    if (nsteps == 0 || nsteps > MTR_ROOT_MAX_STEPS) return fail(d, MTR_E_INVALID, "events collect: 1 to 8 steps per instance");
    if (n == 0 || n > ev->max_instances) return fail(d, MTR_E_INVALID, "events collect: 1 to max_instances instances");
    if (capacity > 0 && !out) return fail(d, MTR_E_INVALID, "events collect: a capacity and no list");
    if (device) {
        if (((uintptr_t)steps & 15u) || ((uintptr_t)out & 15u)) return fail(d, MTR_E_INVALID, "events collect: device steps and the list must be 16-byte aligned");
        if (((uintptr_t)count & 3u) || ((uintptr_t)bits & 3u)) return fail(d, MTR_E_INVALID, "events collect: device count and bits must be 4-byte aligned");
    }
    if ((uint64_t)n * nsteps * ev->max_count > 0xFFFFFFFFull)  // at most 2^27 * 8 * 2^24: no 64-bit product wraps
        return fail(d, MTR_E_INVALID, "events collect: n * nsteps * the largest marker count of a clip exceeds 2^32 - 1");
    if (!mtr_launch_events) return fail(d, MTR_E_UNSUPPORTED, "events collect: built without k_events");
    return set_device(d);
}

// k_events on `s` between the set's events: its calls are ordered among themselves (the block sums)
int32_t events_launch(mtr_anim_events* ev, const void* steps_dev, size_t nsteps, size_t n, float min_weight, void* out_dev, size_t capacity, uint32_t* count_dev,
                      uint32_t* bits_dev, hipStream_t s) {
    mtr_device* d = ev->dev;
    int32_t rc = set_before(ev, s);
    if (rc) return rc;
    EventParams ep{};
    ep.clips = ev->d;
    ep.ranges = ev->d + (size_t)ev->nclips * 4;
    ep.markers = ep.ranges + ev->w_ranges;
    ep.sums = ev->d + (size_t)ev->nclips * 4 + ev->w_ranges + ev->w_markers;
    ep.steps = static_cast<const uint32_t*>(steps_dev);
    ep.out = capacity ? static_cast<uint32_t*>(out_dev) : nullptr;
    ep.count = count_dev;
    ep.bits = bits_dev;
    ep.nclips = ev->nclips; ep.nsteps = (uint32_t)nsteps; ep.n = (uint32_t)n;
    ep.capacity = capacity > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)capacity;  // no more than 2^32 - 1 events fire
    ep.min_weight = min_weight;
    mtr_launch_events(ep, s);
    HIPCHK(d, hipGetLastError());
    return set_after(ev, s);
}

}  // namespace

}  // namespace mtr_host

using namespace mtr_host;

extern "C" {

static_assert(sizeof(mtr_event_marker) == 8 && sizeof(mtr_anim_event) == 16 && sizeof(mtr_root_step) == 16, "mtr_event_marker, mtr_anim_event, mtr_root_step");

int32_t mtr_anim_events_create(mtr_device* d, size_t nclips, const uint32_t* nkeys, const uint32_t* clip_flags, const uint32_t* counts,
                               const mtr_event_marker* markers, size_t max_instances, mtr_anim_events** out) {
    if (!d || !out) return MTR_E_INVALID;
    *out = nullptr;
    if (nclips == 0 || nclips > kClipMaxKeys) return fail(d, MTR_E_INVALID, "anim events: 1 to 2^24 clips");
    if (!nkeys) return fail(d, MTR_E_INVALID, "anim events: no key counts");
    if (max_instances == 0 || max_instances > kEvMaxInstances) return fail(d, MTR_E_INVALID, "anim events: 1 to 2^27 instances");
    size_t total = 0;
    uint32_t max_count = 0;
    for (size_t c = 0; counts && c < nclips; c++) {
        total += counts[c];  // at most 2^24 * 2^32
        max_count = std::max(max_count, counts[c]);
    }
    if (total > kEvMaxMarkers) return fail(d, MTR_E_INVALID, "anim events: more than 2^24 markers");
    if (total > 0 && !markers) return fail(d, MTR_E_INVALID, "anim events: markers counted and none given");
    const size_t w_ranges = (nclips * 2 + 3) / 4 * 4, w_markers = (total * 2 + 3) / 4 * 4;
    std::vector<uint32_t> img(nclips * 4 + w_ranges + w_markers);
    size_t first = 0;
    int32_t rc;
    for (size_t c = 0; c < nclips; c++) {  // a clip's entry, then its markers, before the next clip's
        const uint32_t fl = clip_flags ? clip_flags[c] : 0u;
        if ((rc = clip_entry(d, "anim events", c, nkeys, fl, nullptr, &img[c * 4]))) return rc;
        const std::string who = "anim events: clip " + std::to_string(c) + " ";
        const bool loop = (fl & MTR_CLIP_LOOP) != 0;
        float period;
        std::memcpy(&period, &img[c * 4], 4);
        const uint32_t cnt = counts ? counts[c] : 0u;
        img[nclips * 4 + c * 2] = (uint32_t)first;
        img[nclips * 4 + c * 2 + 1] = cnt;
        for (uint32_t k = 0; k < cnt; k++) {
            const float x = markers[first + k].x;
            const std::string which = who + "marker " + std::to_string(k) + " ";
            if (!std::isfinite(x)) return fail(d, MTR_E_INVALID, which + "has a position that is not finite");
            if (!(x >= 0.0f) || (loop ? !(x < period) : !(x <= period))) return fail(d, MTR_E_INVALID, which + "lies outside the clip");
            if (k > 0 && x < markers[first + k - 1].x) return fail(d, MTR_E_INVALID, which + "lies before the marker ahead of it");
        }
        first += cnt;
    }
    if (total) std::memcpy(&img[nclips * 4 + w_ranges], markers, total * sizeof(mtr_event_marker));
    if ((rc = set_device(d))) return rc;
    auto ev = std::make_unique<mtr_anim_events>();
    ev->dev = d; ev->nclips = (uint32_t)nclips; ev->max_instances = (uint32_t)max_instances; ev->nmarkers = (uint32_t)total; ev->max_count = max_count;
    ev->w_ranges = w_ranges; ev->w_markers = w_markers;
    const size_t nsums = (max_instances + MTR_EVENTS_BLOCK - 1) / MTR_EVENTS_BLOCK;
    if ((rc = set_upload(ev.get(), "anim events", {{img.data(), img.size() * 4}, {nullptr, nsums * 4}}))) return rc;  // the tables, the block sums
    *out = ev.release();
    return MTR_OK;
}

void mtr_anim_events_destroy(mtr_anim_events* ev) { set_destroy(ev); }

int32_t mtr_anim_events_collect_device(mtr_anim_events* ev, const mtr_root_step* steps_dev, size_t nsteps, size_t n, float min_weight, mtr_anim_event* out_dev,
                                       size_t capacity, uint32_t* count_dev, uint32_t* bits_dev, void* hip_stream) {
    if (!ev) return MTR_E_INVALID;
    int32_t rc = events_check(ev, steps_dev, nsteps, n, out_dev, capacity, count_dev, bits_dev, true);
    if (rc) return rc;
    return events_launch(ev, steps_dev, nsteps, n, min_weight, out_dev, capacity, count_dev, bits_dev, caller_stream(ev->dev, hip_stream));
}

int32_t mtr_anim_events_collect_host(mtr_anim_events* ev, const mtr_root_step* steps, size_t nsteps, size_t n, float min_weight, mtr_anim_event* out,
                                     size_t capacity, uint32_t* count, uint32_t* bits) {
    if (!ev) return MTR_E_INVALID;
    mtr_device* d = ev->dev;
    int32_t rc = events_check(ev, steps, nsteps, n, out, capacity, count, bits, false);
    if (rc) return rc;
    if (capacity > 0xFFFFFFFFull) return fail(d, MTR_E_INVALID, "events collect: the host hook takes a capacity below 2^32");
    // one block: the steps and the list (16-byte words), then the bits and the two words of the count
    StagedBlock blk(d);
    StagedPart &p_steps = blk.part(steps, n * nsteps * 4), &p_out = blk.part(out, capacity * 4), &p_bits = blk.part(bits, bits ? n : 0),
               &p_count = blk.part(count, 2);
    return blk.run([&]() -> int32_t {
        int32_t r2;
        if ((r2 = blk.up({&p_steps, &p_out})) ||
            (r2 = events_launch(ev, p_steps.at, nsteps, n, min_weight, p_out.dev<void>(), capacity, p_count.dev<uint32_t>(), p_bits.dev<uint32_t>(), d->s_copy)))
            return r2;
        return blk.down({&p_out, &p_bits, &p_count});
    });
}

}  // extern "C"
