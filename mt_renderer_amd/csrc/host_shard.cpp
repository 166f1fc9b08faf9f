// host_shard.cpp -- sharded frames: ownership maps, shard sizes, pack / unpack, the exchange thread.
#include "host.h"

namespace mtr_host {

namespace {

// ---- ownership maps (mtr_internal.h: Ownership) ----
bool valid_own_args(uint32_t w, uint32_t h, uint32_t world, uint32_t map, uint32_t param, const uint32_t* band_rows) {
    if (w == 0 || h == 0 || w > 16384 || h > 16384 || world == 0 || world > 4096) return false;
    const uint32_t nby = (h + MTR_BIN - 1) / MTR_BIN;
    if (map == MTR_OWN_INTERLEAVED) return true;
    if (map == MTR_OWN_SUPERTILES) return param <= 6;
    if (map != MTR_OWN_BANDS) return false;
    if (band_rows) {
        if (band_rows[0] != 0 || band_rows[world] != nby) return false;
        for (uint32_t r = 0; r < world; r++)
            if (band_rows[r] > band_rows[r + 1]) return false;
    }
    return true;
}

// host lists of a map: lists = every bin, rank after rank; offs[r] = where rank r's share starts
void build_own_lists(uint32_t w, uint32_t h, uint32_t world, uint32_t map, uint32_t param, const uint32_t* band_rows,
                     std::vector<uint32_t>& bands, std::vector<uint32_t>& lists, std::vector<uint32_t>& offs) {
    const uint32_t nbx = (w + MTR_BIN - 1) / MTR_BIN, nby = (h + MTR_BIN - 1) / MTR_BIN, nbins = nbx * nby;
    bands.clear();
    if (map == MTR_OWN_BANDS) {
        bands.resize(world + 1);
        for (uint32_t r = 0; r <= world; r++) bands[r] = band_rows ? band_rows[r] : (uint32_t)((uint64_t)r * nby / world);
    }
    std::vector<std::vector<uint32_t>> per(world);
    if (map == MTR_OWN_BANDS) {
        for (uint32_t r = 0; r < world; r++)
            for (uint32_t b = bands[r] * nbx; b < bands[r + 1] * nbx; b++) per[r].push_back(b);
    } else if (map == MTR_OWN_SUPERTILES) {
        const uint32_t S = 1u << param, nsx = (nbx + S - 1) >> param, nsy = (nby + S - 1) >> param;
        for (uint32_t st = 0; st < nsx * nsy; st++) {
            const uint32_t sx = st % nsx, sy = st / nsx;
            for (uint32_t by = sy * S; by < std::min(nby, (sy + 1) * S); by++)
                for (uint32_t bx = sx * S; bx < std::min(nbx, (sx + 1) * S); bx++) per[st % world].push_back(by * nbx + bx);
        }
    } else {
        for (uint32_t b = 0; b < nbins; b++) per[b % world].push_back(b);
    }
    lists.clear();
    offs.assign(world + 1, 0);
    for (uint32_t r = 0; r < world; r++) {
        lists.insert(lists.end(), per[r].begin(), per[r].end());
        offs[r + 1] = (uint32_t)lists.size();
    }
}

uint32_t stride_of(const std::vector<uint32_t>& offs) {
    uint32_t s = 0;
    for (size_t r = 0; r + 1 < offs.size(); r++) s = std::max(s, offs[r + 1] - offs[r]);
    return s;
}

}  // namespace

// the device's cached table for a map (built and uploaded on first use); submit_mu held
int32_t get_own_table(mtr_device* d, uint32_t w, uint32_t h, uint32_t world, uint32_t map, uint32_t param, const uint32_t* band_rows,
                      const OwnTable** out) {
    *out = nullptr;
    if (!valid_own_args(w, h, world, map, param, band_rows)) return fail(d, MTR_E_INVALID, "bad ownership map arguments");
    if (map != MTR_OWN_SUPERTILES) param = 0;
    const uint32_t nby = (h + MTR_BIN - 1) / MTR_BIN;
    std::vector<uint32_t> bands;
    if (map == MTR_OWN_BANDS) {
        bands.resize(world + 1);
        for (uint32_t r = 0; r <= world; r++) bands[r] = band_rows ? band_rows[r] : (uint32_t)((uint64_t)r * nby / world);
    }
    for (auto& t : d->own_tables)
        if (t->w == w && t->h == h && t->map == map && t->param == param && t->world == world && t->bands == bands) { *out = t.get(); return MTR_OK; }
    if (d->own_tables.size() >= 64) {  // a host that keeps changing the map: drop the tables no live frame uses
        int32_t rc = drain_all(d);        // (nothing in flight may still read them)
        if (rc) return rc;
        size_t keep = 0;
        for (auto& t : d->own_tables) {
            if (t->refs) { d->own_tables[keep++] = std::move(t); continue; }
            (void)hipFree(t->d_lists); (void)hipFree(t->d_src_of_bin);
        }
        d->own_tables.resize(keep);
    }
    auto t = std::make_unique<OwnTable>();
    t->w = w; t->h = h; t->map = map; t->param = param; t->world = world;
    std::vector<uint32_t> lists;
    build_own_lists(w, h, world, map, param, band_rows, t->bands, lists, t->offs);
    t->stride_bins = stride_of(t->offs);
    t->st_shift = param; t->nsx = (((w + MTR_BIN - 1) / MTR_BIN) + (1u << param) - 1) >> param;
    std::vector<uint32_t> src(lists.size());
    for (uint32_t r = 0; r < world; r++)
        for (uint32_t k = t->offs[r]; k < t->offs[r + 1]; k++) src[lists[k]] = r * t->stride_bins + (k - t->offs[r]);
    int32_t rc = dev_alloc(d, &t->d_lists, lists.size());
    if (!rc) rc = dev_alloc(d, &t->d_src_of_bin, src.size());
    if (rc) return rc;
    HIPCHK(d, hipMemcpy(t->d_lists, lists.data(), lists.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(d, hipMemcpy(t->d_src_of_bin, src.data(), src.size() * 4, hipMemcpyHostToDevice));
    t->lists = std::move(lists);
    *out = t.get();
    d->own_tables.push_back(std::move(t));
    return MTR_OK;
}

namespace {

// the frame's ownership table; an unsharded frame packs / unpacks as a world of one
int32_t frame_table(mtr_frame* f, const OwnTable** t) {
    *t = f->own;
    if (*t) return MTR_OK;
    std::lock_guard<std::mutex> submit_lock(f->dev->submit_mu);
    return get_own_table(f->dev, f->w, f->h, 1, MTR_OWN_INTERLEAVED, 0, nullptr, t);
}

int32_t pack_shard_on(mtr_frame* f, void* dst_dev, size_t dst_bytes, hipStream_t s, bool wait_frame) {
    if (!f || !dst_dev) return MTR_E_INVALID;
    mtr_device* d = f->dev;
    if (!f->submitted) return fail(d, MTR_E_INVALID, "frame not submitted");
    if (dst_bytes < mtr_frame_shard_bytes(f)) return fail(d, MTR_E_INVALID, "shard buffer too small");
    int32_t rc = set_device(d);
    if (rc) return rc;
    const OwnTable* t = nullptr;
    if ((rc = frame_table(f, &t))) return rc;
    if (wait_frame) HIPCHK(d, hipStreamWaitEvent(s, f->fb.done, 0));  // the public stream already waits for every frame
    const uint32_t r = f->own ? f->shard_rank : 0;
    mtr_launch_pack_shard(f->fb.color, static_cast<uint8_t*>(dst_dev), f->w, f->h, t->d_lists + t->offs[r], t->offs[r + 1] - t->offs[r],
                          t->stride_bins, s);
    HIPCHK(d, hipGetLastError());
    // the colour buffer now has a reader after the tile kernel: whoever recycles it (the frame may be destroyed at
    // once) must wait for the pack too, so the buffer's completion event moves behind it
    HIPCHK(d, hipEventRecord(f->fb.done, s));
    return MTR_OK;
}

int32_t unpack_table_on(mtr_device* d, const OwnTable* t, const void* gathered_dev, void* dst_dev, hipStream_t s) {
    mtr_launch_unpack_shards(static_cast<const uint8_t*>(gathered_dev), static_cast<uint8_t*>(dst_dev), t->w, t->h, t->d_src_of_bin, s);
    HIPCHK(d, hipGetLastError());
    return MTR_OK;
}

int32_t unpack_shards_on(mtr_device* d, const void* gathered_dev, uint32_t world, uint32_t w, uint32_t h, void* dst_dev, hipStream_t s) {
    if (!d || !gathered_dev || !dst_dev) return MTR_E_INVALID;
    if (world == 0 || w == 0 || h == 0 || w > 16384 || h > 16384) return fail(d, MTR_E_INVALID, "bad unpack arguments");
    int32_t rc = set_device(d);
    if (rc) return rc;
    const OwnTable* t = nullptr;
    {
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        if ((rc = get_own_table(d, w, h, world, MTR_OWN_INTERLEAVED, 0, nullptr, &t))) return rc;
    }
    return unpack_table_on(d, t, gathered_dev, dst_dev, s);
}

// ---------------------------------------------------------------------------------------------
// exchange thread
// ---------------------------------------------------------------------------------------------
void exchange_main(mtr_device* d, Exchange* x) {
    (void)hipSetDevice(d->hip_dev);
    for (;;) {
        mtr_frame* f = nullptr;
        // a frame arrives every few tens of microseconds: poll briefly before sleeping on the condition variable
        for (int spin = 0; spin < 20000 && !f; spin++) {
            if (x->pending.load(std::memory_order_acquire)) {
                std::lock_guard<std::mutex> g(x->mu);
                if (!x->q.empty()) { f = x->q.front(); x->q.pop_front(); }
            } else {
                __builtin_ia32_pause();
            }
        }
        if (!f) {
            std::unique_lock<std::mutex> lk(x->mu);
            x->cv_items.wait(lk, [&] { return x->stop || !x->q.empty(); });
            if (x->q.empty()) return;  // stop requested and nothing left
            f = x->q.front(); x->q.pop_front();
        }
        x->cv_items.notify_all();  // room in the queue
        int32_t rc;
        { std::lock_guard<std::mutex> g(x->mu); rc = x->err; }
        std::string msg;
        // NO RANK MAY SKIP A COLLECTIVE.  The all-gather of frame k completes only when every rank has issued it: a rank
        // that failed (this frame, or an earlier one whose error has not been collected yet) still takes part, sending a
        // shard filled with the frame's clear colour, and carries its status out of band -- mtr_device_exchange_drain
        // returns it, and the host agrees on it across the ranks (bench.py: a MIN all-reduce after the drain).  Skipping
        // the call instead would leave the healthy ranks waiting in frame k's collective for ever.
        const Exchange::Lane ln = x->lanes[(size_t)(x->dealt++ % x->lanes.size())];
        // every rank sends exactly its shard of THIS frame: the unpack derives the per-rank stride from the frame size
        const size_t count = mtr_frame_shard_bytes(f);
        if (rc == MTR_OK) {
            // a frame whose bin queues overflowed is re-run (exact two-pass queues) BEFORE its colour is packed: the
            // gathered frame is never missing triangles.  The flags are known when the frame's tile kernel starts, so
            // in the normal case this does not wait for the frame to finish.
            rc = settle_frame(f, false);
            if (rc == MTR_OK) rc = mtr_frame_pack_color_shard_on_stream(f, ln.send, count, ln.stream);
            if (rc != MTR_OK) { std::lock_guard<std::mutex> g(g_err_mu); msg = d->err; }
        }
        if (rc != MTR_OK) {  // the shard of a rank in error: the clear colour (count is a multiple of 4)
            std::vector<uint32_t> fill(count / 4, f->clear_rgba8);
            (void)hipMemcpyAsync(ln.send, fill.data(), count, hipMemcpyHostToDevice, ln.stream);
            (void)hipStreamSynchronize(ln.stream);  // `fill` goes out of scope
        }
        {
            const int nrc = x->fn(ln.send, ln.gathered, count, x->dtype_u8, ln.comm, ln.stream);
            if (nrc != 0 && rc == MTR_OK) { rc = MTR_E_HIP; msg = "all-gather callback returned " + std::to_string(nrc); }
        }
        if (rc == MTR_OK) {
            rc = mtr_frame_unpack_color_shards_on_stream(f, ln.gathered, ln.dst, ln.stream);
            if (rc != MTR_OK) { std::lock_guard<std::mutex> g(g_err_mu); msg = d->err; }
        }
        mtr_frame_destroy(f);
        {
            std::lock_guard<std::mutex> g(x->mu);
            if (rc != MTR_OK && x->err == MTR_OK) { x->err = rc; x->err_msg = msg; }
            x->pending.fetch_sub(1, std::memory_order_release);
        }
        x->cv_idle.notify_all();
    }
}

}  // namespace

}  // namespace mtr_host

using namespace mtr_host;

extern "C" {

size_t mtr_shard_bytes(uint32_t w, uint32_t h, uint32_t world) {
    if (world == 0) return 0;
    const size_t nbins = (size_t)((w + MTR_BIN - 1) / MTR_BIN) * ((h + MTR_BIN - 1) / MTR_BIN);
    return (nbins + world - 1) / world * (MTR_BIN * MTR_BIN * 4);
}

size_t mtr_shard_bytes_map(uint32_t w, uint32_t h, uint32_t world, uint32_t map, uint32_t param, const uint32_t* band_rows) {
    if (!valid_own_args(w, h, world, map, param, band_rows)) return 0;
    std::vector<uint32_t> bands, lists, offs;
    build_own_lists(w, h, world, map, map == MTR_OWN_SUPERTILES ? param : 0, band_rows, bands, lists, offs);
    return (size_t)stride_of(offs) * (MTR_BIN * MTR_BIN * 4);
}

size_t mtr_frame_shard_bytes(mtr_frame* f) {
    if (!f) return 0;
    if (!f->own) return mtr_shard_bytes(f->w, f->h, 1);
    return (size_t)f->own->stride_bins * (MTR_BIN * MTR_BIN * 4);
}

int32_t mtr_frame_pack_color_shard(mtr_frame* f, void* dst_dev, size_t dst_bytes) {
    return pack_shard_on(f, dst_dev, dst_bytes, f ? f->dev->stream : nullptr, false);
}

int32_t mtr_frame_pack_color_shard_on_stream(mtr_frame* f, void* dst_dev, size_t dst_bytes, void* hip_stream) {
    return pack_shard_on(f, dst_dev, dst_bytes, reinterpret_cast<hipStream_t>(hip_stream), true);
}

int32_t mtr_device_unpack_color_shards(mtr_device* d, const void* gathered_dev, uint32_t world, uint32_t w, uint32_t h,
                                       void* dst_dev) {
    return unpack_shards_on(d, gathered_dev, world, w, h, dst_dev, d ? d->stream : nullptr);
}

int32_t mtr_device_unpack_color_shards_on_stream(mtr_device* d, const void* gathered_dev, uint32_t world, uint32_t w, uint32_t h,
                                                 void* dst_dev, void* hip_stream) {
    return unpack_shards_on(d, gathered_dev, world, w, h, dst_dev, reinterpret_cast<hipStream_t>(hip_stream));
}

int32_t mtr_frame_unpack_color_shards_on_stream(mtr_frame* f, const void* gathered_dev, void* dst_dev, void* hip_stream) {
    if (!f || !gathered_dev || !dst_dev) return MTR_E_INVALID;
    mtr_device* d = f->dev;
    int32_t rc = set_device(d);
    if (rc) return rc;
    const OwnTable* t = nullptr;
    if ((rc = frame_table(f, &t))) return rc;
    return unpack_table_on(d, t, gathered_dev, dst_dev, hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : d->stream);
}

int32_t mtr_device_exchange_start(mtr_device* d, mtr_allgather_fn fn, void* comm, int dtype_u8, void* send_dev, size_t send_bytes,
                                  void* gathered_dev, void* dst_dev, uint32_t world, void* hip_stream) {
    if (!d) return MTR_E_INVALID;
    if (!fn || !send_dev || !gathered_dev || !dst_dev || world == 0 || !hip_stream)
        return fail(d, MTR_E_INVALID, "bad exchange arguments");
    if (d->xchg) return fail(d, MTR_E_INVALID, "exchange already started");
    auto* x = new Exchange();
    x->fn = fn; x->comm = comm; x->dtype_u8 = dtype_u8;
    x->send = static_cast<uint8_t*>(send_dev); x->send_bytes = send_bytes;
    x->gathered = static_cast<uint8_t*>(gathered_dev); x->dst = static_cast<uint8_t*>(dst_dev);
    x->world = world; x->stream = reinterpret_cast<hipStream_t>(hip_stream);
    x->lanes.push_back({x->comm, x->send, x->gathered, x->dst, x->stream});
    d->xchg = x;
    x->th = std::thread(exchange_main, d, x);
    return MTR_OK;
}

int32_t mtr_device_exchange_add_lane(mtr_device* d, void* comm, void* send_dev, void* gathered_dev, void* dst_dev, void* hip_stream) {
    if (!d) return MTR_E_INVALID;
    Exchange* x = d->xchg;
    if (!x) return fail(d, MTR_E_INVALID, "no exchange thread (mtr_device_exchange_start)");
    if (!send_dev || !gathered_dev || !dst_dev || !hip_stream) return fail(d, MTR_E_INVALID, "bad exchange lane arguments");
    std::lock_guard<std::mutex> g(x->mu);
    if (x->pending.load(std::memory_order_acquire) != 0) return fail(d, MTR_E_INVALID, "exchange lanes change only while the thread is idle");
    if (x->lanes.size() >= 4) return fail(d, MTR_E_INVALID, "at most 4 exchange lanes");
    for (const Exchange::Lane& ln : x->lanes)
        if (ln.stream == hip_stream || ln.send == send_dev || ln.gathered == gathered_dev)
            return fail(d, MTR_E_INVALID, "an exchange lane needs a stream and buffers of its own");
    x->lanes.push_back({comm, static_cast<uint8_t*>(send_dev), static_cast<uint8_t*>(gathered_dev), static_cast<uint8_t*>(dst_dev),
                        reinterpret_cast<hipStream_t>(hip_stream)});
    return MTR_OK;
}

int32_t mtr_frame_submit_exchange(mtr_frame* f) {
    if (!f) return MTR_E_INVALID;
    mtr_device* d = f->dev;
    Exchange* x = d->xchg;
    if (!x) return fail(d, MTR_E_INVALID, "no exchange thread (mtr_device_exchange_start)");
    if (f->shard_world != x->world) return fail(d, MTR_E_INVALID, "frame shard world differs from the exchange's");
    if (x->send_bytes < mtr_frame_shard_bytes(f)) return fail(d, MTR_E_INVALID, "exchange send buffer too small");
    if (f->waited) f->flags_checked = true;
    if (!f->submitted) {
        f->for_exchange = true;  // its only consumer is the exchange thread, which waits for the frame on its own stream
        int32_t rc = mtr_frame_submit(f);
        if (rc) { f->for_exchange = false; return rc; }
    }
    {
        std::unique_lock<std::mutex> lk(x->mu);
        x->cv_items.wait(lk, [&] { return x->q.size() < Exchange::kDepth; });
        x->q.push_back(f);
        x->pending.fetch_add(1, std::memory_order_release);
    }
    x->cv_items.notify_all();
    return MTR_OK;
}

int32_t mtr_device_exchange_drain(mtr_device* d) {
    if (!d) return MTR_E_INVALID;
    Exchange* x = d->xchg;
    if (!x) return MTR_OK;
    std::unique_lock<std::mutex> lk(x->mu);
    x->cv_idle.wait(lk, [&] { return x->pending.load(std::memory_order_acquire) == 0; });
    if (x->err != MTR_OK) {
        const int32_t rc = x->err;
        const std::string msg = "exchange thread: " + x->err_msg;
        x->err = MTR_OK;
        lk.unlock();
        return fail(d, rc, msg);
    }
    return MTR_OK;
}

int32_t mtr_device_exchange_stop(mtr_device* d) {
    if (!d) return MTR_E_INVALID;
    Exchange* x = d->xchg;
    if (!x) return MTR_OK;
    const int32_t rc = mtr_device_exchange_drain(d);
    {
        std::lock_guard<std::mutex> g(x->mu);
        x->stop = true;
    }
    x->cv_items.notify_all();
    x->th.join();
    for (const Exchange::Lane& ln : x->lanes) (void)hipStreamSynchronize(ln.stream);
    d->xchg = nullptr;
    delete x;
    return rc;
}

}  // extern "C"
