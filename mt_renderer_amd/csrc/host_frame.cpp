// host_frame.cpp -- frames: begin / destroy, sharding, draw recording, read-backs, statistics and timings.
#include "host.h"

namespace mtr_host {

namespace {

// validates the draw and snapshots the model's chunk table (its visible primitives) as of now
int32_t check_model_for_draw(mtr_frame* f, mtr_model* m, std::shared_ptr<const ChunkTable>* table) {
    mtr_device* d = f->dev;
    if (!m || m->dev != d) return fail(d, MTR_E_INVALID, "model belongs to another device");
    if (f->submitted) return fail(d, MTR_E_INVALID, "frame already submitted");
    int32_t rc = set_device(d);
    if (rc) return rc;
    std::lock_guard<std::mutex> submit_lock(d->submit_mu);
    for (size_t p = 0; p < m->prims.size(); p++)
        if (m->prims[p].parts_no >= m->parts_disp.size())  // self.parts_disp[parts_no] would panic, src/model.rs:318
            return fail(d, MTR_E_INVALID, "primitive " + std::to_string(p) + ": parts_no outside parts_disp");
    return current_table(m, table);
}

}  // namespace

// the frame can no longer (re-)run: its draws let go of the palette ring buffers and batch versions they hold.  submit_mu held.
void release_palette_pins(mtr_frame* f) {
    for (Draw& dr : f->draws) {
        if (dr.pal_pinned && dr.pal_slot >= 0 && (size_t)dr.pal_slot < dr.model->pal_ring.size()) {
            dr.model->pal_ring[(size_t)dr.pal_slot].pinned--;
            dr.pal_pinned = false;
        }
        if (dr.ver_pinned && dr.batch) {
            dr.batch->vers[(size_t)dr.batch_ver].pinned--;
            dr.ver_pinned = false;
        }
    }
}

}  // namespace mtr_host

using namespace mtr_host;

extern "C" {

// ---------------------------------------------------------------------------------------------
// frame
// ---------------------------------------------------------------------------------------------
int32_t mtr_frame_begin(mtr_device* d, uint32_t w, uint32_t h, const float clear_rgba[4], float clear_depth,
                        mtr_frame** out) {
    if (!d || !out) return MTR_E_INVALID;
    *out = nullptr;
    if (w == 0 || h == 0 || w > 16384 || h > 16384 || !clear_rgba) return fail(d, MTR_E_INVALID, "bad frame size");
    int32_t rc = set_device(d);
    if (rc) return rc;
    {
        // an earlier frame that was released without a wait and turns out to have dropped triangles is reported here
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        poll_released(d);
        if ((rc = report_sticky(d))) return rc;
    }
    auto f = std::make_unique<mtr_frame>();
    f->dev = d; f->w = w; f->h = h;
    f->clear_rgba8 = pack_rgba8(clear_rgba);
    f->clear_depth = clear_depth;
    // recycle colour / depth buffers: prefer a set whose last frame has finished; while fewer than nslots + 2 sets
    // of this size exist, allocate another rather than wait for one still in flight (a host that begins and
    // destroys a frame per step would otherwise chain every frame to its predecessor)
    bool found = false;
    size_t same = 0, oldest = SIZE_MAX, ready = SIZE_MAX;
    std::unique_lock<std::mutex> pool_lock(d->pool_mu);
    for (size_t i = 0; i < d->free_fb.size(); i++)
        if (d->free_fb[i].w == w && d->free_fb[i].h == h) {
            same++;
            if (oldest == SIZE_MAX) oldest = i;
            if (ready == SIZE_MAX && (!d->free_fb[i].used || hipEventQuery(d->free_fb[i].done) == hipSuccess)) ready = i;
        }
    (void)hipGetLastError();  // hipEventQuery reports "not ready" as an error code
    // total sets of this size, parked or held by live frames: past nslots + 1 the pool stops growing as long as a
    // parked set exists (its last frame is waited for on the device, not on the host)
    uint32_t* total = nullptr;
    for (auto& e : d->fb_allocated)
        if (e.first == (((uint64_t)w << 32) | h)) total = &e.second;
    if (!total) { d->fb_allocated.push_back({((uint64_t)w << 32) | h, 0u}); total = &d->fb_allocated.back().second; }
    const size_t pick = ready != SIZE_MAX ? ready : ((same > 0 && *total > d->nslots) ? oldest : SIZE_MAX);
    if (pick != SIZE_MAX) {
        f->fb = d->free_fb[pick];
        d->free_fb.erase(d->free_fb.begin() + (long)pick);
        found = true;
        // the last frame on this set zeroed the other counter block in its tile kernel: count there
        if (f->fb.next_zeroed) { f->fb.ctr_live ^= 1u; f->fb.next_zeroed = false; f->fb.ctr_dirty = false; }
    }
    if (!found) ++*total;
    pool_lock.unlock();
    if (!found) {
        f->fb.w = w; f->fb.h = h;
        if (!(rc = dev_alloc(d, &f->fb.color, (size_t)w * h * 4)) && !(rc = dev_alloc(d, &f->fb.depth, (size_t)w * h)) &&
            !(rc = dev_alloc(d, &f->fb.counters, (size_t)CTR_NUM * 2)) &&
            hipEventCreateWithFlags(&f->fb.done, hipEventDisableTiming) != hipSuccess)
            rc = fail(d, MTR_E_HIP, "hipEventCreate failed");
        if (rc) {  // give the partial set back
            if (f->fb.color) (void)hipFree(f->fb.color);
            if (f->fb.depth) (void)hipFree(f->fb.depth);
            if (f->fb.counters) (void)hipFree(f->fb.counters);
            std::lock_guard<std::mutex> g(d->pool_mu);
            for (auto& e : d->fb_allocated)
                if (e.first == (((uint64_t)w << 32) | h)) --e.second;
            return rc;
        }
    }
    *out = f.release();
    return MTR_OK;
}

void mtr_frame_destroy(mtr_frame* f) {
    if (!f) return;
    mtr_device* d = f->dev;
    (void)hipSetDevice(d->hip_dev);
    if (f->have_events)
        for (auto& e : f->ev)
            if (e) (void)hipEventDestroy(e);
    if (f->own) {
        std::lock_guard<std::mutex> g(d->submit_mu);
        const_cast<OwnTable*>(f->own)->refs--;
    }
    {
        FreeList fl;
        {
            std::lock_guard<std::mutex> g(d->submit_mu);
            release_palette_pins(f);  // drawn and never submitted, or submitted and never waited for
            for (Draw& dr : f->draws)
                if (dr.batch) { batch_unref(dr.batch, fl); dr.batch = nullptr; }  // the batch may have been destroyed since
        }
        release_now(fl);
    }
    if (f->submitted && !f->flags_checked && f->status_idx >= 0) {
        // nobody looked at this frame's overflow flags: they are examined when its status word is polled or recycled,
        // and a frame that dropped triangles is then reported by the next call that can return an error
        std::lock_guard<std::mutex> g(d->submit_mu);
        if (d->status_owner[f->status_idx] == f->frame_index && !d->status_checked[f->status_idx]) d->status_released[f->status_idx] = true;
    }
    // the buffers may still be written by this frame's kernels: whoever recycles them waits on fb.done
    {
        std::lock_guard<std::mutex> g(d->pool_mu);
        d->free_fb.push_back(f->fb);
    }
    delete f;
}

int32_t mtr_frame_set_shard_map(mtr_frame* f, uint32_t rank, uint32_t world, uint32_t map, uint32_t param, const uint32_t* band_rows) {
    if (!f) return MTR_E_INVALID;
    mtr_device* d = f->dev;
    if (world == 0 || rank >= world) return fail(d, MTR_E_INVALID, "bad shard rank/world");
    if (f->submitted) return fail(d, MTR_E_INVALID, "frame already submitted");
    int32_t rc = set_device(d);
    if (rc) return rc;
    const OwnTable* t = nullptr;
    {
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        if ((rc = get_own_table(d, f->w, f->h, world, map, param, band_rows, &t))) return rc;
        if (f->own) const_cast<OwnTable*>(f->own)->refs--;
        const_cast<OwnTable*>(t)->refs++;
    }
    f->shard_rank = rank; f->shard_world = world; f->own = t;
    return MTR_OK;
}

int32_t mtr_frame_set_shard(mtr_frame* f, uint32_t rank, uint32_t world) {
    return mtr_frame_set_shard_map(f, rank, world, MTR_OWN_INTERLEAVED, 0, nullptr);
}

int32_t mtr_frame_draw_model(mtr_frame* f, mtr_model* m, const float view_proj[16]) {
    if (!f || !view_proj) return MTR_E_INVALID;
    std::shared_ptr<const ChunkTable> table;
    int32_t rc = check_model_for_draw(f, m, &table);
    if (rc) return rc;
    Draw dr{};
    dr.table = std::move(table);
    dr.model = m; dr.d_model_mats = nullptr; dr.d_palettes = m->d_palette; dr.npal = m->npal; dr.pal_ready = m->pal_ready; dr.pal_slot = m->pal_slot;
    dr.pal_stride = 0; dr.ninst = 1; dr.shader_override = -1; dr.blend = true;
    memcpy(dr.vp, view_proj, sizeof dr.vp);
    if (dr.pal_slot >= 0) {  // the ring buffer must not come round again before this frame has been submitted
        std::lock_guard<std::mutex> submit_lock(f->dev->submit_mu);
        m->pal_ring[(size_t)dr.pal_slot].pinned++;
        dr.pal_pinned = true;
    }
    f->draws.push_back(std::move(dr));
    return MTR_OK;
}

int32_t mtr_frame_draw_batch(mtr_frame* f, mtr_batch* b, const float view_proj[16]) {
    if (!f || !b || !view_proj) return MTR_E_INVALID;
    if (b->dev != f->dev) return fail(f->dev, MTR_E_INVALID, "batch belongs to another device");
    std::shared_ptr<const ChunkTable> table;
    int32_t rc = check_model_for_draw(f, b->model, &table);
    if (rc) return rc;
    Draw dr{};
    dr.table = std::move(table);
    dr.model = b->model; dr.batch = b; dr.pal_slot = -1; dr.ninst = b->n;
    dr.tex_override = b->tex_override; dr.shader_override = -1; dr.blend = true;
    memcpy(dr.vp, view_proj, sizeof dr.vp);
    {
        // the draw uses the version that is current now, whatever later updates write, for as long as its frame may run
        std::lock_guard<std::mutex> submit_lock(f->dev->submit_mu);
        mtr_batch::Ver& v = b->vers[(size_t)b->cur];
        dr.d_model_mats = v.d; dr.pal_ready = v.ready;
        dr.d_palettes = v.npal ? v.d + (size_t)b->n * 16 : nullptr;
        dr.npal = v.npal; dr.pal_stride = v.npal * 16;
        dr.batch_ver = b->cur;
        v.pinned++;
        dr.ver_pinned = true;
        b->refs++;
    }
    f->draws.push_back(std::move(dr));
    return MTR_OK;
}

int32_t mtr_frame_draw_instances(mtr_frame* f, mtr_model* m, const float* model_mats, const float* palettes,
                                 size_t npal, size_t n, const float view_proj[16]) {
    if (!f || !view_proj) return MTR_E_INVALID;
    mtr_batch* b = nullptr;
    int32_t rc = mtr_batch_create(f->dev, m, n, model_mats, palettes, npal, nullptr, &b);
    if (rc) return rc;
    rc = mtr_frame_draw_batch(f, b, view_proj);
    if (rc) { mtr_batch_destroy(b); return rc; }
    f->draws.back().owned_batch.reset(b);
    return MTR_OK;
}

int32_t mtr_frame_draw_model_joints(mtr_frame* f, mtr_model* m, const float camera[16]) {
    if (!f || !m || !camera) return MTR_E_INVALID;
    if (m->dev != f->dev) return fail(f->dev, MTR_E_INVALID, "model belongs to another device");
    return mtr_frame_draw_overlay_cubes(f, camera, m->joint_cubes.data(), m->joint_cubes.size() / 16);
}

int32_t mtr_frame_draw_overlay_cubes(mtr_frame* f, const float camera[16], const float* inst_mats, size_t n) {
    if (!f || !camera || (!inst_mats && n)) return MTR_E_INVALID;
    mtr_device* d = f->dev;
    if (n == 0) return MTR_OK;
    if (!d->cube) {
        // src/debug_overlay.rs:10-35
        static const float verts[24] = {1, 1, -1, 1, -1, -1, 1, 1, 1, 1, -1, 1, -1, 1, -1, -1, -1, -1, -1, 1, 1, -1, -1, 1};
        static const uint16_t idx[36] = {4, 2, 0, 2, 7, 3, 6, 5, 7, 1, 7, 5, 0, 3, 1, 4, 1, 5,
                                         4, 6, 2, 2, 6, 7, 6, 4, 5, 1, 3, 7, 0, 2, 3, 4, 0, 1};
        mtr_primitive pr{};
        pr.w[0] = 8u << 16;
        pr.w[2] = (12u << 16) | (3u << 24);
        pr.w[7] = 36;
        mtr_layout lay{};
        lay.num_elements = 1;
        lay.elements[0].semantic = MTR_SEM_POSITION;
        lay.elements[0].format = MTR_IEF_F32;
        lay.elements[0].count = 3;
        int32_t rc = mtr_model_create(d, verts, sizeof verts, idx, 36, &pr, 1, &lay, nullptr, nullptr, 0, nullptr, &d->cube);
        if (rc) return rc;
    }
    mtr_batch* b = nullptr;
    int32_t rc = mtr_batch_create(d, d->cube, n, inst_mats, nullptr, 0, nullptr, &b);
    if (rc) return rc;
    rc = mtr_frame_draw_batch(f, b, camera);
    if (rc) { mtr_batch_destroy(b); return rc; }
    Draw& dr = f->draws.back();
    dr.owned_batch.reset(b);
    dr.shader_override = MTR_SH_CONST;
    const float c[4] = {0.1f, 0.2f, 0.3f, 1.0f};  // src/shaders/debug_overlay.wgsl:30
    dr.const_rgba8 = pack_rgba8(c);
    dr.blend = false;  // blend: None, src/debug_overlay.rs:174
    return MTR_OK;
}

int32_t mtr_frame_read_color(mtr_frame* f, void* rgba8, size_t len) {
    if (!f || !rgba8) return MTR_E_INVALID;
    mtr_device* d = f->dev;
    if (len < (size_t)f->w * f->h * 4) return fail(d, MTR_E_INVALID, "output too small");
    int32_t rc = mtr_frame_wait(f);
    if (rc) return rc;
    // the frame is complete (mtr_frame_wait): read it on the copy stream, not behind the later frames in flight
    HIPCHK(d, hipMemcpyAsync(rgba8, f->fb.color, (size_t)f->w * f->h * 4, hipMemcpyDeviceToHost, d->s_copy));
    HIPCHK(d, hipStreamSynchronize(d->s_copy));
    return MTR_OK;
}

int32_t mtr_frame_read_depth(mtr_frame* f, float* depth, size_t count) {
    if (!f || !depth) return MTR_E_INVALID;
    mtr_device* d = f->dev;
    if (count < (size_t)f->w * f->h) return fail(d, MTR_E_INVALID, "output too small");
    int32_t rc = mtr_frame_wait(f);
    if (rc) return rc;
    HIPCHK(d, hipMemcpyAsync(depth, f->fb.depth, (size_t)f->w * f->h * 4, hipMemcpyDeviceToHost, d->s_copy));
    HIPCHK(d, hipStreamSynchronize(d->s_copy));
    return MTR_OK;
}

void* mtr_frame_color_devptr(mtr_frame* f) { return f ? f->fb.color : nullptr; }
void* mtr_frame_depth_devptr(mtr_frame* f) { return f ? f->fb.depth : nullptr; }

int32_t mtr_frame_get_stats(mtr_frame* f, mtr_frame_stats* out) {
    if (!f || !out) return MTR_E_INVALID;
    int32_t rc = fetch_stats(f);
    if (rc) return rc;
    *out = f->stats;
    return MTR_OK;
}

int32_t mtr_frame_get_timings(mtr_frame* f, float ms[MTR_STAGE_COUNT]) {
    if (!f || !ms) return MTR_E_INVALID;
    if (!f->have_events) return fail(f->dev, MTR_E_INVALID, "profiling was not enabled for this frame");
    int32_t rc = mtr_frame_wait(f);
    if (rc) return rc;
    memcpy(ms, f->ms, sizeof f->ms);
    return MTR_OK;
}

// ---------------------------------------------------------------------------------------------
// unit-test hooks
// ---------------------------------------------------------------------------------------------
int32_t mtr_frame_read_bin_counts(mtr_frame* f, uint32_t* entries, uint32_t* segments, size_t nbins) {
    if (!f || !entries || !segments) return MTR_E_INVALID;
    mtr_device* d = f->dev;
    if (nbins != f->stats.nbins) return fail(d, MTR_E_INVALID, "nbins mismatch");
    Slot& sl = d->slots[f->slot];
    int32_t rc = mtr_frame_wait(f);
    if (rc) return rc;
    std::vector<uint32_t> bs(nbins + 1), ss(nbins + 1);
    HIPCHK(d, hipMemcpyAsync(bs.data(), sl.bin_start, (nbins + 1) * 4, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(d, hipMemcpyAsync(ss.data(), sl.seg_start, (nbins + 1) * 4, hipMemcpyDeviceToHost, d->stream));
    HIPCHK(d, hipStreamSynchronize(d->stream));
    if (f->ran_direct) {
        std::vector<unsigned long long> bf(nbins);  // the tile kernels moved the counts here when they cleaned bin_fill
        HIPCHK(d, hipMemcpyAsync(bf.data(), sl.bin_count, nbins * 8, hipMemcpyDeviceToHost, d->stream));
        HIPCHK(d, hipStreamSynchronize(d->stream));
        for (size_t b = 0; b < nbins; b++) { entries[b] = (uint32_t)bf[b]; segments[b] = (uint32_t)(bf[b] >> 32); }
        if (f->own && f->shard_world > 1) {
            // only the tile workgroups of the rank's own bins park a count: the words of the other bins hold whatever an
            // earlier frame on this slot left there
            std::vector<uint8_t> mine(nbins, 0);
            for (uint32_t k = f->own->offs[f->shard_rank]; k < f->own->offs[f->shard_rank + 1]; k++) mine[f->own->lists[k]] = 1;
            for (size_t b = 0; b < nbins; b++)
                if (!mine[b]) entries[b] = segments[b] = 0;
        }
        return MTR_OK;
    }
    for (size_t b = 0; b < nbins; b++) { entries[b] = bs[b + 1] - bs[b]; segments[b] = ss[b + 1] - ss[b]; }
    return MTR_OK;
}

}  // extern "C"
