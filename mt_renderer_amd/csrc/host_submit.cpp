// host_submit.cpp -- the submit path: run_frame and its phases, the overflow re-run, submit / wait / end.
#include "host.h"

namespace mtr_host {

namespace {

// run_frame's phases, in the order it calls them.  They run under d->submit_mu, which run_frame's caller holds: none takes
// a lock.  FrameRun is what they hand to each other during one run, on run_frame's stack.
struct FrameRun {
    uint32_t nbins = 0;
    uint64_t total_chunks = 0, nmats = 0, tris_in = 0;
    uint64_t this_frame = 0; int sidx = 0;               // index of this run in submission order, its status word
    std::vector<uint32_t> mat_base, mat_stride;          // per draw: its materials in the frame's table
    std::vector<uint32_t> inst_off, work_off, comp_off;  // per draw: its share of the slot's culling buffers (prepare_stream)
    uint32_t strad_base = 0;   // the second half of inst_list: the slots of the instances that straddle the rank's border
    uint32_t chunk_base = 0;   // global chunk id of the next draw's first chunk
    uint32_t clip_seq = 0;     // k_geom_clip launches queued so far (one behind every draw that launches geometry)
    uint32_t nhint = 0;        // batch draws whose culling counters this frame's tile kernel reports to the host (launch sizing)
    uint16_t hint_word[4] = {}, hint_slot[4] = {};
    bool use_vis = false, prof = false;
    FrameBuffers fb{};
};

// Phase 1, the work of the frame: reads the draws; writes r.nbins and the totals; rejects a frame with too many chunks.
int32_t count_work(mtr_frame* f, FrameRun& r) {
    r.nbins = ((f->w + MTR_BIN - 1) / MTR_BIN) * ((f->h + MTR_BIN - 1) / MTR_BIN);
    for (auto& dr : f->draws) {
        r.total_chunks += (uint64_t)dr.table->chunks.size() * dr.ninst;
        r.nmats += (uint64_t)dr.model->prims.size() * (dr.tex_override.empty() ? 1 : dr.ninst);
        r.tris_in += dr.table->ntris_visible * dr.ninst;
    }
    // a (triangle, bin) entry is the 32-bit submission order chunk * 128 + slot, and the visibility key stores order + 1:
    // fewer than 2^25 - 1 chunks (2 G triangles) per frame
    if (r.total_chunks >= (1ull << 25) - 1) return fail(f->dev, MTR_E_OVERFLOW, "too many geometry chunks in one frame");
    return MTR_OK;
}

// Frees what only frames up to this_frame - max_inflight could still read (they have all been waited for): d->garbage.
void collect_garbage(mtr_device* d, uint64_t this_frame) {
    if (d->garbage.empty()) return;
    size_t keep = 0;
    for (auto& g : d->garbage) {
        if (g.last_frame + d->max_inflight <= this_frame && (!g.ev || hipEventQuery(g.ev) == hipSuccess)) {
            if (g.ev) (void)hipEventDestroy(g.ev);
            if (g.p) (void)hipFree(g.p);
        } else {
            d->garbage[keep++] = g;
        }
    }
    (void)hipGetLastError();  // hipEventQuery reports "not ready" as an error code
    d->garbage.resize(keep);
}

// Phase 2, the frame's place in the device: takes the next frame index (d->frames_submitted) and waits for the frame that
// held its place in the in-flight ring, recycles that frame's status word (examining it if nobody has), collects garbage
// and picks the slot (d->frame_counter).  Writes r.this_frame, r.sidx, and f->status_idx, frame_index, slot and flags.
int32_t claim_frame(mtr_device* d, mtr_frame* f, FrameRun& r) {
    // this frame's slot: the other slots may still be feeding earlier frames' tile kernels
    const uint64_t this_frame = r.this_frame = d->frames_submitted++;
    hipEvent_t& ring = d->inflight[this_frame % d->max_inflight];
    if (ring) HIPCHK(d, hipEventSynchronize(ring));  // frame (i - max_inflight) has left the GPU
    else HIPCHK(d, hipEventCreateWithFlags(&ring, hipEventDisableTiming));
    // its status word is recycled for this frame: if nobody looked at that frame's overflow flags, do it now
    const int sidx = r.sidx = (int)(this_frame % d->max_inflight);
    examine_status(d, sidx, true);
    __atomic_store_n(&d->status_host[sidx], 0u, __ATOMIC_RELEASE);
    d->status_checked[sidx] = false; d->status_released[sidx] = false; d->status_owner[sidx] = this_frame;
    f->status_idx = sidx; f->frame_index = this_frame; f->flags_checked = false; f->stats_valid = false;
    collect_garbage(d, this_frame);
    f->slot = (int)(d->frame_counter++ % d->nslots);
    d->status_slot_of[sidx] = f->slot;
    return MTR_OK;
}

// Phase 3, room in the slot for everything but culling: reads r's totals and the frame's queue demands (min_entries,
// min_segs, force_two_pass); grows the slot's record, chunk, bin, queue buffers (grow-only); may halve d->qcap for a huge
// bin grid; writes f->ran_direct and sl.bin_fill_dirty.
int32_t reserve_slot_buffers(mtr_device* d, mtr_frame* f, Slot& sl, const FrameRun& r) {
    int32_t rc;
    const uint32_t nbins = r.nbins;
    const uint64_t rec_need = r.total_chunks * MTR_CHUNK_SLOTS;
    if (rec_need > 0xFFFFFFF0ull) return fail(d, MTR_E_OVERFLOW, "too many triangles in one frame");
    if ((rc = grow_slot(d, sl, nullptr, nullptr, rec_need, &sl.rec_cap, &sl.rec_hdr, &sl.rec_a, &sl.rec_l, &sl.rec_b))) return rc;
    if ((rc = grow_slot(d, sl, nullptr, nullptr, r.total_chunks, &sl.chunk_cap, &sl.chunk_info, &sl.defer_list))) return rc;
    bool grew;  // mtr_frame_read_bin_counts copies from the bin arrays on the public stream
    if ((rc = grow_slot(d, sl, d->stream, &grew, nbins + 1, &sl.bin_cap, &sl.bin_count, &sl.bin_fill, &sl.bin_start, &sl.seg_start, &sl.bin_flag))) return rc;
    if (grew) sl.bin_fill_dirty = true;
    // direct mode: nbins bounded queues; the bound shrinks if the bin grid is so large that the queues would not
    // be addressable with 32 bits
    while ((uint64_t)nbins * d->qcap > 0xF0000000ull && d->qcap > 64) d->qcap /= 2;
    f->ran_direct = d->direct_enabled && !f->force_two_pass;
    uint64_t e_need = std::max<uint64_t>(1u << 20, rec_need / 2) * d->queue_scale, s_need = std::max<uint64_t>(1u << 18, r.total_chunks * 8) * d->queue_scale;
    e_need = std::max<uint64_t>(e_need, f->min_entries);
    s_need = std::max<uint64_t>(s_need, f->min_segs);
    if (f->ran_direct) {
        e_need = std::max<uint64_t>(e_need, (uint64_t)nbins * d->qcap);
        s_need = std::max<uint64_t>(s_need, (uint64_t)nbins * d->scap);
    }
    if ((rc = grow_slot(d, sl, nullptr, nullptr, std::min<uint64_t>(e_need, 0xFFFFFFF0ull), &sl.entry_cap, &sl.entries))) return rc;
    return grow_slot(d, sl, nullptr, nullptr, std::min<uint64_t>(s_need, 0xFFFFFFF0ull), &sl.seg_cap, &sl.segs);
}

// Phase 4, the material table: reads the draws' models, states and textures; rebuilds f->mats_host and f->all_opaque,
// writes r.mat_base / r.mat_stride; grows sl.mats and uploads the table on the slot's stream when it differs from what the
// slot holds (sl.mats_uploaded).
int32_t upload_materials(mtr_device* d, mtr_frame* f, Slot& sl, FrameRun& r) {
    std::vector<DMat>& mats = f->mats_host;
    mats.clear();
    f->all_opaque = true;
    mats.reserve(r.nmats);
    r.mat_base.resize(f->draws.size()); r.mat_stride.resize(f->draws.size());
    for (size_t di = 0; di < f->draws.size(); di++) {
        Draw& dr = f->draws[di];
        mtr_model* m = dr.model;
        r.mat_base[di] = (uint32_t)mats.size();
        r.mat_stride[di] = dr.tex_override.empty() ? 0 : (uint32_t)m->prims.size();
        const uint32_t reps = dr.tex_override.empty() ? 1 : dr.ninst;
        for (uint32_t rep = 0; rep < reps; rep++)
            for (size_t p = 0; p < m->prims.size(); p++) {
                DMat dm{};
                int32_t tex = m->prim_to_texture[p];
                if (tex >= 0 && !dr.tex_override.empty() && dr.tex_override[rep] >= 0) tex = dr.tex_override[rep];
                dm.blend = dr.blend ? MTR_DB_ALPHA : MTR_DB_OFF;
                dm.dstate = 3u;  // depth write | depth test << 1
                dm.tlevels = 1;
                if (!m->states.empty() && dr.shader_override != MTR_SH_CONST) {  // material state (row f-4)
                    const mtr_prim_state& st = m->states[p];
                    dm.blend = st.blend == MTR_BLEND_OFF ? MTR_DB_OFF : (st.blend == MTR_BLEND_ADD ? MTR_DB_ADD : MTR_DB_ALPHA);
                    dm.dstate = (st.depth_write ? 1u : 0u) | (st.depth_test ? 2u : 0u);
                }
                // order-dependent: an additive blend, or a depth state in which a fragment's fate depends on what came before
                bool order_dep = dm.blend == MTR_DB_ADD || dm.dstate != 3u;
                if (dr.shader_override == MTR_SH_CONST) {
                    dm.shader = MTR_SH_CONST; dm.rgba8 = dr.const_rgba8;
                } else if (tex >= 0 && m->prims[p].has_uv) {  // src/model.rs:212-216
                    dm.shader = MTR_SH_TEXTURED;
                    const mtr_texture* t = m->textures[(size_t)tex];
                    if (!t->opaque && dm.blend == MTR_DB_ALPHA) order_dep = true;  // a texel with alpha < 255 really blends
                    dm.tex = t->d_rgba; dm.tw = t->w; dm.th = t->h; dm.tlevels = t->levels | (t->resident << 8);
                } else {
                    dm.shader = MTR_SH_DEBUG; dm.rgba8 = m->debug_rgba8[p];
                }
                if (order_dep) { dm.translucent = 1; f->all_opaque = false; }
                mats.push_back(dm);
            }
    }
    if (mats.size() >= MTR_MAX_TEXTURED_MATERIALS) return fail(d, MTR_E_OVERFLOW, "too many materials in one frame (a record holds a 24-bit material id)");
    bool grew;
    int32_t rc = grow_slot(d, sl, nullptr, &grew, std::max<size_t>(mats.size(), 64), &sl.mat_cap, &sl.mats);
    if (rc) return rc;
    if (grew) sl.mats_uploaded.clear();
    // the material table is tiny; the copy is ordered on the stream before the kernels that read it
    if (mats.size() != sl.mats_uploaded.size() ||
        (!mats.empty() && memcmp(mats.data(), sl.mats_uploaded.data(), mats.size() * sizeof(DMat)) != 0)) {
        HIPCHK(d, hipMemcpyAsync(sl.mats, mats.data(), mats.size() * sizeof(DMat), hipMemcpyHostToDevice, sl.stream));
        sl.mats_uploaded = mats;
    }
    return MTR_OK;
}

// Phase 5, what every kernel of the frame is handed: reads the slot's buffers and capacities, the frame's size, ownership
// table and f->all_opaque / ran_direct, the device's culling, queue and tile-mode settings; writes r.fb (ownership record
// included) and r.use_vis.  Mutates nothing else.
void fill_frame_buffers(const mtr_device* d, const mtr_frame* f, const Slot& sl, FrameRun& r) {
    FrameBuffers& fb = r.fb;
    fb.rec_hdr = sl.rec_hdr; fb.rec_a = sl.rec_a; fb.rec_l = sl.rec_l; fb.rec_b = sl.rec_b; fb.chunk_info = sl.chunk_info;
    fb.bin_count = sl.bin_count; fb.bin_fill = sl.bin_fill; fb.bin_start = sl.bin_start; fb.seg_start = sl.seg_start;
    fb.entries = sl.entries; fb.segs = sl.segs; fb.counters = f->fb.live();
    fb.rec_cap = sl.rec_cap; fb.entry_cap = sl.entry_cap; fb.seg_cap = sl.seg_cap;
    fb.W = f->w; fb.H = f->h; fb.nbx = (f->w + MTR_BIN - 1) / MTR_BIN; fb.nby = (f->h + MTR_BIN - 1) / MTR_BIN;
    fb.own.map = MTR_OWN_INTERLEAVED; fb.own.rank = 0; fb.own.world = 1; fb.own.own_count = r.nbins; fb.own.own_list = nullptr;
    if (f->own && f->shard_world > 1) {
        const OwnTable& t = *f->own;
        fb.own.map = t.map; fb.own.rank = f->shard_rank; fb.own.world = f->shard_world;
        if (t.map == MTR_OWN_BANDS) { fb.own.y0 = t.bands[f->shard_rank]; fb.own.y1 = t.bands[f->shard_rank + 1]; }
        fb.own.st_shift = t.st_shift; fb.own.nsx = t.nsx;
        fb.own.own_count = t.offs[f->shard_rank + 1] - t.offs[f->shard_rank];
        fb.own.own_list = t.d_lists + t.offs[f->shard_rank];
        // interleaved bins: a chunk's rectangle holds a bin of every rank as soon as it is `world` bins wide, so there
        // is next to nothing to cull (and the work list would only cost): culling is for bands and super-tiles
        fb.own.cull = (d->cull_enabled && t.map != MTR_OWN_INTERLEAVED) ? 1u : 0u;
        if (fb.own.cull && d->cull_debug != 0xFFFFFFFFu) fb.own.cull = d->cull_debug;  // timing ablations only (MTR_CULL_DEBUG at device creation)
    }
    else if (d->cull_unsharded && d->cull_enabled) {
        fb.own.cull = 1u;  // world 1: "a bin of this rank" = a bin of the target, so what is culled is what is off the target
    }
    fb.direct = f->ran_direct ? 1u : 0u; fb.qcap = d->qcap; fb.scap = d->scap;
    // every material opaque (debug / overlay colours have a == 1; opaque textures sample a == 1): the frame is a
    // per-pixel (min z, latest) reduction and the visibility-key kernel applies; otherwise blend order matters
    r.use_vis = f->all_opaque && d->tile_mode != MTR_TILE_ORDERED;
    fb.unordered = (f->ran_direct && r.use_vis) ? 1u : 0u;
}

// Phase 6, what is queued ahead of the draws.  Creates the frame's profiling events once (f->ev, r.prof), orders the run
// behind the last frame that used the colour / depth / counter set, zeroes what this run counts into: the frame's counter
// block (f->fb.ctr_dirty) and the slot's bin_count or bin_fill (sl.bin_fill_dirty).  Then plans the culling of a sharded
// frame (r.fb.own.cull): k_cull_instances compacts the instance list of a batch draw to the instances that may reach this
// rank's bins, k_cull_chunks bounds every chunk of the survivors and writes the work list of k_geom.  Reads the draws; writes
// each draw's offsets into the slot's four culling buffers (r.inst_off, work_off, comp_off, strad_base), grows those, and
// zeroes the culling counters when no tile kernel has (sl.cull_counts_dirty, ctr_clean_draws).
int32_t prepare_stream(mtr_device* d, mtr_frame* f, Slot& sl, FrameRun& r) {
    if (d->profiling && !f->have_events) {
        for (auto& e : f->ev) HIPCHK(d, hipEventCreate(&e));
        f->have_events = true;
    }
    r.prof = d->profiling && f->have_events;
    // one stream per slot: the slot's previous frame is ordered before this one by the stream itself; recycled colour /
    // depth / counter buffers: their last frame may have run on another slot's stream
    hipStream_t sg = sl.stream;
    if (f->fb.used) HIPCHK(d, hipStreamWaitEvent(sg, f->fb.done, 0));
    if (f->fb.ctr_dirty) HIPCHK(d, hipMemsetAsync(f->fb.live(), 0, CTR_NUM * sizeof(uint32_t), sg));
    f->fb.ctr_dirty = true;  // a second run of this frame (queue overflow) starts from a fill again
    if (!r.fb.direct) {
        HIPCHK(d, hipMemsetAsync(sl.bin_count, 0, (size_t)(r.nbins + 1) * sizeof(unsigned long long), sg));
        sl.bin_fill_dirty = true;
    } else if (sl.bin_fill_dirty) {
        HIPCHK(d, hipMemsetAsync(sl.bin_fill, 0, (size_t)sl.bin_cap * sizeof(unsigned long long), sg));
        sl.bin_fill_dirty = false;
    }
    if (!r.fb.own.cull) return MTR_OK;
    const size_t ndraws = f->draws.size();
    r.inst_off.assign(ndraws, 0xFFFFFFFFu); r.work_off.assign(ndraws, 0u); r.comp_off.assign(ndraws, 0u);
    uint64_t ninst_total = 0, work_total = 0, comp_total = 0;
    for (size_t di = 0; di < ndraws; di++) {
        const Draw& dr = f->draws[di];
        const mtr_model* m = dr.model;
        const bool sk = dr.d_palettes && dr.npal;
        // one 16-bit mask per (instance slot, group of 16 chunks)
        const uint64_t nx = ((uint64_t)dr.table->chunks.size() + 15) / 16;
        // one-dimensional launch of nx * 4 * slots workgroups of 256 threads: HIP rejects 2^32 threads or more per dimension
        if (nx * 4 * dr.ninst > 0xFFFFFFull) return fail(d, MTR_E_OVERFLOW, "too many geometry chunks in one sharded draw");
        r.work_off[di] = (uint32_t)work_total;
        work_total += (nx * dr.ninst + 1) & ~1ull;  // even: k_geom reads a mask through the aligned dword that holds it
        if (!dr.d_model_mats) continue;  // a single model: chunk culling only
        if (sk ? (!m->inst_skinned_boundable || m->n_inst_skinned == 0) : (m->n_inst_unskinned == 0)) continue;
        r.inst_off[di] = (uint32_t)ninst_total;
        ninst_total += dr.ninst;
        r.comp_off[di] = (uint32_t)comp_total;
        comp_total += (uint64_t)dr.ninst * (sk ? dr.npal + 1u : 1u);
    }
    if (work_total > 0xFFFFFFF0ull || comp_total > 0xFFFFFFF0ull) return fail(d, MTR_E_OVERFLOW, "too many geometry chunks in one sharded frame");
    int32_t rc;
    if ((rc = grow_slot(d, sl, nullptr, nullptr, std::max<uint64_t>(comp_total, 64), &sl.comp_cap, &sl.comp))) return rc;
    if ((rc = grow_slot(d, sl, nullptr, nullptr, std::max<uint64_t>(work_total, 64), &sl.work_cap, &sl.work_mask))) return rc;
    r.strad_base = (uint32_t)ninst_total;
    if ((rc = grow_slot(d, sl, nullptr, nullptr, std::max<uint64_t>(2 * ninst_total, 64), &sl.inst_cap, &sl.inst_list))) return rc;
    bool grew;
    uint32_t words = sl.draw_cap * MTR_CULL_CTR_WORDS;  // inst_count is sized in words, its capacity kept in draws
    if ((rc = grow_slot(d, sl, nullptr, &grew, (size_t)MTR_CULL_CTR_WORDS * std::max<size_t>(ndraws, 4), &words, &sl.inst_count))) return rc;
    if (grew) { sl.draw_cap = words / MTR_CULL_CTR_WORDS; sl.cull_counts_dirty = true; }
    // the counters start from zero: the tile kernel of the slot's previous frame cleared them (TileParams::zero_words)
    if (sl.cull_counts_dirty || ndraws > sl.ctr_clean_draws)
        HIPCHK(d, hipMemsetAsync(sl.inst_count, 0, (size_t)sl.draw_cap * MTR_CULL_CTR_WORDS * sizeof(uint32_t), sg));
    sl.cull_counts_dirty = true;  // until a tile kernel that clears them has been queued (record_tiles)
    // the exact two-pass fill walks every chunk's run descriptor: culled chunks write none
    if (!r.fb.direct) HIPCHK(d, hipMemsetAsync(sl.chunk_info, 0, r.total_chunks * sizeof(ChunkInfo), sg));
    return MTR_OK;
}

// Launch sizes of a culled batch draw from what a recent frame of this batch kept under the same ownership (k_geom.hip, k_cull.hip); a
// camera that moves changes the count gradually: the margin and the second geometry launch take what the hint misses.
// Gives the batch a hint slot at its first culled draw (d->hint_used, b->hint_slot / hint_key), and books the draw's
// counters for this frame's tile kernel to report (r.nhint, hint_word, hint_slot).
void pick_launch_hints(mtr_device* d, const mtr_frame* f, FrameRun& r, mtr_batch* b, size_t di, uint32_t* slots_hint, uint32_t* strad_hint) {
    if (b->hint_slot < 0)
        for (uint32_t i = 0; i < mtr_device::kHintSlots; i++)
            if (!d->hint_used[i]) { d->hint_used[i] = true; b->hint_slot = (int)i; b->hint_key = 0; break; }
    if (b->hint_slot < 0) return;
    uint64_t key = 0xcbf29ce484222325ull;  // FNV-1a over what the kept set depends on
    auto mix = [&](const void* p, size_t n) { for (size_t i = 0; i < n; i++) key = (key ^ static_cast<const uint8_t*>(p)[i]) * 0x100000001b3ull; };
    const void* own_id = f->own;
    mix(&own_id, sizeof own_id); mix(&f->shard_rank, sizeof f->shard_rank); mix(&r.fb.own.cull, sizeof r.fb.own.cull);
    volatile uint32_t* hw = d->hint_host + 2 * b->hint_slot;
    if (key != b->hint_key) { b->hint_key = key; hw[0] = hw[1] = 0u; }  // other bands, another rank: start over
    *slots_hint = hw[0]; *strad_hint = hw[1];
    if (r.nhint < 4 && di * MTR_CULL_CTR_WORDS < 0xFFFFu) { r.hint_word[r.nhint] = (uint16_t)(di * MTR_CULL_CTR_WORDS); r.hint_slot[r.nhint++] = (uint16_t)b->hint_slot; }
}

// Phase 7, one draw: stamps the batch, its version and the palette ring buffer the draw reads with r.this_frame (before
// the first launch: they protect the buffers while this run's kernels are in flight), orders the slot's stream behind
// their upload, then launches the draw's cull kernels (sharded frames) and k_geom.  Advances r.chunk_base.
int32_t record_draw(mtr_device* d, mtr_frame* f, Slot& sl, FrameRun& r, size_t di) {
    const FrameBuffers& fb = r.fb; hipStream_t sg = sl.stream;
    Draw& dr = f->draws[di];
    mtr_model* m = dr.model;
    GeomParams gp{};
    gp.vbuf = m->d_vbuf; gp.ibuf = m->d_ibuf; gp.prims = m->d_prims; gp.chunks = dr.table->d_chunks;
    gp.boxes = m->d_boxes;
    gp.nchunks = (uint32_t)dr.table->chunks.size(); gp.ninst = dr.ninst;
    if (dr.batch) {
        dr.batch->last_frame = r.this_frame; dr.batch->used = true;
        mtr_batch::Ver& v = dr.batch->vers[(size_t)dr.batch_ver];
        v.last_frame = r.this_frame; v.used = true;  // protects the version while this run's kernels are in flight
    }
    if (dr.pal_ready) {  // uploads of a model palette (ring) or of a batch, made on the copy stream
        HIPCHK(d, hipStreamWaitEvent(sg, dr.pal_ready, 0));
        if (dr.pal_slot >= 0 && (size_t)dr.pal_slot < m->pal_ring.size()) {
            mtr_model::PalBuf& pb = m->pal_ring[(size_t)dr.pal_slot];
            pb.last_frame = r.this_frame;  // protects the buffer while this run's kernels are in flight
            pb.used = true;
            // the pin stays: until the frame's overflow flags have been looked at it may be re-run (settle_frame, by
            // mtr_frame_wait or the exchange thread, several submits later) and must then skin with the SAME palette
        }
    }
    gp.model_mats = dr.d_model_mats; gp.palettes = dr.d_palettes; gp.npal = dr.d_palettes ? dr.npal : 0;
    gp.pal_stride = dr.pal_stride;
    memcpy(gp.vp, dr.vp, sizeof gp.vp);
    gp.chunk_base = r.chunk_base; gp.mat_base = r.mat_base[di]; gp.mat_inst_stride = r.mat_stride[di];
    gp.fb = fb;
    gp.mats = sl.mats;
    if (fb.own.cull) {
        const bool sk = dr.d_palettes && dr.npal;
        const uint32_t inst_off = r.inst_off[di];
        uint32_t* inst_cnt = nullptr;
        if (inst_off != 0xFFFFFFFFu) {
            CullParams cp{};
            cp.boxes = m->d_inst_boxes + (sk ? m->n_inst_unskinned : 0); cp.nboxes = sk ? m->n_inst_skinned : m->n_inst_unskinned;
            cp.ninst = dr.ninst; cp.model_mats = dr.d_model_mats; cp.palettes = gp.palettes; cp.npal = gp.npal; cp.pal_stride = gp.pal_stride;
            memcpy(cp.vp, dr.vp, sizeof cp.vp);
            cp.W = f->w; cp.H = f->h; cp.nbx = fb.nbx; cp.nby = fb.nby; cp.own = fb.own;
            cp.list = sl.inst_list + inst_off; cp.count = inst_cnt = sl.inst_count + di * MTR_CULL_CTR_WORDS;
            cp.comp = sl.comp + r.comp_off[di]; cp.ncomp = sk ? dr.npal + 1u : 1u;
            cp.work_mask = sl.work_mask + r.work_off[di]; cp.strad = sl.inst_list + r.strad_base + inst_off; cp.nchunks = gp.nchunks;
            cp.counters = fb.counters;
            mtr_launch_cull_instances(cp, sg);
            HIPCHK(d, hipGetLastError());  // a rejected launch must not pass as an empty frame (a later successful call clears the error)
        }
        ChunkCullParams cc{};
        cc.chunks = dr.table->d_chunks; cc.boxes = m->d_boxes; cc.nchunks = gp.nchunks; cc.ninst = dr.ninst;
        cc.inst_list = inst_cnt ? sl.inst_list + inst_off : nullptr; cc.inst_count = inst_cnt;
        cc.strad = inst_cnt ? sl.inst_list + r.strad_base + inst_off : nullptr;
        cc.model_mats = dr.d_model_mats; cc.palettes = gp.palettes; cc.npal = gp.npal; cc.pal_stride = gp.pal_stride;
        memcpy(cc.vp, dr.vp, sizeof cc.vp);
        cc.fb = fb;
        cc.comp = inst_cnt ? sl.comp + r.comp_off[di] : nullptr;
        cc.work_mask = sl.work_mask + r.work_off[di];
        cc.keep_all = (fb.own.cull == 3u || fb.own.cull == 4u) ? 1u : 0u;
        if (inst_cnt && dr.batch && !dr.owned_batch) pick_launch_hints(d, f, r, dr.batch, di, &gp.slots_hint, &cc.strad_hint);
        mtr_launch_cull_chunks(cc, sg);
        HIPCHK(d, hipGetLastError());
        gp.work_mask = cc.work_mask; gp.work_nx = (gp.nchunks + 15u) / 16u;
        gp.inst_list = cc.inst_list; gp.inst_count = cc.inst_count;
    }
    gp.slots_override = d->geom_slots;
    // a draw of fewer than ~64 k geometry waves (the headline model: 16 k) overlaps with the neighbouring frames' tile
    // kernels for most of its life: the build that leaves them a wave slot per SIMD (k_geom.hip: GEOM_OCC_SMALL)
    gp.small_draw = ((uint64_t)gp.nchunks * dr.ninst < 65536u) ? 1u : 0u;
    // the chunks with a triangle to clip go through the frame's deferred list to k_geom_clip, which mtr_launch_geom queues
    // behind the draw's geometry launches -- for every draw: the host keeps no bound of a skinned vertex's depth that
    // would prove a draw free of them
    gp.defer_list = sl.defer_list; gp.defer_cap = sl.chunk_cap; gp.clip_seq = r.clip_seq;
    if (mtr_geom_has_work(gp)) r.clip_seq++;
    mtr_launch_geom(gp, sg);
    HIPCHK(d, hipGetLastError());
    r.chunk_base += gp.nchunks * dr.ninst;
    return MTR_OK;
}

// Phase 8, binning and the tile kernels: scan and fill for the two-pass queues (with their profiling events), then the
// visibility kernel, the ordered kernel, or both (a mixed frame).  Reads f->mats_host, r.use_vis, the hints; hands the tile
// kernel the frame's other counter block and the slot's culling counters to zero for the next frame (f->fb.next_zeroed,
// sl.cull_counts_dirty, ctr_clean_draws), writes f->stats.tile_kernel, publishes the status word of a rank without a bin.
int32_t record_tiles(mtr_device* d, mtr_frame* f, Slot& sl, FrameRun& r) {
    const FrameBuffers& fb = r.fb; hipStream_t st = sl.stream;
    // single-pass binning launches neither kernel: no event either (an event costs the stream ~5 us, which would count
    // as frame latency); mtr_frame_wait reports both stages as 0
    if (!fb.direct) { mtr_launch_scan(fb, st); HIPCHK(d, hipGetLastError()); }
    if (r.prof && !fb.direct) HIPCHK(d, hipEventRecord(f->ev[2], st));
    if (!fb.direct) { mtr_launch_fill(fb, (uint32_t)r.total_chunks, st); HIPCHK(d, hipGetLastError()); }
    if (r.prof && !fb.direct) HIPCHK(d, hipEventRecord(f->ev[3], st));
    TileParams tp{};
    tp.fb = fb; tp.mats = sl.mats; tp.color = f->fb.color; tp.depth = f->fb.depth;
    tp.clear_rgba8 = f->clear_rgba8; tp.clear_depth = f->clear_depth;
    bool any_textured = false;
    for (const DMat& dm : f->mats_host) any_textured = any_textured || dm.shader == MTR_SH_TEXTURED;
    // some material translucent, some not: the visibility kernel takes the bins whose queue holds only opaque
    // triangles (order-free), flags the others, and the ordered kernel renders those in submission order
    // ... and also the bins whose translucent triangles are merely alpha-blended in the default depth state (prefix minima
    // of z, k_tile_vis.hip: STAIR).  Only when every material is HARD order-dependent (additive blend, depth write / test
    // off) is there nothing for it to do.
    bool any_soft = false;
    for (const DMat& dm : f->mats_host) any_soft = any_soft || !dm.translucent || !(dm.blend == MTR_DB_ADD || dm.dstate != 3u);
    const bool use_vis = r.use_vis, mixed = !use_vis && d->tile_mode == MTR_TILE_AUTO && any_soft;
    tp.bin_flag = sl.bin_flag; tp.mixed = mixed ? 1u : 0u;
    tp.zero_next = f->fb.other();
    f->fb.next_zeroed = fb.own.own_count != 0;  // a rank without a bin launches no tile workgroup
    tp.host_status = d->status_dev + r.sidx;
    tp.vis_waves = d->vis_waves;
    // the previous frame still on the GPU: this one will share it, balance across the XCDs wins; otherwise the frame
    // has the GPU to itself and the contiguous order's locality gives the shorter kernel (latency)
    bool shared = false;
    if (r.this_frame > 0) {
        hipEvent_t prev = d->inflight[(r.this_frame - 1) % d->max_inflight];
        shared = prev && hipEventQuery(prev) == hipErrorNotReady;
    }
    tp.xcd_run = d->xcd_run != mtr_device::kXcdRunAuto ? d->xcd_run : ((fb.own.world <= 1 && shared) ? std::max(16u, fb.nbx / 4u) : 0u);
    if (fb.own.cull && fb.own.own_count) {  // this frame's tile kernel clears the slot's culling counters for the next one
        const uint32_t ndraws = (uint32_t)f->draws.size();
        tp.zero_words = sl.inst_count; tp.zero_nwords = ndraws * MTR_CULL_CTR_WORDS;
        tp.hint_out = d->hint_dev; tp.nhint = r.nhint;
        for (uint32_t k = 0; k < r.nhint; k++) { tp.hint_word[k] = r.hint_word[k]; tp.hint_slot[k] = r.hint_slot[k]; }
        sl.cull_counts_dirty = false;
        sl.ctr_clean_draws = ndraws;  // what a frame with more draws than this one finds beyond is stale
    }
    f->stats.tile_kernel = use_vis ? MTR_TILE_VISIBILITY : (mixed ? MTR_TILE_MIXED : MTR_TILE_ORDERED);
    if (use_vis || mixed) { mtr_launch_tile_vis(tp, any_textured, st); HIPCHK(d, hipGetLastError()); }
    if (mixed) tp.nhint = 0;  // the visibility kernel of a mixed frame has reported (and cleared) the counters: the second kernel would report zeros
    if (!use_vis) { mtr_launch_tile(tp, any_textured, st); HIPCHK(d, hipGetLastError()); }
    // a rank without a bin launches no tile workgroup: nobody else would publish the (clean) status
    if (fb.own.own_count == 0) __atomic_store_n(&d->status_host[r.sidx], 0x80000000u, __ATOMIC_RELEASE);
    return MTR_OK;
}

// Phase 9, the end of a successful run: records the last profiling event, the framebuffer's and the in-flight ring's
// events behind the tile kernel, makes the public stream wait for the frame (unless the exchange thread consumes it),
// and only then resets f->stats (keeping the tile kernel chosen) and f->total_chunks.
int32_t finish_frame(mtr_device* d, mtr_frame* f, Slot& sl, const FrameRun& r) {
    if (r.prof) HIPCHK(d, hipEventRecord(f->ev[4], sl.stream));
    HIPCHK(d, hipEventRecord(f->fb.done, sl.stream));
    HIPCHK(d, hipEventRecord(d->inflight[r.this_frame % d->max_inflight], sl.stream));
    f->fb.used = true;
    // the device's public stream (read-backs, shard packing, the caller's own work) sees the framebuffer complete
    if (!f->for_exchange) HIPCHK(d, hipStreamWaitEvent(d->stream, f->fb.done, 0));
    HIPCHK(d, hipGetLastError());
    const uint32_t tk = f->stats.tile_kernel;
    f->stats = mtr_frame_stats{};
    f->stats.tile_kernel = tk;
    f->stats.binning = f->ran_direct ? 1u : 2u;
    f->stats.tris_in = r.tris_in;
    f->total_chunks = r.total_chunks;
    f->stats.width = f->w; f->stats.height = f->h; f->stats.nbins = r.nbins; f->stats.ndraws = (uint32_t)f->draws.size();
    return MTR_OK;
}

// Enqueues every kernel of the frame.  The caller holds d->submit_mu.
int32_t run_frame(mtr_frame* f) {
    mtr_device* d = f->dev;
    int32_t rc = set_device(d);
    if (rc) return rc;
    FrameRun r;
    if ((rc = count_work(f, r))) return rc;
    if ((rc = claim_frame(d, f, r))) return rc;
    Slot& sl = d->slots[f->slot];
    if ((rc = reserve_slot_buffers(d, f, sl, r))) return rc;
    if ((rc = upload_materials(d, f, sl, r))) return rc;
    fill_frame_buffers(d, f, sl, r);
    if ((rc = prepare_stream(d, f, sl, r))) return rc;
    if (r.prof) HIPCHK(d, hipEventRecord(f->ev[0], sl.stream));
    for (size_t di = 0; di < f->draws.size(); di++)
        if ((rc = record_draw(d, f, sl, r, di))) return rc;
    if (r.prof) HIPCHK(d, hipEventRecord(f->ev[1], sl.stream));
    if ((rc = record_tiles(d, f, sl, r))) return rc;
    return finish_frame(d, f, sl, r);
}

}  // namespace

// Makes sure the frame's kernels ran with complete bin queues: reads the overflow flags its tile kernel published and,
// when one is set, re-runs the frame (bounded per-bin queue full: through the exact two-pass queues, and later frames get
// twice the bound; two-pass queues too small: grown to what the scan measured).  wait_done: block until the frame has
// left the GPU first (mtr_frame_wait); otherwise return as soon as the flags are known to be clean, which the tile
// kernel announces when it STARTS -- the exchange thread can then queue the pack behind the frame without a host-side
// wait for its completion.  Called by the render thread and by the exchange thread (run_frame under submit_mu).
int32_t settle_frame(mtr_frame* f, bool wait_done) {
    mtr_device* d = f->dev;
    for (int attempt = 0; attempt < 6; attempt++) {
        uint32_t v = 0;
        if (!wait_done)
            for (int spin = 0; spin < 100000 && !((v = status_load(d, f->status_idx)) & 0x80000000u); spin++) __builtin_ia32_pause();
        if (!(v & 0x80000000u)) {
            HIPCHK(d, hipEventSynchronize(f->fb.done));
            v = status_load(d, f->status_idx);  // still 0: no tile workgroup ran (a rank that owns no bin), nothing to check
        }
        const uint32_t flags = v & 0x7fffffffu;
        {
            std::lock_guard<std::mutex> g(d->submit_mu);
            if (d->status_owner[f->status_idx] == f->frame_index) d->status_checked[f->status_idx] = true;
            if (!flags) release_palette_pins(f);  // this frame will not run again
        }
        f->flags_checked = true;
        if (!flags) return MTR_OK;
        if (flags & 1u) return fail(d, MTR_E_OVERFLOW, "a geometry chunk (62 strip positions) needed more than 124 records: guard-band clipping fanned too many of its triangles");
        if (!(flags & 4u)) {
            // exact queues too small: grow to what the scan measured
            uint32_t two[2] = {0, 0};
            HIPCHK(d, hipEventSynchronize(f->fb.done));
            HIPCHK(d, hipMemcpyAsync(two, f->fb.live() + CTR_ENTRIES, sizeof two, hipMemcpyDeviceToHost, d->s_copy));
            HIPCHK(d, hipStreamSynchronize(d->s_copy));
            const uint64_t e_need = (uint64_t)two[0] + two[0] / 4 + 1024, s_need = (uint64_t)two[1] + two[1] / 4 + 1024;
            if (e_need > 0xFFFFFFF0ull || s_need > 0xFFFFFFF0ull) return fail(d, MTR_E_OVERFLOW, "bin queues exceed 2^32 entries");
            f->min_entries = e_need;  // run_frame grows the queues of the slot it picks
            f->min_segs = s_need;
        }
        std::lock_guard<std::mutex> g(d->submit_mu);
        if (flags & 4u) {
            // a bounded per-bin queue filled up: this frame takes the exact two-pass path, later frames get twice the bound
            f->force_two_pass = true;
            grow_direct_queues(d);
        }
        const int32_t rc = run_frame(f);
        if (rc) return rc;
    }
    return fail(d, MTR_E_OVERFLOW, "bin queues still overflow after growing");
}

// device counters of the finished frame -> f->stats (read back on demand: mtr_frame_wait itself copies nothing)
int32_t fetch_stats(mtr_frame* f) {
    mtr_device* d = f->dev;
    int32_t rc = mtr_frame_wait(f);
    if (rc) return rc;
    if (f->stats_valid) return MTR_OK;
    uint32_t ctr[CTR_NUM];
    HIPCHK(d, hipMemcpyAsync(ctr, f->fb.live(), sizeof ctr, hipMemcpyDeviceToHost, d->s_copy));
    HIPCHK(d, hipStreamSynchronize(d->s_copy));
    f->stats.tris_setup = 0;
    for (int k = 0; k < CTR_NSHARDS; k++) f->stats.tris_setup += ctr[MTR_CTR(CTR_REC, k)];
    f->stats.bin_entries = ctr[CTR_ENTRIES];
    f->stats.segments = ctr[CTR_SEGS];
    if (f->ran_direct) {  // no scan in direct mode: the tile kernels counted the queues
        f->stats.bin_entries = f->stats.segments = 0;
        for (int k = 0; k < CTR_NSHARDS; k++) {
            f->stats.bin_entries += ctr[MTR_CTR(CTR_ENT, k)];
            f->stats.segments += ctr[MTR_CTR(CTR_SEG, k)];
        }
    }
    f->stats.binning = f->ran_direct ? 1u : 2u;
    f->stats.chunks = f->total_chunks;
    f->stats.chunks_culled = 0;
    for (int k = 0; k < CTR_NSHARDS; k++) f->stats.chunks_culled += ctr[MTR_CTR(CTR_CULL, k)];
    f->stats.shard_map = f->own ? f->own->map : 0u;
    f->stats.shard_bins = f->own ? f->own->offs[f->shard_rank + 1] - f->own->offs[f->shard_rank] : f->stats.nbins;
    f->stats_valid = true;
    return MTR_OK;
}

}  // namespace mtr_host

using namespace mtr_host;

extern "C" {

int32_t mtr_frame_submit(mtr_frame* f) {
    if (!f) return MTR_E_INVALID;
    mtr_device* d = f->dev;
    if (f->submitted) return fail(d, MTR_E_INVALID, "frame already submitted");
    std::lock_guard<std::mutex> submit_lock(d->submit_mu);
    poll_released(d);
    int32_t rc = report_sticky(d);  // an earlier frame that nobody waited for dropped triangles
    if (rc) return rc;
    rc = run_frame(f);
    if (rc) return rc;
    f->submitted = true;
    return MTR_OK;
}

int32_t mtr_frame_wait(mtr_frame* f) {
    if (!f) return MTR_E_INVALID;
    mtr_device* d = f->dev;
    if (!f->submitted) return fail(d, MTR_E_INVALID, "frame not submitted");
    if (f->waited) return MTR_OK;
    int32_t rc = set_device(d);
    if (rc) return rc;
    // wait for THIS frame only (the public stream also carries the completion of every later frame)
    if ((rc = settle_frame(f, true))) return rc;
    HIPCHK(d, hipEventSynchronize(f->fb.done));  // of the last run
    if (d->profiling && f->have_events) {
        if (f->ran_direct) {
            HIPCHK(d, hipEventElapsedTime(&f->ms[MTR_STAGE_GEOM], f->ev[0], f->ev[1]));
            f->ms[MTR_STAGE_SCAN] = f->ms[MTR_STAGE_FILL] = 0.0f;
            HIPCHK(d, hipEventElapsedTime(&f->ms[MTR_STAGE_TILE], f->ev[1], f->ev[4]));
        } else {
            for (int s = 0; s < MTR_STAGE_COUNT; s++) HIPCHK(d, hipEventElapsedTime(&f->ms[s], f->ev[s], f->ev[s + 1]));
        }
    }
    f->waited = true;
    return MTR_OK;
}

int32_t mtr_frame_end(mtr_frame* f) {
    int32_t rc = mtr_frame_submit(f);
    if (rc) return rc;
    return mtr_frame_wait(f);
}

}  // extern "C"
