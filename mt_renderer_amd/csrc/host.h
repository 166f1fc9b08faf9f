// host.h -- what the host files of libmtr.so (host_*.cpp) share: the handle structs of include/mtr.h, the internal types
// behind them, and the helpers that cross files.  Internal: mtr_files.cpp and mtr_group.cpp are written against the public
// ABI and do not include it.  Everything declared here has hidden visibility, so libmtr.so exports none of it and the
// calls between host files bind directly; everything but the handle structs (which mtr.h names) lives in mtr_host.
// Mirrors the reference's object model: Texture::new (src/texture.rs:11), Model::new / render /
// set_parts_disp (src/model.rs:36-363) and the render pass of src/bin/modelviewer.rs:190-234.
#pragma once
#include "../../include/mtr.h"
#include "mtr_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <initializer_list>
#include <thread>
#include <string>
#include <utility>
#include <vector>

#pragma GCC visibility push(hidden)

namespace mtr_host {

struct ColorDepth {
    uint32_t w, h;
    uint8_t* color;
    float* depth;
    uint32_t* counters;  // two blocks of CTR_NUM words: a frame counts in block ctr_live and its tile kernel zeroes the other
    uint32_t ctr_live = 0;
    bool ctr_dirty = true;     // the live block must be zeroed by a fill before the next run (fresh memory, or a re-run)
    bool next_zeroed = false;  // a tile kernel has been queued that zeroes the other block
    uint32_t* live() const { return counters + (size_t)ctr_live * CTR_NUM; }
    uint32_t* other() const { return counters + (size_t)(ctr_live ^ 1u) * CTR_NUM; }
    // recorded after the tile kernel of the last frame that rendered into these buffers; a frame that recycles
    // them (possibly on another internal stream) waits on it before its first write
    hipEvent_t done = nullptr;
    bool used = false;
};

// Intermediate buffers of one frame in flight, and the internal stream its kernels run on.  The device keeps
// `nslots` slots and deals frames to them round-robin: the kernels of one frame follow each other on one stream
// with no cross-stream dependency in between, and the frames of different slots overlap (frame k+1's geometry runs
// while frame k's tile kernel is still rasterising; DESIGN.md "frames in flight").  Grow-only.
// 3 slots by default (headline scene, ms per frame: 1 slot 0.094, 2: 0.066, 3: 0.056, 4: 0.071, 6: 0.058); the environment
// variable MTR_NSLOTS (1..MTR_MAX_SLOTS) overrides it at device creation.
#define MTR_MAX_SLOTS 8
struct Slot {
    RecHdr* rec_hdr = nullptr;
    RecP* rec_a = nullptr;
    int4* rec_l = nullptr;
    RecB* rec_b = nullptr;
    ChunkInfo* chunk_info = nullptr;
    uint32_t* defer_list = nullptr;  // chunks k_geom left to k_geom_clip (GeomParams::defer_list); shares chunk_cap
    uint32_t rec_cap = 0, chunk_cap = 0;
    unsigned long long* bin_count = nullptr;
    unsigned long long* bin_fill = nullptr;
    uint32_t* bin_start = nullptr;
    uint32_t* seg_start = nullptr;
    uint8_t* bin_flag = nullptr;   // mixed frames: 1 = the bin holds a translucent triangle (ordered kernel's)
    uint32_t* inst_list = nullptr;   // sharded batch draws: compacted instance lists, draw after draw
    uint32_t* inst_count = nullptr;  // one counter per draw
    uint32_t inst_cap = 0, draw_cap = 0;
    uint16_t* work_mask = nullptr;   // sharded draws: which chunks survive culling, one bit each (k_cull_chunks -> k_geom), draw after draw
    uint32_t work_cap = 0;
    bool cull_counts_dirty = true;   // inst_count (MTR_CULL_CTR_WORDS per draw: word 0 = instance-list length) needs a fill
    uint32_t ctr_clean_draws = 0;    // draws whose counters the last tile kernel cleared
    CompMat* comp = nullptr;         // sharded batch draws: per (instance, joint) composites, k_cull_instances -> k_cull_chunks
    uint32_t comp_cap = 0;
    uint32_t bin_cap = 0;
    uint32_t* entries = nullptr;  // submission order of every (triangle, bin) pair
    Seg* segs = nullptr;
    uint32_t entry_cap = 0, seg_cap = 0;
    DMat* mats = nullptr;
    uint32_t mat_cap = 0;
    bool bin_fill_dirty = true;      // direct frames leave bin_fill zeroed (the tile kernels clean up); others do not
    std::vector<DMat> mats_uploaded;  // what `mats` currently holds: steady-state frames skip the upload
    hipStream_t stream = nullptr;     // a slot's frames are ordered by this stream: reuse needs no event
};

// Which rank owns which bin, for one (frame size, map, world) combination: host lists + their device image.
struct OwnTable {
    uint32_t w = 0, h = 0, map = 0, param = 0, world = 1;
    std::vector<uint32_t> bands;  // BANDS: world + 1 bin rows
    std::vector<uint32_t> offs;   // world + 1: rank r's bins are lists[offs[r] .. offs[r+1])
    uint32_t stride_bins = 0;     // the largest share = bins per rank in an all-gather buffer
    uint32_t nsx = 0, st_shift = 0;
    std::vector<uint32_t> lists;       // host copy of d_lists (mtr_frame_read_bin_counts masks the bins a rank does not own)
    uint32_t* d_lists = nullptr;       // nbins bin ids, rank after rank, each in tile-kernel order
    uint32_t* d_src_of_bin = nullptr;  // nbins: rank * stride_bins + k
    uint32_t refs = 0;                 // live frames that use it (submit_mu)
};

struct Exchange;

}  // namespace mtr_host

struct mtr_device {
    int hip_dev = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool profiling = false;
    uint32_t texture_residency = MTR_TEXRES_DECODED;
    int tile_mode = MTR_TILE_AUTO;
    std::string err;
    mtr_host::Slot slots[MTR_MAX_SLOTS];
    uint32_t nslots = 3;
    // host run-ahead bound: submitting frame i first waits (on the host) for frame i - max_inflight.  Without it a
    // host that never waits queues thousands of commands and the runtime's per-call cost grows with the backlog
    // and memory held by queued frames is unbounded.  Default 16 (no measurable cost); MTR_MAX_INFLIGHT overrides.
    static constexpr uint32_t kMaxInflight = 64;
    hipEvent_t inflight[kMaxInflight] = {};
    uint32_t max_inflight = 16;
    uint64_t frames_submitted = 0;  // index of the next frame; frame i records inflight[i % max_inflight]
    // device buffers of destroyed batches (and retired batch versions) whose last frame may still be in flight; ev, when
    // set, is the last write into the buffer (a pose kernel or copy no frame has waited for), owned by the entry
    struct Garbage { void* p; uint64_t last_frame; hipEvent_t ev = nullptr; };
    std::vector<Garbage> garbage;
    // host poses (mtr_model_set_pose, mtr_batch_set_poses): the local matrices are copied here on s_copy and read there by
    // k_pose, so the stream orders every reuse; grown (after a sync of s_copy) only while the largest pose grows
    float* pose_stage = nullptr;
    size_t pose_stage_cap = 0;  // floats
    // Everything a frame submission touches (slots, the in-flight ring, frames_submitted, garbage, the models' chunk
    // tables and palette rings) is guarded by submit_mu: the render thread submits, but the exchange thread re-runs a
    // frame whose bin queues overflowed and destroys frames (which may own batches).  Uncontended in steady state.
    std::mutex submit_mu;
    // Frame status words, pinned host memory, one per frame in flight (frame i uses word i % max_inflight): the tile
    // kernel stores 0x80000000 | overflow flags there when it starts.  status_pending[i]: the frame that used word i
    // was released (destroyed, or handed to a consumer) without anyone having looked at its flags; they are examined
    // when the word is next polled / recycled, and a set flag is latched in sticky_err for the next API call to report.
    uint32_t* status_host = nullptr;
    uint32_t* status_dev = nullptr;
    bool status_checked[kMaxInflight] = {};   // somebody (mtr_frame_wait, the exchange thread) has looked at the word
    bool status_released[kMaxInflight] = {};  // its frame was destroyed without that: examine it at the next poll
    uint64_t status_owner[kMaxInflight] = {}; // index of the frame the word belongs to
    int status_slot_of[kMaxInflight] = {};    // which Slot that frame ran on
    int32_t sticky_err = MTR_OK;
    std::string sticky_msg;
    uint32_t queue_scale = 1;  // two-pass queues: multiplier on the default sizes, doubled when an un-waited frame overflowed them
    hipStream_t s_copy = nullptr;  // small read-backs of finished frames (statistics), independent of frames in flight
    uint32_t frame_counter = 0;
    // single-pass binning (bounded per-bin queues); a frame that overflows them is re-run with the exact
    // two-pass queues and the bound is doubled for later frames
    bool direct_enabled = true;
    uint32_t qcap = 1024, scap = 128;
    // parked colour / depth sets.  The one piece of device state a second host thread may touch: a frame can be packed
    // (mtr_frame_pack_color_shard_on_stream) and destroyed on an exchange thread while the render thread begins others.
    std::mutex pool_mu;
    std::vector<mtr_host::ColorDepth> free_fb;
    std::vector<std::pair<uint64_t, uint32_t>> fb_allocated;  // (w << 32 | h) -> colour / depth sets ever allocated
    std::vector<std::unique_ptr<mtr_host::OwnTable>> own_tables;  // grow-only cache (submit_mu)
    bool cull_enabled = true;   // sharded frames cull chunks / instances against the rank's bins
    bool cull_unsharded = false;  // MTR_GEOM_CULL_ALL_FRAMES: unsharded frames cull against the target too (frustum culling)
    uint32_t vis_waves = 0;     // MTR_VIS_WAVES: waves per bin of the visibility kernel, 0 = by the number of bins
    // timing-ablation hooks, read ONCE at device creation (never in the submit path): MTR_CULL_DEBUG in {0, 1, 3, 4, 5}
    // replaces the culling mode of maps that cull (k_cull.hip: k_cull_instances), MTR_GEOM_SLOTS bounds the instance
    // slots the full-rate sharded geometry launch covers (tests force k_geom_rest with it); 0xFFFFFFFF / 0: not set
    uint32_t cull_debug = 0xFFFFFFFFu;
    uint32_t geom_slots = 0;
    // launch-size feedback of sharded batch draws (TileParams::hint_out): two words of pinned host memory per hint slot; a
    // batch takes a slot at its first culled draw and gives it back when it is destroyed.  A late write of a frame still
    // in flight into a slot that has changed hands only mis-sizes a launch (the second geometry launch covers the rest).
    static constexpr uint32_t kHintSlots = 256;
    uint32_t* hint_host = nullptr;
    uint32_t* hint_dev = nullptr;
    bool hint_used[kHintSlots] = {};

    // Tile-kernel bin order across the 8 XCDs.  One contiguous eighth of the bins per XCD keeps the records of
    // neighbouring bins in one L2 and gives the shortest stand-alone kernel (48.9 us), but the XCDs that own the empty top
    // and bottom of a frame run dry while the middle ones work; dealing runs of a quarter bin row to the XCDs in turn
    // costs the stand-alone kernel 2-3 us (locality) and gains 4-5 % of pipelined throughput on the headline scene
    // (0.0541 -> 0.0516 ms per frame, four runs each; runs of 16 / 60 bins: 0.0518 / 0.0514), neutral on C3-C5.
    // Unsharded frames only: a rank's band is a few rows (N = 4, 8: 32.6 -> 35.5, 30.3 -> 35.0 us per frame with runs).
    // And only while the previous frame is still on the GPU (one event query per frame): a frame that has the GPU to
    // itself keeps the contiguous order and its shorter kernel.  MTR_TILE_RUN overrides (0 = contiguous eighths).
    static constexpr uint32_t kXcdRunAuto = 0xFFFFFFFFu;
    uint32_t xcd_run = kXcdRunAuto;
    mtr_model* cube = nullptr;  // debug-overlay cube, created lazily
    mtr_host::Exchange* xchg = nullptr;  // exchange thread of a sharded device (mtr_device_exchange_start)
};

namespace mtr_host {

// The exchange of a sharded frame (pack -> the host's all-gather -> unpack -> frame destroy) issued by a second host
// thread: a rank's share of a small frame is ~30 us of GPU time, the render submission alone costs the host ~30 us, and
// the three exchange calls another ~15 us -- on one thread they add, on two they overlap.
struct Exchange {
    mtr_allgather_fn fn = nullptr;
    void* comm = nullptr;
    int dtype_u8 = 0;
    uint8_t *send = nullptr, *gathered = nullptr, *dst = nullptr;
    size_t send_bytes = 0;
    uint32_t world = 1;
    hipStream_t stream = nullptr;
    // further lanes (mtr_device_exchange_add_lane): frames are dealt to the lanes in turn, lane 0 being the fields above.
    // A lane is an in-order stream, so one lane completes one (pack + all-gather + unpack) latency per frame; two lanes
    // with a communicator each keep two collectives in flight.
    struct Lane { void* comm; uint8_t *send, *gathered, *dst; hipStream_t stream; };
    std::vector<Lane> lanes;
    uint64_t dealt = 0;  // frames taken by the thread so far
    std::thread th;
    std::mutex mu;
    std::condition_variable cv_items, cv_idle;
    std::deque<mtr_frame*> q;
    std::atomic<uint32_t> pending{0};  // queued + being processed
    bool stop = false;
    int32_t err = MTR_OK;
    std::string err_msg;
    static constexpr size_t kDepth = 8;  // frames handed over and not yet issued
};

}  // namespace mtr_host

struct mtr_texture {
    mtr_device* dev;
    uint32_t w, h, fmt;
    uint32_t levels = 1;  // mip levels in d_rgba, level 0 first
    uint8_t* d_rgba;          // decoded RGBA8 texels (MTR_TR_RGBA8) or the BC blocks as uploaded (MTR_TR_BC1 / MTR_TR_BC7)
    uint32_t resident = MTR_TR_RGBA8;
    bool opaque;  // every decoded texel (of every level) has alpha == 255: sampling it yields a == 1 exactly
};

namespace mtr_host {

// The chunk table of a model under one parts_disp: immutable once built.  A draw holds the table that was current when
// it was recorded (Model::render reads parts_disp while it records, src/model.rs:318-320), so a frame that is re-run
// after a queue overflow -- possibly by the exchange thread, possibly after the host has changed parts_disp for a later
// frame -- reproduces exactly what was submitted, and nobody rewrites a table a kernel or another thread is reading.
struct ChunkTable {
    int hip_dev = 0;
    std::vector<DChunk> chunks;
    DChunk* d_chunks = nullptr;
    uint64_t ntris_visible = 0;
    ~ChunkTable() {
        if (!d_chunks) return;
        (void)hipSetDevice(hip_dev);
        (void)hipDeviceSynchronize();  // frames that drew with it may still be in flight; tables die rarely (parts_disp changed)
        (void)hipFree(d_chunks);
    }
};

}  // namespace mtr_host

struct mtr_model {
    mtr_device* dev;
    uint8_t* d_vbuf = nullptr;
    uint16_t* d_ibuf = nullptr;
    DPrim* d_prims = nullptr;
    std::shared_ptr<const mtr_host::ChunkTable> table;  // for the current parts_disp; rebuilt by the next draw when chunks_dirty (submit_mu)
    float* d_palette = nullptr;   // the current palette: one buffer of pal_ring
    // skeleton of mtr_model_set_skeleton (what k_pose needs): immutable once uploaded; replacing it waits for the device
    struct Skeleton {
        uint32_t njoints = 0, path_bytes = 0;
        float* d = nullptr;            /* imats (njoints * 16 f32), paths (njoints u32), path bytes */
        std::vector<uint8_t> parents;  /* as given, a root as 255: what an IK set's parents are compared with */
    };
    Skeleton skel;
    uint32_t npal = 0;
    // mtr_model_set_palette does not wait for frames in flight: every call uploads into the next buffer of a ring
    // (max_inflight + 1 of them) on the copy stream and records an event; a frame captures pointer + event when the
    // model is drawn and its stream waits on the event.  A ring buffer comes round again only after max_inflight + 1
    // palette changes; if the last frame that read it can still be in flight (many changes, few frames) the call waits
    // for exactly that frame first.
    // pinned: frames that drew the model with this buffer and may still (re-)run: recorded and not yet submitted, or
    // submitted and their overflow flags not yet examined (a frame whose bin queues overflowed is run again); the pin is
    // dropped when the flags turn out clean, or when the frame is destroyed
    struct PalBuf { float* d = nullptr; uint32_t cap = 0; hipEvent_t ready = nullptr; uint64_t last_frame = 0; bool used = false; uint32_t pinned = 0; };
    std::vector<PalBuf> pal_ring;
    size_t pal_next = 0;
    hipEvent_t pal_ready = nullptr;  // of the current palette
    int pal_slot = -1;               // its index in pal_ring
    std::vector<DPrim> prims;
    std::vector<uint16_t> indices;
    std::vector<uint32_t> run;  // consecutive non-restart indices ending at each position
    std::vector<uint8_t> parts_disp;
    std::vector<int32_t> prim_to_texture;
    std::vector<mtr_texture*> textures;
    std::vector<uint32_t> debug_rgba8;
    std::vector<mtr_prim_state> states;  // material state per primitive, empty: the reference's pipeline state
    std::vector<float> joint_cubes;      // one instance matrix per joint: scale 0.005, translation = offset * 0.01 (src/model.rs:309-315)
    bool chunks_dirty = true;
    size_t vertex_len = 0;
    // culling bounds (multi-GPU v2), computed once at creation over every chunk of every primitive, whatever parts_disp
    // says: chunk k of primitive p is static chunk prim_chunk_base[p] + k
    std::vector<uint32_t> prim_chunk_base;
    std::vector<uint32_t> cb_first, cb_count, cb_flags;  // per static chunk: its boxes in d_boxes
    BoneBox* d_boxes = nullptr;
    // whole-model boxes for instance culling: [0, n_inst_unskinned) what a draw without palette transforms (one box),
    // [n_inst_unskinned, +n_inst_skinned) what a skinned draw does (the unskinnable primitives' box, then one per joint)
    BoneBox* d_inst_boxes = nullptr;
    uint32_t n_inst_unskinned = 0, n_inst_skinned = 0;
    bool inst_skinned_boundable = false;  // every skinned vertex's weights sum to 255
};

struct mtr_batch {
    mtr_device* dev;
    mtr_model* model;
    uint32_t n = 0;
    // Versions of the instance data.  mtr_batch_create writes the first; every mtr_batch_update / _set_poses writes a fresh
    // one (never the current one, nor one a frame may still read) and makes it current.  A draw records the current version
    // and pins it until its frame can no longer (re-)run, like the model's palette ring; the ring grows while every version
    // is held or in flight (up to max_inflight + 1 before it waits for a frame), so the steady state allocates nothing.
    // d: n model matrices, then n * npal palette matrices (cap floats); ready: the last write into d (copy stream, or the
    // caller's stream of mtr_batch_set_poses_device); frames that draw the version wait on it.
    // read: recorded behind the last outside reader of d, a k_attach launched for ANOTHER batch's update or for a socket call
    // (SPEC.md section 18), on a stream this batch's updates need not share.  A reader queued on another stream than the one
    // before first waits for it, so the one event covers every reader (as DeviceSet::last does).  read_pending: recorded since
    // the version's last write; that write's successor waits for it, and a buffer retired meanwhile is parked behind it.
    struct Ver {
        float* d = nullptr; size_t cap = 0; uint32_t npal = 0; hipEvent_t ready = nullptr; uint64_t last_frame = 0; bool used = false; uint32_t pinned = 0;
        hipEvent_t read = nullptr; hipStream_t read_stream = nullptr; bool read_pending = false;
    };
    std::vector<Ver> vers;
    int cur = 0;
    uint32_t refs = 1;           // the handle + every recorded draw (submit_mu): the last one parks the versions
    std::vector<int32_t> tex_override;
    uint64_t last_frame = 0;     // last frame that drew it: its buffers are freed only once that frame has left the GPU
    bool used = false;
    int hint_slot = -1;          // mtr_device::hint_host slot, or -1
    uint64_t hint_key = 0;       // the ownership (table, rank) the slot's numbers were reported under
};

namespace mtr_host {

// What the ten set handles below share: device memory `d`, uploaded once, and the event that covers its readers.  `last` is
// recorded behind every kernel that reads d (set_after); a kernel queued on another stream than the one before first waits
// for it (set_before), so the one event always covers every reader and the set's destroy can park d behind it (set_park).
struct DeviceSet {
    mtr_device* dev = nullptr;
    uint32_t* d = nullptr;
    hipEvent_t last = nullptr;
    hipStream_t last_stream = nullptr;
    bool recorded = false;
};

}  // namespace mtr_host

// An animation set (SPEC.md section 14): immutable once uploaded.  d: the clip table (nclips x 4 words: first key, key count,
// flags, 0), then the keys.  A track set (section 15) is the same object with tracks set.  Then d holds: the clip table (0,
// length in ticks, flags, 0), nclips * njoints * 3 descriptors of 32 bytes, nkeys key values of 8 bytes, nkeys u16 key times
// (host_anim.cpp: ClipImage).
struct mtr_anim : mtr_host::DeviceSet {
    uint32_t njoints = 0, nclips = 0;
    bool tracks = false;
    uint32_t nkeys = 0;          // a track set's key total
    bool has_loop = false;       // a clip carries MTR_CLIP_LOOP: no trajectory for root motion (section 19)
};

// A mask set (SPEC.md section 16): immutable once uploaded.  d: nmasks x njoints weights (the user's masks 1..nmasks).
struct mtr_anim_masks : mtr_host::DeviceSet {
    uint32_t njoints = 0, nmasks = 0;
    const float* weights() const { return reinterpret_cast<const float*>(d); }
};

// An IK set (SPEC.md section 17): immutable once uploaded.  d: nchains x 8 words of validated chains, the path table
// (njoints u32) and the path bytes of the skeleton its parents describe (what mtr_anim_sample_ik walks; the animate calls
// walk the model's own, after comparing the parents).
struct mtr_anim_ik : mtr_host::DeviceSet {
    uint32_t njoints = 0, nchains = 0, path_bytes = 0;
    std::vector<uint8_t> parents;  // a root as 255
};

// A spring set (SPEC.md section 24): immutable once uploaded.  d: nsprings x 12 words of validated springs, the joint table
// (njoints u32: the joint's spring | its round << 8, or MTR_SPRING_NONE), then the path table and the path bytes as in an IK
// set.  Its kernels write the caller's states, not d; `last` orders the calls on one set among themselves all the same.
struct mtr_anim_spring : mtr_host::DeviceSet {
    uint32_t njoints = 0, nsprings = 0, nrounds = 0, path_bytes = 0;
    std::vector<uint8_t> parents;  // a root as 255
};

// A root set (SPEC.md section 19): immutable once uploaded.  d: nclips flag words (MTR_ROOT_CYCLIC).
struct mtr_anim_root : mtr_host::DeviceSet {
    uint32_t njoints = 0, nclips = 0, joint = 0;
};

// A player set (SPEC.md section 20).  d: nclips table entries of 4 words (period, flags, rate, key count), immutable, then
// the scratch array of max_instances words, zero between calls.  cmds: where host commands are staged, grown on demand
// (the outgrown buffer parked behind cmd_last, the event of the last kernel that read it).  A player's kernels also WRITE d
// (the scratch), so `last` orders the calls on one player among themselves.
struct mtr_anim_player : mtr_host::DeviceSet {
    uint32_t nclips = 0, max_instances = 0;
    uint32_t* cmds = nullptr;
    size_t cmd_cap = 0;  // commands
    hipEvent_t cmd_last = nullptr;
};

// A controller (SPEC.md section 21): immutable once uploaded and only read by its kernels.  d: nclips table entries of 4
// words (period, flags, 0, key count), then nnodes nodes of 4 words, then ntrans transitions of 12 words, each part a
// multiple of 16 bytes.
struct mtr_anim_ctrl : mtr_host::DeviceSet {
    uint32_t nclips = 0, nnodes = 0, ntrans = 0, nany = 0, nparams = 0;
};

// An event set (SPEC.md section 22).  d: nclips table entries of 4 words (period, flags, 0, key count), then nclips ranges of
// 2 words (first marker, marker count), then the markers of 2 words, each part padded to a multiple of 16 bytes, all
// immutable; then the scratch array of ceil(max_instances / 256) block sums.  Its kernels WRITE the scratch, so `last`
// orders the calls on one set among themselves, as a player's.
struct mtr_anim_events : mtr_host::DeviceSet {
    uint32_t nclips = 0, max_instances = 0, nmarkers = 0, max_count = 0;
    size_t w_ranges = 0, w_markers = 0;  // words of the padded range and marker parts
};

// A blend set (SPEC.md section 23): immutable once uploaded and only read by its kernel.  d: nclips table entries of 4 words
// (period, flags, rate, key count), then nsamples samples of 4 words, then ntris triangles of 4 words.
struct mtr_anim_blend : mtr_host::DeviceSet {
    uint32_t nclips = 0, nsamples = 0, ntris = 0, nparams = 0, param_x = 0, param_y = 0, max_instances = 0;
    float damp = 0.0f;
};

// A match set (SPEC.md section 25).  d: nclips table entries of 4 words (period, flags, 0, key count), nclips ranges of 2 words
// (first row, row count), the rows of 4 words, Rp (R rounded up to 32) c_r, Rp tag words, Rp x Dp features tile-major
// (match_math.h: match_slot), Dp means and Dp scales, each part padded to a multiple of 16 bytes, all immutable; then the
// scratch: the queries of max_instances rounded up to 32 (tile-major), max_instances current rows and max_instances 64-bit
// winner keys.  Its kernels WRITE the scratch, so `last` orders the calls on one set among themselves, as a player's.
struct mtr_anim_match : mtr_host::DeviceSet {
    uint32_t nclips = 0, R = 0, D = 0, flags = 0, max_instances = 0;
    uint64_t pose_dims = 0;
    float seconds = 0.0f, near_x = 0.0f, margin = 0.0f;
    size_t w_ranges = 0;  // words of the padded range part
};

namespace mtr_host {

struct BatchDeleter {
    void operator()(mtr_batch* b) const { mtr_batch_destroy(b); }
};

struct Draw {
    mtr_model* model;
    std::shared_ptr<const ChunkTable> table;  // the model's chunk table when the draw was recorded
    const float* d_model_mats;  // nullptr: M = view_proj
    const float* d_palettes;
    hipEvent_t pal_ready;  // upload of d_palettes / d_model_mats on the copy stream (model palette ring, or the batch)
    mtr_batch* batch;      // drawn batch (not owned unless owned_batch), for its last-use bookkeeping
    int pal_slot;          // ring buffer of the model palette, or -1
    uint32_t npal, pal_stride, ninst;
    float vp[16];
    std::vector<int32_t> tex_override;  // per instance or empty
    int shader_override;                // -1 or MTR_SH_CONST (overlay)
    uint32_t const_rgba8;
    bool blend;
    bool pal_pinned = false;  // holds a pin on the model's palette ring buffer pal_slot until the frame is submitted
    int batch_ver = -1;       // version of `batch` the draw recorded, pinned while ver_pinned; the draw holds a batch ref
    bool ver_pinned = false;
    std::unique_ptr<mtr_batch, BatchDeleter> owned_batch;
};

}  // namespace mtr_host

struct mtr_frame {
    mtr_device* dev;
    uint32_t w, h;
    uint32_t clear_rgba8;
    float clear_depth;
    mtr_host::ColorDepth fb;
    uint32_t shard_rank = 0, shard_world = 1;
    const mtr_host::OwnTable* own = nullptr;  // ownership map of a sharded frame (cached in the device), nullptr: not sharded
    std::vector<mtr_host::Draw> draws;
    std::vector<DMat> mats_host;  // kept alive until the async upload has certainly been consumed
    bool submitted = false, waited = false, all_opaque = true, force_two_pass = false, ran_direct = false;
    mtr_frame_stats stats{};
    hipEvent_t ev[MTR_STAGE_COUNT + 1] = {};
    bool have_events = false;
    float ms[MTR_STAGE_COUNT] = {};
    int slot = 0;
    uint64_t total_chunks = 0;
    uint64_t min_entries = 0, min_segs = 0;  // queue sizes measured by a previous, overflowed attempt
    bool for_exchange = false;  // submitted through mtr_frame_submit_exchange: no public-stream consumer
    int status_idx = -1;        // this frame's word of mtr_device::status_host (set by run_frame)
    uint64_t frame_index = 0;   // its index in submission order (of the last run)
    bool flags_checked = false; // somebody has examined this run's overflow flags
    bool stats_valid = false;   // f->stats holds the device counters of the last run
};

namespace mtr_host {

// ---- host_device.cpp ----
extern std::mutex g_err_mu;  // two host threads (render + exchange) may fail at once
int32_t fail(mtr_device* d, int32_t code, const std::string& msg);

#define HIPCHK(dev, call)                                                                          \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail((dev), MTR_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));      \
    } while (0)

inline uint32_t quant8(float x) {
    if (!(x > 0.0f)) x = 0.0f;
    if (x > 1.0f) x = 1.0f;
    return (uint32_t)std::rint(x * 255.0f);
}

inline uint32_t pack_rgba8(const float c[4]) {
    return quant8(c[0]) | (quant8(c[1]) << 8) | (quant8(c[2]) << 16) | (quant8(c[3]) << 24);
}

template <class T>
int32_t dev_alloc(mtr_device* d, T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T));
    if (e != hipSuccess) return fail(d, MTR_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return MTR_OK;
}

template <class T>
int32_t dev_grow(mtr_device* d, T** p, uint32_t* cap, size_t need) {
    if (need <= *cap && *p) return MTR_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    int32_t rc = dev_alloc(d, p, need);
    if (rc) return rc;
    *cap = (uint32_t)need;
    return MTR_OK;
}

// Grows the buffers of a slot that share the capacity *cap to `need` elements, if `need` exceeds it or any of them is null
// (an earlier growth that ran out of memory): waits for the slot's stream (and for `also`, if another stream reads the
// buffers) once, grows every pointer, and commits the capacity only when all of them succeeded, so that a failure leaves a
// state the next frame grows again.  *grew (optional): whether it did.  The only place that pairs a sync with dev_grow.
template <class... T>
int32_t grow_slot(mtr_device* d, Slot& sl, hipStream_t also, bool* grew, size_t need, uint32_t* cap, T**... ptrs) {
    const bool grow = need > *cap || (!*ptrs || ...);
    if (grew) *grew = grow;
    if (!grow) return MTR_OK;
    HIPCHK(d, hipStreamSynchronize(sl.stream));
    if (also) HIPCHK(d, hipStreamSynchronize(also));
    int32_t rc = MTR_OK;
    auto one = [&](auto** p) { uint32_t c = *cap; if (!rc) rc = dev_grow(d, p, &c, need); };
    (one(ptrs), ...);
    if (!rc) *cap = (uint32_t)need;
    return rc;
}

int32_t set_device(mtr_device* d);
int32_t drain_all(mtr_device* d);
inline uint32_t status_load(const mtr_device* d, int i) { return __atomic_load_n(&d->status_host[i], __ATOMIC_ACQUIRE); }

void grow_direct_queues(mtr_device* d);
void examine_status(mtr_device* d, int i, bool force);
void poll_released(mtr_device* d);
int32_t report_sticky(mtr_device* d);

// ---- host_model.cpp ----
int32_t current_table(mtr_model* m, std::shared_ptr<const ChunkTable>* out);
int32_t next_palette_buffer(mtr_model* m, size_t n, mtr_model::PalBuf** out);
bool pose_paths(const uint8_t* parents, size_t n, std::vector<uint32_t>& paths, std::vector<uint8_t>& bytes);

// ---- host_batch.cpp ----
int32_t stage_pose(mtr_device* d, const float* local_mats, size_t count);
int32_t stage_ik(mtr_device* d, const mtr_anim_layer* layers, size_t nl, const mtr_ik_target* targets, size_t nt, const void** targets_dev);
PoseParams pose_params(const mtr_model::Skeleton& sk, const float* locals, float* out);
// Buffers and events nobody can use any more, collected under submit_mu and released after it (release_now).
struct FreeList {
    std::vector<void*> bufs;
    std::vector<hipEvent_t> events;
};
void release_now(FreeList& fl);
void batch_unref(mtr_batch* b, FreeList& fl);

// ---- host_anim.cpp ----
// the stream of a device call: the caller's, or the device's own
inline hipStream_t caller_stream(const mtr_device* d, void* hip_stream) { return hip_stream ? static_cast<hipStream_t>(hip_stream) : d->stream; }
// One part of a set's device image: bytes from p, or bytes of zeroes (p == nullptr: filled on the copy stream and waited for).
struct Part { const void* p; size_t bytes; };
// Allocates s->d for the parts behind each other, uploads them in order and creates s->last; "<what> upload: ..." on failure
int32_t set_upload(DeviceSet* s, const char* what, std::initializer_list<Part> parts);
// One entry of the clip table the clock sets share (players, controllers, event sets, blend sets; play_math.h: PlayClip),
// validated and written: out = period, flags, rate (rates == nullptr: 0, and no rate check), key count.  The one place that
// forms the period, so the sets' periods are bit-equal (SPEC.md sections 21 to 23).  "<who>: clip <c> has ..." on failure.
constexpr size_t kClipMaxKeys = (size_t)1 << 24;
int32_t clip_entry(mtr_device* d, const char* who, size_t c, const uint32_t* nkeys, uint32_t flags, const float* rates, uint32_t* out);
// around a kernel on `st` that reads (a player: also writes) the set: see DeviceSet::last
int32_t set_before(DeviceSet* s, hipStream_t st);
int32_t set_after(DeviceSet* s, hipStream_t st);
// a kernel may still read the set: d is parked behind the event of the last one, collected by a later submit
void set_park(DeviceSet* s);
// Device scratch for one synchronous host call: the caller's arrays as parts of one block, part behind part in the order they
// were named.  A part of 0 words is absent: it takes no room, dev() is nullptr and up / down skip it.
struct StagedPart {
    void* host;
    size_t words;  // 4-byte words
    char* at;      // where the part starts in the block (an absent part: where the next one does), set by StagedBlock::run
    template <class T>
    T* dev() const { return words ? reinterpret_cast<T*>(at) : nullptr; }
};
struct StagedBlock {
    mtr_device* d;
    StagedPart parts[6];
    int nparts = 0;
    explicit StagedBlock(mtr_device* dev) : d(dev) {}
    StagedPart& part(const void* host, size_t words) { return parts[nparts++] = StagedPart{const_cast<void*>(host), words, nullptr}; }
    // copies on the copy stream, in the order given: host to device, device to host
    int32_t up(std::initializer_list<const StagedPart*> ps) {
        for (const StagedPart* p : ps)
            if (p->words) HIPCHK(d, hipMemcpyAsync(p->at, p->host, p->words * 4, hipMemcpyHostToDevice, d->s_copy));
        return MTR_OK;
    }
    int32_t down(std::initializer_list<const StagedPart*> ps) {
        for (const StagedPart* p : ps)
            if (p->words) HIPCHK(d, hipMemcpyAsync(p->host, p->at, p->words * 4, hipMemcpyDeviceToHost, d->s_copy));
        return MTR_OK;
    }
    // Allocates the block and places the parts; call() queues copies in, kernels and copies out on the copy stream, which is
    // waited for also when a step failed, since the block is freed next.
    template <class F>
    int32_t run(F&& call) {
        size_t words = 0;
        for (int i = 0; i < nparts; i++) words += parts[i].words;
        uint32_t* block = nullptr;
        int32_t rc = dev_alloc(d, &block, words);
        if (rc) return rc;
        char* at = reinterpret_cast<char*>(block);
        for (int i = 0; i < nparts; i++) { parts[i].at = at; at += parts[i].words * 4; }
        rc = call();
        const hipError_t e = hipStreamSynchronize(d->s_copy);
        (void)hipFree(block);
        if (!rc && e != hipSuccess) rc = fail(d, MTR_E_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
        return rc;
    }
};
// One animate call: which sets it reads and where its records lie in device memory.  kind says which records: one state per
// instance, nlayers layers per instance (masks optional), such layers and then ik->nchains targets per instance, or such
// layers, targets where there is an IK set (optional here) and spring->nsprings spring states per instance, read and written.
struct AnimCall {
    enum Kind { kStates, kLayers, kIk, kSpring };
    Kind kind = kStates;
    mtr_anim* anim = nullptr;
    mtr_anim_masks* masks = nullptr;
    mtr_anim_ik* ik = nullptr;
    const void* recs = nullptr;     // the states or the layers
    size_t nlayers = 0;             // layers per instance of a layered call, as the caller gave it (anim_check: 1 to 8)
    const void* targets = nullptr;
    mtr_anim_spring* spring = nullptr;
    void* spring_states = nullptr;
    const float* motion = nullptr;  // or nullptr
    float dt = 0.0f;
};
// What every animate call checks of its sets, in one order: against the model's skeleton, or (m == nullptr) for a sample call,
// which has none; no_room: the message of a sample call whose size test failed, reported where that test stands
int32_t anim_check(mtr_device* d, const mtr_model* m, const AnimCall& c, const char* no_room = nullptr);
// The one place that runs k_anim*: the sets' events around the launcher of the call's kind and the set's kind.  sk: the
// skeleton the palettes (out) are folded with; nullptr: a sample call, out takes the local matrices and the caller waits
// for the stream, so no event is touched.
int32_t anim_enqueue(const AnimCall& c, const mtr_model::Skeleton* sk, float* out, uint32_t ninst, hipStream_t s);
// host_batch.cpp: the palettes of an animate call, its records in device memory -- a fresh version of the batch, written on s
int32_t batch_animate(mtr_batch* b, const AnimCall& c, hipStream_t s);
// a set's destroy: parked behind its event, the handle freed
template <class Set>
void set_destroy(Set* s) {
    if (!s) return;
    set_park(s);
    delete s;
}
// root motion (section 19): what every call checks, and k_root (mats_in * D) or k_root_deltas (mats_in == nullptr: D) on s
int32_t root_check(mtr_device* d, const mtr_anim* traj, const mtr_anim_root* root, size_t nsteps, bool deltas);
int32_t root_enqueue(mtr_anim* traj, mtr_anim_root* root, const void* steps_dev, size_t nsteps, size_t n, const float* mats_in, float* out, hipStream_t s);

// ---- host_frame.cpp ----
void release_palette_pins(mtr_frame* f);

// ---- host_submit.cpp ----
int32_t settle_frame(mtr_frame* f, bool wait_done);
int32_t fetch_stats(mtr_frame* f);

// ---- host_shard.cpp ----
int32_t get_own_table(mtr_device* d, uint32_t w, uint32_t h, uint32_t world, uint32_t map, uint32_t param, const uint32_t* band_rows,
                      const OwnTable** out);

}  // namespace mtr_host

#pragma GCC visibility pop
