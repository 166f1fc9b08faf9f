// The launch sequence of a frame, pinned on the CPU: the host side of the library (csrc/host_*.cpp) over the stand-in HIP
// runtime of tests/cpp/hip_stub, with kernel launchers that append one line per launch to a log and a trace hook that adds
// the memsets, uploads, stream waits, event records and stream syncs in between.  A line holds the kernel's name and the
// scalar fields that encode a host decision (DESIGN.md "frames in flight", "binning", "tile kernels", "multi-GPU v2");
// pointers appear only as 0 / 1 (null / set) or as the NAME of the buffer, event or stream they are.  Every launcher also
// requires every buffer of the FrameBuffers it is handed to be non-null.  The expected logs are written out below.
// usage: frame_launch_log            every scenario but the allocation failures
//        frame_launch_log nomem      hipMalloc failing at each allocation of a frame in turn
#define MTR_HARNESS_OWN_GEOM
#define MTR_HARNESS_OWN_SCAN
#define MTR_HARNESS_OWN_FILL
#define MTR_HARNESS_OWN_TILE
#define MTR_HARNESS_OWN_TILE_VIS
#define MTR_HARNESS_OWN_CULL_INSTANCES
#define MTR_HARNESS_OWN_CULL_CHUNKS
#define MTR_HARNESS_OWN_TRACE
#include "harness.h"

#include <cstdarg>

typedef std::vector<std::string> Log;
static Log g_log;
static mtr_frame* g_frame = nullptr;     // the frame being submitted: names its events and buffers in the log
static bool g_null_is_fatal = true;
static std::string g_null;               // nomem: the first null buffer a launcher was handed
static uint32_t g_flag_once = 0;         // overflow flags the next tile launch publishes (once)
static uint32_t g_measured[2] = {0, 0};  // what that launch leaves in CTR_ENTRIES / CTR_SEGS (flag 2: "what the scan measured")
static std::vector<FrameBuffers> g_geom_fb;  // FrameBuffers of every geometry launch since the last clear
static uint32_t g_vis_waves = ~0u;       // TileParams::vis_waves of the last tile launch (remembered, not logged)
// A draw's share of the slot's four culling buffers, as element offsets from the slot's buffer (remembered, not logged): one
// entry per k_cull_chunks launch = per draw of a culled frame, checked against the k_cull_instances launch in front of it and
// the geometry launch behind it.  -1: the launch was handed a null pointer.
struct DrawRanges { uint32_t nx, ninst; long work, list, strad, comp, count; };
static std::vector<DrawRanges> g_ranges;
static const CullParams* g_cull_inst = nullptr;  // the k_cull_instances launch the next k_cull_chunks launch belongs to
static CullParams g_cull_inst_copy;
static int g_range_mismatch = 0;                 // launches of one draw that were handed different ranges
static bool g_remember = false;                  // inside logged(): g_frame is the frame being submitted
template <class T>
static long off_in(const T* p, const T* base) { return p ? (long)(p - base) : -1; }

static std::string S(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}

static void need(const void* p, const char* who, const char* what) {
    if (p) return;
    if (g_null_is_fatal) { fprintf(stderr, "%s was handed a null %s\n", who, what); abort(); }
    if (g_null.empty()) g_null = S("%s: null %s", who, what);
}
static void need_fb(const FrameBuffers& fb, const char* who) {
    need(fb.rec_hdr, who, "rec_hdr"); need(fb.rec_a, who, "rec_a"); need(fb.rec_l, who, "rec_l"); need(fb.rec_b, who, "rec_b");
    need(fb.chunk_info, who, "chunk_info"); need(fb.bin_count, who, "bin_count"); need(fb.bin_fill, who, "bin_fill");
    need(fb.bin_start, who, "bin_start"); need(fb.seg_start, who, "seg_start"); need(fb.entries, who, "entries");
    need(fb.segs, who, "segs"); need(fb.counters, who, "counters");
    if (fb.own.world != 1) need(fb.own.own_list, who, "own.own_list");
}

void mtr_launch_geom(const GeomParams& p, hipStream_t) {
    need_fb(p.fb, "geom"); need(p.mats, "geom", "mats");
    g_geom_fb.push_back(p.fb);
    if (p.work_mask && g_remember) {  // the masks, the list and the counters k_cull_chunks wrote for this draw
        const Slot& sl = g_frame->dev->slots[g_frame->slot];
        if (g_ranges.empty() || g_ranges.back().work != off_in(p.work_mask, sl.work_mask) || g_ranges.back().list != off_in(p.inst_list, sl.inst_list) ||
            g_ranges.back().count != off_in(p.inst_count, sl.inst_count) || g_ranges.back().nx != p.work_nx) g_range_mismatch++;
    }
    g_log.push_back(S("geom nchunks=%u ninst=%u chunk_base=%u mat_base=%u small_draw=%u work_mask=%d inst_list=%d direct=%u unordered=%u "
                      "own={map=%u rank=%u world=%u cull=%u own_count=%u}", p.nchunks, p.ninst, p.chunk_base, p.mat_base, p.small_draw,
                      p.work_mask != nullptr, p.inst_list != nullptr, p.fb.direct, p.fb.unordered, p.fb.own.map, p.fb.own.rank, p.fb.own.world,
                      p.fb.own.cull, p.fb.own.own_count));
}
void mtr_launch_scan(const FrameBuffers& fb, hipStream_t) { need_fb(fb, "scan"); g_log.push_back("scan"); }
void mtr_launch_fill(const FrameBuffers& fb, uint32_t total_chunks, hipStream_t) { need_fb(fb, "fill"); g_log.push_back(S("fill total_chunks=%u", total_chunks)); }
static void tile_stub(const char* name, const TileParams& p, bool textured) {
    need_fb(p.fb, name); need(p.mats, name, "mats"); need(p.bin_flag, name, "bin_flag"); need(p.color, name, "color"); need(p.depth, name, "depth");
    need(p.host_status, name, "host_status");
    if (p.fb.own.own_count == 0) return;  // the real launchers return here: a rank without a bin launches no workgroup
    g_vis_waves = p.vis_waves;
    g_log.push_back(S("%s mixed=%u nhint=%u zero_words=%d zero_nwords=%u hint_out=%d zero_next=%d xcd_run=%u textured=%d", name, p.mixed, p.nhint,
                      p.zero_words != nullptr, p.zero_nwords, p.hint_out != nullptr, p.zero_next != nullptr, p.xcd_run, (int)textured));
    // what tile_prologue does on the device: publish the overflow flags of the frame
    if (g_flag_once & 2u) { p.fb.counters[CTR_ENTRIES] = g_measured[0]; p.fb.counters[CTR_SEGS] = g_measured[1]; }
    if (p.host_status) __atomic_store_n(p.host_status, 0x80000000u | g_flag_once, __ATOMIC_RELEASE);
    g_flag_once = 0;
}
void mtr_launch_tile(const TileParams& p, bool textured, hipStream_t) { tile_stub("tile", p, textured); }
void mtr_launch_tile_vis(const TileParams& p, bool textured, hipStream_t) { tile_stub("tile_vis", p, textured); }
void mtr_launch_cull_instances(const CullParams& p, hipStream_t) {
    need(p.boxes, "cull_instances", "boxes"); need(p.list, "cull_instances", "list"); need(p.count, "cull_instances", "count");
    need(p.comp, "cull_instances", "comp"); need(p.work_mask, "cull_instances", "work_mask"); need(p.strad, "cull_instances", "strad");
    need(p.counters, "cull_instances", "counters");
    g_cull_inst_copy = p; g_cull_inst = &g_cull_inst_copy;
    g_log.push_back(S("cull_instances ninst=%u", p.ninst));
}
void mtr_launch_cull_chunks(const ChunkCullParams& p, hipStream_t) {
    need_fb(p.fb, "cull_chunks"); need(p.work_mask, "cull_chunks", "work_mask");
    g_log.push_back(S("cull_chunks keep_all=%u inst_count=%d comp=%d", p.keep_all, p.inst_count != nullptr, p.comp != nullptr));
    if (!g_remember) return;
    const Slot& sl = g_frame->dev->slots[g_frame->slot];
    g_ranges.push_back(DrawRanges{(p.nchunks + 15u) / 16u, p.ninst, off_in(p.work_mask, sl.work_mask), off_in(p.inst_list, sl.inst_list),
                                  off_in(p.strad, sl.inst_list), off_in(p.comp, sl.comp), off_in(p.inst_count, sl.inst_count)});
    if (p.inst_count) {  // k_cull_instances wrote what this launch reads
        const CullParams* ci = g_cull_inst;
        if (!ci || ci->work_mask != p.work_mask || ci->list != p.inst_list || ci->strad != p.strad || ci->comp != p.comp || ci->count != p.inst_count ||
            ci->ninst != p.ninst || ci->nchunks != p.nchunks) g_range_mismatch++;
    } else if (g_cull_inst) g_range_mismatch++;
    g_cull_inst = nullptr;
}

// ---- the trace hook: streams, events and buffers by name ----
static std::string stream_name(const mtr_device* d, const void* s) {
    for (uint32_t i = 0; i < d->nslots; i++)
        if (s == d->slots[i].stream) return S("slot%u", i);
    return s == d->stream ? "public" : s == d->s_copy ? "copy" : "?";
}
static const char* what_name(const mtr_frame* f, const void* w) {
    const mtr_device* d = f->dev;
    static const char* evs[] = {"ev[0]", "ev[1]", "ev[2]", "ev[3]", "ev[4]"};
    for (int i = 0; i <= MTR_STAGE_COUNT; i++)
        if (f->have_events && w == f->ev[i]) return evs[i];
    if (w == f->fb.done) return "fb.done";
    if (w == f->fb.live()) return "counters";
    for (const Draw& dr : f->draws)
        if (w == dr.pal_ready) return "pal_ready";
    for (hipEvent_t e : d->inflight)
        if (e && w == e) return "ring";
    for (uint32_t i = 0; i < d->nslots; i++) {
        const Slot& sl = d->slots[i];
        if (w == sl.bin_count) return "bin_count";
        if (w == sl.bin_fill) return "bin_fill";
        if (w == sl.chunk_info) return "chunk_info";
        if (w == sl.inst_count) return "cull_counters";
        if (w == sl.mats) return "mats";
    }
    return "other";
}
static void trace(const char* name, size_t bytes, const void* what, const void* stream) {
    std::string line = name;
    if (what) line += std::string(" ") + what_name(g_frame, what);
    if (bytes) line += S(" %zu", bytes);
    g_log.push_back(line + " " + stream_name(g_frame->dev, stream));
}

// ---- scenes ----
static const float kClear[4] = {1, 1, 1, 1}, kI[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
#define MUST(x) do { if ((x) != MTR_OK) { fprintf(stderr, "line %d: %s failed\n", __LINE__, #x); exit(4); } } while (0)

struct Scene {  // one device with a single slot (every frame then runs on slot0), what lives on it, destroyed in order
    mtr_device* d = nullptr;
    std::vector<mtr_frame*> frames;
    std::vector<mtr_batch*> batches;
    std::vector<mtr_model*> models;
    Scene() { setenv("MTR_NSLOTS", "1", 1); MUST(mtr_device_create(0, &d)); }
    ~Scene() {
        for (mtr_frame* f : frames) mtr_frame_destroy(f);
        for (mtr_batch* b : batches) mtr_batch_destroy(b);
        for (mtr_model* m : models) mtr_model_destroy(m);
        mtr_device_destroy(d);
    }
    // nprims primitives of one triangle each (one geometry chunk each), debug-id shaded
    mtr_model* model(uint32_t nprims) {
        const float verts[9] = {-0.5f, -0.5f, 0.5f, 0.5f, -0.5f, 0.5f, 0.0f, 0.5f, 0.5f};
        std::vector<uint16_t> idx;
        std::vector<mtr_primitive> pr(nprims);
        std::vector<mtr_layout> l(nprims);
        for (uint32_t p = 0; p < nprims; p++) {
            for (uint16_t i = 0; i < 3; i++) idx.push_back(i);
            memset(&pr[p], 0, sizeof pr[p]);
            pr[p].w[0] = 3u << 16; pr[p].w[1] = p | (p << 12); pr[p].w[2] = 1 | (12u << 16) | (3u << 24); pr[p].w[6] = 3 * p; pr[p].w[7] = 3;
            memset(&l[p], 0, sizeof l[p]);
            l[p].elements[l[p].num_elements++] = mtr_element{MTR_SEM_POSITION, MTR_IEF_F32, 3, 0, 0, 0};
        }
        mtr_model* m = nullptr;
        MUST(mtr_model_create(d, verts, sizeof verts, idx.data(), idx.size(), pr.data(), nprims, l.data(), nullptr, nullptr, 0, nullptr, &m));
        models.push_back(m);
        return m;
    }
    mtr_batch* batch3(mtr_model* m) {
        float mm[3 * 16];
        for (int i = 0; i < 3; i++) memcpy(mm + 16 * i, kI, sizeof kI);
        mtr_batch* b = nullptr;
        MUST(mtr_batch_create(d, m, 3, mm, nullptr, 0, nullptr, &b));
        batches.push_back(b);
        return b;
    }
    mtr_frame* frame(uint32_t w = 64) {
        mtr_frame* f = nullptr;
        MUST(mtr_frame_begin(d, w, 64, kClear, 1.0f, &f));
        frames.push_back(f);
        return f;
    }
    void drop(mtr_frame* f) { frames.erase(std::find(frames.begin(), frames.end(), f)); mtr_frame_destroy(f); }
};

template <class F>
static Log logged(mtr_frame* f, int32_t* rc, F call) {
    g_frame = f; g_log.clear(); g_geom_fb.clear(); g_ranges.clear(); g_cull_inst = nullptr; g_range_mismatch = 0;
    hipStubTrace() = trace; g_remember = true;
    *rc = call(f);
    hipStubTrace() = nullptr; g_remember = false;
    return g_log;
}
static Log submit(mtr_frame* f, int32_t want = MTR_OK) {
    int32_t rc;
    Log l = logged(f, &rc, mtr_frame_submit);
    if (rc != want) { fprintf(stderr, "mtr_frame_submit returned %d, expected %d: %s\n", rc, want, mtr_last_error(f->dev)); g_failed++; }
    return l;
}

static Log operator+(Log a, const Log& b) { a.insert(a.end(), b.begin(), b.end()); return a; }

static void expect(const char* what, const Log& got, const Log& want) {
    if (got == want) return;
    g_failed++;
    fprintf(stderr, "---- %s: the launch log differs ----\n", what);
    for (size_t i = 0; i < std::max(got.size(), want.size()); i++) {
        const std::string g = i < got.size() ? got[i] : "(nothing)", w = i < want.size() ? want[i] : "(nothing)";
        fprintf(stderr, "%s %2zu  got      %s\n", g == w ? " " : "!", i, g.c_str());
        if (g != w) fprintf(stderr, "       expected %s\n", w.c_str());
    }
}
static bool has(const Log& l, const std::string& prefix) {
    for (const std::string& s : l)
        if (s.compare(0, prefix.size(), prefix) == 0) return true;
    return false;
}

// ---- the expected logs (64 x 64 target: 4 x 4 bins; one slot) ----
#define SYNC "hipStreamSynchronize slot0"
static const std::string kZeroCounters = S("hipMemsetAsync counters %zu slot0", CTR_NUM * sizeof(uint32_t));  // the frame's counter block
static const std::string kZeroBinFill = S("hipMemsetAsync bin_fill %zu slot0", 17 * sizeof(unsigned long long));  // direct mode, fresh slot
static const std::string kZeroBinCount = S("hipMemsetAsync bin_count %zu slot0", 17 * sizeof(unsigned long long));  // two-pass: every frame
static const std::string kZeroCullCounters = S("hipMemsetAsync cull_counters %zu slot0", 4 * MTR_CULL_CTR_WORDS * sizeof(uint32_t));
static std::string upload_mats(size_t n) { return S("hipMemcpyAsync mats %zu slot0", n * sizeof(DMat)); }
// the first frame of a slot grows its buffers: one sync of the slot's stream per group of buffers that share a capacity
static const Log kGrowSlot = {
    SYNC,                                  // rec_hdr, rec_a, rec_l, rec_b
    SYNC,                                  // chunk_info
    SYNC, "hipStreamSynchronize public",   // bin_count, bin_fill, bin_start, seg_start, bin_flag (read-backs use the public stream)
    SYNC,                                  // entries
    SYNC,                                  // segs
    SYNC,                                  // mats
};
static const Log kGrowCull = {SYNC, SYNC, SYNC, SYNC};  // comp, work_mask, inst_list, inst_count
// the end of every run: the framebuffer's event, the in-flight ring's, and the public stream behind the frame
static const Log kFinish = {"hipEventRecord fb.done slot0", "hipEventRecord ring slot0", "hipStreamWaitEvent fb.done public"};
#define OWN_ALL "own={map=0 rank=0 world=1 cull=0 own_count=16}"
#define TILE_ARGS_PLAIN "nhint=0 zero_words=0 zero_nwords=0 hint_out=0 zero_next=1 xcd_run=0 textured=0"

static void scenario_1_2_3_direct_two_pass_ordered() {
    {   // 1: an opaque model, single-pass binning: no scan, no fill; the frame goes to the visibility kernel, queue order is free
        Scene s;
        mtr_frame* f = s.frame();
        MUST(mtr_frame_draw_model(f, s.model(1), kI));
        expect("1: opaque, direct", submit(f), kGrowSlot + Log{
            upload_mats(1), kZeroCounters, kZeroBinFill,
            "geom nchunks=1 ninst=1 chunk_base=0 mat_base=0 small_draw=1 work_mask=0 inst_list=0 direct=1 unordered=1 " OWN_ALL,
            "tile_vis mixed=0 " TILE_ARGS_PLAIN,
        } + kFinish);
        MUST(mtr_frame_wait(f));
        mtr_frame_stats st;
        MUST(mtr_frame_get_stats(f, &st));
        CHECK(st.tile_kernel == MTR_TILE_VISIBILITY && st.binning == 1);
    }
    {   // 2: the same through the exact two-pass queues: bin_count zeroed, geom counts, scan, fill
        Scene s;
        MUST(mtr_device_set_binning(s.d, 0, 0));
        mtr_frame* f = s.frame();
        MUST(mtr_frame_draw_model(f, s.model(1), kI));
        expect("2: opaque, two-pass", submit(f), kGrowSlot + Log{
            upload_mats(1), kZeroCounters, kZeroBinCount,
            "geom nchunks=1 ninst=1 chunk_base=0 mat_base=0 small_draw=1 work_mask=0 inst_list=0 direct=0 unordered=0 " OWN_ALL,
            "scan",
            "fill total_chunks=1",
            "tile_vis mixed=0 " TILE_ARGS_PLAIN,
        } + kFinish);
        MUST(mtr_frame_wait(f));
        mtr_frame_stats st;
        MUST(mtr_frame_get_stats(f, &st));
        CHECK(st.tile_kernel == MTR_TILE_VISIBILITY && st.binning == 2);
    }
    {   // 3: MTR_TILE_ORDERED: the ordered kernel alone, and the queues keep submission order
        Scene s;
        MUST(mtr_device_set_tile_mode(s.d, MTR_TILE_ORDERED));
        mtr_frame* f = s.frame();
        MUST(mtr_frame_draw_model(f, s.model(1), kI));
        expect("3: ordered", submit(f), kGrowSlot + Log{
            upload_mats(1), kZeroCounters, kZeroBinFill,
            "geom nchunks=1 ninst=1 chunk_base=0 mat_base=0 small_draw=1 work_mask=0 inst_list=0 direct=1 unordered=0 " OWN_ALL,
            "tile mixed=0 " TILE_ARGS_PLAIN,
        } + kFinish);
        MUST(mtr_frame_wait(f));
        mtr_frame_stats st;
        MUST(mtr_frame_get_stats(f, &st));
        CHECK(st.tile_kernel == MTR_TILE_ORDERED);
    }
}

static void scenario_4_5_mixed_and_additive() {
    const mtr_prim_state off = {MTR_BLEND_OFF, 1, 1, MTR_CULL_BACK}, add = {MTR_BLEND_ADD, 1, 1, MTR_CULL_BACK};
    {   // 4: one primitive replaces, one adds: the visibility kernel takes the bins it can, the ordered kernel the flagged rest
        Scene s;
        mtr_model* m = s.model(2);
        const mtr_prim_state states[2] = {off, add};
        MUST(mtr_model_set_prim_states(m, states, 2));
        mtr_frame* f = s.frame();
        MUST(mtr_frame_draw_model(f, m, kI));
        expect("4: mixed", submit(f), kGrowSlot + Log{
            upload_mats(2), kZeroCounters, kZeroBinFill,
            "geom nchunks=2 ninst=1 chunk_base=0 mat_base=0 small_draw=1 work_mask=0 inst_list=0 direct=1 unordered=0 " OWN_ALL,
            "tile_vis mixed=1 " TILE_ARGS_PLAIN,
            "tile mixed=1 " TILE_ARGS_PLAIN,  // nhint = 0: the first kernel has reported (and cleared) the culling counters
        } + kFinish);
        MUST(mtr_frame_wait(f));
        mtr_frame_stats st;
        MUST(mtr_frame_get_stats(f, &st));
        CHECK(st.tile_kernel == MTR_TILE_MIXED);
    }
    {   // 5: every material additive (hard order-dependent): nothing for the visibility kernel to do
        Scene s;
        mtr_model* m = s.model(2);
        const mtr_prim_state states[2] = {add, add};
        MUST(mtr_model_set_prim_states(m, states, 2));
        mtr_frame* f = s.frame();
        MUST(mtr_frame_draw_model(f, m, kI));
        expect("5: all additive", submit(f), kGrowSlot + Log{
            upload_mats(2), kZeroCounters, kZeroBinFill,
            "geom nchunks=2 ninst=1 chunk_base=0 mat_base=0 small_draw=1 work_mask=0 inst_list=0 direct=1 unordered=0 " OWN_ALL,
            "tile mixed=0 " TILE_ARGS_PLAIN,
        } + kFinish);
        MUST(mtr_frame_wait(f));
        mtr_frame_stats st;
        MUST(mtr_frame_get_stats(f, &st));
        CHECK(st.tile_kernel == MTR_TILE_ORDERED);
    }
}

// rank 0 of 2 under bands: bin rows [0, 2) of 4, 8 bins
#define OWN_BAND0 "own={map=1 rank=0 world=2 cull=1 own_count=8}"
static void scenario_6_7_sharded() {
    {   // 6: a batch of three instances: instances culled, then their chunks; the tile kernel clears the slot's culling counters
        // for the next frame (so only a first frame zeroes them with a fill) and reports the instance count as a launch hint
        Scene s;
        mtr_batch* b = s.batch3(s.model(1));
        mtr_frame* f = s.frame();
        MUST(mtr_frame_set_shard_map(f, 0, 2, MTR_OWN_BANDS, 0, nullptr));
        MUST(mtr_frame_draw_batch(f, b, kI));
        const Log kernels = {
            "hipStreamWaitEvent pal_ready slot0",  // the batch's upload on the copy stream
            "cull_instances ninst=3",
            "cull_chunks keep_all=0 inst_count=1 comp=1",
            "geom nchunks=1 ninst=3 chunk_base=0 mat_base=0 small_draw=1 work_mask=1 inst_list=1 direct=1 unordered=1 " OWN_BAND0,
            S("tile_vis mixed=0 nhint=1 zero_words=1 zero_nwords=%u hint_out=1 zero_next=1 xcd_run=0 textured=0", MTR_CULL_CTR_WORDS),
        };
        expect("6: sharded batch, first frame", submit(f), kGrowSlot + Log{upload_mats(1), kZeroCounters, kZeroBinFill} + kGrowCull +
               Log{kZeroCullCounters} + kernels + kFinish);
        MUST(mtr_frame_wait(f));
        s.drop(f);
        f = s.frame();  // recycles the colour / depth / counter set: its other counter block was zeroed by the tile kernel
        MUST(mtr_frame_set_shard_map(f, 0, 2, MTR_OWN_BANDS, 0, nullptr));
        MUST(mtr_frame_draw_batch(f, b, kI));
        expect("6: sharded batch, second frame on the slot", submit(f), Log{"hipStreamWaitEvent fb.done slot0"} + kernels + kFinish);
        MUST(mtr_frame_wait(f));
    }
    {   // 7: a single model under bands: its chunks are culled, there is no instance list
        Scene s;
        mtr_frame* f = s.frame();
        MUST(mtr_frame_set_shard_map(f, 0, 2, MTR_OWN_BANDS, 0, nullptr));
        MUST(mtr_frame_draw_model(f, s.model(1), kI));
        expect("7: sharded model, bands", submit(f), kGrowSlot + Log{upload_mats(1), kZeroCounters, kZeroBinFill} + kGrowCull + Log{
            kZeroCullCounters,
            "cull_chunks keep_all=0 inst_count=0 comp=0",
            "geom nchunks=1 ninst=1 chunk_base=0 mat_base=0 small_draw=1 work_mask=1 inst_list=0 direct=1 unordered=1 " OWN_BAND0,
            S("tile_vis mixed=0 nhint=0 zero_words=1 zero_nwords=%u hint_out=1 zero_next=1 xcd_run=0 textured=0", MTR_CULL_CTR_WORDS),
        } + kFinish);
        MUST(mtr_frame_wait(f));
    }
    {   // 7b: interleaved bins: every chunk touches every rank, nothing is culled and no cull kernel runs
        Scene s;
        mtr_frame* f = s.frame();
        MUST(mtr_frame_set_shard_map(f, 0, 2, MTR_OWN_INTERLEAVED, 0, nullptr));
        MUST(mtr_frame_draw_model(f, s.model(1), kI));
        expect("7: sharded model, interleaved", submit(f), kGrowSlot + Log{
            upload_mats(1), kZeroCounters, kZeroBinFill,
            "geom nchunks=1 ninst=1 chunk_base=0 mat_base=0 small_draw=1 work_mask=0 inst_list=0 direct=1 unordered=1 "
            "own={map=0 rank=0 world=2 cull=0 own_count=8}",
            "tile_vis mixed=0 " TILE_ARGS_PLAIN,
        } + kFinish);
        MUST(mtr_frame_wait(f));
    }
}

static void scenario_8_overflow_reruns() {
    {   // flag 4, a bounded per-bin queue filled up: mtr_frame_wait runs the frame again through the two-pass queues, and
        // later frames get twice the bound
        Scene s;
        mtr_model* m = s.model(1);
        mtr_frame* f = s.frame();
        MUST(mtr_frame_draw_model(f, m, kI));
        g_flag_once = 4;
        submit(f);
        CHECK(g_geom_fb.size() == 1 && g_geom_fb[0].direct == 1 && g_geom_fb[0].qcap == 1024);
        int32_t rc;
        expect("8: re-run after flag 4", logged(f, &rc, mtr_frame_wait), Log{
            "hipStreamWaitEvent fb.done slot0",  // the frame's own first run
            kZeroCounters,                       // a second run starts from a fill again
            kZeroBinCount,
            "geom nchunks=1 ninst=1 chunk_base=0 mat_base=0 small_draw=1 work_mask=0 inst_list=0 direct=0 unordered=0 " OWN_ALL,
            "scan",
            "fill total_chunks=1",
            "tile_vis mixed=0 " TILE_ARGS_PLAIN,
        } + kFinish);
        CHECK(rc == MTR_OK);
        mtr_frame_stats st;
        MUST(mtr_frame_get_stats(f, &st));
        CHECK(st.binning == 2);
        mtr_frame* f2 = s.frame();
        MUST(mtr_frame_draw_model(f2, m, kI));
        submit(f2);
        CHECK(g_geom_fb.size() == 1 && g_geom_fb[0].direct == 1 && g_geom_fb[0].qcap == 2048);
        MUST(mtr_frame_wait(f2));
    }
    {   // flag 2, the exact queues too small: the re-run's are at least what the scan measured, plus a quarter, plus 1024
        Scene s;
        MUST(mtr_device_set_binning(s.d, 0, 0));
        mtr_frame* f = s.frame();
        MUST(mtr_frame_draw_model(f, s.model(1), kI));
        g_flag_once = 2; g_measured[0] = 3000000; g_measured[1] = 400000;
        submit(f);
        CHECK(g_geom_fb.size() == 1 && g_geom_fb[0].entry_cap < 3000000u && g_geom_fb[0].seg_cap < 400000u);
        int32_t rc;
        const Log l = logged(f, &rc, mtr_frame_wait);
        CHECK(rc == MTR_OK);
        CHECK(has(l, "geom ") && has(l, "scan") && has(l, "fill ") && has(l, "tile_vis "));
        CHECK(g_geom_fb.size() == 1 && g_geom_fb[0].direct == 0);
        CHECK(g_geom_fb.size() == 1 && g_geom_fb[0].entry_cap >= 3000000u + 3000000u / 4 + 1024 && g_geom_fb[0].seg_cap >= 400000u + 400000u / 4 + 1024);
    }
    {   // flag 1, a chunk needed more records than it has slots: nothing to grow
        Scene s;
        mtr_frame* f = s.frame();
        MUST(mtr_frame_draw_model(f, s.model(1), kI));
        g_flag_once = 1;
        submit(f);
        int32_t rc;
        const Log l = logged(f, &rc, mtr_frame_wait);
        CHECK(rc == MTR_E_OVERFLOW);
        CHECK(!has(l, "geom "));
    }
}

static void scenario_9_empty_band() {
    // rank 0 of 2 owns no bin row: no tile workgroup will publish the frame's status word, so the host does
    Scene s;
    const uint32_t bands[3] = {0, 0, 4};
    mtr_frame* f = s.frame();
    MUST(mtr_frame_set_shard_map(f, 0, 2, MTR_OWN_BANDS, 0, bands));
    MUST(mtr_frame_draw_model(f, s.model(1), kI));
    const Log l = submit(f);
    expect("9: empty band", l, kGrowSlot + Log{upload_mats(1), kZeroCounters, kZeroBinFill} + kGrowCull + Log{
        kZeroCullCounters,
        "cull_chunks keep_all=0 inst_count=0 comp=0",
        "geom nchunks=1 ninst=1 chunk_base=0 mat_base=0 small_draw=1 work_mask=1 inst_list=0 direct=1 unordered=1 "
        "own={map=1 rank=0 world=2 cull=1 own_count=0}",
    } + kFinish);
    CHECK(!has(l, "tile"));
    CHECK(status_load(s.d, f->status_idx) == 0x80000000u);
    CHECK(mtr_frame_wait(f) == MTR_OK);
}

static void scenario_11_profiling() {
    {   // direct mode: scan and fill do not run and get no event
        Scene s;
        MUST(mtr_device_set_profiling(s.d, 1));
        mtr_frame* f = s.frame();
        MUST(mtr_frame_draw_model(f, s.model(1), kI));
        expect("11: profiling, direct", submit(f), kGrowSlot + Log{
            upload_mats(1), kZeroCounters, kZeroBinFill,
            "hipEventRecord ev[0] slot0",
            "geom nchunks=1 ninst=1 chunk_base=0 mat_base=0 small_draw=1 work_mask=0 inst_list=0 direct=1 unordered=1 " OWN_ALL,
            "hipEventRecord ev[1] slot0",
            "tile_vis mixed=0 " TILE_ARGS_PLAIN,
            "hipEventRecord ev[4] slot0",
        } + kFinish);
        MUST(mtr_frame_wait(f));
    }
    {   // two-pass: an event between every two stages, all on the slot's stream
        Scene s;
        MUST(mtr_device_set_profiling(s.d, 1));
        MUST(mtr_device_set_binning(s.d, 0, 0));
        mtr_frame* f = s.frame();
        MUST(mtr_frame_draw_model(f, s.model(1), kI));
        expect("11: profiling, two-pass", submit(f), kGrowSlot + Log{
            upload_mats(1), kZeroCounters, kZeroBinCount,
            "hipEventRecord ev[0] slot0",
            "geom nchunks=1 ninst=1 chunk_base=0 mat_base=0 small_draw=1 work_mask=0 inst_list=0 direct=0 unordered=0 " OWN_ALL,
            "hipEventRecord ev[1] slot0",
            "scan",
            "hipEventRecord ev[2] slot0",
            "fill total_chunks=1",
            "hipEventRecord ev[3] slot0",
            "tile_vis mixed=0 " TILE_ARGS_PLAIN,
            "hipEventRecord ev[4] slot0",
        } + kFinish);
        MUST(mtr_frame_wait(f));
    }
}

// 12: MTR_VIS_WAVES, read when the device is created, reaches the visibility kernel's launcher as TileParams::vis_waves -- 2, 4
// and 8 as they are, anything else as 0 (the launcher's choice) -- and the launcher's rule (mtr_internal.h) picks the build
static void scenario_12_vis_waves() {
    const struct { const char* env; uint32_t want; } cases[] = {{nullptr, 0}, {"2", 2}, {"4", 4}, {"8", 8}, {"3", 0}, {"16", 0}};
    for (const auto& c : cases) {
        if (c.env) setenv("MTR_VIS_WAVES", c.env, 1);
        else unsetenv("MTR_VIS_WAVES");
        {
            Scene s;
            mtr_frame* f = s.frame();
            MUST(mtr_frame_draw_model(f, s.model(1), kI));
            g_vis_waves = ~0u;
            const Log l = submit(f);
            CHECK(has(l, "tile_vis "));
            if (g_vis_waves != c.want) {
                fprintf(stderr, "12: MTR_VIS_WAVES=%s reached the launcher as %u, expected %u\n", c.env ? c.env : "(unset)", g_vis_waves, c.want);
                g_failed++;
            }
            MUST(mtr_frame_wait(f));
        }
        unsetenv("MTR_VIS_WAVES");
    }
    CHECK(mtr_vis_waves_for(0, 1) == 8 && mtr_vis_waves_for(0, 1536) == 8);
    CHECK(mtr_vis_waves_for(0, 1537) == 4 && mtr_vis_waves_for(0, 4096) == 4);
    CHECK(mtr_vis_waves_for(0, 4097) == 2 && mtr_vis_waves_for(0, 129600) == 2);
    for (uint32_t w : {2u, 4u, 8u})
        for (uint32_t n : {1u, 1536u, 1537u, 4096u, 4097u, 129600u}) CHECK(mtr_vis_waves_for(w, n) == w);
}

// ---- 10: hipMalloc fails at the k-th allocation of a submit, for every k the submit reaches ----
// `grown`: the slot has already served a smaller frame, so its capacities are not zero when the allocation fails.  After
// the failure a frame that fits what the slot held before (grown) or a fresh frame of the same size (first frame) is
// submitted: it succeeds or fails with MTR_E_NOMEM again, and no launcher is ever handed a null buffer.
static std::vector<int> nomem_case(bool grown) {
    std::vector<int> bad;
    for (int k = 1;; k++) {
        Scene s;
        mtr_model* m = s.model(1);
        mtr_batch* b = s.batch3(m);
        auto sharded_batch_frame = [&](uint32_t w) {
            mtr_frame* f = s.frame(w);
            MUST(mtr_frame_set_shard_map(f, 0, 2, MTR_OWN_BANDS, 0, nullptr));
            MUST(mtr_frame_draw_batch(f, b, kI));
            return f;
        };
        auto small_frame = [&] {
            mtr_frame* f = s.frame();
            MUST(mtr_frame_draw_model(f, m, kI));
            return f;
        };
        if (grown) {
            mtr_frame* f0 = small_frame();
            MUST(mtr_frame_submit(f0));
            MUST(mtr_frame_wait(f0));
        }
        mtr_frame* f = sharded_batch_frame(grown ? 128 : 64);  // more chunks, more bins (and the culling buffers) than the small frame
        g_null.clear();
        hipStubFailMallocIn() = k;
        const int32_t rc = mtr_frame_submit(f);
        const bool reached = hipStubFailMallocIn() == 0;
        hipStubFailMallocIn() = 0;
        if (!reached) {  // the submit makes fewer than k allocations: every one of them has been failed
            CHECK(rc == MTR_OK && k > (grown ? 10 : 17));
            return bad;
        }
        CHECK(rc == MTR_E_NOMEM);
        mtr_frame* again = grown ? small_frame() : sharded_batch_frame(64);
        const int32_t rc2 = mtr_frame_submit(again);
        CHECK(rc2 == MTR_OK || rc2 == MTR_E_NOMEM);
        if (rc2 == MTR_OK) CHECK(mtr_frame_wait(again) == MTR_OK);
        if (!g_null.empty()) {
            fprintf(stderr, "%s, allocation %d failed: the next frame reached %s\n", grown ? "grown slot" : "first frame", k, g_null.c_str());
            bad.push_back(k);
        }
    }
}

static int scenario_10_nomem() {
    g_null_is_fatal = false;
    const std::vector<int> first = nomem_case(false), grown = nomem_case(true);
    printf("first_frame_bad=%zu grown_slot_bad=%zu:", first.size(), grown.size());
    for (int k : grown) printf(" %d", k);
    printf("\n");
    return (first.empty() && grown.empty() && !g_failed) ? 0 : 1;
}

// ---- 13 - 17: frames of several draws (one slot, 64 x 64, rank 0 of 2 under bands) ----
// A draw of these scenarios: a model of `prims` one-triangle primitives (one chunk each), drawn alone (ninst 0) or as a
// persistent batch of three instances.  What the host must hand each launch follows from the draw list alone: chunk_base and
// mat_base are running sums, every batch draw gets an instance list, the first four of them report a launch hint.
struct DrawSpec { uint32_t prims, ninst; };
static Log draw_kernels(const std::vector<DrawSpec>& draws, const char* own, uint32_t unordered) {
    Log l;
    uint32_t chunk_base = 0, mat_base = 0;
    for (const DrawSpec& d : draws) {
        const uint32_t n = d.ninst ? d.ninst : 1u;
        if (d.ninst) { l.push_back("hipStreamWaitEvent pal_ready slot0"); l.push_back(S("cull_instances ninst=%u", n)); }
        l.push_back(S("cull_chunks keep_all=0 inst_count=%d comp=%d", d.ninst != 0, d.ninst != 0));
        l.push_back(S("geom nchunks=%u ninst=%u chunk_base=%u mat_base=%u small_draw=1 work_mask=1 inst_list=%d direct=1 unordered=%u %s", d.prims, n,
                      chunk_base, mat_base, d.ninst != 0, unordered, own));
        chunk_base += d.prims * n; mat_base += d.prims;
    }
    return l;
}
static std::string tile_line(const char* name, uint32_t mixed, uint32_t nhint, size_t ndraws) {
    return S("%s mixed=%u nhint=%u zero_words=1 zero_nwords=%zu hint_out=1 zero_next=1 xcd_run=0 textured=0", name, mixed, nhint, ndraws * MTR_CULL_CTR_WORDS);
}
static std::string zero_cull_counters(size_t draw_cap) { return S("hipMemsetAsync cull_counters %zu slot0", draw_cap * MTR_CULL_CTR_WORDS * sizeof(uint32_t)); }

// the ranges the launches of the frame just submitted were handed (g_ranges): no two draws share an element
static void check_ranges(const char* what, const std::vector<DrawSpec>& draws) {
    bool ok = g_ranges.size() == draws.size() && g_range_mismatch == 0;
    uint64_t ninst_total = 0;
    for (const DrawSpec& d : draws) ninst_total += d.ninst;
    for (size_t i = 0; ok && i < draws.size(); i++) {
        const DrawRanges& a = g_ranges[i];
        const uint32_t n = draws[i].ninst ? draws[i].ninst : 1u;
        ok = ok && a.ninst == n && a.nx == (draws[i].prims + 15u) / 16u;
        ok = ok && a.work >= 0 && a.work % 2 == 0;  // k_geom reads a 16-bit mask through the aligned dword that holds it
        if (!draws[i].ninst) { ok = ok && a.list == -1 && a.strad == -1 && a.comp == -1 && a.count == -1; continue; }
        ok = ok && a.list >= 0 && a.strad >= 0 && a.comp >= 0 && a.count == (long)(i * MTR_CULL_CTR_WORDS);
        ok = ok && (uint64_t)a.list + n <= ninst_total && (uint64_t)a.strad >= ninst_total;  // lists in front, straddler lists behind all of them
    }
    auto disjoint = [](long a, long an, long b, long bn) { return a + an <= b || b + bn <= a; };
    for (size_t i = 0; ok && i < draws.size(); i++)
        for (size_t j = i + 1; ok && j < draws.size(); j++) {
            const DrawRanges &a = g_ranges[i], &b = g_ranges[j];
            ok = ok && disjoint(a.work, (long)a.nx * a.ninst, b.work, (long)b.nx * b.ninst);
            if (a.list < 0 || b.list < 0) continue;
            ok = ok && disjoint(a.list, a.ninst, b.list, b.ninst) && disjoint(a.strad, a.ninst, b.strad, b.ninst);
            ok = ok && disjoint(a.list, a.ninst, b.strad, b.ninst) && disjoint(a.strad, a.ninst, b.list, b.ninst);
            ok = ok && disjoint(a.comp, a.ninst, b.comp, b.ninst);  // unskinned: one composite per instance
        }
    if (ok) return;
    g_failed++;
    fprintf(stderr, "---- %s: the draws' shares of the culling buffers (%d launches of one draw disagree) ----\n", what, g_range_mismatch);
    for (const DrawRanges& a : g_ranges)
        fprintf(stderr, "  nx=%u ninst=%u work_mask=%ld inst_list=%ld strad=%ld comp=%ld inst_count=%ld\n", a.nx, a.ninst, a.work, a.list, a.strad, a.comp, a.count);
}

struct ManyDraws : Scene {  // the models and batches of scenarios 13 - 17
    mtr_model *m1, *m2;
    mtr_batch *a, *b;
    ManyDraws() { m1 = model(1); m2 = model(2); a = batch3(m1); b = batch3(m2); }
    // model m1, batch a, model m2, batch b, batch a again, model m1: chunks 1 + 3 + 2 + 6 + 3 + 1, materials 1 + 1 + 2 + 2 + 1 + 1
    std::vector<DrawSpec> six() const { return {{1, 0}, {1, 3}, {2, 0}, {2, 3}, {1, 3}, {1, 0}}; }
    std::vector<DrawSpec> two() const { return {{1, 0}, {1, 3}}; }
    mtr_frame* sharded(const std::vector<DrawSpec>& draws, const uint32_t* bands = nullptr) {
        mtr_frame* f = frame();
        MUST(mtr_frame_set_shard_map(f, 0, 2, MTR_OWN_BANDS, 0, bands));
        for (const DrawSpec& d : draws) {
            if (!d.ninst) MUST(mtr_frame_draw_model(f, d.prims == 1 ? m1 : m2, kI));
            else MUST(mtr_frame_draw_batch(f, d.prims == 1 ? a : b, kI));
        }
        return f;
    }
};

static void scenario_13_six_draws() {
    // single models and batches in turn: the counter buffer grows past its four lines and is cleared at that size; chunk_base
    // and mat_base run over the draws; the tile kernel clears six lines and reports the three batch draws
    ManyDraws s;
    const std::vector<DrawSpec> six = s.six();
    mtr_frame* f = s.sharded(six);
    expect("13: six draws", submit(f), kGrowSlot + Log{upload_mats(8), kZeroCounters, kZeroBinFill} + kGrowCull + Log{zero_cull_counters(6)} +
           draw_kernels(six, OWN_BAND0, 1) + Log{tile_line("tile_vis", 0, 3, 6)} + kFinish);
    check_ranges("13: six draws", six);
    MUST(mtr_frame_wait(f));
}

static void scenario_14_five_batches() {
    // a frame reports at most four launch hints: the fifth batch draw sizes its launches from what its slot last held
    Scene s;
    mtr_model* m = s.model(1);
    mtr_frame* f = s.frame();
    MUST(mtr_frame_set_shard_map(f, 0, 2, MTR_OWN_BANDS, 0, nullptr));
    std::vector<DrawSpec> five(5, DrawSpec{1, 3});
    for (int i = 0; i < 5; i++) MUST(mtr_frame_draw_batch(f, s.batch3(m), kI));
    expect("14: five batch draws", submit(f), kGrowSlot + Log{upload_mats(5), kZeroCounters, kZeroBinFill} + kGrowCull + Log{zero_cull_counters(5)} +
           draw_kernels(five, OWN_BAND0, 1) + Log{tile_line("tile_vis", 0, 4, 5)} + kFinish);
    check_ranges("14: five batch draws", five);  // 3 masks each: every second draw starts behind a padding mask
    MUST(mtr_frame_wait(f));
}

static void scenario_15_six_two_six() {
    // the tile kernel of a frame clears the culling counters of ITS draws for the slot's next frame: the frame of two draws
    // finds them clean, the frame of six after it finds four lines nobody cleared and zeroes the buffer with a fill
    ManyDraws s;
    const std::vector<DrawSpec> six = s.six(), two = s.two();
    mtr_frame* f = s.sharded(six);
    submit(f);
    check_ranges("15: six draws", six);
    MUST(mtr_frame_wait(f));
    s.drop(f);
    f = s.sharded(two);
    const Log second = submit(f);
    expect("15: two draws after six", second, Log{upload_mats(2), "hipStreamWaitEvent fb.done slot0"} + draw_kernels(two, OWN_BAND0, 1) +
           Log{tile_line("tile_vis", 0, 1, 2)} + kFinish);
    CHECK(!has(second, "hipMemsetAsync cull_counters"));
    check_ranges("15: two draws after six", two);
    MUST(mtr_frame_wait(f));
    s.drop(f);
    f = s.sharded(six);
    expect("15: six draws after two", submit(f), Log{upload_mats(8), "hipStreamWaitEvent fb.done slot0", zero_cull_counters(6)} +
           draw_kernels(six, OWN_BAND0, 1) + Log{tile_line("tile_vis", 0, 3, 6)} + kFinish);
    check_ranges("15: six draws after two", six);
    MUST(mtr_frame_wait(f));
}

static void scenario_16_mixed_with_batches() {
    // a mixed frame: the visibility kernel reports the hints and clears the counters, the ordered kernel behind it must not
    // report again (it would report zeros)
    Scene s;
    mtr_model* m = s.model(2);
    const mtr_prim_state states[2] = {{MTR_BLEND_OFF, 1, 1, MTR_CULL_BACK}, {MTR_BLEND_ADD, 1, 1, MTR_CULL_BACK}};
    MUST(mtr_model_set_prim_states(m, states, 2));
    mtr_frame* f = s.frame();
    MUST(mtr_frame_set_shard_map(f, 0, 2, MTR_OWN_BANDS, 0, nullptr));
    const std::vector<DrawSpec> draws(2, DrawSpec{2, 3});
    for (int i = 0; i < 2; i++) MUST(mtr_frame_draw_batch(f, s.batch3(m), kI));
    expect("16: mixed, two batch draws", submit(f), kGrowSlot + Log{upload_mats(4), kZeroCounters, kZeroBinFill} + kGrowCull + Log{kZeroCullCounters} +
           draw_kernels(draws, OWN_BAND0, 0) + Log{tile_line("tile_vis", 1, 2, 2), tile_line("tile", 1, 0, 2)} + kFinish);
    check_ranges("16: mixed, two batch draws", draws);
    MUST(mtr_frame_wait(f));
    mtr_frame_stats st;
    MUST(mtr_frame_get_stats(f, &st));
    CHECK(st.tile_kernel == MTR_TILE_MIXED);
}

static void scenario_17_empty_band_twice() {
    // a rank without a bin launches no tile kernel: nothing clears the culling counters (or the frame's other counter block),
    // so every frame zeroes them with a fill
    ManyDraws s;
    const uint32_t bands[3] = {0, 0, 4};
    const std::vector<DrawSpec> two = s.two();
    const char* own = "own={map=1 rank=0 world=2 cull=1 own_count=0}";
    mtr_frame* f = s.sharded(two, bands);
    const Log first = submit(f);
    expect("17: empty band, first frame", first, kGrowSlot + Log{upload_mats(2), kZeroCounters, kZeroBinFill} + kGrowCull + Log{kZeroCullCounters} +
           draw_kernels(two, own, 1) + kFinish);
    check_ranges("17: empty band, first frame", two);
    MUST(mtr_frame_wait(f));
    s.drop(f);
    f = s.sharded(two, bands);
    const Log second = submit(f);
    expect("17: empty band, second frame", second, Log{"hipStreamWaitEvent fb.done slot0", kZeroCounters, kZeroCullCounters} + draw_kernels(two, own, 1) + kFinish);
    CHECK(!has(first, "tile") && !has(second, "tile"));
    check_ranges("17: empty band, second frame", two);
    MUST(mtr_frame_wait(f));
}

int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "nomem")) return scenario_10_nomem();
    scenario_1_2_3_direct_two_pass_ordered();
    scenario_4_5_mixed_and_additive();
    scenario_6_7_sharded();
    scenario_8_overflow_reruns();
    scenario_9_empty_band();
    scenario_11_profiling();
    scenario_12_vis_waves();
    scenario_13_six_draws();
    scenario_14_five_batches();
    scenario_15_six_two_six();
    scenario_16_mixed_with_batches();
    scenario_17_empty_band_twice();
    printf("failed=%d\n", g_failed);
    return g_failed ? 1 : 0;
}
