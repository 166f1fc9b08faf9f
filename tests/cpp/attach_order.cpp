// The cross-batch ordering of attachments (SPEC.md section 18, DESIGN.md "k_attach"), pinned on the CPU: the host side of the
// library (csrc/host_*.cpp) over the stand-in HIP runtime of tests/cpp/hip_stub, compiled with AddressSanitizer and UBSan, with
// a k_attach launcher that touches the first and last element of everything it is handed and a trace hook that logs stream
// waits, event records, copies and stream syncs.  Events, buffers and streams are named after the call has returned, from the
// batches' version rings.  Cases:
//   1. attach, then two updates of the source, the second on a caller's stream: the write into the version k_attach read
//      waits for the reader's event;
//   2. attach, then mtr_batch_destroy(src): the buffer is parked behind the reader's event, no host wait, no free;
//   3. batch == src, twice;
//   and every invalid call leaves `cur` and the version ring of both batches untouched.
#define MTR_HARNESS_OWN_CULL_INSTANCES
#include "harness.h"

#define MUST(x) do { if ((x) != MTR_OK) { fprintf(stderr, "line %d: %s failed\n", __LINE__, #x); exit(4); } } while (0)

// ---- the kernels: only k_attach is launched here ----
static AttachParams g_last;
static int g_attach_launches = 0;
static float g_sink = 0.0f;

void mtr_launch_attach(const AttachParams& p, hipStream_t s) {
    g_last = p;
    g_attach_launches++;
    g_sink += (float)(p.recs[0] + p.recs[(size_t)p.n * MTR_ATTACH_WORDS - 1]);  // ASan checks the bounds of what the kernel would read
    g_sink += p.src_mats[0] + p.src_mats[(size_t)p.n_src * 16 - 1];
    if (p.npal) g_sink += p.src_pals[0] + p.src_pals[(size_t)p.n_src * p.npal * 16 - 1];
    p.out[0] = 1.0f;
    p.out[(size_t)p.n * 16 - 1] = 1.0f;
    g_ops.push_back({"attach", 0, p.out, s});
}
void mtr_launch_cull_instances(const CullParams&, hipStream_t) {}

// ---- names ----
struct Named { const char* name; mtr_batch* b; };
static std::vector<Named> g_batches;
static mtr_device* g_dev = nullptr;
static hipStream_t g_caller = nullptr;

static std::string what_name(const void* w) {
    if (!w) return "";
    for (const Named& nb : g_batches)
        for (size_t i = 0; i < nb.b->vers.size(); i++) {
            const mtr_batch::Ver& v = nb.b->vers[i];
            const std::string base = std::string(" ") + nb.name + ".v" + std::to_string(i);
            if (w == v.ready) return base + ".ready";
            if (w == v.read) return base + ".read";
            if (w == v.d) return base;
            if (v.d && w == v.d + (size_t)nb.b->n * 16) return base + ".pals";
        }
    if (w == g_dev->pose_stage) return " stage";
    return " elsewhere";
}
static std::string stream_name(const void* s) { return s == g_dev->s_copy ? "copy" : s == g_dev->stream ? "public" : s == g_caller ? "caller" : "?"; }

// the log of one call, named against the rings as the call left them
template <class F>
static std::vector<std::string> logged(F call) {
    g_ops.clear();
    hipStubTrace() = trace;
    call();
    hipStubTrace() = nullptr;
    std::vector<std::string> out;
    for (const Op& o : g_ops) out.push_back(o.op + what_name(o.what) + " " + stream_name(o.stream));
    return out;
}
static void show(const char* what, const std::vector<std::string>& l) {
    fprintf(stderr, "%s:\n", what);
    for (const std::string& s : l) fprintf(stderr, "    %s\n", s.c_str());
}
static long find(const std::vector<std::string>& l, const std::string& line, long from = 0) {
    for (long i = from; i < (long)l.size(); i++)
        if (l[(size_t)i] == line) return i;
    return -1;
}
static bool has_prefix(const std::vector<std::string>& l, const char* prefix) {
    for (const std::string& s : l)
        if (s.rfind(prefix, 0) == 0) return true;
    return false;
}
// a before b, both present
#define ORDER(l, a, b) do { const long ia_ = find(l, a), ib_ = find(l, b); if (ia_ < 0 || ib_ < 0 || ia_ >= ib_) { \
    fprintf(stderr, "line %d: '%s' (%ld) does not come before '%s' (%ld)\n", __LINE__, a, ia_, b, ib_); show("log", l); g_failed++; } } while (0)

// ---- scene ----
static const float kI[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

static mtr_model* make_model(mtr_device* d) {
    const float verts[9] = {-0.5f, -0.5f, 0.5f, 0.5f, -0.5f, 0.5f, 0.0f, 0.5f, 0.5f};
    const uint16_t idx[3] = {0, 1, 2};
    mtr_primitive pr;
    memset(&pr, 0, sizeof pr);
    pr.w[0] = 3u << 16; pr.w[2] = 1 | (12u << 16) | (3u << 24); pr.w[7] = 3;
    mtr_layout l;
    memset(&l, 0, sizeof l);
    l.elements[l.num_elements++] = mtr_element{MTR_SEM_POSITION, MTR_IEF_F32, 3, 0, 0, 0};
    mtr_model* m = nullptr;
    MUST(mtr_model_create(d, verts, sizeof verts, idx, 3, &pr, 1, &l, nullptr, nullptr, 0, nullptr, &m));
    return m;
}
static mtr_batch* make_batch(mtr_device* d, mtr_model* m, const char* name, size_t n, size_t npal) {
    std::vector<float> mm(n * 16), pal(n * npal * 16, 0.5f);
    for (size_t i = 0; i < n; i++) memcpy(&mm[i * 16], kI, sizeof kI);
    mtr_batch* b = nullptr;
    MUST(mtr_batch_create(d, m, n, mm.data(), npal ? pal.data() : nullptr, npal, nullptr, &b));
    g_batches.push_back({name, b});
    return b;
}
static void forget(mtr_batch* b) {
    for (size_t i = 0; i < g_batches.size(); i++)
        if (g_batches[i].b == b) { g_batches.erase(g_batches.begin() + (long)i); return; }
}

struct Ring {
    int cur;
    std::vector<mtr_batch::Ver> vers;
    bool operator==(const Ring& o) const {
        if (cur != o.cur || vers.size() != o.vers.size()) return false;
        for (size_t i = 0; i < vers.size(); i++) {
            const mtr_batch::Ver &a = vers[i], &b = o.vers[i];
            if (a.d != b.d || a.cap != b.cap || a.npal != b.npal || a.ready != b.ready || a.read != b.read || a.read_pending != b.read_pending ||
                a.read_stream != b.read_stream || a.pinned != b.pinned || a.used != b.used || a.last_frame != b.last_frame) return false;
        }
        return true;
    }
};
static Ring ring(const mtr_batch* b) { return Ring{b->cur, b->vers}; }
static bool unpinned(const mtr_batch* b) {
    for (const auto& v : b->vers)
        if (v.pinned) return false;
    return true;
}

int main() {
    setenv("MTR_NSLOTS", "1", 1);
    mtr_device* d = nullptr;
    MUST(mtr_device_create(0, &d));
    g_dev = d;
    MUST((int32_t)hipStreamCreateWithFlags(&g_caller, hipStreamNonBlocking));
    mtr_model* m = make_model(d);
    std::vector<mtr_attach> recs(5);
    {   // the staging buffer at its steady size: growing it is the one host wait of a host-record call
        const std::vector<float> z(recs.size() * MTR_ATTACH_WORDS, 0.0f);
        MUST(stage_pose(d, z.data(), z.size()));
    }
    for (size_t i = 0; i < recs.size(); i++) {
        recs[i].src_instance = (uint32_t)i; recs[i].joint = (uint32_t)(i * 3); recs[i].flags = (uint32_t)(i & 1); recs[i].pad = 0xDEADBEEFu;
        memcpy(recs[i].offset, kI, sizeof kI);
    }
    // "device" records: the stub's device memory is the heap; 16-byte aligned like hipMalloc's
    mtr_attach* recs_dev = static_cast<mtr_attach*>(aligned_alloc(16, recs.size() * sizeof(mtr_attach)));
    memcpy(recs_dev, recs.data(), recs.size() * sizeof(mtr_attach));

    // ---- 1. attach, then two updates of the source, the second on a caller's stream ----
    {
        mtr_batch* src = make_batch(d, m, "src", 3, 4);
        mtr_batch* tgt = make_batch(d, m, "tgt", 5, 2);
        mtr_batch* other = make_batch(d, m, "other", 2, 0);
        auto l = logged([&] { MUST(mtr_batch_attach(tgt, src, recs.data())); });
        CHECK(g_attach_launches == 1 && g_last.n == 5 && g_last.n_src == 3 && g_last.npal == 4);
        CHECK(g_last.src_mats == src->vers[0].d && g_last.src_pals == src->vers[0].d + 3 * 16 && g_last.out == tgt->vers[1].d);
        CHECK(g_last.recs == reinterpret_cast<const uint32_t*>(d->pose_stage));
        CHECK(tgt->cur == 1 && tgt->vers[1].npal == 2 && src->cur == 0 && unpinned(src) && unpinned(tgt));
        CHECK(src->vers[0].read && src->vers[0].read_pending && src->vers[0].read_stream == d->s_copy);
        ORDER(l, "hipMemcpyAsync stage copy", "attach tgt.v1 copy");
        ORDER(l, "hipStreamWaitEvent src.v0.ready copy", "attach tgt.v1 copy");
        ORDER(l, "hipStreamWaitEvent tgt.v0.ready copy", "hipMemcpyAsync tgt.v1.pals copy");  // the palettes are kept by the device copy
        ORDER(l, "attach tgt.v1 copy", "hipEventRecord src.v0.read copy");
        ORDER(l, "hipEventRecord src.v0.read copy", "hipEventRecord tgt.v1.ready copy");
        CHECK(find(l, "hipMemcpyAsync tgt.v1 copy") < 0);  // the matrices are the kernel's: no copy of the old ones
        CHECK(!has_prefix(l, "hipStreamSynchronize"));
        // a second reader on another stream first waits for the one before: the one event covers both
        float* out_dev = static_cast<float*>(aligned_alloc(16, 5 * 64));
        l = logged([&] { MUST(mtr_batch_sockets_device(src, recs_dev, 5, out_dev, g_caller)); });
        ORDER(l, "hipStreamWaitEvent src.v0.read caller", "attach elsewhere caller");
        ORDER(l, "attach elsewhere caller", "hipEventRecord src.v0.read caller");
        CHECK(src->vers[0].read_stream == g_caller && g_last.out == out_dev && unpinned(src));
        // update 1: a fresh version; the one k_attach read is no longer current and was never drawn
        float mm[3 * 16];
        for (int i = 0; i < 3; i++) memcpy(mm + 16 * i, kI, sizeof kI);
        l = logged([&] { MUST(mtr_batch_update(src, mm, nullptr, 0)); });
        CHECK(src->cur == 1 && src->vers[0].read_pending && !src->vers[0].used);
        CHECK(find(l, "hipStreamWaitEvent src.v0.read copy") < 0);  // nothing was written into v0
        // update 2, on the caller's stream: it takes v0 back, and its write waits for the reader
        l = logged([&] { MUST(mtr_batch_attach_device(src, other, recs_dev, g_caller)); });
        CHECK(src->cur == 0 && !src->vers[0].read_pending && g_last.out == src->vers[0].d && g_last.n == 3 && g_last.n_src == 2 && g_last.npal == 0);
        ORDER(l, "hipStreamWaitEvent src.v0.read caller", "attach src.v0 caller");
        ORDER(l, "hipStreamWaitEvent src.v0.read caller", "hipMemcpyAsync src.v0.pals caller");
        ORDER(l, "attach src.v0 caller", "hipEventRecord other.v0.read caller");
        CHECK(other->vers[0].read_pending && other->vers[0].read_stream == g_caller);
        CHECK(!has_prefix(l, "hipStreamSynchronize"));
        // the host call that waits: mtr_batch_sockets
        std::vector<float> out(5 * 16);
        l = logged([&] { MUST(mtr_batch_sockets(src, recs.data(), 5, out.data(), out.size())); });
        CHECK(has_prefix(l, "hipStreamSynchronize") && out[0] == 1.0f && out[79] == 1.0f && unpinned(src));
        free(out_dev);
        for (mtr_batch* b : {tgt, src, other}) { forget(b); mtr_batch_destroy(b); }
    }

    // ---- 2. attach, then destroy the source ----
    {
        mtr_batch* src = make_batch(d, m, "src", 3, 4);
        mtr_batch* tgt = make_batch(d, m, "tgt", 5, 0);
        MUST(mtr_batch_attach_device(tgt, src, recs_dev, g_caller));
        float* buf = src->vers[0].d;
        hipEvent_t rd = src->vers[0].read, ready = src->vers[0].ready;
        CHECK(rd && src->vers[0].read_pending);
        const size_t g0 = d->garbage.size();
        forget(src);
        auto l = logged([&] { mtr_batch_destroy(src); });
        CHECK(l.empty());  // no wait, no copy, no record: nothing reaches a stream
        bool parked = false, ready_kept = false;
        for (size_t i = g0; i < d->garbage.size(); i++) {
            if (d->garbage[i].p == buf && d->garbage[i].ev == rd) parked = true;
            if (!d->garbage[i].p && d->garbage[i].ev == ready) ready_kept = true;
        }
        CHECK(parked && ready_kept);
        g_sink += buf[0];  // still allocated (AddressSanitizer would say otherwise)
        // (collected by a later submit once the event has passed; mtr_device_destroy frees what is left)
        forget(tgt);
        mtr_batch_destroy(tgt);
    }

    // ---- 3. batch == src ----
    {
        mtr_batch* b = make_batch(d, m, "b", 5, 3);
        auto l = logged([&] { MUST(mtr_batch_attach(b, b, recs.data())); });
        CHECK(b->cur == 1 && g_last.src_mats == b->vers[0].d && g_last.out == b->vers[1].d && g_last.n == 5 && g_last.n_src == 5 && g_last.npal == 3);
        CHECK(b->vers[0].read_pending && !b->vers[1].read_pending && unpinned(b));
        ORDER(l, "hipStreamWaitEvent b.v0.ready copy", "attach b.v1 copy");
        ORDER(l, "attach b.v1 copy", "hipEventRecord b.v0.read copy");
        ORDER(l, "hipEventRecord b.v0.read copy", "hipEventRecord b.v1.ready copy");
        // again, on the caller's stream: reads v1, writes v0 -- after v0's reader
        l = logged([&] { MUST(mtr_batch_attach_device(b, b, recs_dev, g_caller)); });
        CHECK(b->cur == 0 && b->vers.size() == 2 && g_last.src_mats == b->vers[1].d && g_last.out == b->vers[0].d);
        CHECK(!b->vers[0].read_pending && b->vers[1].read_pending && b->vers[1].read_stream == g_caller && unpinned(b));
        ORDER(l, "hipStreamWaitEvent b.v0.read caller", "attach b.v0 caller");
        ORDER(l, "hipStreamWaitEvent b.v1.ready caller", "attach b.v0 caller");
        ORDER(l, "attach b.v0 caller", "hipEventRecord b.v1.read caller");
        forget(b);
        mtr_batch_destroy(b);
    }

    // ---- every invalid call leaves both rings as they were ----
    {
        mtr_batch* src = make_batch(d, m, "src", 3, 4);
        mtr_batch* tgt = make_batch(d, m, "tgt", 5, 2);
        MUST(mtr_batch_attach(tgt, src, recs.data()));
        mtr_device* d2 = nullptr;
        MUST(mtr_device_create(0, &d2));
        mtr_model* m2 = make_model(d2);
        float mm[16];
        memcpy(mm, kI, sizeof kI);
        mtr_batch* far = nullptr;
        MUST(mtr_batch_create(d2, m2, 1, mm, nullptr, 0, nullptr, &far));
        const Ring rs = ring(src), rt = ring(tgt), rf = ring(far);
        const int launches = g_attach_launches;
        const size_t garbage = d->garbage.size();
        std::vector<float> out(5 * 16, 7.0f);
        const mtr_attach* odd = reinterpret_cast<const mtr_attach*>(reinterpret_cast<const char*>(recs_dev) + 8);
        float* out_dev = static_cast<float*>(aligned_alloc(16, 5 * 64 + 16));
        auto l = logged([&] {
            CHECK(mtr_batch_attach(nullptr, src, recs.data()) == MTR_E_INVALID);
            CHECK(mtr_batch_attach(tgt, nullptr, recs.data()) == MTR_E_INVALID);
            CHECK(mtr_batch_attach(tgt, src, nullptr) == MTR_E_INVALID);
            CHECK(mtr_batch_attach(tgt, far, recs.data()) == MTR_E_INVALID);
            CHECK(mtr_batch_attach(far, src, recs.data()) == MTR_E_INVALID);
            CHECK(mtr_batch_attach_device(nullptr, src, recs_dev, nullptr) == MTR_E_INVALID);
            CHECK(mtr_batch_attach_device(tgt, nullptr, recs_dev, nullptr) == MTR_E_INVALID);
            CHECK(mtr_batch_attach_device(tgt, src, nullptr, g_caller) == MTR_E_INVALID);
            CHECK(mtr_batch_attach_device(tgt, src, odd, g_caller) == MTR_E_INVALID);
            CHECK(mtr_batch_attach_device(tgt, far, recs_dev, g_caller) == MTR_E_INVALID);
            CHECK(mtr_batch_sockets(nullptr, recs.data(), 5, out.data(), out.size()) == MTR_E_INVALID);
            CHECK(mtr_batch_sockets(src, nullptr, 5, out.data(), out.size()) == MTR_E_INVALID);
            CHECK(mtr_batch_sockets(src, recs.data(), 5, nullptr, out.size()) == MTR_E_INVALID);
            CHECK(mtr_batch_sockets(src, recs.data(), 0, out.data(), out.size()) == MTR_E_INVALID);
            CHECK(mtr_batch_sockets(src, recs.data(), 5, out.data(), out.size() - 1) == MTR_E_INVALID);
            CHECK(mtr_batch_sockets_device(nullptr, recs_dev, 5, out_dev, g_caller) == MTR_E_INVALID);
            CHECK(mtr_batch_sockets_device(src, nullptr, 5, out_dev, g_caller) == MTR_E_INVALID);
            CHECK(mtr_batch_sockets_device(src, odd, 4, out_dev, g_caller) == MTR_E_INVALID);
            CHECK(mtr_batch_sockets_device(src, recs_dev, 5, nullptr, g_caller) == MTR_E_INVALID);
            CHECK(mtr_batch_sockets_device(src, recs_dev, 5, out_dev + 1, g_caller) == MTR_E_INVALID);
            CHECK(mtr_batch_sockets_device(src, recs_dev, 0, out_dev, g_caller) == MTR_E_INVALID);
            CHECK(mtr_batch_read_model_mats(nullptr, out.data(), out.size()) == MTR_E_INVALID);
            CHECK(mtr_batch_read_model_mats(tgt, nullptr, out.size()) == MTR_E_INVALID);
            CHECK(mtr_batch_read_model_mats(tgt, out.data(), out.size() - 1) == MTR_E_INVALID);
        });
        CHECK(l.empty());  // and nothing reached a stream
        CHECK(ring(src) == rs && ring(tgt) == rt && ring(far) == rf && g_attach_launches == launches && d->garbage.size() == garbage);
        for (float v : out) CHECK(v == 7.0f);
        MUST(mtr_batch_read_model_mats(tgt, out.data(), out.size()));
        CHECK(out[0] == 1.0f && out[79] == 1.0f);  // what the stand-in kernel wrote
        free(out_dev);
        mtr_batch_destroy(far);
        mtr_model_destroy(m2);
        mtr_device_destroy(d2);
        for (mtr_batch* b : {tgt, src}) { forget(b); mtr_batch_destroy(b); }
    }

    free(recs_dev);
    mtr_model_destroy(m);
    (void)hipStreamDestroy(g_caller);
    mtr_device_destroy(d);
    printf("attach_order: launches=%d failed=%d sink=%s\n", g_attach_launches, g_failed, g_sink == g_sink ? "ok" : "nan");
    return g_failed ? 1 : 0;
}
