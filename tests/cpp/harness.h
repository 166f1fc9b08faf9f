// The scaffold of every host-side program of this directory: the host side of libmtr.so as one translation unit
// (host_all.h) over the stand-in HIP runtime (hip_stub), default bodies for the frame launchers of mtr_internal.h that are
// not weak, and the macros and utilities the programs share.  A program includes this file first and nothing else of the
// host side; what it needs differently it says above the include:
//   #define MTR_HARNESS_OWN_<LAUNCHER>   the program defines mtr_launch_<launcher> itself (GEOM, SCAN, FILL, TILE, TILE_VIS,
//                                        ALPHA_MIN, VERTEX_STAGE, BC1_DECODE, BC7_DECODE, PACK_SHARD, UNPACK_SHARDS,
//                                        CULL_INSTANCES, CULL_CHUNKS)
//   #define MTR_HARNESS_OWN_TRACE        the program has a hipStubTrace() hook of its own: no Op, g_ops, trace()
//   #define MTR_RND_SEED <seed>          rnd() and pick() of rnd.h, from the program's seed
// A frame launcher added to mtr_internal.h gets its default here, once; the animation launchers (mtr_launch_anim, _match,
// ...) are weak in the library and stay with the programs that fake them.
#pragma once
#include "host_all.h"
using namespace mtr_host;

#ifdef MTR_RND_SEED
#include "rnd.h"
#endif

// ---- the frame launchers: inert, except where the host reads back what the kernel leaves ----
// what tile_prologue does on the device: publish the (clean) overflow flags of the frame
static inline void harness_tile_status(const TileParams& p) { if (p.host_status) __atomic_store_n(p.host_status, 0x80000000u, __ATOMIC_RELEASE); }
#ifndef MTR_HARNESS_OWN_GEOM
void mtr_launch_geom(const GeomParams&, hipStream_t) {}
#endif
#ifndef MTR_HARNESS_OWN_SCAN
void mtr_launch_scan(const FrameBuffers&, hipStream_t) {}
#endif
#ifndef MTR_HARNESS_OWN_FILL
void mtr_launch_fill(const FrameBuffers&, uint32_t, hipStream_t) {}
#endif
#ifndef MTR_HARNESS_OWN_TILE
void mtr_launch_tile(const TileParams& p, bool, hipStream_t) { harness_tile_status(p); }
#endif
#ifndef MTR_HARNESS_OWN_TILE_VIS
void mtr_launch_tile_vis(const TileParams& p, bool, hipStream_t) { harness_tile_status(p); }
#endif
#ifndef MTR_HARNESS_OWN_ALPHA_MIN
void mtr_launch_alpha_min(const uint8_t*, size_t, uint32_t* out_min, hipStream_t) { *out_min = 255; }
#endif
#ifndef MTR_HARNESS_OWN_VERTEX_STAGE
void mtr_launch_vertex_stage(const GeomParams&, uint32_t, float*, float*, hipStream_t) {}
#endif
#ifndef MTR_HARNESS_OWN_BC1_DECODE
void mtr_launch_bc1_decode(const uint8_t*, uint8_t*, uint32_t, uint32_t, hipStream_t) {}
#endif
#ifndef MTR_HARNESS_OWN_BC7_DECODE
void mtr_launch_bc7_decode(const uint8_t*, uint8_t*, uint32_t, uint32_t, hipStream_t) {}
#endif
#ifndef MTR_HARNESS_OWN_PACK_SHARD
void mtr_launch_pack_shard(const uint8_t*, uint8_t*, uint32_t, uint32_t, const uint32_t*, uint32_t, uint32_t, hipStream_t) {}
#endif
#ifndef MTR_HARNESS_OWN_UNPACK_SHARDS
void mtr_launch_unpack_shards(const uint8_t*, uint8_t*, uint32_t, uint32_t, const uint32_t*, hipStream_t) {}
#endif
#ifndef MTR_HARNESS_OWN_CULL_INSTANCES
// every instance is listed, none straddles
void mtr_launch_cull_instances(const CullParams& p, hipStream_t) { for (uint32_t i = 0; i < p.ninst; i++) { p.strad[p.count[1]++] = *p.count; p.list[(*p.count)++] = i; } }
#endif
#ifndef MTR_HARNESS_OWN_CULL_CHUNKS
void mtr_launch_cull_chunks(const ChunkCullParams&, hipStream_t) {}
#endif

// ---- checks: CHECK counts and goes on; EXPECT and NAMES end main, and read the error of the `dev` in scope ----
static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #c); g_failed++; } } while (0)
#define EXPECT(call, code) do { const int32_t rc_ = (call); if (rc_ != (code)) { fprintf(stderr, "line %d: %s = %d, expected %d (%s)\n", __LINE__, #call, rc_, (int)(code), mtr_last_error(dev)); return 1; } } while (0)
#define NAMES(word) do { if (!strstr(mtr_last_error(dev), word)) { fprintf(stderr, "line %d: the error must say \"%s\": %s\n", __LINE__, word, mtr_last_error(dev)); return 1; } } while (0)

// ---- "device" memory of the program's own: the stub's is the heap; 16-byte aligned like hipMalloc's, sized to the
// vector (and `extra` bytes behind it) so that one record too many is an ASan report; the tail is zero ----
template <class T>
static inline T* dev_copy(const std::vector<T>& v, size_t extra = 0) {
    const size_t used = v.size() * sizeof(T), bytes = std::max<size_t>((used + extra + 15) / 16 * 16, 16);
    T* p = static_cast<T*>(aligned_alloc(16, bytes));
    if (used) memcpy(p, v.data(), used);
    memset(reinterpret_cast<char*>(p) + used, 0, bytes - used);
    return p;
}
static inline bool same(const void* a, const void* b, size_t bytes) { return bytes == 0 || memcmp(a, b, bytes) == 0; }

// ---- the recorder for hipStubTrace(): g_ops.clear(); hipStubTrace() = trace; <call>; hipStubTrace() = nullptr; ----
#ifndef MTR_HARNESS_OWN_TRACE
struct Op { std::string op; size_t bytes; const void* what; const void* stream; };
static std::vector<Op> g_ops;
static inline void trace(const char* name, size_t bytes, const void* what, const void* stream) { g_ops.push_back({name, bytes, what, stream}); }
#endif
