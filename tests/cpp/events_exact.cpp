// events_exact.cpp -- csrc/event_math.h (the scalar rule of SPEC.md section 22) compiled for the host and put together the way
// k_events puts it together (a count per instance, block sums of 256 instances, their exclusive scan, a fill at the block's
// base plus the counts of the instances before it in the block, records stored while the index is below the capacity, the
// masks written), for tests/test_events_exact.py to compare bit for bit with the numpy model.
//   usage: events_exact <blob in> <result out>
// in : u32 n, C, S, M, capacity, 0, min_weight (f32 bits), 0; C x 4 words of clips (period, flags, 0, key count); C x 2 words
//      of ranges (first, count); M x 2 words of markers; n x S x 4 words of steps; capacity x 4 words of the list as it was;
//      n words of bits as they were
// out: capacity x 4 words of the list, 2 words of count, n words of bits
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blob_io.h"
#include <hip/hip_runtime.h>  // the stand-in of tests/cpp/hip_stub

#include "../../mt_renderer_amd/csrc/event_math.h"

using namespace mtr;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    long size = 0;
    std::vector<uint32_t> blob = read_words(argv[1], &size);
    if (blob.size() < 8) return 2;
    const size_t n = blob[0], C = blob[1], S = blob[2], M = blob[3], cap = blob[4];
    float min_weight;
    std::memcpy(&min_weight, &blob[6], 4);
    if ((long)((8 + C * 4 + C * 2 + M * 2 + n * S * 4 + cap * 4 + n) * 4) != size || C == 0 || S == 0 || S > MTR_EVENT_MAX_STEPS || n == 0) {
        std::fprintf(stderr, "blob size\n");
        return 2;
    }
    const uint32_t* at = blob.data() + 8;
    std::vector<PlayClip> clips(C);
    std::memcpy(clips.data(), at, C * 16); at += C * 4;
    std::vector<uint32_t> ranges(at, at + C * 2); at += C * 2;
    std::vector<EventMarker> markers(M + 1);
    std::memcpy(markers.data(), at, M * 8); at += M * 2;
    std::vector<EventStepIn> steps(n * S);
    std::memcpy(steps.data(), at, n * S * 16); at += n * S * 4;
    std::vector<uint32_t> out(cap * 4 + 2 + n);
    std::memcpy(out.data(), at, cap * 16); at += cap * 4;
    uint32_t* o_count = out.data() + cap * 4;
    uint32_t* o_bits = o_count + 2;
    std::memcpy(o_bits, at, n * 4);
    for (size_t c = 0; c < C; c++)
        if ((size_t)ranges[2 * c] + ranges[2 * c + 1] > M) return 3;
    EventTables t;
    t.clips = clips.data(); t.ranges = ranges.data(); t.markers = markers.data(); t.nclips = (uint32_t)C;
    // count, scan, fill
    const size_t nb = (n + 255) / 256;
    std::vector<uint32_t> counts(n), sums(nb, 0u);
    for (size_t i = 0; i < n; i++) {
        counts[i] = event_count(steps.data() + i * S, (uint32_t)S, min_weight, t);
        sums[i / 256] += counts[i];
    }
    uint32_t carry = 0;
    for (size_t b = 0; b < nb; b++) { const uint32_t v = sums[b]; sums[b] = carry; carry += v; }
    o_count[0] = carry;
    o_count[1] = carry < cap ? carry : (uint32_t)cap;
    for (size_t i = 0; i < n; i++) {
        uint32_t idx = sums[i / 256], mask = 0;
        for (size_t j = i / 256 * 256; j < i; j++) idx += counts[j];
        const uint32_t fired = event_walk(steps.data() + i * S, (uint32_t)S, min_weight, t, [&](const EventMarker& m, uint32_t where, float w) {
            if (&m < markers.data() || &m >= markers.data() + M) std::abort();
            if (idx < cap) {
                const EventRecord r{(uint32_t)i, m.id, where, w};
                std::memcpy(&out[(size_t)idx * 4], &r, 16);
            }
            idx++;
            mask |= 1u << (m.id & 31u);
        });
        if (fired != counts[i]) return 4;  // the two passes must agree
        o_bits[i] = mask;
    }
    write_words(argv[2], out);
    return 0;
}
