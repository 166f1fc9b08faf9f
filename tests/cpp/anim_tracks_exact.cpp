// anim_tracks_exact.cpp -- csrc/anim_tracks.h (the scalar rules of SPEC.md section 15 the track source of k_anim.hip is
// made of) compiled for the host, for tests/test_anim_tracks_exact.py to compare bit for bit with the numpy model.
//   usage: anim_tracks_exact <blob in> <result out>
// in : u32 J, C, nkeys, nstates; C x (u32 nticks, flags); C * J * 3 x mtr_anim_track (first, count, lo[3], step[3]);
//      nkeys x 4 u16 values; nkeys u16 times (+ one pad word when odd); nstates x 24-byte states
// out: per state, slot (A, B), joint, channel 12 words: r, k, k1, a, the decoded key k (4 f32), the decoded key k1 (4 f32;
//      the fourth component of a translation / scale key is 0).  Then 65536 f32: the Snorm16 of every 16-bit code.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blob_io.h"
#include "../../mt_renderer_amd/csrc/anim_tracks.h"

struct Track { uint32_t first, count; float lo[3], step[3]; };
static_assert(sizeof(Track) == 32, "mtr_anim_track");

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    long size = 0;
    std::vector<uint32_t> blob = read_words(argv[1], &size);
    const uint32_t J = blob[0], C = blob[1], nkeys = blob[2], n = blob[3];
    const uint32_t* clips = blob.data() + 4;
    const Track* tracks = reinterpret_cast<const Track*>(clips + 2 * C);
    const uint32_t* values = reinterpret_cast<const uint32_t*>(tracks + (size_t)C * J * 3);
    const uint16_t* times = reinterpret_cast<const uint16_t*>(values + (size_t)nkeys * 2);
    const uint32_t* states = reinterpret_cast<const uint32_t*>(times + ((nkeys + 1u) & ~1u));
    if ((const char*)(states + (size_t)n * 6) - (const char*)blob.data() != size) { std::fprintf(stderr, "blob size\n"); return 2; }
    std::vector<uint32_t> out;
    out.reserve((size_t)n * 2 * J * 3 * 12 + 65536);
    auto put_f = [&](float v) { uint32_t u; std::memcpy(&u, &v, 4); out.push_back(u); };
    for (uint32_t i = 0; i < n; i++)
        for (int slot = 0; slot < 2; slot++) {
            const uint32_t raw = states[i * 6 + slot], c = raw < C ? raw : C - 1u;
            float x;
            std::memcpy(&x, &states[i * 6 + 2 + slot], 4);
            const uint32_t nticks = clips[c * 2], flags = clips[c * 2 + 1];
            const float r = mtr::track_position(x, nticks, flags);
            for (uint32_t j = 0; j < J; j++)
                for (int ch = 0; ch < 3; ch++) {
                    const Track& t = tracks[((size_t)c * J + j) * 3 + ch];
                    const mtr::TrackPos p = mtr::track_locate(times, r, t.first, t.count, nticks, flags);
                    put_f(r); out.push_back(p.k); out.push_back(p.k1); put_f(p.a);
                    const uint32_t ks[2] = {p.k, p.k1};
                    for (uint32_t k : ks) {
                        float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                        if (ch == 1) mtr::track_decode_rot(values[(size_t)k * 2], values[(size_t)k * 2 + 1], d);
                        else mtr::track_decode_lin(values[(size_t)k * 2], values[(size_t)k * 2 + 1], t.lo, t.step, d);
                        for (float v : d) put_f(v);
                    }
                }
        }
    for (uint32_t code = 0; code < 65536u; code++) put_f(mtr::track_snorm16(code));
    write_words(argv[2], out);
    return 0;
}
