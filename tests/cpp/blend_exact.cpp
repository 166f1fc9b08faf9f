// blend_exact.cpp -- csrc/blend_math.h (the scalar rule of SPEC.md section 23) compiled for the host and put together the way
// k_blend puts it together (the state as four words, layers 0 to 2 of a stack written and the rest left, three steps, three
// shares), for tests/test_blend_exact.py to compare bit for bit with the numpy model.
//   usage: blend_exact <blob in> <result out>
// in : u32 n, C, K, T, NP, param_x, param_y, nlayers, damp (f32 bits), dt (f32 bits), 0, 0; C x 4 words of clips (period, flags,
//      rate, key count); K x 4 words of samples; T x 4 words of triangles; n x 4 words of states; n x NP parameters;
//      n x nlayers x 4 words of the layers as they were
// out: n x 4 words of states, n x nlayers x 4 words of layers, n x 12 words of steps, n x 3 shares
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blob_io.h"
#include <hip/hip_runtime.h>  // the stand-in of tests/cpp/hip_stub

#include "../../mt_renderer_amd/csrc/blend_math.h"

using namespace mtr;

static uint32_t bits(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    long size = 0;
    std::vector<uint32_t> blob = read_words(argv[1], &size);
    if (blob.size() < 12) return 2;
    const size_t n = blob[0], C = blob[1], K = blob[2], T = blob[3], NP = blob[4], nl = blob[7];
    float damp, dt;
    std::memcpy(&damp, &blob[8], 4);
    std::memcpy(&dt, &blob[9], 4);
    if ((long)((12 + C * 4 + K * 4 + T * 4 + n * 4 + n * NP + n * nl * 4) * 4) != size || C == 0 || K == 0 || K > 32 || T > 64 || NP == 0 || NP > 16 || n == 0 ||
        blob[5] >= NP || blob[6] >= NP || (nl != 0 && (nl < 3 || nl > 8))) {
        std::fprintf(stderr, "blob size\n");
        return 2;
    }
    const uint32_t* at = blob.data() + 12;
    std::vector<PlayClip> clips(C);
    std::memcpy(clips.data(), at, C * 16); at += C * 4;
    std::vector<BlendSample> samples(K);
    std::memcpy(samples.data(), at, K * 16); at += K * 4;
    std::vector<BlendTri> tris(T + 1);
    std::memcpy(tris.data(), at, T * 16); at += T * 4;
    for (size_t k = 0; k < K; k++)
        if (samples[k].clip >= C) return 3;
    for (size_t k = 0; k < T; k++)
        if (tris[k].v[0] >= K || tris[k].v[1] >= K || tris[k].v[2] >= K) return 3;
    std::vector<uint32_t> out(n * 4 + n * nl * 4 + n * 12 + n * 3);
    std::memcpy(out.data(), at, n * 16); at += n * 4;
    std::vector<float> params(n * NP);
    std::memcpy(params.data(), at, n * NP * 4); at += n * NP;
    uint32_t* o_layers = out.data() + n * 4;
    std::memcpy(o_layers, at, n * nl * 16);
    uint32_t* o_steps = o_layers + n * nl * 4;
    uint32_t* o_shares = o_steps + n * 12;
    BlendTables t;
    t.clips = clips.data(); t.samples = samples.data(); t.tris = tris.data();
    t.nclips = (uint32_t)C; t.nsamples = (uint32_t)K; t.ntris = (uint32_t)T;
    t.param_x = blob[5]; t.param_y = blob[6]; t.nparams = (uint32_t)NP; t.damp = damp;
    for (size_t i = 0; i < n; i++) {
        BlendState st;
        std::memcpy(&st, &out[i * 4], 16);
        const uint32_t speed = out[i * 4 + 3];
        const BlendFrame fr = blend_advance(st, params.data() + i * NP, dt, t);
        std::memcpy(&out[i * 4], &st, 16);
        out[i * 4 + 3] = speed;  // never written
        for (size_t s = 0; s < 3; s++) {
            if (nl) {
                uint32_t* l = o_layers + (i * nl + s) * 4;
                l[0] = fr.clip[s]; l[1] = bits(fr.x[s]); l[2] = bits(fr.e[s]); l[3] = 0u;
            }
            uint32_t* p = o_steps + (i * 3 + s) * 4;
            p[0] = fr.clip[s]; p[1] = bits(fr.x0[s]); p[2] = bits(fr.dx[s]); p[3] = bits(fr.e[s]);
            o_shares[i * 3 + s] = bits(fr.share[s]);
        }
    }
    write_words(argv[2], out);
    return 0;
}
