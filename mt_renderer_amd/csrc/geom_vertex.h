// geom_vertex.h -- vertex fetch, format decode and the vertex shader (skinning + clip transform) of the geometry kernels.
#pragma once
#include "mtr_internal.h"

namespace mtr {

// ---------------------------------------------------------------------------------------------
// vertex fetch: byte address = vertex_base + (index + index_base) * stride + element.offset
// (src/model.rs:337-342,357-361); format table of src/rshader2.rs:516-564.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ld16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ __forceinline__ uint32_t ld32(const uint8_t* p, bool al4) {
    if (al4) return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// x / d for a small integer x: bit-identical to the IEEE division (tests/test_div_exact.py) in three instructions instead
// of the ten of the IEEE expansion.  Seven of these per vertex (SNORM16 position, UNORM8 weights).  Rounds 1-2 measured it
// slower in k_geom (the 80-VGPR allocation then spilled in the prologue); with the vertex stage feeding LDS instead of
// living across the whole kernel it is the default.  -DMTR_DIV_IEEE restores the plain division for A/B runs.
__device__ __forceinline__ float div_small(float x, float d, float r) {
#ifndef MTR_DIV_IEEE
    const float q0 = x * r;
    return fmaf(fmaf(-q0, d, x), r, q0);
#else
    (void)r;
    return x / d;
#endif
}
__device__ __forceinline__ float snorm16f(uint32_t lo16) {
    float f = div_small((float)(int16_t)lo16, 32767.0f, __uint_as_float(0x38000100u));
    return f < -1.0f ? -1.0f : f;
}
__device__ __forceinline__ float snorm8f(uint32_t lo8) {
    float f = div_small((float)(int8_t)lo8, 127.0f, __uint_as_float(0x3c010204u));
    return f < -1.0f ? -1.0f : f;
}
__device__ __forceinline__ float unorm8f(uint32_t lo8) { return div_small((float)(lo8 & 0xffu), 255.0f, __uint_as_float(0x3b808081u)); }
__device__ __forceinline__ float half_bits_to_float(uint32_t lo16) {
    return (float)__builtin_bit_cast(_Float16, (unsigned short)lo16);  // v_cvt_f32_f16: exact, denormals kept
}

// The format table decoding an element that is already in registers (w0 = its first four bytes, w1, w2 the next eight;
// little-endian): the vertex stage issues every load of a vertex first and decodes afterwards, so that a wave pays one
// memory round trip per vertex instead of one per element (decode_elem below waits for each element's load in turn).
__device__ __forceinline__ void decode_regs(uint32_t fmt, uint32_t cnt, uint32_t w0, uint32_t w1, uint32_t w2, float& x, float& y, float& z) {
    x = 0.0f; y = 0.0f; z = 0.0f;
    switch (fmt) {
    case 10: /* U8N */
    case 13: /* U8NL */
        x = unorm8f(w0); y = unorm8f(w0 >> 8);
        if (!(fmt == 10 && cnt == 1)) z = unorm8f(w0 >> 16);
        break;
    case 9: /* S8N */
        x = snorm8f(w0 & 0xff); y = snorm8f((w0 >> 8) & 0xff);
        if (cnt != 1) z = snorm8f((w0 >> 16) & 0xff);
        break;
    case 5: /* S16N */
        x = snorm16f(w0 & 0xffff); y = snorm16f(w0 >> 16);
        if (cnt == 3) z = snorm16f(w1 & 0xffff);
        break;
    case 2: /* F16 x2 */
        x = half_bits_to_float(w0 & 0xffff); y = half_bits_to_float(w0 >> 16);
        break;
    case 1: /* F32 x3 */
        x = __uint_as_float(w0); y = __uint_as_float(w1); z = __uint_as_float(w2);
        break;
    case 11: /* SCMP3N, opted into by MTR_ELEM_DECODE_SCMP3N: three signed 10-bit fields, max(v / 511, -1) */ {
        const float fx = (float)((int32_t)(w0 << 22) >> 22) / 511.0f, fy = (float)((int32_t)(w0 << 12) >> 22) / 511.0f,
                    fz = (float)((int32_t)(w0 << 2) >> 22) / 511.0f;
        x = fx < -1.0f ? -1.0f : fx; y = fy < -1.0f ? -1.0f : fy; z = fz < -1.0f ? -1.0f : fz;
        break;
    }
    default: break;
    }
}
// bytes of an element the decode reads (host: elem_bytes in host_model.cpp); 0 for formats the table does not hold
__device__ __forceinline__ uint32_t elem_nbytes(uint32_t fmt, uint32_t cnt) {
    switch (fmt) {
    case 10: return cnt == 1 ? 2u : 4u;
    case 13: return 4u;
    case 9: return cnt == 1 ? 2u : 4u;
    case 5: return cnt == 1 ? 4u : 8u;
    case 2: return 4u;
    case 1: return 12u;
    case 11: return 4u;
    default: return 0u;
    }
}
// the raw bytes of an element: up to three dwords, loads only (nothing waits here).  The vertex buffer is padded by 16
// bytes on the device, so a whole-dword read of a 2-byte element at the end of the last vertex stays inside it.
__device__ __forceinline__ void load_elem(const uint8_t* p, bool al4, uint32_t nbytes, uint32_t& w0, uint32_t& w1, uint32_t& w2) {
    w0 = 0; w1 = 0; w2 = 0;
    if (nbytes == 0) return;
    if (al4) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        w0 = q[0];
        if (nbytes > 4) w1 = q[1];
        if (nbytes > 8) w2 = q[2];
    } else {
        w0 = nbytes >= 4 ? ld32(p, false) : ld16(p);
        if (nbytes > 4) w1 = ld32(p + 4, false);
        if (nbytes > 8) w2 = ld32(p + 8, false);
    }
}
// The same table with its own loads, for the clipper's re-shade (shade_vertex): (x,y,z) of one float-class element (w is
// never consumed: position.xyz / texcoord.xy).  Written as load_elem + decode_regs it costs the hot kernels 250-470 bytes of
// code, 16 bytes of scratch at 72 registers, and 3-4 % of C4 / C5, so the second copy stays;
// tests/test_gpu_vertex_decode.py holds both to the reference tables code by code.
__device__ __forceinline__ void decode_elem(uint32_t fmt, uint32_t cnt, const uint8_t* p, bool al4, float& x,
                                            float& y, float& z) {
    x = 0.0f; y = 0.0f; z = 0.0f;
    switch (fmt) {
    case 10: /* U8N */
    case 13: /* U8NL */
        if (fmt == 10 && cnt == 1) { x = unorm8f(p[0]); y = unorm8f(p[1]); }
        else { uint32_t w = ld32(p, al4); x = unorm8f(w); y = unorm8f(w >> 8); z = unorm8f(w >> 16); }
        break;
    case 9: /* S8N */
        if (cnt == 1) { x = snorm8f(p[0]); y = snorm8f(p[1]); }
        else { uint32_t w = ld32(p, al4); x = snorm8f(w & 0xff); y = snorm8f((w >> 8) & 0xff); z = snorm8f((w >> 16) & 0xff); }
        break;
    case 5: /* S16N */ {
        uint32_t w0 = ld32(p, al4);
        x = snorm16f(w0 & 0xffff); y = snorm16f(w0 >> 16);
        if (cnt == 3) { uint32_t w1 = ld32(p + 4, al4); z = snorm16f(w1 & 0xffff); }
        break;
    }
    case 2: /* F16 x2 */ {
        uint32_t w0 = ld32(p, al4);
        x = half_bits_to_float(w0 & 0xffff); y = half_bits_to_float(w0 >> 16);
        break;
    }
    case 1: /* F32 x3 */
        x = __uint_as_float(ld32(p, al4)); y = __uint_as_float(ld32(p + 4, al4)); z = __uint_as_float(ld32(p + 8, al4));
        break;
    case 11: /* SCMP3N, opted into by MTR_ELEM_DECODE_SCMP3N: three signed 10-bit fields, max(v / 511, -1) */ {
        const uint32_t w = ld32(p, al4);
        const float fx = (float)((int32_t)(w << 22) >> 22) / 511.0f, fy = (float)((int32_t)(w << 12) >> 22) / 511.0f,
                    fz = (float)((int32_t)(w << 2) >> 22) / 511.0f;
        x = fx < -1.0f ? -1.0f : fx; y = fy < -1.0f ? -1.0f : fy; z = fz < -1.0f ? -1.0f : fz;
        break;
    }
    default: break;
    }
}

struct VOut {
    float x, y, z, w, u, v;
};

// Linear-blend skinning of one vertex on the VALU: q = sum_k w_k * P[j_k] * (p,1), a k-ordered fmaf chain from 0 per
// component (jw, ww: the four joint and weight bytes).
__device__ __forceinline__ void skin_valu(uint32_t jw, uint32_t ww, const float (&pin)[4], const float* s_pal, uint32_t npal, float& q0,
                                          float& q1, float& q2) {
    float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t j = (jw >> (8 * k)) & 0xff;
        if (j >= npal) j = npal - 1;
        const float4* P = reinterpret_cast<const float4*>(s_pal + j * 16);
        const float wk = unorm8f(ww >> (8 * k));
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const float4 col = P[c];
            const float s = wk * pin[c];
            a0 = fmaf(col.x, s, a0);
            a1 = fmaf(col.y, s, a1);
            a2 = fmaf(col.z, s, a2);
        }
    }
    q0 = a0; q1 = a1; q2 = a2;
}

// The vertex shader: linear-blend skinning against the LDS-staged palette (build extension,
// SPEC.md "LBS"), then clip = M * (q,1) (src/shaders/textured.wgsl:15, debug_ids.wgsl:13).
// Both contractions are k-ordered fmaf chains starting from 0 -- the exact arithmetic of the
// f32 MFMA (v_mfma_f32_4x4x1_16b_f32) used by the batched variant in k_geom.
__device__ __forceinline__ VOut shade_vertex(const uint8_t* vbuf, const DPrim& pr, uint32_t vid, const float (&M)[16],
                                             const float* s_pal, uint32_t npal, bool skinned) {
    const uint8_t* vp = vbuf + pr.vertex_base + (size_t)vid * pr.stride;
    const bool al4 = pr.aligned4 != 0;
    float px, py, pz, tu = 0.0f, tv = 0.0f, tz;
    decode_elem(pr.pos_fmt, pr.pos_cnt, vp + pr.pos_off, al4, px, py, pz);
    if (pr.has_uv) decode_elem(pr.uv_fmt, pr.uv_cnt, vp + pr.uv_off, al4, tu, tv, tz);
    float q0 = px, q1 = py, q2 = pz;
    if (skinned) {
        const uint32_t jw = ld32(vp + pr.joint_off, al4), ww = ld32(vp + pr.weight_off, al4);
        const float pin[4] = {px, py, pz, 1.0f};
        skin_valu(jw, ww, pin, s_pal, npal, q0, q1, q2);
    }
    const float q[4] = {q0, q1, q2, 1.0f};
    float cl[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        float a = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; c++) a = fmaf(M[c * 4 + i], q[c], a);
        cl[i] = a;
    }
    VOut r = {cl[0], cl[1], cl[2], cl[3], tu, tv};
    return r;
}

// ---------------------------------------------------------------------------------------------
// The same vertex shader on the matrix cores: v_mfma_f32_4x4x1_16b_f32 = 16 independent
// (4x1)*(1x4) outer products per wave; block = 4 consecutive lanes, D[lane][v] = A[block*4+v] * B[lane]
// + C, and a k-step chain is bitwise an fmaf chain (tools/mfma_probe.hip on benign values; tests/test_gpu_vertex_edges.py
// under cancellation, with subnormal operands, products and sums, signed zeros, overflow and NaN, in coherent, incoherent
// and partial blocks: 0 of 2 188 vertices differ from the oracle at five palette sizes).  One lane =
// one vertex supplies B (its own w_k*p_c, or q_c) and row (lane & 3) of the 4x4 matrix as A:
//   * clip = M * (q,1): A is the wave-uniform M -> 4 MFMAs for 64 vertices;
//   * skinning: A is the bone matrix P[j_k], so a block must share its four joint indices (rows of a
//     skinned mesh do) -> 16 MFMAs; blocks that do not are redone by their lanes with the VALU chain (skin_valu),
//     which is the identical arithmetic.
// Must be called by all 64 lanes of the wave (the MFMA is wave-wide); `active` masks the loads.
// ---------------------------------------------------------------------------------------------
typedef float v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ VOut shade_vertex_mfma(const uint8_t* vbuf, const DPrim& pr, uint32_t vid, bool active,
                                                  const float* s_M, const float* s_pal, uint32_t npal, bool skinned, bool want_uv) {
    const uint32_t lane = threadIdx.x & 63, row = lane & 3;
    const bool al4 = pr.aligned4 != 0;
    float px = 0.0f, py = 0.0f, pz = 0.0f, tu = 0.0f, tv = 0.0f, tz;
    uint32_t jw = 0, ww = 0;
    want_uv = want_uv && pr.has_uv;
    {
        // every load of the vertex first (element sizes are wave-uniform), decode once they are all on their way
        uint32_t p0 = 0, p1 = 0, p2 = 0, u0 = 0, u1 = 0, u2 = 0;
        if (active) {
            const uint8_t* vp = vbuf + pr.vertex_base + (size_t)vid * pr.stride;
            load_elem(vp + pr.pos_off, al4, elem_nbytes(pr.pos_fmt, pr.pos_cnt), p0, p1, p2);
            if (want_uv) load_elem(vp + pr.uv_off, al4, elem_nbytes(pr.uv_fmt, pr.uv_cnt), u0, u1, u2);
            if (skinned) { jw = ld32(vp + pr.joint_off, al4); ww = ld32(vp + pr.weight_off, al4); }
        }
        decode_regs(pr.pos_fmt, pr.pos_cnt, p0, p1, p2, px, py, pz);
        if (want_uv) decode_regs(pr.uv_fmt, pr.uv_cnt, u0, u1, u2, tu, tv, tz);
        // inactive lanes hold zero bits, which every format decodes to 0.0
    }
    float q0 = px, q1 = py, q2 = pz;
    if (skinned) {  // wave-uniform
        const float pin[4] = {px, py, pz, 1.0f};
        const uint32_t jw0 = (uint32_t)__shfl((int)jw, (int)(lane & ~3u));
        const uint64_t okm = __ballot(active && jw == jw0);
        const bool coherent = ((okm >> (lane & ~3u)) & 0xFull) == 0xFull;
        v4f acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t j = (jw0 >> (8 * k)) & 0xff;
            if (j >= npal) j = npal - 1;
            const float wk = unorm8f(ww >> (8 * k));
#pragma unroll
            for (int c = 0; c < 4; c++)
                acc = __builtin_amdgcn_mfma_f32_4x4x1f32(s_pal[j * 16 + c * 4 + row], wk * pin[c], acc, 0, 0, 0);
        }
        q0 = acc[0]; q1 = acc[1]; q2 = acc[2];
        if (__ballot(active && !coherent)) {
            if (active && !coherent) skin_valu(jw, ww, pin, s_pal, npal, q0, q1, q2);
        }
    }
    // clip = M * (q, 1): A = row (lane & 3) of the workgroup's matrix, straight from LDS (s_M: 16 floats, column-major)
    const float q[4] = {q0, q1, q2, 1.0f};
    v4f cl = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int c = 0; c < 4; c++) cl = __builtin_amdgcn_mfma_f32_4x4x1f32(s_M[c * 4 + row], q[c], cl, 0, 0, 0);
    VOut r = {cl[0], cl[1], cl[2], cl[3], tu, tv};
    return r;
}

}  // namespace mtr
