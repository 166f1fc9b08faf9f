// pose_common.h -- what k_pose.hip and k_anim.hip share: the matrix product of SPEC.md section 12 and the path fold that
// turns the local matrices of one instance (staged in LDS) into its palette.
#pragma once
#include "mtr_internal.h"

namespace mtr {

// out = A * B, column-major: out[c * 4 + i] = fma chain over k = 0..3 of A[k * 4 + i] * B[c * 4 + k], starting from 0
__device__ __forceinline__ void pose_mul(const float4 (&A)[4], const float4 (&B)[4], float4 (&out)[4]) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const float b[4] = {B[c].x, B[c].y, B[c].z, B[c].w};
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            r.x = fmaf(A[k].x, b[k], r.x);
            r.y = fmaf(A[k].y, b[k], r.y);
            r.z = fmaf(A[k].z, b[k], r.z);
            r.w = fmaf(A[k].w, b[k], r.w);
        }
        out[c] = r;
    }
}

// Palette matrix of joint t of instance inst: folds the joint's path over the local matrices in loc[] (LDS, 4 float4 per
// joint; path_lds holds the skeleton's path bytes), multiplies by imat_t and stores it.  The caller has filled loc[] and
// path_lds and passed the barrier; t < p.njoints.
__device__ __forceinline__ void pose_fold_store(const PoseParams& p, const float4* loc, const uint32_t* path_lds, uint32_t inst, uint32_t t) {
    const uint32_t w = p.paths[t];
    const uint8_t* path = reinterpret_cast<const uint8_t*>(path_lds) + (w & 0xFFFFu);
    const uint32_t len = w >> 16;  // >= 1: the root first, t itself last
    float4 W[4], N[4];
    uint32_t a = path[0];
#pragma unroll
    for (int c = 0; c < 4; c++) W[c] = loc[a * 4 + c];
    uint32_t a_next = len > 2 ? path[2] : 0u;
    if (len > 1) {
        a = path[1];
#pragma unroll
        for (int c = 0; c < 4; c++) N[c] = loc[a * 4 + c];
    }
    for (uint32_t s = 1; s < len; s++) {
        float4 L[4];
#pragma unroll
        for (int c = 0; c < 4; c++) L[c] = N[c];
        if (s + 1 < len) {  // the next step's local, and the index of the one after
#pragma unroll
            for (int c = 0; c < 4; c++) N[c] = loc[a_next * 4 + c];
            a_next = s + 2 < len ? path[s + 2] : 0u;
        }
        float4 R[4];
        pose_mul(W, L, R);
#pragma unroll
        for (int c = 0; c < 4; c++) W[c] = R[c];
    }
    const float4* im = reinterpret_cast<const float4*>(p.imats + (size_t)t * 16);
    float4 I[4], P[4];
#pragma unroll
    for (int c = 0; c < 4; c++) I[c] = im[c];
    pose_mul(W, I, P);
    float4* out = reinterpret_cast<float4*>(p.out + ((size_t)inst * p.njoints + t) * 16);
#pragma unroll
    for (int c = 0; c < 4; c++) out[c] = P[c];
}

}  // namespace mtr
