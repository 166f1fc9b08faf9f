// k_pose.hip -- skin palettes from skeletal poses (SPEC.md section 12).  For every instance and joint j:
//   world_j   = local_j                    (a root: parent 255 or itself)
//             = world_parent(j) * local_j  (otherwise)
//   palette_j = world_j * imat_j
// every product the k-ordered fma chain from 0 of SPEC.md section 4 (mtr_files.cpp: mat4_mul_fma), so the result is bit
// for bit what mtr_rmodel_palette forms on the host.
//
// One workgroup per instance, one thread per joint.  The instance's local matrices and the skeleton's paths (for joint j:
// the joints from its root down to j) are staged in LDS once; thread j then folds its own path,
//   W = local_root;  W = W * local_a;  W = W * local_b;  ...  W = W * local_j
// which is the same sequence of products, in the same order, as forming the worlds level by level (each prefix is the
// world of that ancestor), but with no barrier per level: a 64-deep chain cost 25 us at 1 024 instances with one barrier
// per level (the chain is latency-bound), the fold pays one LDS read per step, issued a step ahead.  The output is the
// palette layout k_geom and the culling kernels read (GeomParams::palettes, pal_stride = njoints * 16).
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

__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_pose(PoseParams p) {
    __shared__ float4 loc[MTR_POSE_MAX_JOINTS * 4];
    extern __shared__ uint32_t path_lds[];  // p.path_bytes / 4 words
    const uint32_t inst = blockIdx.x, t = threadIdx.x, J = p.njoints;
    const float4* src = reinterpret_cast<const float4*>(p.locals + (size_t)inst * J * 16);
    for (uint32_t i = t; i < J * 4; i += blockDim.x) loc[i] = src[i];
    for (uint32_t i = t; i < p.path_bytes / 4; i += blockDim.x) path_lds[i] = p.path_words[i];
    __syncthreads();
    if (t >= J) return;
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
    float4* out = reinterpret_cast<float4*>(p.out + ((size_t)inst * J + t) * 16);
#pragma unroll
    for (int c = 0; c < 4; c++) out[c] = P[c];
}

}  // namespace mtr

void mtr_launch_pose(const PoseParams& p, uint32_t ninst, hipStream_t s) {
    if (ninst == 0 || p.njoints == 0 || p.njoints > MTR_POSE_MAX_JOINTS || p.path_bytes > MTR_POSE_MAX_PATH_BYTES) return;
    const uint32_t threads = (p.njoints + 63u) & ~63u;
    hipLaunchKernelGGL(mtr::k_pose, dim3(ninst), dim3(threads), p.path_bytes, s, p);
}
