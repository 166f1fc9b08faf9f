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
#include "pose_common.h"

namespace mtr {

__global__ __launch_bounds__(MTR_POSE_MAX_JOINTS) void k_pose(PoseParams p) {
    __shared__ float4 loc[MTR_POSE_MAX_JOINTS * 4];
    extern __shared__ uint32_t path_lds[];  // p.path_bytes / 4 words
    const uint32_t inst = blockIdx.x, t = threadIdx.x, J = p.njoints;
    const float4* src = reinterpret_cast<const float4*>(p.locals + (size_t)inst * J * 16);
    for (uint32_t i = t; i < J * 4; i += blockDim.x) loc[i] = src[i];
    for (uint32_t i = t; i < p.path_bytes / 4; i += blockDim.x) path_lds[i] = p.path_words[i];
    __syncthreads();
    if (t >= J) return;
    pose_fold_store(p, loc, path_lds, inst, t);
}

}  // namespace mtr

void mtr_launch_pose(const PoseParams& p, uint32_t ninst, hipStream_t s) {
    if (ninst == 0 || p.njoints == 0 || p.njoints > MTR_POSE_MAX_JOINTS || p.path_bytes > MTR_POSE_MAX_PATH_BYTES) return;
    const uint32_t threads = (p.njoints + 63u) & ~63u;
    hipLaunchKernelGGL(mtr::k_pose, dim3(ninst), dim3(threads), p.path_bytes, s, p);
}
