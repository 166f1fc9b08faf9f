// k_attach.hip -- instance matrices from another batch's joints (SPEC.md section 18).  For record r against a source of n_src
// instances with npal palette matrices each:
//   s = min(src_instance, n_src - 1);  A = M_src[s]  or  M_src[s] * P_src[s][min(joint, npal - 1)];
//   MTR_ATTACH_POSITION_ONLY: A's columns 0..2 become the identity's, its column 3 (A[12], A[13], A[14], 1);
//   out[r] = A * O_r
// every product the k-ordered fma chain from 0 of section 12, through attach_math.h, which the host test compiles too.
//
// 16 lanes per record, lane e = c * 4 + i writes out[r][e]: four records per wave, 16 per workgroup of 256.  A lane forms
// row i of A itself (16 fmas from row i of M and the whole of P) and then its one element of A * O, so no lane waits for
// another: no LDS, no cross-lane move, no barrier.  The kernel is a chain of three dependent loads (record -> indices ->
// M_src and P) and nothing else; every load of a step is issued before the first use of any of them.  The 16 lanes of a
// record read the same header, M and P (one request each per row of 16 lanes) and one column of O each.
#include "mtr_internal.h"
#include "attach_math.h"

namespace mtr {

__global__ __launch_bounds__(256) void k_attach(AttachParams p) {
    const uint32_t r = blockIdx.x * 16u + (threadIdx.x >> 4), e = threadIdx.x & 15u;
    if (r >= p.n) return;
    const uint32_t i = e & 3u, c = e >> 2;
    const uint4* rec = reinterpret_cast<const uint4*>(p.recs + (size_t)r * MTR_ATTACH_WORDS);
    const uint4 hdr = rec[0];       // src_instance, joint, flags, pad
    const uint4 ocol = rec[1 + c];  // column c of O
    const uint32_t s = attach_instance(hdr.x, p.n_src), j = attach_joint(hdr.y, p.npal);
    const float* Mp = p.src_mats + (size_t)s * 16;
    float m[4], P[16] = {};
#pragma unroll
    for (int k = 0; k < 4; k++) m[k] = Mp[k * 4 + i];  // row i of M
    const bool joint = j != MTR_ATTACH_NO_JOINT;
    if (joint) {
        const float4* P4 = reinterpret_cast<const float4*>(p.src_pals + ((size_t)s * p.npal + j) * 16);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float4 v = P4[k];
            P[k * 4 + 0] = v.x; P[k * 4 + 1] = v.y; P[k * 4 + 2] = v.z; P[k * 4 + 3] = v.w;
        }
    }
    float a[4];
    attach_joint_row(m, P, joint, hdr.z, i, a);
    const float Oc[4] = {__uint_as_float(ocol.x), __uint_as_float(ocol.y), __uint_as_float(ocol.z), __uint_as_float(ocol.w)};
    p.out[(size_t)r * 16 + e] = attach_elem(a, Oc);
}

}  // namespace mtr

void mtr_launch_attach(const AttachParams& p, hipStream_t s) {
    if (p.n == 0 || p.n_src == 0) return;
    hipLaunchKernelGGL(mtr::k_attach, dim3((p.n + 15u) / 16u), dim3(256), 0, s, p);
}
