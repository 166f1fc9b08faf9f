// attach_math.h -- the scalar rule of SPEC.md section 18 (attachments) that k_attach.hip is made of: the two clamps, one row
// of the joint matrix A = M_src * P (or M_src alone, or its position-only replacement) and one element of A * O.  Plain C++
// besides the macro, like anim_ik.h, so that tests/test_attach_exact.py compiles this very source for the host
// (-ffp-contract=off) and compares it bit for bit with the numpy model of section 18.
//
// Every product is section 12's chain: out[c * 4 + i] = fmaf over k = 0..3 of A[k * 4 + i] * B[c * 4 + k], from 0.  Nothing
// else is rounded here, and nothing is skipped: the zeros and ones of a position-only A go through the fmas like any value.
#pragma once
#include "clip_math.h"

#ifndef MTR_ATTACH_NO_JOINT  // include/mtr.h has the same
#define MTR_ATTACH_NO_JOINT 0xFFFFFFFFu
#define MTR_ATTACH_POSITION_ONLY 1u
#endif
#define MTR_ATTACH_WORDS 20u  // one record: src_instance, joint, flags, pad, offset[16]

namespace mtr {

// the source instance a record reads: clamped, never rejected (n_src >= 1)
MTR_HD uint32_t attach_instance(uint32_t src_instance, uint32_t n_src) { return src_instance < n_src ? src_instance : n_src - 1u; }

// the palette matrix a record reads, or MTR_ATTACH_NO_JOINT: the record names none, or the source has no palettes
MTR_HD uint32_t attach_joint(uint32_t joint, uint32_t npal) {
    if (joint == MTR_ATTACH_NO_JOINT || npal == 0u) return MTR_ATTACH_NO_JOINT;
    return joint < npal ? joint : npal - 1u;
}

// Row i of the joint matrix: a[k] = A[k * 4 + i].  m: row i of the source instance's matrix (m[k] = M[k * 4 + i]); P: the
// palette matrix, read only with `joint` (attach_joint named one); without, A = M, copied.  With MTR_ATTACH_POSITION_ONLY (bit 0
// of flags, the only bit read) the row is the identity's in columns 0..2 and A's own in column 3, whose last element is 1.
// (P by reference and a flag, not a pointer that may be null: a pointer sends the kernel's copy of P to scratch memory.)
MTR_HD void attach_joint_row(const float (&m)[4], const float (&P)[16], bool joint, uint32_t flags, uint32_t i, float (&a)[4]) {
    for (int c = 0; c < 4; c++) {
        float r = 0.0f;
        for (int k = 0; k < 4; k++) r = fmaf(m[k], P[c * 4 + k], r);
        a[c] = joint ? r : m[c];
    }
    if (flags & MTR_ATTACH_POSITION_ONLY) {
        a[0] = i == 0u ? 1.0f : 0.0f;
        a[1] = i == 1u ? 1.0f : 0.0f;
        a[2] = i == 2u ? 1.0f : 0.0f;
        if (i == 3u) a[3] = 1.0f;
    }
}

// element [c * 4 + i] of A * O from row i of A and column c of O (Oc[k] = O[c * 4 + k])
MTR_HD float attach_elem(const float (&a)[4], const float* Oc) {
    float r = 0.0f;
    for (int k = 0; k < 4; k++) r = fmaf(a[k], Oc[k], r);
    return r;
}

}  // namespace mtr
