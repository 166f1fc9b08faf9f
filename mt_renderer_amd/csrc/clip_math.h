// clip_math.h -- the scalar rules of SPEC.md section 14 that every animation kernel shares: the wrap of a position into
// [0, P) with its fall-back, its clamp to [0, P], and the clamp of a weight.  The only copy: the key positions of k_anim.hip
// (anim_tracks.h), the players (play_math.h), the events (event_math.h) and root motion (root_math.h) call these, and
// sections 19 to 23 require them to agree bit for bit.  Also MTR_HD, the one function qualifier of the animation headers.
// Plain C++ besides the macro, so that the tests compile this very source for the host (-ffp-contract=off).
//
// One rounded operation per operator; nothing here is fused.  NaN compares false, which every test below is written for.
#pragma once
#include <cstdint>
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MTR_HD __host__ __device__ __forceinline__
#else
#define MTR_HD inline
#endif

#ifndef MTR_CLIP_LOOP  // include/mtr.h has the same
#define MTR_CLIP_LOOP 1u
#endif

namespace mtr {

// x into [0, P): NaN, +-inf, a huge x, and r == P for a tiny negative x fall back to 0
MTR_HD float clip_wrap(float x, float P) {
    const float r = x - floorf(x / P) * P;
    return (r >= 0.0f && r < P) ? r : 0.0f;
}

// x into [0, P]: NaN -> 0, -0 stays
MTR_HD float clip_clamp(float x, float P) {
    const float r = x >= 0.0f ? x : 0.0f;
    return r > P ? P : r;
}

// a cross-fade, layer, chain or step weight: NaN -> 0, then [0, 1]
MTR_HD float anim_weight(float w) {
    w = w > 0.0f ? w : 0.0f;
    return w > 1.0f ? 1.0f : w;
}

}  // namespace mtr
