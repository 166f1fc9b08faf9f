// anim_launch.h -- whether a launcher of k_anim.hip launches, and with how many threads and how much dynamic LDS: one
// function per stage (plain, layers, IK, spring), given the stage's parameters, the set's kind (tracks) and fold or sample.
// The only copy of these rules.  A launcher whose plan says no launches nothing.  Plain C++, so that
// tests/test_anim_launch_plan.py compiles this very source for the host and pins every term below, one violated at a time.
//
// Every launch: a block per instance, a thread per joint in whole waves.  What the stages differ in, on purpose:
//   - the plain stage wants p.tracks of a track set and asks nothing of p.keys of a uniform one; the layer stage on wants either;
//   - a fold of the plain and layer stages takes pose.path_bytes of LDS for the path table, which must fit; their sample
//     launches take none.  The chain and spring walks need the path table also where nothing is folded: the IK and spring
//     stages take their own path_bytes either way, and a fold reads the same table, so pose.path_bytes must equal it;
//   - the IK part of a spring call may be empty (no chains, no targets); the spring states are written and the motion read
//     16 bytes at a time.
#pragma once
#include "mtr_internal.h"

struct AnimLaunchPlan {
    bool ok;
    uint32_t threads, lds_bytes;
};

inline AnimLaunchPlan anim_launch_plan_of(bool ok, const PoseParams& pose, uint32_t lds_bytes) { return {ok, (pose.njoints + 63u) & ~63u, lds_bytes}; }

inline bool anim_launch_shape_ok(const AnimParams& p, uint32_t ninst) {
    return ninst != 0 && p.nclips != 0 && p.pose.njoints != 0 && p.pose.njoints <= MTR_POSE_MAX_JOINTS;
}
// the layer stack, by whatever stage it is evaluated
inline bool anim_launch_layers_ok(const AnimLayerParams& p, bool tracks, uint32_t ninst) {
    return anim_launch_shape_ok(p.anim, ninst) && p.layers && p.nlayers >= 1u && p.nlayers <= MTR_ANIM_MAX_LAYERS && (p.nmasks == 0u || p.masks) &&
           (tracks ? p.anim.tracks != nullptr : p.anim.keys != nullptr);
}
// the path table the chains and the springs walk
inline bool anim_launch_paths_ok(const AnimIkParams& p, bool fold) {
    return p.paths && p.path_words && p.path_bytes != 0u && p.path_bytes <= MTR_POSE_MAX_PATH_BYTES && (!fold || p.layers.anim.pose.path_bytes == p.path_bytes);
}

inline AnimLaunchPlan anim_launch_plan(const AnimParams& p, bool tracks, bool fold, uint32_t ninst) {
    const bool ok = anim_launch_shape_ok(p, ninst) && (!tracks || p.tracks) && (!fold || p.pose.path_bytes <= MTR_POSE_MAX_PATH_BYTES);
    return anim_launch_plan_of(ok, p.pose, fold ? p.pose.path_bytes : 0u);
}

inline AnimLaunchPlan anim_launch_plan(const AnimLayerParams& p, bool tracks, bool fold, uint32_t ninst) {
    const bool ok = anim_launch_layers_ok(p, tracks, ninst) && (!fold || p.anim.pose.path_bytes <= MTR_POSE_MAX_PATH_BYTES);
    return anim_launch_plan_of(ok, p.anim.pose, fold ? p.anim.pose.path_bytes : 0u);
}

inline AnimLaunchPlan anim_launch_plan(const AnimIkParams& p, bool tracks, bool fold, uint32_t ninst) {
    const bool ok = anim_launch_layers_ok(p.layers, tracks, ninst) && p.chains && p.targets && p.nchains >= 1u && p.nchains <= MTR_ANIM_MAX_IK &&
                    anim_launch_paths_ok(p, fold);
    return anim_launch_plan_of(ok, p.layers.anim.pose, p.path_bytes);
}

inline AnimLaunchPlan anim_launch_plan(const AnimSpringParams& p, bool tracks, bool fold, uint32_t ninst) {
    const AnimIkParams& ip = p.ik;
    const bool ok = anim_launch_layers_ok(ip.layers, tracks, ninst) && ip.nchains <= MTR_ANIM_MAX_IK && (ip.nchains == 0u || (ip.chains && ip.targets)) &&
                    anim_launch_paths_ok(ip, fold) && p.springs && p.joint_tab && p.states && ((uintptr_t)p.states & 15u) == 0u &&
                    ((uintptr_t)p.motion & 15u) == 0u && p.nsprings >= 1u && p.nsprings <= MTR_ANIM_MAX_SPRINGS && p.nrounds >= 1u && p.nrounds <= p.nsprings;
    return anim_launch_plan_of(ok, ip.layers.anim.pose, ip.path_bytes);
}
