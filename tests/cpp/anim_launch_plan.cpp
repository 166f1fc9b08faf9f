// The launch decisions of k_anim.hip's four launchers, pinned on the CPU: csrc/anim_launch.h over the stand-in HIP runtime of
// tests/cpp/hip_stub, compiled with AddressSanitizer and UBSan.  A launcher whose decision says no launches nothing and
// reports nothing, so a lost test would go unseen everywhere else.  For each of the sixteen (stage, tracks, fold)
// combinations the program builds one valid parameter block as the host fills it (4 joints, 1 clip, 3 instances, 12 path
// bytes, 1 layer, 1 chain, 1 spring, 1 round, no masks; a fold carries the skeleton's path bytes in pose, a sample call 0)
// and prints `ok threads lds` for it and for the block with one thing wrong at a time.  No pointer is read through: only
// null-ness, alignment and the counts matter.  tests/test_anim_launch_plan.py compares the text with
// tests/golden/anim_launch_plan.txt, which was recorded from the sixteen launchers this header replaced.
#include "../../mt_renderer_amd/csrc/anim_launch.h"
#include <cstdio>
#include <functional>
#include <string>
#include <vector>

enum Stage { kPlain, kLayers, kIk, kSpring };
static const char* const kStageName[4] = {"anim", "anim_layers", "anim_ik", "anim_spring"};

struct Case {
    AnimSpringParams sp;  // the four blocks nest: each stage is handed the part it knows
    uint32_t ninst;
};

alignas(16) static uint32_t g_mem[64];  // every pointer of a valid block points here, 16-byte aligned
template <class T> static T* at(size_t byte_off = 0) { return reinterpret_cast<T*>(reinterpret_cast<char*>(g_mem) + byte_off); }

static Case valid(int stage, bool tracks, bool fold) {
    Case c{};
    c.ninst = 3;
    AnimIkParams& ip = c.sp.ik;
    AnimLayerParams& lp = ip.layers;
    AnimParams& ap = lp.anim;
    ap.pose.out = at<float>();
    ap.pose.njoints = 4;
    if (fold) { ap.pose.imats = at<float>(); ap.pose.paths = at<uint32_t>(); ap.pose.path_words = at<uint32_t>(); ap.pose.path_bytes = 12; }
    ap.clips = at<uint32_t>();
    ap.nclips = 1;
    if (tracks) { ap.tracks = at<uint32_t>(); ap.values = at<uint32_t>(); ap.times = at<uint16_t>(); }
    else ap.keys = at<float>();
    if (stage == kPlain) { ap.states = at<uint32_t>(); return c; }
    lp.layers = at<uint32_t>();
    lp.nlayers = 1;
    if (stage == kLayers) return c;
    ip.chains = at<uint32_t>(); ip.targets = at<uint32_t>(); ip.nchains = 1;
    ip.paths = at<uint32_t>(); ip.path_words = at<uint32_t>(); ip.path_bytes = 12;
    if (stage == kIk) return c;
    c.sp.springs = at<uint32_t>(); c.sp.joint_tab = at<uint32_t>(); c.sp.states = at<uint32_t>(); c.sp.motion = at<float>();
    c.sp.dt = 0.016f; c.sp.nsprings = 1; c.sp.nrounds = 1;
    return c;
}

static AnimLaunchPlan plan(int stage, const Case& c, bool tracks, bool fold) {
    switch (stage) {
    case kPlain: return anim_launch_plan(c.sp.ik.layers.anim, tracks, fold, c.ninst);
    case kLayers: return anim_launch_plan(c.sp.ik.layers, tracks, fold, c.ninst);
    case kIk: return anim_launch_plan(c.sp.ik, tracks, fold, c.ninst);
    default: return anim_launch_plan(c.sp, tracks, fold, c.ninst);
    }
}

struct Violation {
    std::string name;
    int from;  // the first stage it applies to
    std::function<void(Case&)> make;
};

int main() {
    for (int stage = 0; stage < 4; stage++)
        for (int tracks = 0; tracks < 2; tracks++)
            for (int fold = 1; fold >= 0; fold--) {
                const std::string who = std::string(kStageName[stage]) + (tracks ? "_tracks" : "") + (fold ? "" : "_sample");
                // the path bytes a stage launches with: pose's for the plain and layer stages, its own from the IK stage on, where a
                // fold wants pose's equal: both are set together, and the mismatch is a case of its own
                auto path_bytes = [=](Case& c, uint32_t v) {
                    if (stage >= kIk) c.sp.ik.path_bytes = v;
                    if (stage < kIk || fold) c.sp.ik.layers.anim.pose.path_bytes = v;
                };
                std::vector<Violation> vs;
                auto add = [&](const char* name, int from, std::function<void(Case&)> f) { vs.push_back({name, from, std::move(f)}); };
                auto anim = [](Case& c) -> AnimParams& { return c.sp.ik.layers.anim; };
                add("ninst=0", kPlain, [](Case& c) { c.ninst = 0; });
                add("nclips=0", kPlain, [=](Case& c) { anim(c).nclips = 0; });
                add("njoints=0", kPlain, [=](Case& c) { anim(c).pose.njoints = 0; });
                add("njoints=256", kPlain, [=](Case& c) { anim(c).pose.njoints = 256; });
                add("njoints=257", kPlain, [=](Case& c) { anim(c).pose.njoints = 257; });
                add("clips=null", kPlain, [=](Case& c) { anim(c).clips = nullptr; });
                add("source=null", kPlain, [=](Case& c) { anim(c).keys = nullptr; anim(c).tracks = nullptr; });  // keys or tracks, whichever the set has
                add("values=null", kPlain, [=](Case& c) { anim(c).values = nullptr; });
                add("times=null", kPlain, [=](Case& c) { anim(c).times = nullptr; });
                add("states=null", kPlain, [=](Case& c) { anim(c).states = nullptr; });
                add("out=null", kPlain, [=](Case& c) { anim(c).pose.out = nullptr; });
                add("path_bytes=0", kPlain, [=](Case& c) { path_bytes(c, 0); });
                add("path_bytes=max", kPlain, [=](Case& c) { path_bytes(c, MTR_POSE_MAX_PATH_BYTES); });
                add("path_bytes=max+4", kPlain, [=](Case& c) { path_bytes(c, MTR_POSE_MAX_PATH_BYTES + 4); });
                add("pose.path_bytes!=path_bytes", kPlain, [=](Case& c) { anim(c).pose.path_bytes = 16; });
                add("layers=null", kLayers, [](Case& c) { c.sp.ik.layers.layers = nullptr; });
                add("nlayers=0", kLayers, [](Case& c) { c.sp.ik.layers.nlayers = 0; });
                add("nlayers=8", kLayers, [](Case& c) { c.sp.ik.layers.nlayers = 8; });
                add("nlayers=9", kLayers, [](Case& c) { c.sp.ik.layers.nlayers = 9; });
                add("nmasks=2 masks=null", kLayers, [](Case& c) { c.sp.ik.layers.nmasks = 2; });
                add("nmasks=2", kLayers, [](Case& c) { c.sp.ik.layers.nmasks = 2; c.sp.ik.layers.masks = at<float>(); });
                add("chains=null", kIk, [](Case& c) { c.sp.ik.chains = nullptr; });
                add("targets=null", kIk, [](Case& c) { c.sp.ik.targets = nullptr; });
                add("paths=null", kIk, [](Case& c) { c.sp.ik.paths = nullptr; });
                add("path_words=null", kIk, [](Case& c) { c.sp.ik.path_words = nullptr; });
                add("nchains=0", kIk, [](Case& c) { c.sp.ik.nchains = 0; });
                add("nchains=0 chains=null targets=null", kIk, [](Case& c) { c.sp.ik.nchains = 0; c.sp.ik.chains = nullptr; c.sp.ik.targets = nullptr; });
                add("nchains=4", kIk, [](Case& c) { c.sp.ik.nchains = 4; });
                add("nchains=5", kIk, [](Case& c) { c.sp.ik.nchains = 5; });
                add("springs=null", kSpring, [](Case& c) { c.sp.springs = nullptr; });
                add("joint_tab=null", kSpring, [](Case& c) { c.sp.joint_tab = nullptr; });
                add("spring_states=null", kSpring, [](Case& c) { c.sp.states = nullptr; });
                add("motion=null", kSpring, [](Case& c) { c.sp.motion = nullptr; });
                add("spring_states+8", kSpring, [](Case& c) { c.sp.states = at<uint32_t>(8); });
                add("motion+8", kSpring, [](Case& c) { c.sp.motion = at<float>(8); });
                add("nsprings=0", kSpring, [](Case& c) { c.sp.nsprings = 0; });
                add("nsprings=16", kSpring, [](Case& c) { c.sp.nsprings = 16; });
                add("nsprings=17", kSpring, [](Case& c) { c.sp.nsprings = 17; });
                add("nrounds=0", kSpring, [](Case& c) { c.sp.nrounds = 0; });
                add("nrounds=nsprings", kSpring, [](Case& c) { c.sp.nsprings = 16; c.sp.nrounds = 16; });
                add("nrounds=nsprings+1", kSpring, [](Case& c) { c.sp.nsprings = 16; c.sp.nrounds = 17; });

                const Case ok = valid(stage, tracks, fold);
                const AnimLaunchPlan p0 = plan(stage, ok, tracks, fold);
                printf("%s valid: %d %u %u\n", who.c_str(), (int)p0.ok, p0.threads, p0.lds_bytes);
                for (const Violation& v : vs) {
                    if (v.from > stage) continue;
                    Case c = ok;
                    v.make(c);
                    const AnimLaunchPlan p = plan(stage, c, tracks, fold);
                    printf("  %s: %d %u %u\n", v.name.c_str(), (int)p.ok, p.threads, p.lds_bytes);
                }
                for (uint32_t nj : {1u, 64u, 65u, 256u}) {
                    Case c = ok;
                    c.sp.ik.layers.anim.pose.njoints = nj;
                    printf("  njoints=%u threads: %u\n", nj, plan(stage, c, tracks, fold).threads);
                }
            }
    return 0;
}
