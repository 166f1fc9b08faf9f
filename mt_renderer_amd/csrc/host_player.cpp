// host_player.cpp -- players (SPEC.md section 20): the player set, and the advance calls that run k_play on play states in
// device memory.
#include "host.h"

// k_play.hip.  Weak: the host-only builds of this file (tests/cpp, over the HIP stub runtime) link no kernels; libmtr.so
// links k_play.o.
void mtr_launch_play(const PlayParams& p, hipStream_t s) __attribute__((weak));

namespace mtr_host {

namespace {

constexpr size_t kPlayMaxInstances = (size_t)1 << 27, kPlayMaxCmds = ((size_t)1 << 31) - 1;

struct PlayOuts {
    mtr_anim_state* states = nullptr;
    mtr_anim_layer* layers = nullptr;
    size_t nlayers = 0;
    mtr_root_step* steps = nullptr;
};

// what every advance call checks before it touches anything; device: the pointers are device memory and must be aligned
int32_t play_check(const mtr_anim_player* pl, const void* states, size_t n, const void* cmds, size_t ncmds, const PlayOuts& o, bool device) {
    mtr_device* d = pl->dev;
    if (!states) return fail(d, MTR_E_INVALID, "player advance: no states");
    if (n == 0 || n > pl->max_instances) return fail(d, MTR_E_INVALID, "player advance: 1 to max_instances instances");
    if (ncmds > 0 && !cmds) return fail(d, MTR_E_INVALID, "player advance: commands counted and none given");
    if (ncmds > kPlayMaxCmds) return fail(d, MTR_E_INVALID, "player advance: fewer than 2^31 commands");
    if (o.layers && (o.nlayers < 2 || o.nlayers > MTR_ANIM_MAX_LAYERS)) return fail(d, MTR_E_INVALID, "player advance: 2 to 8 layers per instance");
    if (device) {
        if (((uintptr_t)states & 15u) || ((uintptr_t)o.layers & 15u) || ((uintptr_t)o.steps & 15u))
            return fail(d, MTR_E_INVALID, "player advance: device states, layers and steps must be 16-byte aligned");
        if ((uintptr_t)o.states & 7u) return fail(d, MTR_E_INVALID, "player advance: device animation states must be 8-byte aligned");
    }
    if (!mtr_launch_play) return fail(d, MTR_E_UNSUPPORTED, "player advance: built without k_play");
    return set_device(d);
}

// k_play on `s` between the player's events: its calls are ordered among themselves (the scratch array, the staged commands)
int32_t play_launch(mtr_anim_player* pl, void* states_dev, size_t n, float dt, const void* cmds_dev, size_t ncmds, const PlayOuts& o, hipStream_t s) {
    mtr_device* d = pl->dev;
    PlayParams pp{};
    pp.table = pl->d;
    pp.scratch = pl->d + (size_t)pl->nclips * 4;
    pp.states = static_cast<uint32_t*>(states_dev);
    pp.cmds = static_cast<const uint32_t*>(cmds_dev);
    pp.out_states = reinterpret_cast<uint32_t*>(o.states);
    pp.out_layers = reinterpret_cast<uint32_t*>(o.layers);
    pp.out_steps = reinterpret_cast<uint32_t*>(o.steps);
    pp.ncmds = (uint32_t)ncmds; pp.nclips = pl->nclips; pp.nlayers = (uint32_t)o.nlayers; pp.n = (uint32_t)n; pp.dt = dt;
    mtr_launch_play(pp, s);
    HIPCHK(d, hipGetLastError());
    return set_after(pl, s);
}

// room for ncmds commands in the player's staging buffer; an outgrown buffer is parked behind the last kernel that read it
int32_t play_reserve_cmds(mtr_anim_player* pl, size_t ncmds) {
    mtr_device* d = pl->dev;
    if (ncmds <= pl->cmd_cap) return MTR_OK;
    uint32_t* fresh = nullptr;
    hipEvent_t ev = nullptr;
    int32_t rc = dev_alloc(d, &fresh, ncmds * 4);
    if (rc) return rc;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { (void)hipFree(fresh); return fail(d, MTR_E_HIP, "hipEventCreate failed"); }
    if (pl->cmds) {
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        d->garbage.push_back({pl->cmds, 0, pl->cmd_last});
    } else if (pl->cmd_last) {
        (void)hipEventDestroy(pl->cmd_last);
    }
    pl->cmds = fresh; pl->cmd_cap = ncmds; pl->cmd_last = ev;
    return MTR_OK;
}

int32_t play_advance_device(mtr_anim_player* pl, mtr_play_state* states_dev, size_t n, float dt, const mtr_play_cmd* cmds, size_t ncmds, bool cmds_on_device,
                            const PlayOuts& o, void* hip_stream) {
    if (!pl) return MTR_E_INVALID;
    mtr_device* d = pl->dev;
    if (cmds_on_device && ncmds > 0 && ((uintptr_t)cmds & 15u)) return fail(d, MTR_E_INVALID, "player advance: device commands must be 16-byte aligned");
    int32_t rc = play_check(pl, states_dev, n, cmds, ncmds, o, true);
    if (rc) return rc;
    hipStream_t s = caller_stream(d, hip_stream);
    const void* cmds_dev = cmds;
    if (ncmds > 0 && !cmds_on_device && (rc = play_reserve_cmds(pl, ncmds))) return rc;
    if ((rc = set_before(pl, s))) return rc;
    if (ncmds > 0 && !cmds_on_device) {
        HIPCHK(d, hipMemcpyAsync(pl->cmds, cmds, ncmds * sizeof(mtr_play_cmd), hipMemcpyHostToDevice, s));
        cmds_dev = pl->cmds;
    }
    if ((rc = play_launch(pl, states_dev, n, dt, cmds_dev, ncmds, o, s))) return rc;
    if (ncmds > 0 && !cmds_on_device) HIPCHK(d, hipEventRecord(pl->cmd_last, s));
    return MTR_OK;
}

}  // namespace

}  // namespace mtr_host

using namespace mtr_host;

extern "C" {

static_assert(sizeof(mtr_play_state) == 32 && sizeof(mtr_play_cmd) == 16, "mtr_play_state, mtr_play_cmd");

int32_t mtr_anim_player_create(mtr_device* d, size_t nclips, const uint32_t* nkeys, const uint32_t* flags, const float* rates, size_t max_instances,
                               mtr_anim_player** out) {
    if (!d || !out) return MTR_E_INVALID;
    *out = nullptr;
    if (nclips == 0 || nclips > kClipMaxKeys) return fail(d, MTR_E_INVALID, "anim player: at least one clip");
    if (!nkeys || !rates) return fail(d, MTR_E_INVALID, "anim player: no key counts or no rates");
    if (max_instances == 0 || max_instances > kPlayMaxInstances) return fail(d, MTR_E_INVALID, "anim player: 1 to 2^27 instances");
    std::vector<uint32_t> img(nclips * 4);
    int32_t rc;
    for (size_t c = 0; c < nclips; c++)
        if ((rc = clip_entry(d, "anim player", c, nkeys, flags ? flags[c] : 0u, rates, &img[c * 4]))) return rc;
    if ((rc = set_device(d))) return rc;
    auto pl = std::make_unique<mtr_anim_player>();
    pl->dev = d; pl->nclips = (uint32_t)nclips; pl->max_instances = (uint32_t)max_instances;
    if ((rc = set_upload(pl.get(), "anim player", {{img.data(), img.size() * 4}, {nullptr, max_instances * 4}}))) return rc;  // the table, the zeroed scratch
    *out = pl.release();
    return MTR_OK;
}

void mtr_anim_player_destroy(mtr_anim_player* pl) {
    if (!pl) return;
    mtr_device* d = pl->dev;
    set_park(pl);
    if (pl->cmds || pl->cmd_last) {  // the staged commands likewise, behind the last kernel that read them
        std::lock_guard<std::mutex> submit_lock(d->submit_mu);
        d->garbage.push_back({pl->cmds, 0, pl->cmd_last});
    }
    delete pl;
}

int32_t mtr_anim_player_advance_device(mtr_anim_player* pl, mtr_play_state* states_dev, size_t n, float dt, const mtr_play_cmd* cmds, size_t ncmds,
                                       mtr_anim_state* out_states_dev, mtr_anim_layer* out_layers_dev, size_t nlayers, mtr_root_step* out_steps_dev,
                                       void* hip_stream) {
    return play_advance_device(pl, states_dev, n, dt, cmds, ncmds, false, PlayOuts{out_states_dev, out_layers_dev, nlayers, out_steps_dev}, hip_stream);
}

int32_t mtr_anim_player_advance_device_cmds(mtr_anim_player* pl, mtr_play_state* states_dev, size_t n, float dt, const mtr_play_cmd* cmds_dev, size_t ncmds,
                                            mtr_anim_state* out_states_dev, mtr_anim_layer* out_layers_dev, size_t nlayers, mtr_root_step* out_steps_dev,
                                            void* hip_stream) {
    return play_advance_device(pl, states_dev, n, dt, cmds_dev, ncmds, true, PlayOuts{out_states_dev, out_layers_dev, nlayers, out_steps_dev}, hip_stream);
}

int32_t mtr_anim_player_advance_host(mtr_anim_player* pl, mtr_play_state* states, size_t n, float dt, const mtr_play_cmd* cmds, size_t ncmds,
                                     mtr_anim_state* out_states, mtr_anim_layer* out_layers, size_t nlayers, mtr_root_step* out_steps) {
    if (!pl) return MTR_E_INVALID;
    mtr_device* d = pl->dev;
    const PlayOuts host{out_states, out_layers, nlayers, out_steps};
    int32_t rc = play_check(pl, states, n, cmds, ncmds, host, false);
    if (rc) return rc;
    // one block of 16-byte words: the states, the commands, the steps, the layers, then the animation states (24 bytes each)
    StagedBlock blk(d);
    StagedPart &p_states = blk.part(states, n * 8), &p_cmds = blk.part(cmds, ncmds * 4), &p_steps = blk.part(out_steps, out_steps ? n * 8 : 0),
               &p_layers = blk.part(out_layers, out_layers ? n * nlayers * 4 : 0), &p_anim = blk.part(out_states, out_states ? n * 6 : 0);
    return blk.run([&]() -> int32_t {
        int32_t r2;
        if ((r2 = blk.up({&p_states, &p_cmds, &p_layers})) || (r2 = set_before(pl, d->s_copy))) return r2;
        const PlayOuts o{p_anim.dev<mtr_anim_state>(), p_layers.dev<mtr_anim_layer>(), nlayers, p_steps.dev<mtr_root_step>()};
        if ((r2 = play_launch(pl, p_states.at, n, dt, p_cmds.at, ncmds, o, d->s_copy))) return r2;  // no commands: where they would lie, unread
        return blk.down({&p_states, &p_steps, &p_layers, &p_anim});
    });
}

}  // extern "C"
