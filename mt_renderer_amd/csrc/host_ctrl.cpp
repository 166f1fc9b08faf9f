// host_ctrl.cpp -- controllers (SPEC.md section 21): the controller handle, its validated tables, and the step calls that
// run k_ctrl on controller states, play states and parameters in device memory.
#include "host.h"

// k_ctrl.hip.  Weak: the host-only builds of this file (tests/cpp, over the HIP stub runtime) link no kernels; libmtr.so
// links k_ctrl.o.
void mtr_launch_ctrl(const CtrlParams& p, hipStream_t s) __attribute__((weak));

namespace mtr_host {

namespace {

constexpr size_t kCtrlMaxInstances = (size_t)1 << 27, kCtrlMaxNodes = 65535, kCtrlMaxTrans = (size_t)1 << 20,
                 kCtrlMaxParams = 16;
constexpr uint32_t kCtrlFlags = MTR_TR_INTERRUPT | MTR_TR_SELF | MTR_TR_SYNC | MTR_TR_CONSUME;

// what every step call checks before it touches anything; device: the pointers are device memory and must be aligned
int32_t ctrl_check(const mtr_anim_ctrl* c, const void* states, const void* play, const void* params, size_t n, const void* cmds, const void* counts,
                   bool device) {
    mtr_device* d = c->dev;
    if (!states || !play || !cmds) return fail(d, MTR_E_INVALID, "ctrl step: no states, no play states or no commands");
    if (n == 0 || n > kCtrlMaxInstances) return fail(d, MTR_E_INVALID, "ctrl step: 1 to 2^27 instances");
    if (c->nparams > 0 && !params) return fail(d, MTR_E_INVALID, "ctrl step: the controller has parameters and none are given");
    if (device) {
        if (((uintptr_t)states & 15u) || ((uintptr_t)play & 15u) || ((uintptr_t)cmds & 15u))
            return fail(d, MTR_E_INVALID, "ctrl step: device states, play states and commands must be 16-byte aligned");
        if (((uintptr_t)params & 3u) || ((uintptr_t)counts & 3u)) return fail(d, MTR_E_INVALID, "ctrl step: device parameters and counts must be 4-byte aligned");
    }
    if (!mtr_launch_ctrl) return fail(d, MTR_E_UNSUPPORTED, "ctrl step: built without k_ctrl");
    return set_device(d);
}

// k_ctrl on `s` between the controller's events: a step on another stream than the one before first waits for it, so the
// one event covers every reader of the tables and the destroy can park them behind it (DeviceSet::last)
int32_t ctrl_launch(mtr_anim_ctrl* c, void* states_dev, const void* play_dev, float* params_dev, size_t n, float dt, void* cmds_dev, uint32_t* counts_dev,
                    hipStream_t s) {
    mtr_device* d = c->dev;
    int32_t rc = set_before(c, s);
    if (rc) return rc;
    CtrlParams cp{};
    cp.clips = c->d;
    cp.nodes = c->d + (size_t)c->nclips * 4;
    cp.trans = cp.nodes + (size_t)c->nnodes * 4;
    cp.states = static_cast<uint32_t*>(states_dev);
    cp.play = static_cast<const uint32_t*>(play_dev);
    cp.params = c->nparams ? params_dev : nullptr;
    cp.cmds = static_cast<uint32_t*>(cmds_dev);
    cp.counts = counts_dev;
    cp.nnodes = c->nnodes; cp.nany = c->nany; cp.nclips = c->nclips; cp.nparams = c->nparams; cp.n = (uint32_t)n; cp.dt = dt;
    mtr_launch_ctrl(cp, s);
    HIPCHK(d, hipGetLastError());
    return set_after(c, s);
}

}  // namespace

}  // namespace mtr_host

using namespace mtr_host;

extern "C" {

static_assert(sizeof(mtr_ctrl_node) == 16 && sizeof(mtr_ctrl_cond) == 8 && sizeof(mtr_ctrl_trans) == 48 && sizeof(mtr_ctrl_state) == 16,
              "mtr_ctrl_node, mtr_ctrl_cond, mtr_ctrl_trans, mtr_ctrl_state");

int32_t mtr_anim_ctrl_create(mtr_device* d, size_t nclips, const uint32_t* nkeys, const uint32_t* clip_flags, const mtr_ctrl_node* nodes, size_t nnodes,
                             const mtr_ctrl_trans* trans, size_t ntrans, size_t nany, size_t nparams, mtr_anim_ctrl** out) {
    if (!d || !out) return MTR_E_INVALID;
    *out = nullptr;
    if (nclips == 0 || nclips > kClipMaxKeys) return fail(d, MTR_E_INVALID, "anim ctrl: 1 to 2^24 clips");
    if (!nkeys) return fail(d, MTR_E_INVALID, "anim ctrl: no key counts");
    if (!nodes || nnodes == 0 || nnodes > kCtrlMaxNodes) return fail(d, MTR_E_INVALID, "anim ctrl: 1 to 65535 nodes");
    if (ntrans > kCtrlMaxTrans || (ntrans > 0 && !trans)) return fail(d, MTR_E_INVALID, "anim ctrl: 0 to 2^20 transitions");
    if (nany > ntrans) return fail(d, MTR_E_INVALID, "anim ctrl: more any-state transitions than transitions");
    if (nparams > kCtrlMaxParams) return fail(d, MTR_E_INVALID, "anim ctrl: 0 to 16 parameters");
    std::vector<uint32_t> img(nclips * 4);
    int32_t rc;
    for (size_t c = 0; c < nclips; c++)
        if ((rc = clip_entry(d, "anim ctrl", c, nkeys, clip_flags ? clip_flags[c] : 0u, nullptr, &img[c * 4]))) return rc;
    for (size_t i = 0; i < nnodes; i++) {
        const mtr_ctrl_node& nd = nodes[i];
        const std::string who = "anim ctrl: node " + std::to_string(i) + " ";
        if (nd.clip >= nclips) return fail(d, MTR_E_INVALID, who + "names a clip the set does not have");
        if (nd.first < nany || nd.first > ntrans || nd.count > ntrans - nd.first)  // no 32-bit sum: nothing wraps
            return fail(d, MTR_E_INVALID, who + "has transitions outside [nany, ntrans]");
    }
    for (size_t i = 0; i < ntrans; i++) {
        const mtr_ctrl_trans& t = trans[i];
        const std::string who = "anim ctrl: transition " + std::to_string(i) + " ";
        if (t.target >= nnodes) return fail(d, MTR_E_INVALID, who + "targets a node the controller does not have");
        if (t.flags & ~kCtrlFlags) return fail(d, MTR_E_INVALID, who + "has unknown flag bits");
        if (t.ncond > MTR_CTRL_MAX_COND) return fail(d, MTR_E_INVALID, who + "has more than 3 conditions");
        for (uint32_t k = 0; k < t.ncond; k++) {
            if (t.cond[k].op > MTR_OP_NE) return fail(d, MTR_E_INVALID, who + "has a condition with an unknown op");
            if (t.cond[k].param >= nparams && t.cond[k].param < MTR_CTRL_FADING)
                return fail(d, MTR_E_INVALID, who + "has a condition on a parameter the controller does not have");
        }
    }
    if ((rc = set_device(d))) return rc;
    auto c = std::make_unique<mtr_anim_ctrl>();
    c->dev = d; c->nclips = (uint32_t)nclips; c->nnodes = (uint32_t)nnodes; c->ntrans = (uint32_t)ntrans; c->nany = (uint32_t)nany; c->nparams = (uint32_t)nparams;
    const Part p_clips{img.data(), img.size() * 4}, p_nodes{nodes, nnodes * sizeof(mtr_ctrl_node)}, p_trans{trans, ntrans * sizeof(mtr_ctrl_trans)};
    rc = ntrans ? set_upload(c.get(), "anim ctrl", {p_clips, p_nodes, p_trans}) : set_upload(c.get(), "anim ctrl", {p_clips, p_nodes});  // no empty copy
    if (rc) return rc;
    *out = c.release();
    return MTR_OK;
}

void mtr_anim_ctrl_destroy(mtr_anim_ctrl* c) { set_destroy(c); }

int32_t mtr_anim_ctrl_step_device(mtr_anim_ctrl* c, mtr_ctrl_state* states_dev, const mtr_play_state* play_dev, float* params_dev, size_t n, float dt,
                                  mtr_play_cmd* cmds_out_dev, uint32_t* counts_dev, void* hip_stream) {
    if (!c) return MTR_E_INVALID;
    int32_t rc = ctrl_check(c, states_dev, play_dev, params_dev, n, cmds_out_dev, counts_dev, true);
    if (rc) return rc;
    return ctrl_launch(c, states_dev, play_dev, params_dev, n, dt, cmds_out_dev, counts_dev, caller_stream(c->dev, hip_stream));
}

int32_t mtr_anim_ctrl_step_host(mtr_anim_ctrl* c, mtr_ctrl_state* states, const mtr_play_state* play, float* params, size_t n, float dt, mtr_play_cmd* cmds_out,
                                uint32_t* counts) {
    if (!c) return MTR_E_INVALID;
    mtr_device* d = c->dev;
    int32_t rc = ctrl_check(c, states, play, params, n, cmds_out, counts, false);
    if (rc) return rc;
    // one block: the states, the play states and the commands (16-byte words), then the parameter rows and the counts
    StagedBlock blk(d);
    StagedPart &p_states = blk.part(states, n * 4), &p_play = blk.part(play, n * 8), &p_cmds = blk.part(cmds_out, n * 4),
               &p_params = blk.part(params, n * c->nparams), &p_counts = blk.part(counts, counts ? c->ntrans : 0);
    return blk.run([&]() -> int32_t {
        int32_t r2;
        if ((r2 = blk.up({&p_states, &p_play, &p_params, &p_counts})) ||
            (r2 = ctrl_launch(c, p_states.at, p_play.at, p_params.dev<float>(), n, dt, p_cmds.at, p_counts.dev<uint32_t>(), d->s_copy)))
            return r2;
        return blk.down({&p_states, &p_cmds, &p_params, &p_counts});
    });
}

}  // extern "C"
