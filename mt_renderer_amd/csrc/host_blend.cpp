// host_blend.cpp -- blend spaces (SPEC.md section 23): the blend set, its validated samples and triangles, and the advance calls
// that run k_blend on blend states and parameter rows in device memory.
#include "host.h"
#include "blend_math.h"

// k_blend.hip.  Weak: the host-only builds of this file (tests/cpp, over the HIP stub runtime) link no kernels; libmtr.so
// links k_blend.o.
void mtr_launch_blend(const BlendParams& p, hipStream_t s) __attribute__((weak));

namespace mtr_host {

namespace {

constexpr size_t kBlendMaxInstances = (size_t)1 << 27, kBlendMaxSamples = 32, kBlendMaxTris = 64, kBlendMaxParams = 16;

// what every advance call checks before it touches anything; device: the pointers are device memory and must be aligned
int32_t blend_check(const mtr_anim_blend* bl, const void* states, const void* params, size_t n, const void* layers, size_t nlayers, const void* steps,
                    const void* shares, bool device) {
    mtr_device* d = bl->dev;
    if (!states || !params) return fail(d, MTR_E_INVALID, "blend advance: no states or no parameters");
    if (n == 0 || n > bl->max_instances) return fail(d, MTR_E_INVALID, "blend advance: 1 to max_instances instances");
    if (layers && (nlayers < 3 || nlayers > MTR_ANIM_MAX_LAYERS)) return fail(d, MTR_E_INVALID, "blend advance: 3 to 8 layers per instance");
    if (device) {
        if (((uintptr_t)states & 15u) || ((uintptr_t)layers & 15u) || ((uintptr_t)steps & 15u))
            return fail(d, MTR_E_INVALID, "blend advance: device states, layers and steps must be 16-byte aligned");
        if (((uintptr_t)params & 3u) || ((uintptr_t)shares & 3u)) return fail(d, MTR_E_INVALID, "blend advance: device parameters and shares must be 4-byte aligned");
    }
    if (!mtr_launch_blend) return fail(d, MTR_E_UNSUPPORTED, "blend advance: built without k_blend");
    return set_device(d);
}

// k_blend on `s` between the set's events: a call on another stream than the one before first waits for it, so the one event
// covers every reader of the tables and the destroy can park them behind it (DeviceSet::last)
int32_t blend_launch(mtr_anim_blend* bl, void* states_dev, const float* params_dev, size_t n, float dt, void* layers_dev, size_t nlayers, void* steps_dev,
                     float* shares_dev, hipStream_t s) {
    mtr_device* d = bl->dev;
    int32_t rc = set_before(bl, s);
    if (rc) return rc;
    BlendParams bp{};
    bp.clips = bl->d;
    bp.samples = bl->d + (size_t)bl->nclips * 4;
    bp.tris = bp.samples + (size_t)bl->nsamples * 4;
    bp.states = static_cast<uint32_t*>(states_dev);
    bp.params = params_dev;
    bp.out_layers = static_cast<uint32_t*>(layers_dev);
    bp.out_steps = static_cast<uint32_t*>(steps_dev);
    bp.out_shares = shares_dev;
    bp.nclips = bl->nclips; bp.nsamples = bl->nsamples; bp.ntris = bl->ntris; bp.nparams = bl->nparams; bp.param_x = bl->param_x; bp.param_y = bl->param_y;
    bp.nlayers = layers_dev ? (uint32_t)nlayers : 0u; bp.n = (uint32_t)n; bp.damp = bl->damp; bp.dt = dt;
    mtr_launch_blend(bp, s);
    HIPCHK(d, hipGetLastError());
    return set_after(bl, s);
}

}  // namespace

}  // namespace mtr_host

using namespace mtr_host;

extern "C" {

static_assert(sizeof(mtr_blend_sample) == 16 && sizeof(mtr_blend_tri) == 16 && sizeof(mtr_blend_state) == 16 && sizeof(mtr_anim_layer) == 16 &&
                  sizeof(mtr_root_step) == 16,
              "mtr_blend_sample, mtr_blend_tri, mtr_blend_state, mtr_anim_layer, mtr_root_step");

int32_t mtr_anim_blend_create(mtr_device* d, size_t nclips, const uint32_t* nkeys, const uint32_t* clip_flags, const float* rates, const mtr_blend_sample* samples,
                              size_t nsamples, const mtr_blend_tri* tris, size_t ntris, size_t nparams, uint32_t param_x, uint32_t param_y, float damp,
                              size_t max_instances, mtr_anim_blend** out) {
    if (!d || !out) return MTR_E_INVALID;
    *out = nullptr;
    if (nclips == 0 || nclips > kClipMaxKeys) return fail(d, MTR_E_INVALID, "anim blend: 1 to 2^24 clips");
    if (!nkeys || !rates) return fail(d, MTR_E_INVALID, "anim blend: no key counts or no rates");
    if (!samples || nsamples == 0 || nsamples > kBlendMaxSamples) return fail(d, MTR_E_INVALID, "anim blend: 1 to 32 samples");
    if (ntris > kBlendMaxTris || (ntris > 0 && !tris)) return fail(d, MTR_E_INVALID, "anim blend: 0 to 64 triangles");
    if (nparams == 0 || nparams > kBlendMaxParams) return fail(d, MTR_E_INVALID, "anim blend: 1 to 16 parameters");
    if (param_x >= nparams || (ntris > 0 && param_y >= nparams)) return fail(d, MTR_E_INVALID, "anim blend: param_x or param_y names a parameter the rows do not have");
    if (!(damp > 0.0f)) return fail(d, MTR_E_INVALID, "anim blend: damp must be above 0 (+inf: no smoothing)");
    if (max_instances == 0 || max_instances > kBlendMaxInstances) return fail(d, MTR_E_INVALID, "anim blend: 1 to 2^27 instances");
    std::vector<uint32_t> img((nclips + nsamples + ntris) * 4);
    int32_t rc;
    for (size_t c = 0; c < nclips; c++)
        if ((rc = clip_entry(d, "anim blend", c, nkeys, clip_flags ? clip_flags[c] : 0u, rates, &img[c * 4]))) return rc;
    for (size_t k = 0; k < nsamples; k++) {
        const mtr_blend_sample& sm = samples[k];
        const std::string who = "anim blend: sample " + std::to_string(k) + " ";
        if (sm.clip >= nclips) return fail(d, MTR_E_INVALID, who + "names a clip the set does not have");
        if (!((clip_flags ? clip_flags[sm.clip] : 0u) & MTR_CLIP_LOOP)) return fail(d, MTR_E_INVALID, who + "names a clip that is not LOOP");
        if (!std::isfinite(sm.px) || (ntris > 0 && !std::isfinite(sm.py))) return fail(d, MTR_E_INVALID, who + "has a position that is not finite");
        if (ntris == 0 && k > 0) {
            const float step = sm.px - samples[k - 1].px;  // binary32, the denominator of the rule
            if (!(step > 0.0f) || !std::isfinite(step)) return fail(d, MTR_E_INVALID, who + "does not lie above the sample before it by a finite step");
        }
        img[(nclips + k) * 4] = sm.clip;
        std::memcpy(&img[(nclips + k) * 4 + 1], &sm.px, 4);
        std::memcpy(&img[(nclips + k) * 4 + 2], &sm.py, 4);
        img[(nclips + k) * 4 + 3] = 0u;
    }
    for (size_t k = 0; k < ntris; k++) {
        const uint32_t* v = tris[k].v;
        const std::string who = "anim blend: triangle " + std::to_string(k) + " ";
        if (v[0] >= nsamples || v[1] >= nsamples || v[2] >= nsamples) return fail(d, MTR_E_INVALID, who + "names a sample the set does not have");
        if (v[0] == v[1] || v[1] == v[2] || v[2] == v[0]) return fail(d, MTR_E_INVALID, who + "names a sample twice");
        const float A = mtr::blend_area(samples[v[0]].px, samples[v[0]].py, samples[v[1]].px, samples[v[1]].py, samples[v[2]].px, samples[v[2]].py);
        if (!(A > 0.0f) || !std::isfinite(A)) return fail(d, MTR_E_INVALID, who + "is not counter-clockwise with a finite area");
        for (int j = 0; j < 3; j++) img[(nclips + nsamples + k) * 4 + j] = v[j];
        img[(nclips + nsamples + k) * 4 + 3] = 0u;
    }
    if ((rc = set_device(d))) return rc;
    auto bl = std::make_unique<mtr_anim_blend>();
    bl->dev = d; bl->nclips = (uint32_t)nclips; bl->nsamples = (uint32_t)nsamples; bl->ntris = (uint32_t)ntris; bl->nparams = (uint32_t)nparams;
    bl->param_x = param_x; bl->param_y = ntris ? param_y : 0u; bl->damp = damp; bl->max_instances = (uint32_t)max_instances;
    if ((rc = set_upload(bl.get(), "anim blend", {{img.data(), img.size() * 4}}))) return rc;
    *out = bl.release();
    return MTR_OK;
}

void mtr_anim_blend_destroy(mtr_anim_blend* bl) { set_destroy(bl); }

int32_t mtr_anim_blend_advance_device(mtr_anim_blend* bl, mtr_blend_state* states_dev, const float* params_dev, size_t n, float dt, mtr_anim_layer* out_layers_dev,
                                      size_t nlayers, mtr_root_step* out_steps_dev, float* out_shares_dev, void* hip_stream) {
    if (!bl) return MTR_E_INVALID;
    int32_t rc = blend_check(bl, states_dev, params_dev, n, out_layers_dev, nlayers, out_steps_dev, out_shares_dev, true);
    if (rc) return rc;
    return blend_launch(bl, states_dev, params_dev, n, dt, out_layers_dev, nlayers, out_steps_dev, out_shares_dev, caller_stream(bl->dev, hip_stream));
}

int32_t mtr_anim_blend_advance_host(mtr_anim_blend* bl, mtr_blend_state* states, const float* params, size_t n, float dt, mtr_anim_layer* out_layers,
                                    size_t nlayers, mtr_root_step* out_steps, float* out_shares) {
    if (!bl) return MTR_E_INVALID;
    mtr_device* d = bl->dev;
    int32_t rc = blend_check(bl, states, params, n, out_layers, nlayers, out_steps, out_shares, false);
    if (rc) return rc;
    // one block: the states, the layers and the steps (16-byte words), then the parameter rows and the shares
    StagedBlock blk(d);
    StagedPart &p_states = blk.part(states, n * 4), &p_layers = blk.part(out_layers, out_layers ? n * nlayers * 4 : 0),
               &p_steps = blk.part(out_steps, out_steps ? n * 12 : 0), &p_params = blk.part(params, n * bl->nparams),
               &p_shares = blk.part(out_shares, out_shares ? n * 3 : 0);
    return blk.run([&]() -> int32_t {
        int32_t r2;
        if ((r2 = blk.up({&p_states, &p_params, &p_layers})) ||  // layers 3.. come back as they went in
            (r2 = blend_launch(bl, p_states.at, p_params.dev<float>(), n, dt, p_layers.dev<void>(), nlayers, p_steps.dev<void>(), p_shares.dev<float>(), d->s_copy)))
            return r2;
        return blk.down({&p_states, &p_layers, &p_steps, &p_shares});
    });
}

}  // extern "C"
