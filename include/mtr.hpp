// mtr.hpp -- C++ host mirror of the reference's GPU-object layer over the C ABI (mtr.h).
// Same names and argument roles as mt-renderer's Rust API: Texture::new (src/texture.rs:11),
// Model::new / set_parts_disp / render (src/model.rs:36-45, :295, :299-305); wgpu::Device+Queue -> mtr::Device,
// wgpu::RenderPass -> mtr::Frame.  Errors (the reference's anyhow::Result / panics) become mtr::Error.
#pragma once
#include "mtr.h"

#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace mtr {

struct Error : std::runtime_error {
    int32_t code;
    Error(int32_t c, const std::string& m) : std::runtime_error("mtr error " + std::to_string(c) + ": " + m), code(c) {}
};

class Device {
  public:
    explicit Device(int hip_device = 0) {
        int32_t rc = mtr_device_create(hip_device, &h_);
        if (rc) throw Error(rc, mtr_last_error(nullptr));
    }
    // rank r of a Group: the group owns the device
    struct Borrowed {};
    Device(mtr_device* of_group, Borrowed) : h_(of_group), owned_(false) {}
    Device(const Device&) = delete;
    Device& operator=(const Device&) = delete;
    ~Device() {
        if (owned_) mtr_device_destroy(h_);
    }
    mtr_device* handle() const { return h_; }
    void set_tile_mode(int32_t mode) const { check(mtr_device_set_tile_mode(h_, mode)); }  // MTR_TILE_AUTO / ORDERED / VISIBILITY
    void set_binning(bool single_pass, uint32_t queue_capacity = 0) const { check(mtr_device_set_binning(h_, single_pass ? 1 : 0, queue_capacity)); }
    void unpack_color_shards(const void* gathered_dev, uint32_t world, uint32_t w, uint32_t h, void* dst_dev) const {
        check(mtr_device_unpack_color_shards(h_, gathered_dev, world, w, h, dst_dev));
    }
    // the exchange of sharded frames on a second host thread (mtr.h): fn = &ncclAllGather for an RCCL host
    void exchange_start(mtr_allgather_fn fn, void* comm, int dtype_u8, void* send_dev, size_t send_bytes, void* gathered_dev,
                        void* dst_dev, uint32_t world, void* hip_stream) const {
        check(mtr_device_exchange_start(h_, fn, comm, dtype_u8, send_dev, send_bytes, gathered_dev, dst_dev, world, hip_stream));
    }
    void exchange_add_lane(void* comm, void* send_dev, void* gathered_dev, void* dst_dev, void* hip_stream) const {
        check(mtr_device_exchange_add_lane(h_, comm, send_dev, gathered_dev, dst_dev, hip_stream));
    }
    // waits for every frame in flight; reports (once) an overflow latched by a frame nobody waited for
    void synchronize() const { check(mtr_device_synchronize(h_)); }
    void set_culling(int32_t mode) const { check(mtr_device_set_culling(h_, mode)); }  // MTR_GEOM_CULL_OFF / _SHARDED (default) / _ALL_FRAMES
    void set_texture_residency(uint32_t mode) const { check(mtr_device_set_texture_residency(h_, mode)); }  // MTR_TEXRES_*
    void exchange_drain() const { check(mtr_device_exchange_drain(h_)); }
    void exchange_stop() const { check(mtr_device_exchange_stop(h_)); }
    void check(int32_t rc) const {
        if (rc) throw Error(rc, mtr_last_error(h_));
    }

  private:
    mtr_device* h_ = nullptr;
    bool owned_ = true;
};

class Texture {
  public:
    // Texture::new(device, queue, resource) -- src/texture.rs:11
    Texture(const Device& dev, uint32_t width, uint32_t height, uint32_t format, const void* data, size_t len) {
        dev.check(mtr_texture_create(dev.handle(), width, height, format, data, len, &h_));
    }
    // the same with the file's mip chain (level 0 first); the reference uploads level 0 only (src/texture.rs:21)
    Texture(const Device& dev, uint32_t width, uint32_t height, uint32_t format, uint32_t levels, const void* data, size_t len) {
        dev.check(mtr_texture_create_mips(dev.handle(), width, height, format, levels, data, len, &h_));
    }
    Texture(Texture&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Texture(const Texture&) = delete;
    ~Texture() { mtr_texture_destroy(h_); }
    mtr_texture* handle() const { return h_; }

  private:
    mtr_texture* h_ = nullptr;
};

class Frame;

// An animation set (include/mtr.h, SPEC.md section 14): clips of uniformly spaced keys, resident in HBM.  keys: clip after
// clip, sum(nkeys) * njoints entries; flags: MTR_CLIP_* per clip (empty = 0 for all).
class Anim {
  public:
    Anim(const Device& dev, size_t njoints, const std::vector<uint32_t>& nkeys, const std::vector<uint32_t>& flags, const mtr_anim_key* keys)
        : dev_(dev), njoints_(njoints) {
        if (!flags.empty() && flags.size() != nkeys.size()) throw Error(MTR_E_INVALID, "one flag word per clip");
        dev.check(mtr_anim_create(dev.handle(), njoints, nkeys.size(), nkeys.data(), flags.empty() ? nullptr : flags.data(), keys, &h_));
    }
    // a track set (SPEC.md section 15): tracks holds nticks.size() * njoints * 3 descriptors, times / values nkeys_total keys
    Anim(const Device& dev, size_t njoints, const std::vector<uint32_t>& nticks, const std::vector<uint32_t>& flags, const mtr_anim_track* tracks,
         const uint16_t* times, const uint16_t* values, size_t nkeys_total)
        : dev_(dev), njoints_(njoints) {
        if (!flags.empty() && flags.size() != nticks.size()) throw Error(MTR_E_INVALID, "one flag word per clip");
        dev.check(mtr_anim_create_tracks(dev.handle(), njoints, nticks.size(), nticks.data(), flags.empty() ? nullptr : flags.data(), tracks, times,
                                         values, nkeys_total, &h_));
    }
    Anim(Anim&& o) noexcept : dev_(o.dev_), njoints_(o.njoints_), h_(std::exchange(o.h_, nullptr)) {}
    Anim(const Anim&) = delete;
    ~Anim() { mtr_anim_destroy(h_); }
    size_t njoints() const { return njoints_; }
    // test / debug hook: the local matrices of n states, n * njoints * 16 floats
    std::vector<float> sample(const mtr_anim_state* states, size_t n) const {
        std::vector<float> out(n * njoints_ * 16);
        dev_.check(mtr_anim_sample(h_, states, n, out.data(), out.size()));
        return out;
    }
    // the local matrices of n layer stacks of nlayers layers each (SPEC.md section 16); masks may be nullptr
    std::vector<float> sample_layers(mtr_anim_masks* masks, const mtr_anim_layer* layers, size_t nlayers, size_t n) const {
        std::vector<float> out(n * njoints_ * 16);
        dev_.check(mtr_anim_sample_layers(h_, masks, layers, nlayers, n, out.data(), out.size()));
        return out;
    }
    // one step of the springs of a spring set after the chains of ik (or nullptr, then targets is nullptr too), everything
    // in host memory (SPEC.md section 24): states (n * nsprings) are read and written back, motion is n * 16 floats or nullptr
    std::vector<float> sample_spring(mtr_anim_masks* masks, mtr_anim_ik* ik, mtr_anim_spring* spring, const mtr_anim_layer* layers, size_t nlayers,
                                     const mtr_ik_target* targets, mtr_spring_state* states, const float* motion, float dt, size_t n) const {
        std::vector<float> out(n * njoints_ * 16);
        dev_.check(mtr_anim_sample_spring(h_, masks, ik, spring, layers, nlayers, targets, states, motion, dt, n, out.data(), out.size()));
        return out;
    }
    // the same after the chains of an IK set, against n * nchains targets (SPEC.md section 17)
    std::vector<float> sample_ik(mtr_anim_masks* masks, mtr_anim_ik* ik, const mtr_anim_layer* layers, size_t nlayers, const mtr_ik_target* targets,
                                 size_t n) const {
        std::vector<float> out(n * njoints_ * 16);
        dev_.check(mtr_anim_sample_ik(h_, masks, ik, layers, nlayers, targets, n, out.data(), out.size()));
        return out;
    }
    mtr_anim* handle() const { return h_; }

  private:
    const Device& dev_;
    size_t njoints_;
    mtr_anim* h_ = nullptr;
};

// A mask set for animation layers (include/mtr.h, SPEC.md section 16): nmasks masks of njoints weights in [0, 1]
class AnimMasks {
  public:
    AnimMasks(const Device& dev, size_t njoints, size_t nmasks, const float* weights) : dev_(dev) {
        dev.check(mtr_anim_masks_create(dev.handle(), njoints, nmasks, weights, &h_));
    }
    AnimMasks(AnimMasks&& o) noexcept : dev_(o.dev_), h_(std::exchange(o.h_, nullptr)) {}
    AnimMasks(const AnimMasks&) = delete;
    ~AnimMasks() { mtr_anim_masks_destroy(h_); }
    mtr_anim_masks* handle() const { return h_; }

  private:
    const Device& dev_;
    mtr_anim_masks* h_ = nullptr;
};

// An IK set (include/mtr.h, SPEC.md section 17): the parents of a skeleton and 1..MTR_ANIM_MAX_IK chains over it
class AnimIK {
  public:
    AnimIK(const Device& dev, size_t njoints, const uint8_t* parents, size_t nchains, const mtr_ik_chain* chains) : dev_(dev), nchains_(nchains) {
        dev.check(mtr_anim_ik_create(dev.handle(), njoints, parents, nchains, chains, &h_));
    }
    AnimIK(AnimIK&& o) noexcept : dev_(o.dev_), nchains_(o.nchains_), h_(std::exchange(o.h_, nullptr)) {}
    AnimIK(const AnimIK&) = delete;
    ~AnimIK() { mtr_anim_ik_destroy(h_); }
    size_t nchains() const { return nchains_; }
    mtr_anim_ik* handle() const { return h_; }

  private:
    const Device& dev_;
    size_t nchains_;
    mtr_anim_ik* h_ = nullptr;
};

// A root set (include/mtr.h, SPEC.md section 19): the trajectory joint and one flag word per clip (MTR_ROOT_CYCLIC) for
// trajectory sets of njoints joints and nclips clips
class AnimRoot {
  public:
    AnimRoot(const Device& dev, size_t njoints, size_t nclips, uint32_t joint = 0, const uint32_t* flags = nullptr) : dev_(dev) {
        dev.check(mtr_anim_root_create(dev.handle(), njoints, nclips, joint, flags, &h_));
    }
    AnimRoot(AnimRoot&& o) noexcept : dev_(o.dev_), h_(std::exchange(o.h_, nullptr)) {}
    AnimRoot(const AnimRoot&) = delete;
    ~AnimRoot() { mtr_anim_root_destroy(h_); }
    // the delta matrices alone, n x 16 floats, of n * nsteps steps on traj: to host memory (waits), or in stream order
    std::vector<float> deltas(const Anim& traj, const mtr_root_step* steps, size_t nsteps, size_t n) const {
        std::vector<float> out(n * 16);
        dev_.check(mtr_anim_root_deltas(traj.handle(), h_, steps, nsteps, n, out.data(), out.size()));
        return out;
    }
    void deltas_device(const Anim& traj, const mtr_root_step* steps_dev, size_t nsteps, size_t n, float* out_dev, void* hip_stream = nullptr) const {
        dev_.check(mtr_anim_root_deltas_device(traj.handle(), h_, steps_dev, nsteps, n, out_dev, hip_stream));
    }
    mtr_anim_root* handle() const { return h_; }

  private:
    const Device& dev_;
    mtr_anim_root* h_ = nullptr;
};

// A player set (include/mtr.h, SPEC.md section 20), the library's clock: per clip the key count, the flag word and the rate in
// positions per second, for up to max_instances play states that live in device memory of the caller's
class AnimPlayer {
  public:
    AnimPlayer(const Device& dev, size_t nclips, const uint32_t* nkeys, const uint32_t* flags, const float* rates, size_t max_instances) : dev_(dev) {
        dev.check(mtr_anim_player_create(dev.handle(), nclips, nkeys, flags, rates, max_instances, &h_));
    }
    AnimPlayer(AnimPlayer&& o) noexcept : dev_(o.dev_), h_(std::exchange(o.h_, nullptr)) {}
    AnimPlayer(const AnimPlayer&) = delete;
    ~AnimPlayer() { mtr_anim_player_destroy(h_); }
    // n states advanced by dt in place in stream order, at most one of ncmds host commands applied to each (copied before the
    // call returns); the records of the frame go where a pointer is given
    void advance(mtr_play_state* states_dev, size_t n, float dt, const mtr_play_cmd* cmds = nullptr, size_t ncmds = 0, mtr_anim_state* out_states_dev = nullptr,
                 mtr_anim_layer* out_layers_dev = nullptr, size_t nlayers = 0, mtr_root_step* out_steps_dev = nullptr, void* hip_stream = nullptr) const {
        dev_.check(mtr_anim_player_advance_device(h_, states_dev, n, dt, cmds, ncmds, out_states_dev, out_layers_dev, nlayers, out_steps_dev, hip_stream));
    }
    // the same with the commands in device memory
    void advance_cmds(mtr_play_state* states_dev, size_t n, float dt, const mtr_play_cmd* cmds_dev, size_t ncmds, mtr_anim_state* out_states_dev = nullptr,
                      mtr_anim_layer* out_layers_dev = nullptr, size_t nlayers = 0, mtr_root_step* out_steps_dev = nullptr, void* hip_stream = nullptr) const {
        dev_.check(mtr_anim_player_advance_device_cmds(h_, states_dev, n, dt, cmds_dev, ncmds, out_states_dev, out_layers_dev, nlayers, out_steps_dev, hip_stream));
    }
    // the test and debug hook: everything in host memory, waits
    void advance_host(mtr_play_state* states, size_t n, float dt, const mtr_play_cmd* cmds = nullptr, size_t ncmds = 0, mtr_anim_state* out_states = nullptr,
                      mtr_anim_layer* out_layers = nullptr, size_t nlayers = 0, mtr_root_step* out_steps = nullptr) const {
        dev_.check(mtr_anim_player_advance_host(h_, states, n, dt, cmds, ncmds, out_states, out_layers, nlayers, out_steps));
    }
    mtr_anim_player* handle() const { return h_; }

  private:
    const Device& dev_;
    mtr_anim_player* h_ = nullptr;
};

// A match set (include/mtr.h, SPEC.md section 25): nearest-pose search per instance over a database of feature rows, writing a
// player's commands on the device; nkeys and clip_flags are what the player was created with
class AnimMatch {
  public:
    AnimMatch(const Device& dev, size_t nclips, const uint32_t* nkeys, const uint32_t* clip_flags, size_t D, uint64_t pose_dims, uint32_t flags, float seconds,
              float near_x, float margin, const mtr_match_row* rows, size_t nrows, const float* features, const float* mean, const float* scale,
              size_t max_instances) : dev_(dev) {
        dev.check(mtr_anim_match_create(dev.handle(), nclips, nkeys, clip_flags, D, pose_dims, flags, seconds, near_x, margin, rows, nrows, features, mean, scale,
                                        max_instances, &h_));
    }
    AnimMatch(AnimMatch&& o) noexcept : dev_(o.dev_), h_(std::exchange(o.h_, nullptr)) {}
    AnimMatch(const AnimMatch&) = delete;
    ~AnimMatch() { mtr_anim_match_destroy(h_); }
    // one search for n instances in stream order; command slot i of cmds_out_dev is instance instance_base + i's, for the
    // player's advance_cmds(states, n, dt, cmds_out_dev, n, ...)
    void search(const mtr_play_state* play_dev, const float* query_dev, const mtr_match_filter* filter_dev, size_t n, uint32_t instance_base,
                mtr_play_cmd* cmds_out_dev, mtr_match_result* results_dev = nullptr, void* hip_stream = nullptr) const {
        dev_.check(mtr_anim_match_search_device(h_, play_dev, query_dev, filter_dev, n, instance_base, cmds_out_dev, results_dev, hip_stream));
    }
    // the test and debug hooks: everything in host memory, waits
    void search_host(const mtr_play_state* play, const float* query, const mtr_match_filter* filter, size_t n, uint32_t instance_base, mtr_play_cmd* cmds_out,
                     mtr_match_result* results = nullptr) const {
        dev_.check(mtr_anim_match_search_host(h_, play, query, filter, n, instance_base, cmds_out, results));
    }
    void scores_host(const mtr_play_state* play, const float* query, size_t n, float* out) const {
        dev_.check(mtr_anim_match_scores_host(h_, play, query, n, out));
    }
    mtr_anim_match* handle() const { return h_; }

  private:
    const Device& dev_;
    mtr_anim_match* h_ = nullptr;
};

// A controller (include/mtr.h, SPEC.md section 21): per-instance state machines over one graph of nodes and transitions that
// write a player's commands on the device; nkeys and clip_flags are what the player was created with
class AnimCtrl {
  public:
    AnimCtrl(const Device& dev, size_t nclips, const uint32_t* nkeys, const uint32_t* clip_flags, const mtr_ctrl_node* nodes, size_t nnodes,
             const mtr_ctrl_trans* trans, size_t ntrans, size_t nany, size_t nparams) : dev_(dev) {
        dev.check(mtr_anim_ctrl_create(dev.handle(), nclips, nkeys, clip_flags, nodes, nnodes, trans, ntrans, nany, nparams, &h_));
    }
    AnimCtrl(AnimCtrl&& o) noexcept : dev_(o.dev_), h_(std::exchange(o.h_, nullptr)) {}
    AnimCtrl(const AnimCtrl&) = delete;
    ~AnimCtrl() { mtr_anim_ctrl_destroy(h_); }
    // n states stepped in place in stream order against their play states and parameter rows; command slot i of cmds_out_dev is
    // instance i's, for the player's advance_cmds(states, n, dt, cmds_out_dev, n, ...)
    void step(mtr_ctrl_state* states_dev, const mtr_play_state* play_dev, float* params_dev, size_t n, float dt, mtr_play_cmd* cmds_out_dev,
              uint32_t* counts_dev = nullptr, void* hip_stream = nullptr) const {
        dev_.check(mtr_anim_ctrl_step_device(h_, states_dev, play_dev, params_dev, n, dt, cmds_out_dev, counts_dev, hip_stream));
    }
    // the test and debug hook: everything in host memory, waits
    void step_host(mtr_ctrl_state* states, const mtr_play_state* play, float* params, size_t n, float dt, mtr_play_cmd* cmds_out, uint32_t* counts = nullptr) const {
        dev_.check(mtr_anim_ctrl_step_host(h_, states, play, params, n, dt, cmds_out, counts));
    }
    mtr_anim_ctrl* handle() const { return h_; }

  private:
    const Device& dev_;
    mtr_anim_ctrl* h_ = nullptr;
};

// An event set (include/mtr.h, SPEC.md section 22): sorted markers per clip that fire into a list on the device; nkeys and
// clip_flags are what the player was created with, counts[c] markers per clip lie behind each other in markers
class AnimEvents {
  public:
    AnimEvents(const Device& dev, size_t nclips, const uint32_t* nkeys, const uint32_t* clip_flags, const uint32_t* counts, const mtr_event_marker* markers,
               size_t max_instances) : dev_(dev) {
        dev.check(mtr_anim_events_create(dev.handle(), nclips, nkeys, clip_flags, counts, markers, max_instances, &h_));
    }
    AnimEvents(AnimEvents&& o) noexcept : dev_(o.dev_), h_(std::exchange(o.h_, nullptr)) {}
    AnimEvents(const AnimEvents&) = delete;
    ~AnimEvents() { mtr_anim_events_destroy(h_); }
    // the markers that the nsteps steps of each of n instances passed, in stream order: up to capacity records into out_dev,
    // count_dev[0] = fired, count_dev[1] = written, bits_dev[i] = the mask of instance i (optional)
    void collect(const mtr_root_step* steps_dev, size_t nsteps, size_t n, float min_weight, mtr_anim_event* out_dev, size_t capacity, uint32_t* count_dev,
                 uint32_t* bits_dev = nullptr, void* hip_stream = nullptr) const {
        dev_.check(mtr_anim_events_collect_device(h_, steps_dev, nsteps, n, min_weight, out_dev, capacity, count_dev, bits_dev, hip_stream));
    }
    // the test and debug hook: everything in host memory, waits
    void collect_host(const mtr_root_step* steps, size_t nsteps, size_t n, float min_weight, mtr_anim_event* out, size_t capacity, uint32_t* count,
                      uint32_t* bits = nullptr) const {
        dev_.check(mtr_anim_events_collect_host(h_, steps, nsteps, n, min_weight, out, capacity, count, bits));
    }
    mtr_anim_events* handle() const { return h_; }

  private:
    const Device& dev_;
    mtr_anim_events* h_ = nullptr;
};

// A blend set (include/mtr.h, SPEC.md section 23): samples in a 1-D (ntris == 0) or 2-D parameter space, each with a LOOP
// clip; nkeys, clip_flags and rates are what a player is created with
class AnimBlend {
  public:
    AnimBlend(const Device& dev, size_t nclips, const uint32_t* nkeys, const uint32_t* clip_flags, const float* rates, const mtr_blend_sample* samples,
              size_t nsamples, const mtr_blend_tri* tris, size_t ntris, size_t nparams, uint32_t param_x, uint32_t param_y, float damp, size_t max_instances)
        : dev_(dev) {
        dev.check(mtr_anim_blend_create(dev.handle(), nclips, nkeys, clip_flags, rates, samples, nsamples, tris, ntris, nparams, param_x, param_y, damp,
                                        max_instances, &h_));
    }
    AnimBlend(AnimBlend&& o) noexcept : dev_(o.dev_), h_(std::exchange(o.h_, nullptr)) {}
    AnimBlend(const AnimBlend&) = delete;
    ~AnimBlend() { mtr_anim_blend_destroy(h_); }
    // n blend states advanced by dt against their parameter rows, in stream order: layers 0..2 of nlayers per instance, three
    // steps and three shares per instance, each optional
    void advance(mtr_blend_state* states_dev, const float* params_dev, size_t n, float dt, mtr_anim_layer* out_layers_dev, size_t nlayers,
                 mtr_root_step* out_steps_dev, float* out_shares_dev = nullptr, void* hip_stream = nullptr) const {
        dev_.check(mtr_anim_blend_advance_device(h_, states_dev, params_dev, n, dt, out_layers_dev, nlayers, out_steps_dev, out_shares_dev, hip_stream));
    }
    // the test and debug hook: everything in host memory, waits
    void advance_host(mtr_blend_state* states, const float* params, size_t n, float dt, mtr_anim_layer* out_layers, size_t nlayers, mtr_root_step* out_steps,
                      float* out_shares = nullptr) const {
        dev_.check(mtr_anim_blend_advance_host(h_, states, params, n, dt, out_layers, nlayers, out_steps, out_shares));
    }
    mtr_anim_blend* handle() const { return h_; }

  private:
    const Device& dev_;
    mtr_anim_blend* h_ = nullptr;
};

// A spring set (include/mtr.h, SPEC.md section 24): the parents of a skeleton and 1..MTR_ANIM_MAX_SPRINGS springs over it
class AnimSpring {
  public:
    AnimSpring(const Device& dev, size_t njoints, const uint8_t* parents, size_t nsprings, const mtr_spring* springs) : dev_(dev), nsprings_(nsprings) {
        dev.check(mtr_anim_spring_create(dev.handle(), njoints, parents, nsprings, springs, &h_));
    }
    AnimSpring(AnimSpring&& o) noexcept : dev_(o.dev_), nsprings_(o.nsprings_), h_(std::exchange(o.h_, nullptr)) {}
    AnimSpring(const AnimSpring&) = delete;
    ~AnimSpring() { mtr_anim_spring_destroy(h_); }
    size_t nsprings() const { return nsprings_; }
    mtr_anim_spring* handle() const { return h_; }

  private:
    const Device& dev_;
    size_t nsprings_;
    mtr_anim_spring* h_ = nullptr;
};

class Model {
  public:
    // Model::new(model_file, material_file, shader2, resource_manager, device, queue, ..) -- src/model.rs:36-45
    Model(const Device& dev, const void* vertex_buf, size_t vertex_len, const uint16_t* index_buf, size_t index_num,
          const std::vector<mtr_primitive>& prims, const std::vector<mtr_layout>& layouts,
          const std::vector<int32_t>& prim_to_texture, const std::vector<const Texture*>& textures,
          const std::vector<uint32_t>& prim_debug_id)
        : dev_(dev) {
        if (layouts.size() != prims.size() || prim_to_texture.size() != prims.size() || prim_debug_id.size() != prims.size())
            throw Error(MTR_E_INVALID, "per-primitive arrays must have one entry per primitive");
        std::vector<mtr_texture*> th;
        for (const Texture* t : textures) th.push_back(t->handle());
        dev.check(mtr_model_create(dev.handle(), vertex_buf, vertex_len, index_buf, index_num, prims.data(), prims.size(),
                                   layouts.data(), prim_to_texture.data(), th.data(), th.size(), prim_debug_id.data(), &h_));
    }
    Model(const Model&) = delete;
    ~Model() { mtr_model_destroy(h_); }
    // Model::set_parts_disp(&mut self, parts_disp: &[bool]) -- src/model.rs:295
    void set_parts_disp(const std::vector<uint8_t>& parts_disp) {
        dev_.check(mtr_model_set_parts_disp(h_, parts_disp.data(), parts_disp.size()));
    }
    void set_palette(const float* mats, size_t n) { dev_.check(mtr_model_set_palette(h_, mats, n)); }
    // skeletal poses (SPEC.md section 12): parents == nullptr clears the skeleton; set_pose forms the palette on the GPU
    void set_skeleton(const uint8_t* parents, const float* imats, size_t njoints) { dev_.check(mtr_model_set_skeleton(h_, parents, imats, njoints)); }
    void set_pose(const float* local_mats, size_t njoints) { dev_.check(mtr_model_set_pose(h_, local_mats, njoints)); }
    // the palette from one animation state through the skeleton (SPEC.md section 14)
    void animate(const Anim& anim, const mtr_anim_state& state) { dev_.check(mtr_model_animate(h_, anim.handle(), &state)); }
    // the palette from one layer stack (SPEC.md section 16); masks may be nullptr
    void animate_layers(const Anim& anim, const AnimMasks* masks, const mtr_anim_layer* layers, size_t nlayers) {
        dev_.check(mtr_model_animate_layers(h_, anim.handle(), masks ? masks->handle() : nullptr, layers, nlayers));
    }
    // the palette from one layer stack and one target per chain of ik (SPEC.md section 17); masks may be nullptr
    void animate_ik(const Anim& anim, const AnimMasks* masks, const mtr_anim_layer* layers, size_t nlayers, const AnimIK& ik, const mtr_ik_target* targets) {
        dev_.check(mtr_model_animate_ik(h_, anim.handle(), masks ? masks->handle() : nullptr, layers, nlayers, ik.handle(), targets));
    }
    // the state objects a material names (src/rmaterial.rs:211-230), applied per primitive; default = src/model.rs:240-262
    void set_prim_states(const std::vector<mtr_prim_state>& states) { dev_.check(mtr_model_set_prim_states(h_, states.data(), states.size())); }
    // joint positions for the per-joint debug cubes of Model::render (src/model.rs:309-315)
    void set_joint_positions(const float* xyz, size_t njoints) { dev_.check(mtr_model_set_joint_positions(h_, xyz, njoints)); }
    void render_with_joints(Frame& frame, const float view_proj[16]) const;
    // Model::render(&self, rpass, queue, transform_bind_group, debug_overlay) -- src/model.rs:299-305
    void render(Frame& frame, const float view_proj[16]) const;
    mtr_model* handle() const { return h_; }

  private:
    const Device& dev_;
    mtr_model* h_ = nullptr;
};

// n instances of one model resident in HBM, updatable in place (frames use what was current when they were recorded)
class Batch {
  public:
    Batch(const Device& dev, const Model& model, size_t n, const float* model_mats, const float* palettes = nullptr, size_t npal = 0,
          const int32_t* texture_override = nullptr)
        : dev_(dev), n_(n), npal_(palettes ? npal : 0) {
        dev.check(mtr_batch_create(dev.handle(), model.handle(), n, model_mats, palettes, npal, texture_override, &h_));
    }
    Batch(const Batch&) = delete;
    ~Batch() { mtr_batch_destroy(h_); }
    // nullptr keeps that part
    void update(const float* model_mats, const float* palettes = nullptr, size_t npal = 0) {
        dev_.check(mtr_batch_update(h_, model_mats, palettes, npal));
        if (palettes) npal_ = npal;
    }
    void set_poses(const float* local_mats, size_t njoints) { dev_.check(mtr_batch_set_poses(h_, local_mats, njoints)); npal_ = njoints; }
    void set_poses_device(const float* local_mats_dev, size_t njoints, void* hip_stream = nullptr) {
        dev_.check(mtr_batch_set_poses_device(h_, local_mats_dev, njoints, hip_stream));
        npal_ = njoints;
    }
    // one animation state per instance (SPEC.md section 14): host memory, or device memory read in stream order
    void animate(const Anim& anim, const mtr_anim_state* states) { dev_.check(mtr_batch_animate(h_, anim.handle(), states)); npal_ = anim.njoints(); }
    void animate_device(const Anim& anim, const mtr_anim_state* states_dev, void* hip_stream = nullptr) {
        dev_.check(mtr_batch_animate_device(h_, anim.handle(), states_dev, hip_stream));
        npal_ = anim.njoints();
    }
    // nlayers layers per instance (SPEC.md section 16): host memory, or device memory read in stream order; masks may be nullptr
    void animate_layers(const Anim& anim, const AnimMasks* masks, const mtr_anim_layer* layers, size_t nlayers) {
        dev_.check(mtr_batch_animate_layers(h_, anim.handle(), masks ? masks->handle() : nullptr, layers, nlayers));
        npal_ = anim.njoints();
    }
    void animate_layers_device(const Anim& anim, const AnimMasks* masks, const mtr_anim_layer* layers_dev, size_t nlayers, void* hip_stream = nullptr) {
        dev_.check(mtr_batch_animate_layers_device(h_, anim.handle(), masks ? masks->handle() : nullptr, layers_dev, nlayers, hip_stream));
        npal_ = anim.njoints();
    }
    // nlayers layers and ik.nchains() targets per instance (SPEC.md section 17): host memory, or device memory read in stream order
    void animate_ik(const Anim& anim, const AnimMasks* masks, const mtr_anim_layer* layers, size_t nlayers, const AnimIK& ik, const mtr_ik_target* targets) {
        dev_.check(mtr_batch_animate_ik(h_, anim.handle(), masks ? masks->handle() : nullptr, layers, nlayers, ik.handle(), targets));
        npal_ = anim.njoints();
    }
    void animate_ik_device(const Anim& anim, const AnimMasks* masks, const mtr_anim_layer* layers_dev, size_t nlayers, const AnimIK& ik,
                           const mtr_ik_target* targets_dev, void* hip_stream = nullptr) {
        dev_.check(mtr_batch_animate_ik_device(h_, anim.handle(), masks ? masks->handle() : nullptr, layers_dev, nlayers, ik.handle(), targets_dev, hip_stream));
        npal_ = anim.njoints();
    }
    // the same and then one step of dt seconds of the springs of `spring` (SPEC.md section 24): ik may be nullptr (then
    // targets_dev is nullptr too); states_dev (n * nsprings records, device memory) is read and written in stream order;
    // motion_dev is n * 16 floats (mtr_anim_root_deltas_device) or nullptr
    void animate_spring_device(const Anim& anim, const AnimMasks* masks, const mtr_anim_layer* layers_dev, size_t nlayers, const AnimIK* ik,
                               const mtr_ik_target* targets_dev, const AnimSpring& spring, mtr_spring_state* states_dev, const float* motion_dev, float dt,
                               void* hip_stream = nullptr) {
        dev_.check(mtr_batch_animate_spring_device(h_, anim.handle(), masks ? masks->handle() : nullptr, layers_dev, nlayers, ik ? ik->handle() : nullptr,
                                                   targets_dev, spring.handle(), states_dev, motion_dev, dt, hip_stream));
        npal_ = anim.njoints();
    }
    // instance matrices from the joints of src's current version (SPEC.md section 18): one record per instance, host memory
    // or device memory read in stream order; one shot, the palettes are kept; src may be this batch
    void attach(const Batch& src, const mtr_attach* recs) { dev_.check(mtr_batch_attach(h_, src.handle(), recs)); }
    void attach_device(const Batch& src, const mtr_attach* recs_dev, void* hip_stream = nullptr) {
        dev_.check(mtr_batch_attach_device(h_, src.handle(), recs_dev, hip_stream));
    }
    // M := M * D, D the blended delta of nsteps steps per instance on the trajectory set (SPEC.md section 19): host memory or
    // device memory read in stream order; one shot, the palettes are kept
    void root_motion(const Anim& traj, const AnimRoot& root, const mtr_root_step* steps, size_t nsteps) {
        dev_.check(mtr_batch_root_motion(h_, traj.handle(), root.handle(), steps, nsteps));
    }
    void root_motion_device(const Anim& traj, const AnimRoot& root, const mtr_root_step* steps_dev, size_t nsteps, void* hip_stream = nullptr) {
        dev_.check(mtr_batch_root_motion_device(h_, traj.handle(), root.handle(), steps_dev, nsteps, hip_stream));
    }
    // the matrices alone, n x 16 floats, of n records against THIS batch: to host memory (waits), or in stream order
    std::vector<float> sockets(const mtr_attach* recs, size_t n) const {
        std::vector<float> out(n * 16);
        dev_.check(mtr_batch_sockets(h_, recs, n, out.data(), out.size()));
        return out;
    }
    void sockets_device(const mtr_attach* recs_dev, size_t n, float* out_dev, void* hip_stream = nullptr) const {
        dev_.check(mtr_batch_sockets_device(h_, recs_dev, n, out_dev, hip_stream));
    }
    std::vector<float> read_model_mats() const {
        std::vector<float> out(n_ * 16);
        dev_.check(mtr_batch_read_model_mats(h_, out.data(), out.size()));
        return out;
    }
    std::vector<float> read_palettes() const {
        std::vector<float> out(n_ * npal_ * 16);
        dev_.check(mtr_batch_read_palettes(h_, out.data(), out.size()));
        return out;
    }
    mtr_batch* handle() const { return h_; }

  private:
    const Device& dev_;
    size_t n_, npal_;
    mtr_batch* h_ = nullptr;
};

class Frame {
  public:
    // begin_render_pass, LoadOp::Clear(WHITE) / Clear(1.0) -- src/bin/modelviewer.rs:190-210
    Frame(const Device& dev, uint32_t width, uint32_t height, const float clear_rgba[4], float clear_depth) : dev_(dev) {
        dev.check(mtr_frame_begin(dev.handle(), width, height, clear_rgba, clear_depth, &h_));
    }
    // part r of a GroupFrame: the group frame owns (submits, waits for, destroys) it; draw into it, nothing else
    Frame(const Device& dev, mtr_frame* part_of_group_frame) : dev_(dev), h_(part_of_group_frame), owned_(false) {}
    Frame(const Frame&) = delete;
    ~Frame() {
        if (owned_) mtr_frame_destroy(h_);
    }
    void end() { dev_.check(mtr_frame_end(h_)); }  // queue.submit, src/renderer_app_manager.rs:185
    // end() in two halves, so a host can keep several frames in flight (the library overlaps them on its own streams)
    void submit() { dev_.check(mtr_frame_submit(h_)); }
    void wait() { dev_.check(mtr_frame_wait(h_)); }
    // multi-GPU: render only the bins with (bin % world) == rank, then pack them for the all-gather
    void set_shard(uint32_t rank, uint32_t world) { dev_.check(mtr_frame_set_shard(h_, rank, world)); }
    // ownership map of a sharded frame: MTR_OWN_BANDS (band_rows: world + 1 bin rows or nullptr), MTR_OWN_SUPERTILES (param), ...
    void set_shard_map(uint32_t rank, uint32_t world, uint32_t map, uint32_t param = 0, const uint32_t* band_rows = nullptr) {
        dev_.check(mtr_frame_set_shard_map(h_, rank, world, map, param, band_rows));
    }
    size_t shard_bytes() const { return mtr_frame_shard_bytes(h_); }
    void unpack_color_shards_on_stream(const void* gathered_dev, void* dst_dev, void* hip_stream) {
        dev_.check(mtr_frame_unpack_color_shards_on_stream(h_, gathered_dev, dst_dev, hip_stream));
    }
    void pack_color_shard(void* dst_dev, size_t dst_bytes) { dev_.check(mtr_frame_pack_color_shard(h_, dst_dev, dst_bytes)); }
    // hands the frame to the device's exchange thread, which owns (and destroys) it from here on
    void submit_exchange() {
        dev_.check(mtr_frame_submit_exchange(h_));
        h_ = nullptr;
    }
    void* color_devptr() const { return mtr_frame_color_devptr(h_); }
    void* depth_devptr() const { return mtr_frame_depth_devptr(h_); }
    void read_color(void* rgba8, size_t len) { dev_.check(mtr_frame_read_color(h_, rgba8, len)); }
    void read_depth(float* d, size_t count) { dev_.check(mtr_frame_read_depth(h_, d, count)); }
    mtr_frame_stats stats() {
        mtr_frame_stats s{};
        dev_.check(mtr_frame_get_stats(h_, &s));
        return s;
    }
    mtr_frame* handle() const { return h_; }
    const Device& device() const { return dev_; }

  private:
    const Device& dev_;
    mtr_frame* h_ = nullptr;
    bool owned_ = true;
};

inline void Model::render(Frame& frame, const float view_proj[16]) const {
    dev_.check(mtr_frame_draw_model(frame.handle(), h_, view_proj));
}

inline void Model::render_with_joints(Frame& frame, const float view_proj[16]) const {
    dev_.check(mtr_frame_draw_model_joints(frame.handle(), h_, view_proj));
}

// One host thread, N devices (mtr.h: mtr_group_*).  device(r) creates rank r's models / textures; a GroupFrame is one sharded
// Frame per rank -- draw into part(r) with rank r's objects -- and end() leaves the gathered RGBA8 image on rank 0's device.
class Group {
  public:
    explicit Group(const std::vector<int32_t>& hip_devices) {
        int32_t rc = mtr_group_create(hip_devices.data(), (int32_t)hip_devices.size(), &h_);
        if (rc) throw Error(rc, mtr_group_last_error(nullptr));
        for (int32_t r = 0; r < mtr_group_size(h_); r++) devs_.emplace_back(new Device(mtr_group_device(h_, r), Device::Borrowed{}));
    }
    Group(const Group&) = delete;
    Group& operator=(const Group&) = delete;
    ~Group() {
        devs_.clear();
        mtr_group_destroy(h_);
    }
    size_t size() const { return devs_.size(); }
    const Device& device(size_t rank) const { return *devs_.at(rank); }
    mtr_group* handle() const { return h_; }
    void check(int32_t rc) const {
        if (rc) throw Error(rc, mtr_group_last_error(h_));
    }

  private:
    mtr_group* h_ = nullptr;
    std::vector<std::unique_ptr<Device>> devs_;
};

class GroupFrame {
  public:
    GroupFrame(const Group& group, uint32_t width, uint32_t height, const float clear_rgba[4], float clear_depth,
               uint32_t map = MTR_OWN_BANDS, uint32_t param = 0, const uint32_t* band_rows = nullptr) : group_(group) {
        group.check(mtr_group_frame_begin(group.handle(), width, height, clear_rgba, clear_depth, map, param, band_rows, &h_));
        for (size_t r = 0; r < group.size(); r++) parts_.emplace_back(new Frame(group.device(r), mtr_group_frame_part(h_, (int32_t)r)));
    }
    GroupFrame(const GroupFrame&) = delete;
    ~GroupFrame() {
        parts_.clear();
        mtr_group_frame_destroy(h_);
    }
    Frame& part(size_t rank) { return *parts_.at(rank); }
    void end() { group_.check(mtr_group_frame_end(h_)); }
    void read_color(void* rgba8, size_t len) { group_.check(mtr_group_frame_read_color(h_, rgba8, len)); }
    void* color_devptr() const { return mtr_group_frame_color_devptr(h_); }

  private:
    const Group& group_;
    mtr_group_frame* h_ = nullptr;
    std::vector<std::unique_ptr<Frame>> parts_;
};

// The reference's app seam (src/renderer_app_manager.rs:14-32), headless: the "frame_view + encoder" pair is the Frame.
struct RendererApp {
    virtual ~RendererApp() = default;
    virtual void render(Frame& frame) = 0;
    virtual void post_render() {}
};

}  // namespace mtr
