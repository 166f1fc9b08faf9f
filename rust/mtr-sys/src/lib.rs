//! Raw bindings of `include/mtr.h`.  One declaration per exported symbol, same order as the header.
//! NOTE: written without a Rust toolchain available (the build container has none); kept
//! declaration-only so that it is checkable by eye against the header.
#![allow(non_camel_case_types)]
use core::ffi::{c_char, c_void};

pub const MTR_OK: i32 = 0;
pub const MTR_E_INVALID: i32 = 1;
pub const MTR_E_UNSUPPORTED: i32 = 2;
pub const MTR_E_NOMEM: i32 = 3;
pub const MTR_E_HIP: i32 = 4;
pub const MTR_E_OVERFLOW: i32 = 5;

pub const MTR_SEM_POSITION: u8 = 0;
pub const MTR_SEM_TEXCOORD: u8 = 1;
pub const MTR_SEM_JOINT: u8 = 2;
pub const MTR_SEM_WEIGHT: u8 = 3;

#[repr(C)]
#[derive(Clone, Copy)]
pub struct mtr_primitive {
    pub w: [u32; 14], // rmodel::PrimitiveInfo, 0x38 bytes verbatim
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_element {
    pub semantic: u8,
    pub format: u8, // rshader2::InputElementFormat as u32 -> u8
    pub count: u8,
    pub pad0: u8,
    pub offset: u16,
    pub pad1: u16,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_layout {
    pub num_elements: u32,
    pub elements: [mtr_element; 8],
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_frame_stats {
    pub tris_in: u64,
    pub tris_setup: u64,
    pub bin_entries: u64,
    pub segments: u64,
    pub width: u32,
    pub height: u32,
    pub nbins: u32,
    pub ndraws: u32,
    pub tile_kernel: u32,
    pub binning: u32,
    pub chunks: u64,
    pub chunks_culled: u64,
    pub shard_map: u32,  // MTR_OWN_*
    pub shard_bins: u32,
}
/// per-primitive material state (mtr.h): blend MTR_BLEND_*, depth write, depth test, cull MTR_CULL_*
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_prim_state {
    pub blend: u8,
    pub depth_write: u8,
    pub depth_test: u8,
    pub cull: u8,
}
pub const MTR_OWN_INTERLEAVED: u32 = 0;
pub const MTR_OWN_BANDS: u32 = 1;
pub const MTR_OWN_SUPERTILES: u32 = 2;
pub const MTR_TEXRES_DECODED: u32 = 0;
pub const MTR_TEXRES_BLOCKS: u32 = 1;
macro_rules! opaque { ($($n:ident),*) => { $( #[repr(C)] pub struct $n { _p: [u8; 0] } )* } }
opaque!(mtr_device, mtr_texture, mtr_model, mtr_batch, mtr_frame, mtr_anim, mtr_anim_masks, mtr_anim_ik, mtr_anim_root, mtr_anim_player, mtr_anim_ctrl, mtr_anim_events, mtr_anim_blend, mtr_anim_spring, mtr_anim_match);

/// animation clips (mtr.h, SPEC.md section 14): one key of one joint, 48 bytes
pub const MTR_CLIP_LOOP: u32 = 1;
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_anim_key {
    pub t: [f32; 3],
    pub pad0: f32,
    pub q: [f32; 4], // x, y, z, w
    pub s: [f32; 3],
    pub pad1: f32,
}
/// animation tracks (mtr.h, SPEC.md section 15): one track's keys and quantisation, 32 bytes
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_anim_track {
    pub first: u32,
    pub count: u32,
    pub lo: [f32; 3],
    pub step: [f32; 3],
}

/// animation layers (mtr.h, SPEC.md section 16): one layer of one instance, 16 bytes
pub const MTR_ANIM_MAX_LAYERS: usize = 8;
pub const MTR_LAYER_OVERRIDE: u16 = 0;
pub const MTR_LAYER_ADDITIVE: u16 = 1;
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_anim_layer {
    pub clip: u32,
    pub x: f32,
    pub w: f32,
    pub mask: u16,
    pub mode: u16,
}
/// inverse kinematics (mtr.h, SPEC.md section 17): a chain of an IK set and one instance's target for it, 32 bytes each
pub const MTR_ANIM_MAX_IK: usize = 4;
pub const MTR_IK_TWO_BONE: u32 = 0;
pub const MTR_IK_AIM: u32 = 1;
pub const MTR_IK_POLE: u32 = 1;
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_ik_chain {
    pub kind: u32,
    pub joint: [u32; 3],
    pub axis: [f32; 3],
    pub flags: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_ik_target {
    pub pos: [f32; 3],
    pub w: f32,
    pub pole: [f32; 3],
    pub pad: u32,
}
/// spring bones (mtr.h, SPEC.md section 24): a spring of a spring set, 48 bytes, and one instance's particle for it, 32 bytes
pub const MTR_ANIM_MAX_SPRINGS: usize = 16;
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_spring {
    pub joint: u32,
    pub flags: u32,
    pub stiffness: f32,
    pub drag: f32,
    pub tail: [f32; 3],
    pub pad0: f32,
    pub gravity: [f32; 3],
    pub pad1: f32,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_spring_state {
    pub cur: [f32; 3],
    pub live: u32,
    pub prev: [f32; 3],
    pub pad: u32,
}
/// attachments (mtr.h, SPEC.md section 18): one attached instance, 80 bytes; offset is column-major, in the source model's bind space
pub const MTR_ATTACH_NO_JOINT: u32 = 0xFFFF_FFFF;
pub const MTR_ATTACH_POSITION_ONLY: u32 = 1;
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_attach {
    pub src_instance: u32,
    pub joint: u32,
    pub flags: u32,
    pub pad: u32,
    pub offset: [f32; 16],
}
/// root motion (mtr.h, SPEC.md section 19): one step of an instance, 16 bytes; x and dx in keys / ticks
pub const MTR_ROOT_MAX_STEPS: usize = 8;
pub const MTR_ROOT_CYCLIC: u32 = 1;
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_root_step {
    pub clip: u32,
    pub x: f32,
    pub dx: f32,
    pub w: f32,
}
/// players (mtr.h, SPEC.md section 20): the play state an instance keeps on the device, 32 bytes, and a command to it, 16 bytes
pub const MTR_PLAY_ENDED: u32 = 1;
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_play_state {
    pub clip_a: u32,
    pub clip_b: u32,
    pub x_a: f32,
    pub x_b: f32,
    pub w: f32,
    pub fade: f32,
    pub speed: f32,
    pub flags: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_play_cmd {
    pub instance: u32,
    pub clip: u32,
    pub x: f32,
    pub seconds: f32,
}
/// controllers (mtr.h, SPEC.md section 21): the tables of a controller (a node 16 bytes, a condition 8, a transition 48) and
/// the state an instance keeps on the device, 16 bytes
pub const MTR_CTRL_MAX_COND: usize = 3;
pub const MTR_OP_LT: u16 = 0;
pub const MTR_OP_LE: u16 = 1;
pub const MTR_OP_GT: u16 = 2;
pub const MTR_OP_GE: u16 = 3;
pub const MTR_OP_EQ: u16 = 4;
pub const MTR_OP_NE: u16 = 5;
pub const MTR_TR_INTERRUPT: u32 = 1;
pub const MTR_TR_SELF: u32 = 2;
pub const MTR_TR_SYNC: u32 = 4;
pub const MTR_TR_CONSUME: u32 = 8;
pub const MTR_CTRL_TIME: u16 = 0xFFFF;
pub const MTR_CTRL_POS: u16 = 0xFFFE;
pub const MTR_CTRL_PHASE: u16 = 0xFFFD;
pub const MTR_CTRL_ENDED: u16 = 0xFFFC;
pub const MTR_CTRL_FADING: u16 = 0xFFFB;
pub const MTR_CTRL_NONE: u32 = 0xFFFF_FFFF;
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_ctrl_node {
    pub clip: u32,
    pub first: u32,
    pub count: u32,
    pub pad: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_ctrl_cond {
    pub param: u16,
    pub op: u16,
    pub value: f32,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_ctrl_trans {
    pub target: u32,
    pub flags: u32,
    pub seconds: f32,
    pub x: f32,
    pub ncond: u32,
    pub pad: u32,
    pub cond: [mtr_ctrl_cond; MTR_CTRL_MAX_COND],
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_ctrl_state {
    pub node: u32,
    pub t: f32,
    pub fired: u32,
    pub user: u32,
}
// motion matching (SPEC.md section 25)
pub const MTR_MATCH_INTERRUPT: u32 = 1;
pub const MTR_MATCH_NONE: u32 = 0xFFFF_FFFF;
pub const MTR_MATCH_MAX_DIMS: usize = 64;
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_match_row {
    pub clip: u32,
    pub x: f32,
    pub bias: f32,
    pub tags: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_match_filter {
    pub require: u32,
    pub exclude: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_match_result {
    pub row: u32,
    pub cur: u32,
    pub score: f32,
    pub cur_score: f32,
}
// animation events (SPEC.md section 22)
pub const MTR_EVENT_BACKWARD: u32 = 0x8000_0000;
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_event_marker {
    pub x: f32,
    pub id: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_anim_event {
    pub instance: u32,
    pub id: u32,
    pub where_: u32,
    pub w: f32,
}
// blend spaces (SPEC.md section 23)
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_blend_sample {
    pub clip: u32,
    pub px: f32,
    pub py: f32,
    pub pad: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_blend_tri {
    pub v: [u32; 3],
    pub pad: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_blend_state {
    pub phase: f32,
    pub px: f32,
    pub py: f32,
    pub speed: f32,
}
/// what one instance plays: clip A at x_a cross-faded by w with clip B at x_b, positions in keys; 24 bytes
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct mtr_anim_state {
    pub clip_a: u32,
    pub clip_b: u32,
    pub x_a: f32,
    pub x_b: f32,
    pub w: f32,
    pub pad: u32,
}

pub type mtr_allgather_fn = Option<unsafe extern "C" fn(send: *const c_void, recv: *mut c_void, count: usize, datatype: i32,
                                                         comm: *mut c_void, stream: *mut c_void) -> i32>;

extern "C" {
    pub fn mtr_abi_version() -> i32;
    pub fn mtr_device_create(hip_device: i32, out: *mut *mut mtr_device) -> i32;
    pub fn mtr_device_create_on_stream(hip_device: i32, hip_stream: *mut c_void, out: *mut *mut mtr_device) -> i32;
    pub fn mtr_device_destroy(dev: *mut mtr_device);
    pub fn mtr_last_error(dev: *const mtr_device) -> *const c_char;
    pub fn mtr_device_set_profiling(dev: *mut mtr_device, enable: i32) -> i32;
    pub fn mtr_device_set_tile_mode(dev: *mut mtr_device, mode: i32) -> i32;
    pub fn mtr_device_set_binning(dev: *mut mtr_device, single_pass: i32, queue_capacity: u32) -> i32;
    pub fn mtr_frame_read_bin_counts(frame: *mut mtr_frame, entries: *mut u32, segments: *mut u32, nbins: usize) -> i32;
    pub fn mtr_texture_create(dev: *mut mtr_device, width: u32, height: u32, format: u32, data: *const c_void, len: usize,
                              out: *mut *mut mtr_texture) -> i32;
    pub fn mtr_texture_destroy(tex: *mut mtr_texture);
    pub fn mtr_texture_read_rgba8(tex: *mut mtr_texture, out: *mut c_void, len: usize) -> i32;
    pub fn mtr_model_create(dev: *mut mtr_device, vertex_buf: *const c_void, vertex_len: usize, index_buf: *const u16,
                            index_num: usize, prims: *const mtr_primitive, nprims: usize, layouts: *const mtr_layout,
                            prim_to_texture: *const i32, textures: *const *mut mtr_texture, ntextures: usize,
                            prim_debug_id: *const u32, out: *mut *mut mtr_model) -> i32;
    pub fn mtr_model_destroy(model: *mut mtr_model);
    pub fn mtr_model_set_parts_disp(model: *mut mtr_model, parts_disp: *const u8, n: usize) -> i32;
    pub fn mtr_model_set_palette(model: *mut mtr_model, mats: *const f32, n: usize) -> i32;
    pub fn mtr_batch_create(dev: *mut mtr_device, model: *mut mtr_model, n: usize, model_mats: *const f32,
                            palettes: *const f32, npal: usize, texture_override: *const i32, out: *mut *mut mtr_batch) -> i32;
    pub fn mtr_batch_destroy(batch: *mut mtr_batch);
    pub fn mtr_frame_begin(dev: *mut mtr_device, width: u32, height: u32, clear_rgba: *const f32, clear_depth: f32,
                           out: *mut *mut mtr_frame) -> i32;
    pub fn mtr_frame_set_shard(frame: *mut mtr_frame, rank: u32, world: u32) -> i32;
    pub fn mtr_frame_draw_model(frame: *mut mtr_frame, model: *mut mtr_model, view_proj: *const f32) -> i32;
    pub fn mtr_frame_draw_batch(frame: *mut mtr_frame, batch: *mut mtr_batch, view_proj: *const f32) -> i32;
    pub fn mtr_frame_draw_instances(frame: *mut mtr_frame, model: *mut mtr_model, model_mats: *const f32,
                                    palettes: *const f32, npal: usize, n: usize, view_proj: *const f32) -> i32;
    pub fn mtr_frame_draw_overlay_cubes(frame: *mut mtr_frame, camera: *const f32, inst_mats: *const f32, n: usize) -> i32;
    pub fn mtr_frame_submit(frame: *mut mtr_frame) -> i32;
    pub fn mtr_frame_wait(frame: *mut mtr_frame) -> i32;
    pub fn mtr_frame_end(frame: *mut mtr_frame) -> i32;
    pub fn mtr_frame_read_color(frame: *mut mtr_frame, rgba8: *mut c_void, len: usize) -> i32;
    pub fn mtr_frame_read_depth(frame: *mut mtr_frame, depth: *mut f32, count: usize) -> i32;
    pub fn mtr_frame_color_devptr(frame: *mut mtr_frame) -> *mut c_void;
    pub fn mtr_frame_depth_devptr(frame: *mut mtr_frame) -> *mut c_void;
    pub fn mtr_shard_bytes(width: u32, height: u32, world: u32) -> usize;
    pub fn mtr_frame_pack_color_shard(frame: *mut mtr_frame, dst_dev: *mut c_void, dst_bytes: usize) -> i32;
    pub fn mtr_device_unpack_color_shards(dev: *mut mtr_device, gathered_dev: *const c_void, world: u32, width: u32,
                                          height: u32, dst_dev: *mut c_void) -> i32;
    pub fn mtr_frame_pack_color_shard_on_stream(frame: *mut mtr_frame, dst_dev: *mut c_void, dst_bytes: usize, hip_stream: *mut c_void) -> i32;
    pub fn mtr_device_unpack_color_shards_on_stream(dev: *mut mtr_device, gathered_dev: *const c_void, world: u32, width: u32,
                                                    height: u32, dst_dev: *mut c_void, hip_stream: *mut c_void) -> i32;
    /// exchange thread (mtr.h): `fn_` has ncclAllGather's signature; `mtr_frame_submit_exchange` consumes the frame
    pub fn mtr_device_exchange_start(dev: *mut mtr_device, fn_: mtr_allgather_fn, comm: *mut c_void, dtype_u8: i32,
                                     send_dev: *mut c_void, send_bytes: usize, gathered_dev: *mut c_void, dst_dev: *mut c_void,
                                     world: u32, hip_stream: *mut c_void) -> i32;
    pub fn mtr_device_exchange_add_lane(dev: *mut mtr_device, comm: *mut c_void, send_dev: *mut c_void, gathered_dev: *mut c_void,
                                        dst_dev: *mut c_void, hip_stream: *mut c_void) -> i32;
    pub fn mtr_frame_submit_exchange(frame: *mut mtr_frame) -> i32;
    pub fn mtr_device_exchange_drain(dev: *mut mtr_device) -> i32;
    pub fn mtr_device_exchange_stop(dev: *mut mtr_device) -> i32;
    pub fn mtr_frame_get_stats(frame: *mut mtr_frame, out: *mut mtr_frame_stats) -> i32;
    pub fn mtr_frame_get_timings(frame: *mut mtr_frame, ms: *mut f32) -> i32;
    pub fn mtr_frame_destroy(frame: *mut mtr_frame);
    pub fn mtr_model_vertex_stage(model: *mut mtr_model, prim: usize, m: *const f32, out_clip: *mut f32, out_uv: *mut f32) -> i32;
    pub fn mtr_crc32(bytes: *const u8, len: usize, init: u32) -> u32;
    // round 2
    pub fn mtr_device_synchronize(dev: *mut mtr_device) -> i32;
    pub fn mtr_device_set_culling(dev: *mut mtr_device, mode: i32) -> i32; // MTR_GEOM_CULL_OFF / _SHARDED / _ALL_FRAMES = 0 / 1 / 2
    pub fn mtr_device_set_texture_residency(dev: *mut mtr_device, mode: u32) -> i32;
    pub fn mtr_texture_create_mips(dev: *mut mtr_device, width: u32, height: u32, format: u32, levels: u32, data: *const c_void,
                                   len: usize, out: *mut *mut mtr_texture) -> i32;
    pub fn mtr_model_set_prim_states(model: *mut mtr_model, states: *const mtr_prim_state, nprims: usize) -> i32;
    pub fn mtr_model_set_joint_positions(model: *mut mtr_model, xyz: *const f32, njoints: usize) -> i32;
    pub fn mtr_frame_draw_model_joints(frame: *mut mtr_frame, model: *mut mtr_model, camera: *const f32) -> i32;
    pub fn mtr_frame_set_shard_map(frame: *mut mtr_frame, rank: u32, world: u32, map: u32, param: u32, band_rows: *const u32) -> i32;
    pub fn mtr_shard_bytes_map(width: u32, height: u32, world: u32, map: u32, param: u32, band_rows: *const u32) -> usize;
    pub fn mtr_frame_shard_bytes(frame: *mut mtr_frame) -> usize;
    pub fn mtr_frame_unpack_color_shards_on_stream(frame: *mut mtr_frame, gathered_dev: *const c_void, dst_dev: *mut c_void,
                                                   hip_stream: *mut c_void) -> i32;
    // animation clips
    pub fn mtr_anim_create(dev: *mut mtr_device, njoints: usize, nclips: usize, nkeys: *const u32, flags: *const u32,
                           keys: *const mtr_anim_key, out: *mut *mut mtr_anim) -> i32;
    pub fn mtr_anim_destroy(anim: *mut mtr_anim);
    pub fn mtr_model_animate(model: *mut mtr_model, anim: *mut mtr_anim, state: *const mtr_anim_state) -> i32;
    pub fn mtr_batch_animate(batch: *mut mtr_batch, anim: *mut mtr_anim, states: *const mtr_anim_state) -> i32;
    pub fn mtr_batch_animate_device(batch: *mut mtr_batch, anim: *mut mtr_anim, states_dev: *const mtr_anim_state,
                                    hip_stream: *mut c_void) -> i32;
    pub fn mtr_anim_sample(anim: *mut mtr_anim, states: *const mtr_anim_state, n: usize, out_locals: *mut f32, count: usize) -> i32;
    // animation tracks (SPEC.md section 15): declaration only; a descriptor is 32 bytes (u32 first, count; f32 lo[3], step[3])
    pub fn mtr_anim_create_tracks(dev: *mut mtr_device, njoints: usize, nclips: usize, nticks: *const u32, flags: *const u32,
                                  tracks: *const mtr_anim_track, times: *const u16, values: *const u16, nkeys_total: usize,
                                  out: *mut *mut mtr_anim) -> i32;
    // animation layers (SPEC.md section 16): declarations only
    pub fn mtr_anim_masks_create(dev: *mut mtr_device, njoints: usize, nmasks: usize, weights: *const f32, out: *mut *mut mtr_anim_masks) -> i32;
    pub fn mtr_anim_masks_destroy(masks: *mut mtr_anim_masks);
    pub fn mtr_model_animate_layers(model: *mut mtr_model, anim: *mut mtr_anim, masks: *mut mtr_anim_masks, layers: *const mtr_anim_layer,
                                    nlayers: usize) -> i32;
    pub fn mtr_batch_animate_layers(batch: *mut mtr_batch, anim: *mut mtr_anim, masks: *mut mtr_anim_masks, layers: *const mtr_anim_layer,
                                    nlayers: usize) -> i32;
    pub fn mtr_batch_animate_layers_device(batch: *mut mtr_batch, anim: *mut mtr_anim, masks: *mut mtr_anim_masks,
                                           layers_dev: *const mtr_anim_layer, nlayers: usize, hip_stream: *mut c_void) -> i32;
    pub fn mtr_anim_sample_layers(anim: *mut mtr_anim, masks: *mut mtr_anim_masks, layers: *const mtr_anim_layer, nlayers: usize, n: usize,
                                  out_locals: *mut f32, count: usize) -> i32;
    // inverse kinematics (SPEC.md section 17): declarations only
    pub fn mtr_anim_ik_create(dev: *mut mtr_device, njoints: usize, parents: *const u8, nchains: usize, chains: *const mtr_ik_chain,
                              out: *mut *mut mtr_anim_ik) -> i32;
    pub fn mtr_anim_ik_destroy(ik: *mut mtr_anim_ik);
    pub fn mtr_model_animate_ik(model: *mut mtr_model, anim: *mut mtr_anim, masks: *mut mtr_anim_masks, layers: *const mtr_anim_layer,
                                nlayers: usize, ik: *mut mtr_anim_ik, targets: *const mtr_ik_target) -> i32;
    pub fn mtr_batch_animate_ik(batch: *mut mtr_batch, anim: *mut mtr_anim, masks: *mut mtr_anim_masks, layers: *const mtr_anim_layer,
                                nlayers: usize, ik: *mut mtr_anim_ik, targets: *const mtr_ik_target) -> i32;
    pub fn mtr_batch_animate_ik_device(batch: *mut mtr_batch, anim: *mut mtr_anim, masks: *mut mtr_anim_masks,
                                       layers_dev: *const mtr_anim_layer, nlayers: usize, ik: *mut mtr_anim_ik,
                                       targets_dev: *const mtr_ik_target, hip_stream: *mut c_void) -> i32;
    pub fn mtr_anim_sample_ik(anim: *mut mtr_anim, masks: *mut mtr_anim_masks, ik: *mut mtr_anim_ik, layers: *const mtr_anim_layer,
                              nlayers: usize, targets: *const mtr_ik_target, n: usize, out_locals: *mut f32, count: usize) -> i32;
    // attachments (SPEC.md section 18): declarations only
    pub fn mtr_batch_attach(batch: *mut mtr_batch, src: *mut mtr_batch, recs: *const mtr_attach) -> i32;
    pub fn mtr_batch_attach_device(batch: *mut mtr_batch, src: *mut mtr_batch, recs_dev: *const mtr_attach, hip_stream: *mut c_void) -> i32;
    pub fn mtr_batch_sockets(src: *mut mtr_batch, recs: *const mtr_attach, n: usize, out: *mut f32, count: usize) -> i32;
    pub fn mtr_batch_sockets_device(src: *mut mtr_batch, recs_dev: *const mtr_attach, n: usize, out_dev: *mut f32, hip_stream: *mut c_void) -> i32;
    pub fn mtr_batch_read_model_mats(batch: *mut mtr_batch, out: *mut f32, count: usize) -> i32;
    // root motion (SPEC.md section 19): declarations only
    pub fn mtr_anim_root_create(dev: *mut mtr_device, njoints: usize, nclips: usize, joint: u32, flags: *const u32, out: *mut *mut mtr_anim_root) -> i32;
    pub fn mtr_anim_root_destroy(root: *mut mtr_anim_root);
    pub fn mtr_batch_root_motion(batch: *mut mtr_batch, traj: *mut mtr_anim, root: *mut mtr_anim_root, steps: *const mtr_root_step, nsteps: usize) -> i32;
    pub fn mtr_batch_root_motion_device(batch: *mut mtr_batch, traj: *mut mtr_anim, root: *mut mtr_anim_root, steps_dev: *const mtr_root_step,
                                        nsteps: usize, hip_stream: *mut c_void) -> i32;
    pub fn mtr_anim_root_deltas(traj: *mut mtr_anim, root: *mut mtr_anim_root, steps: *const mtr_root_step, nsteps: usize, n: usize, out: *mut f32,
                                count: usize) -> i32;
    pub fn mtr_anim_root_deltas_device(traj: *mut mtr_anim, root: *mut mtr_anim_root, steps_dev: *const mtr_root_step, nsteps: usize, n: usize,
                                       out_dev: *mut f32, hip_stream: *mut c_void) -> i32;
    // players (SPEC.md section 20): declarations only
    pub fn mtr_anim_player_create(dev: *mut mtr_device, nclips: usize, nkeys: *const u32, flags: *const u32, rates: *const f32, max_instances: usize,
                                  out: *mut *mut mtr_anim_player) -> i32;
    pub fn mtr_anim_player_destroy(player: *mut mtr_anim_player);
    pub fn mtr_anim_player_advance_device(player: *mut mtr_anim_player, states_dev: *mut mtr_play_state, n: usize, dt: f32, cmds: *const mtr_play_cmd,
                                          ncmds: usize, out_states_dev: *mut mtr_anim_state, out_layers_dev: *mut mtr_anim_layer, nlayers: usize,
                                          out_steps_dev: *mut mtr_root_step, hip_stream: *mut c_void) -> i32;
    pub fn mtr_anim_player_advance_device_cmds(player: *mut mtr_anim_player, states_dev: *mut mtr_play_state, n: usize, dt: f32,
                                               cmds_dev: *const mtr_play_cmd, ncmds: usize, out_states_dev: *mut mtr_anim_state,
                                               out_layers_dev: *mut mtr_anim_layer, nlayers: usize, out_steps_dev: *mut mtr_root_step,
                                               hip_stream: *mut c_void) -> i32;
    pub fn mtr_anim_player_advance_host(player: *mut mtr_anim_player, states: *mut mtr_play_state, n: usize, dt: f32, cmds: *const mtr_play_cmd, ncmds: usize,
                                        out_states: *mut mtr_anim_state, out_layers: *mut mtr_anim_layer, nlayers: usize, out_steps: *mut mtr_root_step) -> i32;
    // controllers (SPEC.md section 21): declarations only
    pub fn mtr_anim_ctrl_create(dev: *mut mtr_device, nclips: usize, nkeys: *const u32, clip_flags: *const u32, nodes: *const mtr_ctrl_node, nnodes: usize,
                                trans: *const mtr_ctrl_trans, ntrans: usize, nany: usize, nparams: usize, out: *mut *mut mtr_anim_ctrl) -> i32;
    pub fn mtr_anim_ctrl_destroy(ctrl: *mut mtr_anim_ctrl);
    pub fn mtr_anim_ctrl_step_device(ctrl: *mut mtr_anim_ctrl, states_dev: *mut mtr_ctrl_state, play_dev: *const mtr_play_state, params_dev: *mut f32, n: usize,
                                     dt: f32, cmds_out_dev: *mut mtr_play_cmd, counts_dev: *mut u32, hip_stream: *mut c_void) -> i32;
    pub fn mtr_anim_ctrl_step_host(ctrl: *mut mtr_anim_ctrl, states: *mut mtr_ctrl_state, play: *const mtr_play_state, params: *mut f32, n: usize, dt: f32,
                                   cmds_out: *mut mtr_play_cmd, counts: *mut u32) -> i32;
    // motion matching (SPEC.md section 25): declarations only
    pub fn mtr_anim_match_create(dev: *mut mtr_device, nclips: usize, nkeys: *const u32, clip_flags: *const u32, d: usize, pose_dims: u64, flags: u32, seconds: f32,
                                 near_x: f32, margin: f32, rows: *const mtr_match_row, nrows: usize, features: *const f32, mean: *const f32, scale: *const f32,
                                 max_instances: usize, out: *mut *mut mtr_anim_match) -> i32;
    pub fn mtr_anim_match_destroy(m: *mut mtr_anim_match);
    pub fn mtr_anim_match_search_device(m: *mut mtr_anim_match, play_dev: *const mtr_play_state, query_dev: *const f32, filter_dev: *const mtr_match_filter, n: usize,
                                        instance_base: u32, cmds_out_dev: *mut mtr_play_cmd, results_dev: *mut mtr_match_result, hip_stream: *mut c_void) -> i32;
    pub fn mtr_anim_match_search_host(m: *mut mtr_anim_match, play: *const mtr_play_state, query: *const f32, filter: *const mtr_match_filter, n: usize,
                                      instance_base: u32, cmds_out: *mut mtr_play_cmd, results: *mut mtr_match_result) -> i32;
    pub fn mtr_anim_match_scores_host(m: *mut mtr_anim_match, play: *const mtr_play_state, query: *const f32, n: usize, out: *mut f32) -> i32;
    // animation events (SPEC.md section 22): declarations only
    pub fn mtr_anim_events_create(dev: *mut mtr_device, nclips: usize, nkeys: *const u32, clip_flags: *const u32, counts: *const u32,
                                  markers: *const mtr_event_marker, max_instances: usize, out: *mut *mut mtr_anim_events) -> i32;
    pub fn mtr_anim_events_destroy(ev: *mut mtr_anim_events);
    pub fn mtr_anim_events_collect_device(ev: *mut mtr_anim_events, steps_dev: *const mtr_root_step, nsteps: usize, n: usize, min_weight: f32,
                                          out_dev: *mut mtr_anim_event, capacity: usize, count_dev: *mut u32, bits_dev: *mut u32,
                                          hip_stream: *mut c_void) -> i32;
    pub fn mtr_anim_events_collect_host(ev: *mut mtr_anim_events, steps: *const mtr_root_step, nsteps: usize, n: usize, min_weight: f32,
                                        out: *mut mtr_anim_event, capacity: usize, count: *mut u32, bits: *mut u32) -> i32;
    // blend spaces (SPEC.md section 23): declarations only
    pub fn mtr_anim_blend_create(dev: *mut mtr_device, nclips: usize, nkeys: *const u32, clip_flags: *const u32, rates: *const f32,
                                 samples: *const mtr_blend_sample, nsamples: usize, tris: *const mtr_blend_tri, ntris: usize, nparams: usize,
                                 param_x: u32, param_y: u32, damp: f32, max_instances: usize, out: *mut *mut mtr_anim_blend) -> i32;
    pub fn mtr_anim_blend_destroy(blend: *mut mtr_anim_blend);
    pub fn mtr_anim_blend_advance_device(blend: *mut mtr_anim_blend, states_dev: *mut mtr_blend_state, params_dev: *const f32, n: usize, dt: f32,
                                         out_layers_dev: *mut mtr_anim_layer, nlayers: usize, out_steps_dev: *mut mtr_root_step,
                                         out_shares_dev: *mut f32, hip_stream: *mut c_void) -> i32;
    pub fn mtr_anim_blend_advance_host(blend: *mut mtr_anim_blend, states: *mut mtr_blend_state, params: *const f32, n: usize, dt: f32,
                                       out_layers: *mut mtr_anim_layer, nlayers: usize, out_steps: *mut mtr_root_step, out_shares: *mut f32) -> i32;
    // spring bones (SPEC.md section 24): declarations only
    pub fn mtr_anim_spring_create(dev: *mut mtr_device, njoints: usize, parents: *const u8, nsprings: usize, springs: *const mtr_spring,
                                  out: *mut *mut mtr_anim_spring) -> i32;
    pub fn mtr_anim_spring_destroy(spring: *mut mtr_anim_spring);
    pub fn mtr_batch_animate_spring_device(batch: *mut mtr_batch, anim: *mut mtr_anim, masks: *mut mtr_anim_masks,
                                           layers_dev: *const mtr_anim_layer, nlayers: usize, ik: *mut mtr_anim_ik,
                                           targets_dev: *const mtr_ik_target, spring: *mut mtr_anim_spring, states_dev: *mut mtr_spring_state,
                                           motion_dev: *const f32, dt: f32, hip_stream: *mut c_void) -> i32;
    pub fn mtr_anim_sample_spring(anim: *mut mtr_anim, masks: *mut mtr_anim_masks, ik: *mut mtr_anim_ik, spring: *mut mtr_anim_spring,
                                  layers: *const mtr_anim_layer, nlayers: usize, targets: *const mtr_ik_target, states: *mut mtr_spring_state,
                                  motion: *const f32, dt: f32, n: usize, out_locals: *mut f32, count: usize) -> i32;
}
pub mod files;
