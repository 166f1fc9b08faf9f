/* mtr.h -- C ABI of libmtr.so: the MI355X-native (HIP, gfx950) rModel draw path.
 *
 * The reference (ReplayCoding/mt-renderer) has no FFI: its seam is the Rust API typed over wgpu
 *     Model::new / Model::set_parts_disp / Model::render      (src/model.rs:36-45, :295, :299-305)
 *     Texture::new                                            (src/texture.rs:11)
 *     RendererApp::{setup, render, post_render}               (src/renderer_app_manager.rs:14-32)
 * and everything below `wgpu::RenderPass::draw_indexed` happens inside a GPU driver.  This header
 * is what a Rust `mtr-sys` crate would bind: plain pointers and sizes, an
 * int32 status return, out-parameters last, no unwinding, opaque handles freed by the matching
 * *_destroy.  The caller owns every host buffer passed in; the library copies at *_create.
 *
 * Matrix convention: 16 f32, column-major, M*v (glam::Mat4 bytes, src/bin/modelviewer.rs:217-221).
 * Threading: one host thread per mtr_device at a time (externally synchronised), as the reference's
 * single winit thread.  There is no CPU fallback: every entry point needs a HIP device.
 */
#ifndef MTR_H
#define MTR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTR_ABI_VERSION 2

enum {
    MTR_OK = 0,
    MTR_E_INVALID = 1,     /* bad argument / out-of-range offset (reference: panic) */
    MTR_E_UNSUPPORTED = 2, /* vertex/texture format the reference todo!()s: src/rshader2.rs:519-563, src/rtexture.rs:159 */
    MTR_E_NOMEM = 3,
    MTR_E_HIP = 4,         /* a HIP runtime call failed; see mtr_last_error */
    MTR_E_OVERFLOW = 5     /* internal queue capacity exceeded and could not be grown */
};

/* vertex element semantics: Position / TexCoord are the only names the reference binds
 * (src/rshader2.rs:503-507); Joint / Weight are this build's linear-blend-skinning extension */
enum { MTR_SEM_POSITION = 0, MTR_SEM_TEXCOORD = 1, MTR_SEM_JOINT = 2, MTR_SEM_WEIGHT = 3 };

/* InputElementFormat, numeric values of src/rshader2.rs:73-90 */
enum {
    MTR_IEF_F32 = 1, MTR_IEF_F16 = 2, MTR_IEF_S16 = 3, MTR_IEF_U16 = 4, MTR_IEF_S16N = 5,
    MTR_IEF_U16N = 6, MTR_IEF_S8 = 7, MTR_IEF_U8 = 8, MTR_IEF_S8N = 9, MTR_IEF_U8N = 10,
    MTR_IEF_SCMP3N = 11, MTR_IEF_UCMP3N = 12, MTR_IEF_U8NL = 13, MTR_IEF_COLOR4N = 14
};

/* rTexture format ids accepted by TextureFile::format_wgpu (src/rtexture.rs:152-161) */
enum { MTR_TEX_RGBA8 = 7, MTR_TEX_BC1 = 19, MTR_TEX_BC7 = 42, MTR_TEX_BC7_ALT = 54 };

/* PrimitiveInfo, verbatim 0x38 bytes (src/rmodel.rs:135-171; size test :489) */
typedef struct mtr_primitive {
    uint32_t w[14];
} mtr_primitive;

/* one decoded input-layout element (src/rshader2.rs:425-442): replaces the wgpu::VertexAttribute
 * list that Shader2File::create_vertex_buffer_elements builds (src/rshader2.rs:496-571) */
/* mtr_element.flags: the reference skips IEF_SCMP3N elements (src/rshader2.rs:509-512); with this bit a Position /
 * TexCoord element of that format is decoded as three signed 10-bit fields, x = bits 0..9, max(v / 511, -1)
 * (build extension, row f-4; SPEC.md section 2) */
#define MTR_ELEM_DECODE_SCMP3N 1u
typedef struct mtr_element {
    uint8_t semantic; /* MTR_SEM_* */
    uint8_t format;   /* MTR_IEF_* */
    uint8_t count;
    uint8_t flags;    /* MTR_ELEM_* (0 = the reference's behaviour) */
    uint16_t offset;  /* byte offset inside the vertex (9 bits in the file) */
    uint16_t pad1;
} mtr_element;

typedef struct mtr_layout {
    uint32_t num_elements; /* <= 8 */
    mtr_element elements[8];
} mtr_layout;

typedef struct mtr_device mtr_device;
typedef struct mtr_texture mtr_texture;
typedef struct mtr_model mtr_model;
typedef struct mtr_batch mtr_batch;
typedef struct mtr_frame mtr_frame;

/* per-frame counters (device side, read back by mtr_frame_get_stats) */
typedef struct mtr_frame_stats {
    uint64_t tris_in;     /* input triangles, SURVEY 8(d) definition */
    uint64_t tris_setup;  /* triangles that survived clip / cull / empty-bbox (sharded frame: and touch a bin of this rank); one that
                             covers no pixel centre is counted here and queued nowhere: bin_entries counts what is queued */
    uint64_t bin_entries; /* (triangle, 16x16 bin) pairs */
    uint64_t segments;    /* per-bin ordered runs */
    uint32_t width, height, nbins, ndraws;
    uint32_t tile_kernel; /* MTR_TILE_ORDERED, MTR_TILE_VISIBILITY or MTR_TILE_MIXED: which tile kernel(s) rendered the frame */
    uint32_t binning;     /* 1 = single-pass bounded queues, 2 = exact two-pass (count, scan, fill) queues */
    uint64_t chunks;        /* geometry waves of the frame (62 strip positions each, per instance) */
    uint64_t chunks_culled; /* of those, skipped by this rank before any vertex work: bounds outside its bins (sharded frames;
                             * whole instances of a batch and single chunks alike) */
    uint32_t shard_map;     /* MTR_OWN_* */
    uint32_t shard_bins;    /* bins this rank rendered */
} mtr_frame_stats;

/* stage timings of the last submitted frame, milliseconds, from hipEvents recorded on the
 * device's stream (enabled by mtr_device_set_profiling) */
enum { MTR_STAGE_GEOM = 0, MTR_STAGE_SCAN = 1, MTR_STAGE_FILL = 2, MTR_STAGE_TILE = 3, MTR_STAGE_COUNT = 4 };

/* ---- device (replaces wgpu::Device + wgpu::Queue, src/renderer_app_manager.rs:103-115) ---- */
int32_t mtr_device_create(int32_t hip_device, mtr_device **out);
/* same, but all work is issued on a caller-owned hipStream_t (e.g. torch's current stream) */
int32_t mtr_device_create_on_stream(int32_t hip_device, void *hip_stream, mtr_device **out);
void mtr_device_destroy(mtr_device *dev);
const char *mtr_last_error(const mtr_device *dev); /* never NULL; dev may be NULL for create errors */
int32_t mtr_device_set_profiling(mtr_device *dev, int32_t enable);
/* wgpu::Device::poll(Maintain::Wait): returns once every frame submitted so far (and every exchange handed over) has
 * left the GPU, with the error of any frame that was released without mtr_frame_wait and turned out to have overflowed
 * its bin queues (MTR_E_OVERFLOW: that frame is missing triangles; later frames get larger queues). */
int32_t mtr_device_synchronize(mtr_device *dev);
/* tile-kernel choice.  AUTO: the visibility-key kernel when every material of the frame is opaque (debug-id /
 * overlay colours, textures whose alpha is 255 everywhere -- the blend is then a replace), else the ordered
 * kernel.  ORDERED forces the ordered kernel (tests compare both); VISIBILITY is honoured only when eligible. */
enum { MTR_TILE_AUTO = 0, MTR_TILE_ORDERED = 1, MTR_TILE_VISIBILITY = 2,
       MTR_TILE_MIXED = 3 /* reported only: visibility kernel on the bins that hold no translucent triangle, ordered kernel on the rest */ };
int32_t mtr_device_set_tile_mode(mtr_device *dev, int32_t mode);
/* triangle -> bin queues.  single_pass != 0 (default): k_geom writes straight into bounded per-bin queues of
 * queue_capacity entries (0 keeps the current bound); a frame that overflows a queue is transparently re-run with the
 * exact two-pass queues (count, scan, fill) and the bound doubles for later frames.  single_pass == 0: always two-pass. */
int32_t mtr_device_set_binning(mtr_device *dev, int32_t single_pass, uint32_t queue_capacity);
int32_t mtr_abi_version(void);

/* ---- Texture::new (src/texture.rs:11-30): level 0 only, 2-D, decoded on upload ---- */
int32_t mtr_texture_create(mtr_device *dev, uint32_t width, uint32_t height, uint32_t format,
                           const void *data, size_t len, mtr_texture **out);
/* the same with a mip chain (row f-4): `levels` levels in `data`, level l = max(1, width >> l) x max(1, height >> l),
 * level 0 first, each in `format`.  The reference uploads level 0 only (src/texture.rs:21) although rTexture files
 * carry the chain (src/rtexture.rs:111-130); with more levels a minified sample (SPEC.md section 7) takes the nearest
 * texel of the nearest level: level l while max |d(uv)/d(xy)| * size > 2^(l - 1/2).  levels = 1 is mtr_texture_create. */
int32_t mtr_texture_create_mips(mtr_device *dev, uint32_t width, uint32_t height, uint32_t format, uint32_t levels,
                                const void *data, size_t len, mtr_texture **out);
void mtr_texture_destroy(mtr_texture *tex);
/* decoded RGBA8 texels of level 0 (row-major, width*height*4 bytes): what the sampler reads */
int32_t mtr_texture_read_rgba8(mtr_texture *tex, void *out, size_t len);
/* What a BC1 / BC7 texture created AFTER this call keeps in HBM.  The reference hands the blocks to the GPU's texture unit
 * (device feature TEXTURE_COMPRESSION_BC, src/renderer_app_manager.rs:107); here either
 *   MTR_TEXRES_DECODED  (default) the image is decoded to RGBA8 once at creation and the sampler reads plain texels, or
 *   MTR_TEXRES_BLOCKS   the blocks stay as uploaded (1/4 of the bytes for BC7, 1/8 for BC1) and every fetch decodes its
 *                       texel from its block.  Same pixels; mtr_texture_read_rgba8 returns MTR_E_UNSUPPORTED.
 * DESIGN.md section 3 has the measured trade (C5: 64 textures of 1024 x 1024). */
enum { MTR_TEXRES_DECODED = 0, MTR_TEXRES_BLOCKS = 1 };
int32_t mtr_device_set_texture_residency(mtr_device *dev, uint32_t mode);

/* ---- Model::new (src/model.rs:36-293) ----
 * vertex_buf/index_buf: ModelFile::vertex_buf()/index_buf() (src/rmodel.rs:457-463).
 * prims: ModelFile::primitives(), one layout / texture slot / debug id per primitive:
 *   prim_to_texture[p] = index into textures[] or -1 (mat_to_tex, src/model.rs:60-75,167,324)
 *   prim_debug_id[p]   = boundary_infos[prim.boundary_num()].joint() (src/model.rs:140-141)
 * parts_disp defaults to all-true with len = nprims (src/model.rs:270). */
int32_t mtr_model_create(mtr_device *dev, const void *vertex_buf, size_t vertex_len,
                         const uint16_t *index_buf, size_t index_num, const mtr_primitive *prims,
                         size_t nprims, const mtr_layout *layouts, const int32_t *prim_to_texture,
                         mtr_texture *const *textures, size_t ntextures,
                         const uint32_t *prim_debug_id, mtr_model **out);
void mtr_model_destroy(mtr_model *model);
/* Material state per primitive (row f-4).  The reference builds every pipeline with one fixed state (alpha blend,
 * depth LessEqual + write, cull back: src/model.rs:240-262) and only LOGS the blend / depth-stencil / rasterizer
 * state objects a material names (src/rmaterial.rs:104-106, :211-230); applying them is this build's extension:
 *   blend       MTR_BLEND_ALPHA  rgb = src * a + dst * (1 - a), alpha = src (the reference)
 *               MTR_BLEND_OFF    replace
 *               MTR_BLEND_ADD    rgb = src * a + dst, alpha = src
 *   depth_write 1 (the reference) / 0: fragments that pass leave the depth buffer alone
 *   depth_test  1: LessEqual (the reference) / 0: always pass (near / far clipping still applies)
 *   cull        MTR_CULL_BACK (the reference) / MTR_CULL_NONE / MTR_CULL_FRONT; a back face that is kept is
 *               rasterised with its second and third vertex exchanged
 * states: nprims entries, or NULL to go back to the reference state.  Takes effect for frames drawn afterwards.
 * mtr_files.h maps MT Framework state-object names to these (mtr_state_from_names). */
enum { MTR_BLEND_ALPHA = 0, MTR_BLEND_OFF = 1, MTR_BLEND_ADD = 2 };
enum { MTR_CULL_BACK = 0, MTR_CULL_NONE = 1, MTR_CULL_FRONT = 2 };
typedef struct mtr_prim_state {
    uint8_t blend, depth_write, depth_test, cull;
} mtr_prim_state;
int32_t mtr_model_set_prim_states(mtr_model *model, const mtr_prim_state *states, size_t nprims);
/* Model::set_parts_disp (src/model.rs:295-297) */
int32_t mtr_model_set_parts_disp(mtr_model *model, const uint8_t *parts_disp, size_t n);
/* bone palette for linear-blend skinning (build extension; n x 16 f32 column-major, n <= 256) */
int32_t mtr_model_set_palette(mtr_model *model, const float *mats, size_t n);
/* Skeletal poses (build extension, SPEC.md section 12): palettes formed on the GPU (k_pose) from one local matrix per joint,
 *     world_j = local_j (parent 255 or j: a root), else world_parent(j) * local_j;   palette_j = world_j * imat_j
 * bit for bit what mtr_rmodel_palette forms on the host.  mtr_model_create_from_files sets the file's skeleton (JointInfo
 * parent bytes, imats) when it is valid.  Every call below that fails (no skeleton, njoints not the skeleton's, ...)
 * returns MTR_E_INVALID and changes nothing: frames drawn afterwards render the previous state. */
/* parents[j]: 255 or j = a root, else < njoints; no cycles; 1 <= njoints <= 256; imats njoints x 16.  parents == NULL
 * clears it.  Set-up, not per frame: replacing a skeleton waits for the device. */
int32_t mtr_model_set_skeleton(mtr_model *model, const uint8_t *parents, const float *imats, size_t njoints);
/* palette formed on the GPU from a pose (njoints x 16, host memory, free on return); same frame semantics as
 * mtr_model_set_palette */
int32_t mtr_model_set_pose(mtr_model *model, const float *local_mats, size_t njoints);

/* ---- instance batch ("scheduler" submission): n instances of one model, each
 * with its own model matrix and (optionally) palette and albedo override, resident in HBM ---- */
int32_t mtr_batch_create(mtr_device *dev, mtr_model *model, size_t n, const float *model_mats,
                         const float *palettes /* n * npal * 16 or NULL */, size_t npal,
                         const int32_t *texture_override /* n entries or NULL */, mtr_batch **out);
void mtr_batch_destroy(mtr_batch *batch);
/* In-place updates.  A draw uses the matrices and palettes that were current when it was RECORDED, also when its frame is
 * re-run after a bin-queue overflow; every update writes a fresh version of the batch's buffers (a small ring that grows
 * only while frames hold every version: no allocation and no device-wide sync in steady state) and frames drawn afterwards
 * wait for that write.  The instance count and texture overrides are fixed at creation. */
/* new instance matrices (n x 16) and/or palettes (n x npal x 16, 1 <= npal <= 256) from host memory; NULL keeps that part */
int32_t mtr_batch_update(mtr_batch *batch, const float *model_mats, const float *palettes, size_t npal);
/* one pose per instance (n x njoints x 16 local matrices, host memory, free on return) through the model's skeleton;
 * afterwards the batch has npal = njoints */
int32_t mtr_batch_set_poses(mtr_batch *batch, const float *local_mats, size_t njoints);
/* the same from device memory (16-byte aligned): k_pose reads local_mats_dev in stream order on hip_stream (NULL = the
 * device's stream, which is NOT ordered with HIP's legacy null stream: a host whose work runs there passes a stream that
 * waits for it, as api.py does for torch's default stream); frames drawn afterwards wait for it; the caller may overwrite
 * the buffer with work queued later on that stream */
int32_t mtr_batch_set_poses_device(mtr_batch *batch, const float *local_mats_dev, size_t njoints, void *hip_stream);
/* test / debug hook: the batch's current palettes (n x npal x 16 floats; count = room in floats), after its pending
 * update has completed */
int32_t mtr_batch_read_palettes(mtr_batch *batch, float *out, size_t count);

/* ---- animation clips (build extension, SPEC.md section 14): palettes formed on the GPU (k_anim) from keyframes ----
 * An animation set belongs to a joint count and holds nclips >= 1 clips of uniformly spaced keys; a key is, per joint, a
 * translation, a rotation quaternion (x, y, z, w) and a scale.  keys: clip after clip, inside a clip key after key, inside
 * a key joint after joint (sum(nkeys) * njoints entries); flags: MTR_CLIP_* per clip, NULL = 0 for all.  The library copies.
 * An animation state says, for one instance: clip A at position x_a cross-faded by w (0 = A alone .. 1 = B alone) with clip
 * B at x_b.  Positions are in KEYS (seconds times the clip's key rate; a player, section 20 below, keeps them on the device); a LOOP clip wraps
 * them (the last key interpolates towards the first), any other clip holds its first / last key.  Clip indices are
 * clamped to nclips - 1, never rejected (device states cannot be validated; host and device paths agree); with w == 0
 * clip B is not read.  The local matrix of a joint is from_scale_rotation_translation of the interpolated key, the
 * palette is the skeleton's of section 12: bit for bit a binary32 model of section 14 followed by mtr_rmodel_palette.
 * Errors: MTR_E_INVALID, and nothing changes, for a NULL handle, njoints outside 1..256, nclips == 0, a clip without
 * keys (or more than 2^24), a model without skeleton, an animation set whose njoints is not the skeleton's or that
 * belongs to another device, a misaligned device pointer; MTR_E_UNSUPPORTED when the library was built without k_anim. */
#define MTR_CLIP_LOOP 1u
typedef struct mtr_anim mtr_anim;
typedef struct mtr_anim_key   { float t[3], pad0, q[4], s[3], pad1; } mtr_anim_key;      /* 48 bytes */
typedef struct mtr_anim_state { uint32_t clip_a, clip_b; float x_a, x_b, w; uint32_t pad; } mtr_anim_state; /* 24 bytes */
int32_t mtr_anim_create(mtr_device *dev, size_t njoints, size_t nclips, const uint32_t *nkeys, const uint32_t *flags,
                        const mtr_anim_key *keys /* sum(nkeys) * njoints, clip after clip */, mtr_anim **out);
/* may follow an animate call directly: the clip set is parked until the last kernel that reads it has run (no wait) */
void mtr_anim_destroy(mtr_anim *anim);
/* the model's palette from one state (host memory, free on return); same frame semantics as mtr_model_set_pose */
int32_t mtr_model_animate(mtr_model *model, mtr_anim *anim, const mtr_anim_state *state /* one, host */);
/* one state per instance (host memory, free on return); same frame semantics as mtr_batch_set_poses; afterwards the
 * batch has npal = njoints */
int32_t mtr_batch_animate(mtr_batch *batch, mtr_anim *anim, const mtr_anim_state *states /* n, host */);
/* the same from device memory: k_anim reads states_dev in stream order on hip_stream, with the rules of
 * mtr_batch_set_poses_device (NULL = the device's stream; the caller may overwrite the buffer with work queued later) */
int32_t mtr_batch_animate_device(mtr_batch *batch, mtr_anim *anim, const mtr_anim_state *states_dev /* 8-byte aligned */,
                                 void *hip_stream /* as mtr_batch_set_poses_device */);
/* test / debug hook: the local matrices of section 14 for n states, n * njoints * 16 floats to host memory */
int32_t mtr_anim_sample(mtr_anim *anim, const mtr_anim_state *states, size_t n, float *out_locals, size_t count);

/* ---- animation tracks (build extension, SPEC.md section 15): an animation set whose channel values come from tracks ----
 * A track set is an mtr_anim: mtr_model_animate, mtr_batch_animate, mtr_batch_animate_device, mtr_anim_sample and
 * mtr_anim_destroy take it with the same errors, frame semantics and parked destroy.  A clip has a length in TICKS
 * (1..65536) instead of a key count, and positions mean what they mean for a uniform clip of as many keys.  For every
 * clip, joint and channel (0 translation, 1 rotation, 2 scale) there is one track, described by tracks[(clip * njoints +
 * joint) * 3 + channel]: its keys are first .. first + count - 1 of times[] (u16 ticks) and values[] (four 16-bit words per
 * key).  Tracks may share keys.  Translation and scale keys are three u16 words, component = lo + word * step (the fourth
 * word is not read); rotation keys are four s16 words (x, y, z, w), component = max(word / 32767, -1) (lo and step are
 * not read).  Between two keys the channel is interpolated as section 14 interpolates between keys; past a track's last
 * key a LOOP clip interpolates towards the track's first key at tick nticks, any other clip holds the last key.  The
 * library copies every array.
 * Errors: MTR_E_INVALID, nothing is created and *out is NULL, for a NULL argument (flags may be NULL = 0), njoints outside
 * 1..256, nclips == 0, nkeys_total == 0 or above 2^31 - 1, a clip length outside 1..65536, and a track with count == 0,
 * first + count > nkeys_total, times[first] != 0, times that do not strictly increase, or a last time above nticks - 1;
 * mtr_last_error names the clip, joint and channel.  lo and step are not validated (any float, as section 14's keys).
 * MTR_E_UNSUPPORTED from the animate calls when the library was built without the track kernels. */
typedef struct mtr_anim_track { uint32_t first, count; float lo[3], step[3]; } mtr_anim_track;   /* 32 bytes */
int32_t mtr_anim_create_tracks(mtr_device *dev, size_t njoints, size_t nclips, const uint32_t *nticks,
                               const uint32_t *flags /* NULL = 0 */, const mtr_anim_track *tracks /* nclips*njoints*3 */,
                               const uint16_t *times, const uint16_t *values /* 4 per key */, size_t nkeys_total,
                               mtr_anim **out);

/* ---- animation layers (build extension, SPEC.md section 16): a stack of up to 8 layers per instance over one set ----
 * A layer names a clip of the animation set (of either kind), a position x in it (section 14 / 15), a weight w, a per-joint
 * mask and a mode.  Layer 0 is the base: the pose of its clip at x; its w, mask and mode are not read.  Every further layer
 * is blended over the result so far, joint by joint, by e = clamp(w) * mask[joint]: MTR_LAYER_OVERRIDE cross-fades towards
 * the layer's pose as section 14 cross-fades clip A towards clip B; MTR_LAYER_ADDITIVE takes the layer's clip as deltas
 * from a reference pose (translation added, rotation multiplied on the right, scale multiplied; mt_renderer_amd/
 * anim_layers.py makes such clips) and applies e of them.  Where e == 0 the joint is left as it is, bit for bit, and the
 * layer's clip is not read.  Two layers with mask 0 and OVERRIDE are section 14's cross-fade, bit for bit.
 * A mask set belongs to a joint count and holds nmasks >= 1 masks of njoints weights in [0, 1] (mask after mask; the
 * library copies); a layer's mask index 0 is the built-in mask "every joint 1.0", 1..nmasks are the set's.  Clip and mask
 * indices are clamped (to nclips - 1, to nmasks, to 0 without a mask set), never rejected; only bit 0 of mode is read.
 * Every instance of a call has the same number of layers, contiguous per instance: layers[inst * nlayers + l].
 * Errors: MTR_E_INVALID, and nothing changes, for a NULL handle or pointer (masks may be NULL: every mask index is 0),
 * nlayers outside 1..MTR_ANIM_MAX_LAYERS, njoints outside 1..256, nmasks == 0 or above 65535, a weight that is NaN or
 * outside [0, 1] (mtr_last_error names the mask and the joint), a mask set whose njoints is not the skeleton's or that
 * belongs to another device, everything the animate calls of section 14 reject, a misaligned device pointer;
 * MTR_E_UNSUPPORTED when the library was built without the layer kernels. */
#define MTR_ANIM_MAX_LAYERS 8
#define MTR_LAYER_OVERRIDE 0u
#define MTR_LAYER_ADDITIVE 1u
typedef struct mtr_anim_masks mtr_anim_masks;
typedef struct mtr_anim_layer { uint32_t clip; float x, w; uint16_t mask, mode; } mtr_anim_layer;   /* 16 bytes */
int32_t mtr_anim_masks_create(mtr_device *dev, size_t njoints, size_t nmasks, const float *weights /* nmasks*njoints */,
                              mtr_anim_masks **out);
/* may follow an animate call directly: parked like mtr_anim_destroy */
void mtr_anim_masks_destroy(mtr_anim_masks *masks);
/* the model's palette from one layer stack (host memory, free on return); frame semantics of mtr_model_animate */
int32_t mtr_model_animate_layers(mtr_model *model, mtr_anim *anim, mtr_anim_masks *masks /* or NULL */,
                                 const mtr_anim_layer *layers /* nlayers, host */, size_t nlayers);
/* one layer stack per instance (host memory, free on return); frame semantics of mtr_batch_animate */
int32_t mtr_batch_animate_layers(mtr_batch *batch, mtr_anim *anim, mtr_anim_masks *masks /* or NULL */,
                                 const mtr_anim_layer *layers /* n*nlayers, host */, size_t nlayers);
/* the same from device memory, read in stream order on hip_stream with the rules of mtr_batch_animate_device */
int32_t mtr_batch_animate_layers_device(mtr_batch *batch, mtr_anim *anim, mtr_anim_masks *masks /* or NULL */,
                                        const mtr_anim_layer *layers_dev /* 16-byte aligned */, size_t nlayers,
                                        void *hip_stream /* as mtr_batch_set_poses_device */);
/* test / debug hook: the local matrices of section 16 for n layer stacks, n * njoints * 16 floats to host memory */
int32_t mtr_anim_sample_layers(mtr_anim *anim, mtr_anim_masks *masks /* or NULL */, const mtr_anim_layer *layers,
                               size_t nlayers, size_t n, float *out_locals, size_t count);

/* ---- inverse kinematics (build extension, SPEC.md section 17): two-bone reach and aim after the layer stack ----
 * An IK set belongs to a skeleton: it holds the skeleton's parents (the rules of mtr_model_set_skeleton) and 1..4 chains.
 * After the layer stack of section 16 has given every joint its (translation, rotation, scale), the chains are evaluated
 * in order on the GPU, each against one target per instance, before the skeleton is folded; a later chain sees what an
 * earlier one changed.  MTR_IK_TWO_BONE: joint = (a, b, c), b the child of a and c the child of b; the rotations of a and
 * b are changed so that c reaches pos (clamped to what the two bones can reach), bending in the plane the pose already
 * has or, with MTR_IK_POLE, towards pole.  MTR_IK_AIM: the rotation of joint[0] is changed so that axis (in the joint's
 * own space) points at pos; joint[1..2] and MTR_IK_POLE are not read.  Only rotations change.  pos and pole are in the
 * instance's model space (the space of the world matrices of section 12, before the instance matrix).  w blends from the
 * animated rotation (0) to the solved one (1), clamped as a cross-fade weight (NaN -> 0); at w == 0 the chain changes
 * nothing, bit for bit, and reads no other field of its target.  A chain that cannot be solved (a bone or the distance
 * of length 0, a NaN target, an infinite target of a TWO_BONE chain, a pole or a limb on the line to the target) changes
 * nothing either; an infinite target of an AIM chain has no direction and gives a defined rotation without a meaning.
 * The solve reads rotations above a and ignores their scales: it is exact under ancestors of uniform positive scale.
 * Every instance of a call has nchains targets, contiguous per instance: targets[inst * nchains + k].
 * Errors: MTR_E_INVALID, and nothing changes, for everything the layered calls reject, a NULL IK set or NULL targets, an
 * IK set of another device or joint count or whose parents differ from the model's skeleton (mtr_last_error names the
 * first joint), and misaligned device targets; at creation for njoints outside 1..256, invalid parents, nchains outside
 * 1..MTR_ANIM_MAX_IK, a kind other than 0 or 1, unknown flag bits, a joint >= njoints, a TWO_BONE chain whose joints are
 * not a, its child and that child's child, an AIM axis that is not finite or all zero (mtr_last_error names the chain).
 * MTR_E_UNSUPPORTED when the library was built without the IK kernels. */
#define MTR_ANIM_MAX_IK 4
#define MTR_IK_TWO_BONE 0u
#define MTR_IK_AIM 1u
#define MTR_IK_POLE 1u
typedef struct mtr_anim_ik mtr_anim_ik;
typedef struct mtr_ik_chain  { uint32_t kind, joint[3]; float axis[3]; uint32_t flags; } mtr_ik_chain;   /* 32 bytes */
typedef struct mtr_ik_target { float pos[3], w, pole[3]; uint32_t pad; } mtr_ik_target;                  /* 32 bytes */
int32_t mtr_anim_ik_create(mtr_device *dev, size_t njoints, const uint8_t *parents, size_t nchains,
                           const mtr_ik_chain *chains, mtr_anim_ik **out);
/* may follow an animate call directly: parked like mtr_anim_destroy */
void mtr_anim_ik_destroy(mtr_anim_ik *ik);
/* the model's palette from one layer stack and nchains targets (host memory, free on return); frame semantics of
 * mtr_model_animate_layers */
int32_t mtr_model_animate_ik(mtr_model *model, mtr_anim *anim, mtr_anim_masks *masks /* or NULL */,
                             const mtr_anim_layer *layers /* nlayers, host */, size_t nlayers, mtr_anim_ik *ik,
                             const mtr_ik_target *targets /* nchains, host */);
/* one layer stack and nchains targets per instance (host memory, free on return); frame semantics of mtr_batch_animate */
int32_t mtr_batch_animate_ik(mtr_batch *batch, mtr_anim *anim, mtr_anim_masks *masks /* or NULL */,
                             const mtr_anim_layer *layers /* n*nlayers, host */, size_t nlayers, mtr_anim_ik *ik,
                             const mtr_ik_target *targets /* n*nchains, host */);
/* the same from device memory, read in stream order on hip_stream with the rules of mtr_batch_animate_device */
int32_t mtr_batch_animate_ik_device(mtr_batch *batch, mtr_anim *anim, mtr_anim_masks *masks /* or NULL */,
                                    const mtr_anim_layer *layers_dev /* 16-byte aligned */, size_t nlayers, mtr_anim_ik *ik,
                                    const mtr_ik_target *targets_dev /* 16-byte aligned */,
                                    void *hip_stream /* as mtr_batch_set_poses_device */);
/* test / debug hook: the local matrices of section 17 for n layer stacks and n * nchains targets, to host memory */
int32_t mtr_anim_sample_ik(mtr_anim *anim, mtr_anim_masks *masks /* or NULL */, mtr_anim_ik *ik, const mtr_anim_layer *layers,
                           size_t nlayers, const mtr_ik_target *targets, size_t n, float *out_locals, size_t count);

/* ---- attachments (build extension, SPEC.md section 18): instance matrices from another batch's joints (k_attach) ----
 * An object rigidly attached to joint j of instance s of a source batch is a vertex skinned to j with weight 1, so its
 * instance matrix is M_src[s] * palette[s][j] * offset, offset being where the object sits in the source model's BIND
 * space (inverse(imat_j) * a placement relative to the joint; in Python, mt_renderer_amd/attach.py: bind_offsets).  One
 * record per instance of the attached batch:
 *   src_instance, joint : clamped to the source's instance and palette counts, never rejected; joint ==
 *                         MTR_ATTACH_NO_JOINT (or a source without palettes) follows the source instance's matrix alone;
 *   flags               : bit 0, MTR_ATTACH_POSITION_ONLY: the object follows the joint's position and keeps the orientation
 *                         and scale of its offset (name tags, blob shadows); the other bits and pad are not read.
 * The products are section 12's fma chain, (M_src * palette) * offset in that association, so a numpy model reproduces
 * the matrices bit for bit.
 * Every attach call is ONE SHOT, like every animate call: it reads the source's CURRENT version (waiting, on the device,
 * for that version's pending write: an animate call just before it) and writes a fresh version of `batch` whose
 * instance matrices are the kernel's; the batch's palettes and npal are kept.  Frames drawn afterwards wait for it; a
 * draw uses what was current when it was recorded.  The source is not tied to the batch: animate the source again and
 * attach again.  batch == src is allowed (instance 3 rides instance 0 of the same batch): the call reads the current
 * version and writes a fresh one.  A chain of attachments is the host's call order: attach the rider to the mount, then
 * the sword to the rider.  The source may be updated or destroyed directly after the call: the version the kernel reads
 * is kept until the kernel has run (no host wait).  Sources are batches on the same device; a single character drawn
 * with mtr_frame_draw_model is not one -- make it a batch of one.
 * MTR_E_INVALID, nothing changed: a NULL handle or pointer, src on another device, a misaligned device pointer, n == 0 or
 * n > 2^27 or count < n * 16 for the socket calls.  MTR_E_UNSUPPORTED: a library built without k_attach. */
#define MTR_ATTACH_NO_JOINT      0xFFFFFFFFu
#define MTR_ATTACH_POSITION_ONLY 1u
typedef struct mtr_attach { uint32_t src_instance, joint, flags, pad; float offset[16]; } mtr_attach;   /* 80 bytes */
/* one record per instance of batch (host memory, free on return) */
int32_t mtr_batch_attach(mtr_batch *batch, mtr_batch *src, const mtr_attach *recs /* batch's n, host */);
/* the same from device memory, read in stream order on hip_stream with the rules of mtr_batch_set_poses_device */
int32_t mtr_batch_attach_device(mtr_batch *batch, mtr_batch *src, const mtr_attach *recs_dev /* 16-byte aligned */,
                                void *hip_stream /* as mtr_batch_set_poses_device */);
/* the matrices alone, for the host's own use (emitters, hit boxes): n records against src's current version, n x 16 floats
 * out.  Host memory; waits for the result */
int32_t mtr_batch_sockets(mtr_batch *src, const mtr_attach *recs, size_t n, float *out, size_t count /* >= n * 16 */);
/* device memory (both 16-byte aligned), in stream order on hip_stream; no wait */
int32_t mtr_batch_sockets_device(mtr_batch *src, const mtr_attach *recs_dev, size_t n, float *out_dev,
                                 void *hip_stream /* as mtr_batch_set_poses_device */);
/* test / debug hook next to mtr_batch_read_palettes: the batch's current instance matrices (n x 16 floats; count = room in
 * floats), after its pending update has completed */
int32_t mtr_batch_read_model_mats(mtr_batch *batch, float *out, size_t count);

/* ---- root motion (build extension, SPEC.md section 19): clips move their instances (k_root) ----
 * A trajectory is joint `joint` of an ordinary animation set of either kind (uniform keys or tracks; any joint count, 1 is
 * usual; none of its clips may carry MTR_CLIP_LOOP; scale is not read).  A root set belongs to such a set's (njoints,
 * nclips) and holds the joint and one flag word per clip: MTR_ROOT_CYCLIC makes key N - 1 the end of the cycle, where the
 * next cycle's key 0 stands (period N - 1).  Per instance and call there are nsteps (1..MTR_ROOT_MAX_STEPS) steps:
 *   clip  : clamped to the set's clip count, never rejected;
 *   x, dx : the rigid delta of the trajectory joint between position x and x + dx (in keys / ticks), across one cycle seam
 *           where needed; a step that would cross a second seam, a NaN or an infinite dx move nothing;
 *   w     : steps 1 .. nsteps - 1 are blended over step 0 in order by their clamped weight, as section 16's OVERRIDE layers
 *           (a cross-fade of walk into run); step 0's w is not read, and a step of weight 0 does not read its clip.
 * The blended delta D is a local matrix of section 14 and M_new[i] = M_old[i] * D_i in section 12's fma chain, so a numpy
 * model reproduces the matrices bit for bit.  These calls define no clock: the host advances x by dx itself, or a player
 * (section 20, below) writes the steps.
 * mtr_batch_root_motion* is ONE SHOT with the frame semantics of mtr_batch_attach with batch == src: it reads the batch's
 * current version (after its pending write) and writes a fresh one; palettes and npal are kept; a draw uses what was current
 * when it was recorded.  The batch's model needs no skeleton.  A mount moved this way and then mtr_batch_attach carries its
 * rider.  The trajectory set and the root set may be destroyed directly after the call (no host wait).
 * MTR_E_INVALID, nothing changed: a NULL handle or pointer, nsteps outside 1..8, joint >= njoints, unknown flag bits
 * (mtr_last_error names the clip), a root set whose (njoints, nclips) or device is not the trajectory set's, a trajectory set
 * with a LOOP clip, a misaligned device pointer, n == 0 or n > 2^27 or count < n * 16 for the delta calls.
 * MTR_E_UNSUPPORTED: a library built without k_root. */
#define MTR_ROOT_MAX_STEPS 8
#define MTR_ROOT_CYCLIC 1u
typedef struct mtr_anim_root mtr_anim_root;
typedef struct mtr_root_step { uint32_t clip; float x, dx, w; } mtr_root_step;   /* 16 bytes */
int32_t mtr_anim_root_create(mtr_device *dev, size_t njoints, size_t nclips, uint32_t joint,
                             const uint32_t *flags /* nclips, NULL = 0 */, mtr_anim_root **out);
void    mtr_anim_root_destroy(mtr_anim_root *root);      /* parked like mtr_anim_destroy */
/* nsteps steps per instance of batch, steps[inst * nsteps + i] (host memory, free on return) */
int32_t mtr_batch_root_motion(mtr_batch *batch, mtr_anim *traj, mtr_anim_root *root, const mtr_root_step *steps /* n*nsteps, host */,
                              size_t nsteps);
/* the same from device memory, read in stream order on hip_stream with the rules of mtr_batch_set_poses_device */
int32_t mtr_batch_root_motion_device(mtr_batch *batch, mtr_anim *traj, mtr_anim_root *root,
                                     const mtr_root_step *steps_dev /* 16-byte aligned */, size_t nsteps,
                                     void *hip_stream /* as mtr_batch_set_poses_device */);
/* the deltas alone (character controllers, collision): n x 16 floats; the host version waits, the device version does not */
int32_t mtr_anim_root_deltas(mtr_anim *traj, mtr_anim_root *root, const mtr_root_step *steps, size_t nsteps, size_t n, float *out,
                             size_t count /* >= n * 16 */);
int32_t mtr_anim_root_deltas_device(mtr_anim *traj, mtr_anim_root *root, const mtr_root_step *steps_dev, size_t nsteps, size_t n,
                                    float *out_dev /* 16-byte aligned */, void *hip_stream);

/* ---- players (build extension, SPEC.md section 20): a clock that keeps playback states on the device (k_play) ----
 * Sections 14 to 19 take positions and define no clock; a player is the clock.  A player set holds per clip the key count
 * (or tick count of a track set), the flag word (MTR_CLIP_LOOP) and the rate in positions per second, and owns a zeroed
 * scratch array of max_instances words.  It is not tied to an mtr_anim: the same tables drive an in-place set and its
 * trajectory set, clip by clip (a LOOP clip of N keys and its cyclic trajectory of N + 1 keys share the period N).
 * A play state is 32 bytes per instance in DEVICE memory, read and written by every advance:
 *   clip_a, x_a : what plays; clip_b, x_b : what a running fade leads to; w : the fade's weight; fade : weight per second,
 *   a fade is running iff fade > 0; speed : multiplies dt, never written; flags : bit 0 MTR_PLAY_ENDED is written by the
 *   kernel (a one-shot clip_a stands at its end), bits 1..31 are the user's and are kept.
 * The user may write states directly; every bit pattern has a defined outcome and clip indices are clamped.
 * A command {instance, clip, x, seconds} starts clip at x on one instance: a cut unless seconds > 0 and 1 / seconds is
 * positive and finite, else a cross-fade of that duration (a running fade past half its weight first becomes the base).
 * instance >= n is ignored; of several commands to one instance the LAST in array order wins, the others have no effect.
 * An advance moves every state by dt seconds (positions by dt * speed * rate, wrapped on a LOOP clip, clamped otherwise;
 * the weight by max(dt, 0) * fade; a complete fade swaps B into A) and writes, each pointer optional, the records of the
 * frame BEFORE the swap: an mtr_anim_state per instance; layers 0 and 1 of a stack of nlayers (2..8) mtr_anim_layer per
 * instance, the others untouched; two mtr_root_step per instance (x before the advance, and the step).  They are what
 * mtr_batch_animate_device, mtr_batch_animate_layers_device / _ik_device and mtr_batch_root_motion_device (nsteps = 2) take.
 * Both advance calls run in stream order on hip_stream under the rules of mtr_batch_set_poses_device; host commands are
 * copied before the call returns, device commands may be overwritten by work queued later.  Calls on one player are
 * ordered among themselves whatever their streams.  mtr_anim_player_destroy may follow an advance directly (no host wait).
 * MTR_E_INVALID, nothing changed: a NULL handle or states pointer, n == 0 or n > max_instances, nlayers outside 2..8 with
 * out_layers given, a misaligned device pointer (16 bytes: states, layers, steps, commands; 8: mtr_anim_state), ncmds > 0
 * with NULL commands, ncmds >= 2^31; at creation nclips == 0 or > 2^24, nkeys outside 1..2^24, unknown flag bits, a rate
 * that is not finite (mtr_last_error names the clip), max_instances outside 1..2^27.
 * MTR_E_UNSUPPORTED: a library built without k_play. */
#define MTR_PLAY_ENDED 1u
typedef struct mtr_anim_player mtr_anim_player;
typedef struct mtr_play_state { uint32_t clip_a, clip_b; float x_a, x_b, w, fade, speed; uint32_t flags; } mtr_play_state; /* 32 bytes */
typedef struct mtr_play_cmd { uint32_t instance, clip; float x, seconds; } mtr_play_cmd;                                   /* 16 bytes */
int32_t mtr_anim_player_create(mtr_device *dev, size_t nclips, const uint32_t *nkeys /* nclips */,
                               const uint32_t *flags /* nclips, NULL = 0 */, const float *rates /* nclips */,
                               size_t max_instances, mtr_anim_player **out);
void    mtr_anim_player_destroy(mtr_anim_player *player);    /* parked like mtr_anim_destroy */
int32_t mtr_anim_player_advance_device(mtr_anim_player *player, mtr_play_state *states_dev /* n, 16-byte aligned */, size_t n,
                                       float dt, const mtr_play_cmd *cmds /* ncmds, host, or NULL */, size_t ncmds,
                                       mtr_anim_state *out_states_dev /* n, or NULL */,
                                       mtr_anim_layer *out_layers_dev /* n*nlayers, or NULL */, size_t nlayers,
                                       mtr_root_step *out_steps_dev /* n*2, or NULL */,
                                       void *hip_stream /* as mtr_batch_set_poses_device */);
/* the same with the commands in device memory (16-byte aligned), read in stream order */
int32_t mtr_anim_player_advance_device_cmds(mtr_anim_player *player, mtr_play_state *states_dev, size_t n, float dt,
                                            const mtr_play_cmd *cmds_dev, size_t ncmds, mtr_anim_state *out_states_dev,
                                            mtr_anim_layer *out_layers_dev, size_t nlayers, mtr_root_step *out_steps_dev,
                                            void *hip_stream);
/* a test and debug hook: everything in host memory (any alignment), the same kernel, waits; states are read and written
 * back, out_layers is read first so that layers 2.. come back as they went in */
int32_t mtr_anim_player_advance_host(mtr_anim_player *player, mtr_play_state *states /* n, host, in and out */, size_t n, float dt,
                                     const mtr_play_cmd *cmds, size_t ncmds, mtr_anim_state *out_states,
                                     mtr_anim_layer *out_layers, size_t nlayers, mtr_root_step *out_steps);

/* ---- controllers (build extension, SPEC.md section 21): per-instance state machines that decide what plays (k_ctrl) ----
 * A player takes commands; a controller writes them on the device.  It is a graph shared by all instances: nodes, each
 * with a clip and a range [first, first + count) of its own transitions, and transitions, the first nany of which are
 * any-state transitions that every node tries first.  A transition has a target node, flags, the seconds and x of the
 * command it issues, and up to 3 conditions `v op value`, v being a user parameter (param < nparams) or a built-in:
 *   MTR_CTRL_TIME seconds in the node; MTR_CTRL_POS, MTR_CTRL_PHASE the position of what plays and position / period;
 *   MTR_CTRL_ENDED 1.0 where a one-shot clip stands at its end; MTR_CTRL_FADING 1.0 while a fade runs.
 * "What plays" is clip B while a fade runs (fade > 0), clip A otherwise.  Per instance there are 16 bytes of state
 * (node; t, seconds since the node was entered; fired, the transition of the last step or MTR_CTRL_NONE; user, kept) and a
 * row of nparams floats, both in DEVICE memory and free for the user to write: every bit pattern has a defined outcome.
 * A step tries, per instance, transitions 0..nany-1 and then the node's own, in array order, and fires the first that is
 * not skipped (a fade runs and it lacks INTERRUPT; an any-state transition whose target is the current node and that lacks
 * SELF) and whose conditions all hold (NaN compares false, NE is true against NaN, no conditions always pass).  Firing writes
 * command slot i = {i, clip of the target, x (with SYNC: phase of what plays times the target clip's period), seconds},
 * enters the target with t = 0, with CONSUME stores 0 into the user parameters its conditions name, and adds 1 to
 * counts[transition] when counts is given (never cleared by the call).  Otherwise slot i = {0xFFFFFFFF, 0, 0, 0}, which a
 * player ignores, and t += max(dt, 0).  The play states are read and never written.  Pass the n slots as cmds_dev, ncmds = n
 * to the next mtr_anim_player_advance_device_cmds; a host that overrules the controller appends its commands behind slot
 * n - 1 (the last in array order wins) and writes state.node itself.
 * nkeys and clip_flags are what mtr_anim_player_create was given; the controller makes the same periods from them and is
 * not tied to a player handle.  Its tables are immutable.  A step runs in stream order on hip_stream under the rules of
 * mtr_batch_set_poses_device; mtr_anim_ctrl_destroy may follow a step directly (no host wait).
 * MTR_E_INVALID, nothing created (mtr_last_error names the clip, node or transition): nclips == 0 or > 2^24, nkeys outside
 * 1..2^24, clip flag bits other than MTR_CLIP_LOOP, nnodes outside 1..65535, ntrans > 2^20, nany > ntrans, nparams > 16, a
 * NULL array that is counted; a node whose clip >= nclips or whose range leaves [nany, ntrans] (count == 0 is allowed); a
 * transition whose target >= nnodes, with unknown flag bits or ncond > 3; a used condition whose op > 5 or whose param is
 * neither < nparams nor a built-in.  seconds, x and value are any floats.
 * MTR_E_INVALID, nothing changed, at a step: a NULL handle, states, play or cmds pointer, n == 0 or n > 2^27, NULL params with
 * nparams > 0, a misaligned device pointer (16 bytes: states, play, cmds; 4: params, counts).
 * MTR_E_UNSUPPORTED: a library built without k_ctrl. */
#define MTR_CTRL_MAX_COND 3
enum { MTR_OP_LT, MTR_OP_LE, MTR_OP_GT, MTR_OP_GE, MTR_OP_EQ, MTR_OP_NE };          /* 0..5 */
#define MTR_TR_INTERRUPT 1u   /* may fire while a fade runs */
#define MTR_TR_SELF      2u   /* an any-state transition may target the current node */
#define MTR_TR_SYNC      4u   /* start the target at the phase of what plays */
#define MTR_TR_CONSUME   8u   /* firing clears the user parameters its conditions name */
#define MTR_CTRL_TIME   0xFFFFu  /* built-in "parameters" a condition may name */
#define MTR_CTRL_POS    0xFFFEu
#define MTR_CTRL_PHASE  0xFFFDu
#define MTR_CTRL_ENDED  0xFFFCu
#define MTR_CTRL_FADING 0xFFFBu
#define MTR_CTRL_NONE   0xFFFFFFFFu
typedef struct mtr_anim_ctrl mtr_anim_ctrl;
typedef struct mtr_ctrl_node  { uint32_t clip, first, count, pad; } mtr_ctrl_node;                 /* 16 bytes */
typedef struct mtr_ctrl_cond  { uint16_t param, op; float value; } mtr_ctrl_cond;                  /*  8 bytes */
typedef struct mtr_ctrl_trans { uint32_t target, flags; float seconds, x; uint32_t ncond, pad;
                                mtr_ctrl_cond cond[MTR_CTRL_MAX_COND]; } mtr_ctrl_trans;           /* 48 bytes */
typedef struct mtr_ctrl_state { uint32_t node; float t; uint32_t fired, user; } mtr_ctrl_state;    /* 16 bytes */
int32_t mtr_anim_ctrl_create(mtr_device *dev, size_t nclips, const uint32_t *nkeys /* nclips */,
                             const uint32_t *clip_flags /* nclips, NULL = 0 */, const mtr_ctrl_node *nodes, size_t nnodes,
                             const mtr_ctrl_trans *trans, size_t ntrans, size_t nany, size_t nparams, mtr_anim_ctrl **out);
void    mtr_anim_ctrl_destroy(mtr_anim_ctrl *ctrl);          /* parked like mtr_anim_destroy */
int32_t mtr_anim_ctrl_step_device(mtr_anim_ctrl *ctrl, mtr_ctrl_state *states_dev /* n, 16-byte aligned */,
                                  const mtr_play_state *play_dev /* n, 16-byte aligned */,
                                  float *params_dev /* n*nparams, or NULL when nparams == 0 */, size_t n, float dt,
                                  mtr_play_cmd *cmds_out_dev /* n, 16-byte aligned */,
                                  uint32_t *counts_dev /* ntrans, or NULL */, void *hip_stream);
/* a test and debug hook: everything in host memory (any alignment), the same kernel, waits; states, params and counts are
 * read and written back */
int32_t mtr_anim_ctrl_step_host(mtr_anim_ctrl *ctrl, mtr_ctrl_state *states, const mtr_play_state *play, float *params, size_t n,
                                float dt, mtr_play_cmd *cmds_out, uint32_t *counts);

/* ---- animation events (build extension, SPEC.md section 22): markers on clips fire into a device list (k_events) ----
 * The return channel of the players: which markers did each instance arrive at or pass this frame (a footstep, the hit frame
 * of an attack, the end of a one-shot).  An event set holds per clip count_c >= 0 markers {x, id}, clip after clip in one
 * array, x non-decreasing within a clip (ties keep array order), id any word.  nkeys and clip_flags are what
 * mtr_anim_player_create was given; the set makes the same periods P from them and is not tied to a player handle.  It owns
 * a scratch array of ceil(max_instances / 256) words, so calls on one set are ordered among themselves whatever their streams.
 * A collect call reads nsteps (1..8) mtr_root_step per instance, steps[inst * nsteps + i]: exactly what a player's advance
 * writes into out_steps_dev (nsteps = 2) and mtr_batch_root_motion_device reads.  Every bit pattern has a defined outcome
 * and the clip index is clamped.  Per step:
 *   weight    : E_i = e_i * (1 - e_{i+1}) * ... * (1 - e_{nsteps-1}), e_0 = 1 and e_i the clamped w of step i: the share the
 *               step's clip has in the blend.  A step i >= 1 with e_i == 0 fires nothing; a step fires only if
 *               E_i >= min_weight (0 lets everything else through, NaN nothing).
 *   direction : dx > 0 forward, dx < 0 backward, anything else fires nothing.  A marker fires when the position arrives at
 *               it or passes it, not when it leaves it: forward over (a, b] in array order, backward over [b, a) in reverse.
 *   one-shot  : a and b are x and x + dx clamped to [0, P], so a marker at P fires once on arrival.
 *   LOOP      : x is wrapped into [0, P) first; across the seam the markers behind the start fire, then those up to where
 *               the player lands; |dx| >= P fires every marker of the clip once.
 * Consecutive frames of a player abut: a marker fires exactly once per passage.  A clip started AT a marker does not fire it.
 * The list holds mtr_anim_event {instance, id, where, w}: where = clip | step << 24 | MTR_EVENT_BACKWARD, w = E_i; ordered
 * by instance, then step, then firing order, whichever thread ran first.  count_dev[0] = events fired, count_dev[1] =
 * min(count_dev[0], capacity) records written, the first in that order; a longer list is truncated, not an error, and the
 * list behind count_dev[1] is untouched.  bits_dev (optional) takes per instance the OR of 1u << (id & 31) over its fired
 * events, written (not OR-ed into) for every instance on every call, whatever capacity is.
 * The call runs in stream order on hip_stream under the rules of mtr_batch_set_poses_device;
 * mtr_anim_events_destroy may follow a call directly (no host wait).
 * MTR_E_INVALID, nothing created (mtr_last_error names the clip and the marker): a NULL device, out or nkeys pointer,
 * nclips == 0 or > 2^24, nkeys outside 1..2^24, clip flag bits other than MTR_CLIP_LOOP, max_instances outside 1..2^27, more
 * than 2^24 markers in all, NULL counts or markers with a marker counted; a marker whose x is not finite, is negative, lies
 * above P (on a LOOP clip: at or above P) or below the marker before it in its clip.
 * MTR_E_INVALID, nothing changed, at a call: a NULL handle, steps or count pointer, nsteps outside 1..8, n == 0 or
 * n > max_instances, capacity > 0 with a NULL list, a misaligned device pointer (16 bytes: steps, list; 4: count, bits),
 * n * nsteps * (the largest count_c) > 2^32 - 1, a capacity of 2^32 or more at the host hook.
 * MTR_E_UNSUPPORTED: a library built without k_events. */
#define MTR_EVENT_BACKWARD 0x80000000u   /* in mtr_anim_event::where */
typedef struct mtr_anim_events mtr_anim_events;
typedef struct mtr_event_marker { float x; uint32_t id; } mtr_event_marker;                        /*  8 bytes */
typedef struct mtr_anim_event { uint32_t instance, id, where; float w; } mtr_anim_event;           /* 16 bytes */
int32_t mtr_anim_events_create(mtr_device *dev, size_t nclips, const uint32_t *nkeys /* nclips */,
                               const uint32_t *clip_flags /* nclips, NULL = 0 */, const uint32_t *counts /* nclips, NULL = 0 */,
                               const mtr_event_marker *markers /* sum of counts */, size_t max_instances,
                               mtr_anim_events **out);
void    mtr_anim_events_destroy(mtr_anim_events *ev);        /* parked like mtr_anim_destroy */
int32_t mtr_anim_events_collect_device(mtr_anim_events *ev, const mtr_root_step *steps_dev /* n*nsteps, 16-byte aligned */,
                                       size_t nsteps, size_t n, float min_weight,
                                       mtr_anim_event *out_dev /* capacity, 16-byte aligned, or NULL */, size_t capacity,
                                       uint32_t *count_dev /* 2 words */, uint32_t *bits_dev /* n, or NULL */,
                                       void *hip_stream);
/* a test and debug hook: everything in host memory (any alignment), the same kernels, waits; the list and bits are read
 * first so that what the kernels leave untouched comes back as it went in */
int32_t mtr_anim_events_collect_host(mtr_anim_events *ev, const mtr_root_step *steps, size_t nsteps, size_t n, float min_weight,
                                     mtr_anim_event *out, size_t capacity, uint32_t *count, uint32_t *bits);

/* ---- blend spaces (build extension, SPEC.md section 23): parameters mix phase-locked clips (k_blend) ----
 * Plays a character AT a speed or IN a direction: sample points in a 1-D or 2-D parameter space each carry a LOOP clip, and
 * one call per frame turns one or two floats per instance into the layers and steps the animate, root-motion and event calls
 * take.  A blend set holds the clips (nkeys, clip_flags, rates as mtr_anim_player_create takes them; it is not tied to a
 * player or an mtr_anim), K = 1..32 samples {clip, px, py} and T = 0..64 triangles of sample indices.  T == 0 is a 1-D space
 * over px (strictly increasing); T >= 1 a 2-D space whose triangles are counter-clockwise: the doubled area
 * (x1-x0)*(y2-y0) - (x2-x0)*(y1-y0), in binary32 in that order, is finite and > 0 (mt_renderer_amd/anim_blend.py triangulates
 * a point set).  param_x / param_y name the floats of an instance's row params[inst * nparams + p] (a controller's rows),
 * damp is the smoothing rate in 1/seconds (+inf: none).
 * The state is mtr_blend_state {phase, px, py, speed}, 16 bytes in device memory; speed is never written, and every bit
 * pattern has a defined outcome.  Per instance and call:
 *   smooth : a = clamp(max(dt, 0) * damp); px' = px + a * (target - px), or the target itself when a == 1 or the stored px
 *            is not finite (so a NaN parameter heals); py likewise in 2-D.
 *   slots  : three sample indices and two sequential weights e1, e2 (e0 = +0).  1-D: at or below the first sample
 *            (0, 0, 0), at or above the last (K-1, K-1, K-1), else (j, j+1, j) with e1 = (p - px[j]) / (px[j+1] - px[j]).
 *            2-D: the first triangle in array order whose barycentric l0, l1, l2 are all >= 0: (v0, v1, v2), e2 = l2,
 *            e1 = l1 / (1 - l2); where none holds the point (outside the hull, a rounding crack, a NaN) the closest point on
 *            any edge (a, b): (a, b, a), e1 = t.  The shares E0 = (1-e1)(1-e2), E1 = e1(1-e2), E2 = e2 are the barycentric
 *            weights and what section 22 calls E_i.
 *   phase  : one phase in [0, 1) for all three clips, advanced by dt * speed * f, f the rates over the periods blended with
 *            e1, e2, and wrapped; a stored phase outside [0, 1) counts as 0.
 *   out    : layer i = {clip_i, phase' * P_i, e_i, mask 0, OVERRIDE} for i = 0..2 of nlayers (3..8) per instance, layers 3..
 *            untouched; step i = {clip_i, phase * P_i, dphase * P_i, e_i} (three per instance: nsteps = 3 for
 *            mtr_batch_root_motion_device and mtr_anim_events_collect_device); optionally the three shares.
 * Steps of consecutive frames abut only to within a unit in the last place of the position (SPEC.md section 23).
 * The call runs in stream order on hip_stream under the rules of mtr_batch_set_poses_device;
 * mtr_anim_blend_destroy may follow a call directly (no host wait).
 * MTR_E_INVALID, nothing created (mtr_last_error names the clip, the sample or the triangle): a NULL device, out, nkeys, rates
 * or samples pointer, nclips == 0 or > 2^24, nkeys outside 1..2^24, clip flag bits other than MTR_CLIP_LOOP, a rate that is not
 * finite, nsamples outside 1..32, ntris > 64 or NULL tris with ntris > 0, nparams outside 1..16, param_x >= nparams (2-D:
 * or param_y), damp not above 0 (NaN included), max_instances outside 1..2^27; a sample whose clip is >= nclips or not LOOP or
 * whose px (2-D: or py) is not finite; in 1-D a px that does not lie above the one before it by a finite step; a triangle
 * with an index >= nsamples, with two equal indices, or whose doubled area is not finite and > 0.
 * MTR_E_INVALID, nothing changed, at a call: a NULL handle, states or params pointer, n == 0 or n > max_instances, nlayers
 * outside 3..8 with layers given, a misaligned device pointer (16 bytes: states, layers, steps; 4: params, shares).
 * MTR_E_UNSUPPORTED: a library built without k_blend. */
typedef struct mtr_anim_blend mtr_anim_blend;
typedef struct mtr_blend_sample { uint32_t clip; float px, py; uint32_t pad; } mtr_blend_sample;     /* 16 bytes */
typedef struct mtr_blend_tri { uint32_t v[3]; uint32_t pad; } mtr_blend_tri;                        /* 16 bytes */
typedef struct mtr_blend_state { float phase, px, py, speed; } mtr_blend_state;                     /* 16 bytes */
int32_t mtr_anim_blend_create(mtr_device *dev, size_t nclips, const uint32_t *nkeys /* nclips */,
                              const uint32_t *clip_flags /* nclips */, const float *rates /* nclips */,
                              const mtr_blend_sample *samples, size_t nsamples, const mtr_blend_tri *tris /* NULL: 1-D */,
                              size_t ntris, size_t nparams, uint32_t param_x, uint32_t param_y, float damp,
                              size_t max_instances, mtr_anim_blend **out);
void    mtr_anim_blend_destroy(mtr_anim_blend *blend);       /* parked like mtr_anim_destroy */
int32_t mtr_anim_blend_advance_device(mtr_anim_blend *blend, mtr_blend_state *states_dev /* n, 16-byte aligned */,
                                      const float *params_dev /* n*nparams, read only */, size_t n, float dt,
                                      mtr_anim_layer *out_layers_dev /* n*nlayers, 16-byte aligned, or NULL */, size_t nlayers,
                                      mtr_root_step *out_steps_dev /* n*3, 16-byte aligned, or NULL */,
                                      float *out_shares_dev /* n*3, or NULL */, void *hip_stream);
/* a test and debug hook: everything in host memory (any alignment), the same kernel, waits; the layers are read first so
 * that layers 3.. come back as they went in */
int32_t mtr_anim_blend_advance_host(mtr_anim_blend *blend, mtr_blend_state *states, const float *params, size_t n, float dt,
                                    mtr_anim_layer *out_layers, size_t nlayers, mtr_root_step *out_steps, float *out_shares);

/* ---- motion matching (build extension, SPEC.md section 25): nearest-pose search per instance (k_match) ----
 * A controller is authored by hand; a match set chooses by search.  It holds the clips (nkeys, clip_flags as
 * mtr_anim_ctrl_create takes them: the same periods P, no tie to a player handle), D features per row (D a multiple of 4 in
 * 4..64) and R rows {clip, x, bias, tags} sorted by clip, x strictly increasing within a clip: row r says "clip at position x
 * looks like features[r * D ..]".  The features are already normalised and weighted by whoever built the database
 * (mt_renderer_amd/anim_match.py).  pose_dims has bit d set where dimension d describes the pose being played, the other
 * dimensions describe where the game wants to go; mean and scale (D floats each, NULL: 0 and 1) normalise the game's raw
 * query.  Per instance and call:
 *   lead    : clip L and position p of what plays (clip B while fade > 0, else A; L clamped); cur = the row of L with the
 *             largest x <= p, none when L has no rows, p is NaN or p lies below L's first row.
 *   query   : q_d = features[cur][d] for a pose dimension with a cur, else (query[i * D + d] - mean_d) * scale_d.
 *   score   : s_r = fma(q_{D-1}, f_r[D-1], ... fma(q_0, f_r[0], c_r)), c_r = -(0.5 * |f_r|^2 + bias_r): the greatest score is the
 *             least 0.5 * |q - f_r|^2 + bias_r.  -0 counts as +0; a NaN score never wins.
 *   winner  : the greatest score among the rows with (tags & require) == require and (tags & exclude) == 0 (NULL filters:
 *             every row), the lowest row among equals.
 *   command : slot i = {instance_base + i, clip_win, x_win, seconds}, or the ignored command {0xFFFFFFFF, 0, 0, 0} when there
 *             is no winner, when a fade runs and the set lacks MTR_MATCH_INTERRUPT, when cur exists and the winner lies in L
 *             within near_x of p (the test does not look across the seam of a LOOP clip), or when cur exists, its score is
 *             not NaN and the winner's is not above it by more than margin.
 *   result  : optionally {row, cur, score, cur_score}; MTR_MATCH_NONE and 0x7FC00000 where there is none.
 * The n slots are what a controller writes: pass them to the next mtr_anim_player_advance_device_cmds.  instance_base lets a
 * caller search a slice of its crowd per frame: play + k, query + k * D, cmds + k, base k.  The play states are read and never
 * written; every bit pattern of play state, query and filter has a defined outcome.  A search runs in stream order on
 * hip_stream under the rules of mtr_batch_set_poses_device; the set owns scratch its kernels write, so calls on one set are
 * ordered among themselves whatever their streams; mtr_anim_match_destroy may follow a search directly (no host wait).
 * MTR_E_INVALID, nothing created (mtr_last_error names the clip, row or dimension): the clip rules of mtr_anim_ctrl_create, D not
 * a multiple of 4 in 4..64, nrows outside 1..2^22, max_instances outside 1..2^20, unknown flag bits, pose bits at or above D,
 * near_x or margin negative or not finite, a NULL array that is counted; a row whose clip is >= nclips or below the row
 * before it, whose x is not finite, below 0, above P (LOOP: at or above P) or not above the row before it in its clip, whose
 * bias or a feature is not finite or whose c_r is not finite; a mean or scale that is not finite.
 * MTR_E_INVALID, nothing changed, at a call: a NULL handle, play or cmds pointer, NULL query while some dimension is not a pose
 * dimension, n == 0 or n > max_instances, instance_base + n > 2^32 - 1, a misaligned device pointer (16 bytes: play, query,
 * cmds, results; 8: filter).
 * MTR_E_UNSUPPORTED: a library built without k_match. */
#define MTR_MATCH_INTERRUPT 1u   /* may command while a fade runs */
#define MTR_MATCH_NONE 0xFFFFFFFFu
#define MTR_MATCH_MAX_DIMS 64
typedef struct mtr_anim_match mtr_anim_match;
typedef struct mtr_match_row    { uint32_t clip; float x, bias; uint32_t tags; } mtr_match_row;          /* 16 bytes */
typedef struct mtr_match_filter { uint32_t require, exclude; } mtr_match_filter;                       /*  8 bytes */
typedef struct mtr_match_result { uint32_t row, cur; float score, cur_score; } mtr_match_result;        /* 16 bytes */
int32_t mtr_anim_match_create(mtr_device *dev, size_t nclips, const uint32_t *nkeys /* nclips */,
                              const uint32_t *clip_flags /* nclips, NULL = 0 */, size_t D, uint64_t pose_dims, uint32_t flags,
                              float seconds, float near_x, float margin, const mtr_match_row *rows, size_t nrows,
                              const float *features /* nrows*D */, const float *mean /* D, or NULL */,
                              const float *scale /* D, or NULL */, size_t max_instances, mtr_anim_match **out);
void    mtr_anim_match_destroy(mtr_anim_match *match);       /* parked like mtr_anim_destroy */
int32_t mtr_anim_match_search_device(mtr_anim_match *match, const mtr_play_state *play_dev /* n, 16-byte aligned */,
                                     const float *query_dev /* n*D, 16-byte aligned; NULL: every dimension is a pose dimension */,
                                     const mtr_match_filter *filter_dev /* n, or NULL */, size_t n, uint32_t instance_base,
                                     mtr_play_cmd *cmds_out_dev /* n, 16-byte aligned */,
                                     mtr_match_result *results_dev /* n, or NULL */, void *hip_stream);
/* a test and debug hook: everything in host memory (any alignment), the same kernels, waits */
int32_t mtr_anim_match_search_host(mtr_anim_match *match, const mtr_play_state *play, const float *query,
                                   const mtr_match_filter *filter, size_t n, uint32_t instance_base, mtr_play_cmd *cmds_out,
                                   mtr_match_result *results);
/* a test and debug hook: every score s_r of every instance, out[i * nrows + r], from the search kernel itself (a variant
 * that also stores its accumulators); host memory, waits */
int32_t mtr_anim_match_scores_host(mtr_anim_match *match, const mtr_play_state *play, const float *query, size_t n,
                                   float *out /* n*nrows */);

/* ---- spring bones (SPEC.md section 24): joints that lag and sway behind the animated pose ----
 * A spring set belongs to a skeleton, as an IK set does: it holds the skeleton's parents (the rules of
 * mtr_model_set_skeleton) and 1..16 springs.  A spring aims its joint (mtr_ik_chain's AIM, weight 1, axis = tail) at a
 * particle that the library simulates: tail is where the particle rests, in the joint's own space (usually the bind
 * translation of the joint's child); stiffness (per second) pulls it there, drag in [0, 1] is the share of its velocity
 * it loses per step, gravity is a displacement per second in the instance's model space (the space of the IK targets;
 * exact for instances that stay upright).  flags must be 0.  The order of the list is the order of the state records and
 * nothing else: a spring whose joint has spring ancestors sees what they changed, whatever the order.
 *
 * The particle of instance i and spring k lives in states[i * nsprings + k], caller-owned DEVICE memory that every call
 * reads and writes.  cur and prev are its position at this and at the previous step, in the instance's model space.  Every
 * bit pattern has a defined outcome; a ZEROED record means "not started" (live == 0, or a component that is not finite:
 * the particle starts at rest, cur = prev = its rest position).  The user may write states directly.
 *
 * Each call is one simulation step of dt seconds between the IK chains (ik may be NULL: none) and the fold; a dt that is
 * not positive and finite pauses the springs (the particle is carried, constrained and aimed at, not integrated).  motion:
 * n x 16 floats, the rigid delta D every instance moved by this frame (M_new = M_old o D), exactly what
 * mtr_anim_root_deltas_device writes: the particles are carried by its inverse, so that they stay where they were in the
 * world.  NULL: the instances did not move, or moved in a way the springs should ignore (a teleport).  Only rotations
 * change; like IK, the rule ignores scales above the joint.
 *
 * Frame semantics and ordering: mtr_batch_animate_ik_device's.  Calls on one spring set are ordered among themselves by
 * the set's event, whatever their streams.  No host-memory batch call and no mtr_model_* call: a single character is a
 * batch of one.
 *
 * Errors: MTR_E_INVALID, and nothing changes (no kernel runs, the states stay as they were), for everything the IK call
 * rejects, a NULL spring set, one of another device or joint count or whose parents differ from the model's skeleton
 * (mtr_last_error names the joint), NULL or misaligned states, misaligned motion, targets without an IK set or an IK set
 * without targets; at mtr_anim_spring_create (mtr_last_error names the spring): njoints outside 1..256, invalid parents,
 * nsprings outside 1..MTR_ANIM_MAX_SPRINGS, a joint >= njoints, a joint named twice, flag bits, a tail that is not finite
 * or all zero, a stiffness that is not finite or < 0, a drag outside [0, 1] (NaN included), a gravity that is not finite.
 * MTR_E_UNSUPPORTED when the library was built without the spring kernels. */
#define MTR_ANIM_MAX_SPRINGS 16
typedef struct mtr_anim_spring mtr_anim_spring;
typedef struct mtr_spring { uint32_t joint, flags; float stiffness, drag; float tail[3], pad0; float gravity[3], pad1; } mtr_spring; /* 48 bytes */
typedef struct mtr_spring_state { float cur[3]; uint32_t live; float prev[3]; uint32_t pad; } mtr_spring_state;                 /* 32 bytes */
int32_t mtr_anim_spring_create(mtr_device *dev, size_t njoints, const uint8_t *parents, size_t nsprings,
                               const mtr_spring *springs, mtr_anim_spring **out);
/* may follow an animate call directly: parked like mtr_anim_destroy */
void    mtr_anim_spring_destroy(mtr_anim_spring *spring);
int32_t mtr_batch_animate_spring_device(mtr_batch *batch, mtr_anim *anim, mtr_anim_masks *masks /* or NULL */,
                                        const mtr_anim_layer *layers_dev /* 16-byte aligned */, size_t nlayers,
                                        mtr_anim_ik *ik /* or NULL */, const mtr_ik_target *targets_dev /* NULL iff ik is NULL */,
                                        mtr_anim_spring *spring, mtr_spring_state *states_dev /* n*nsprings, in and out, 16-byte aligned */,
                                        const float *motion_dev /* n*16 or NULL, 16-byte aligned */, float dt, void *hip_stream);
/* a test and debug hook: everything in host memory (any alignment), the same kernels, waits; the states are read and
 * written back; the local matrices of n instances as mtr_anim_sample_ik gives them */
int32_t mtr_anim_sample_spring(mtr_anim *anim, mtr_anim_masks *masks /* or NULL */, mtr_anim_ik *ik /* or NULL */,
                               mtr_anim_spring *spring, const mtr_anim_layer *layers, size_t nlayers,
                               const mtr_ik_target *targets /* or NULL */, mtr_spring_state *states, const float *motion /* or NULL */,
                               float dt, size_t n, float *out_locals, size_t count);

/* ---- frame = one render pass (src/bin/modelviewer.rs:190-210: clear colour / clear depth) ---- */
int32_t mtr_frame_begin(mtr_device *dev, uint32_t width, uint32_t height, const float clear_rgba[4],
                        float clear_depth, mtr_frame **out);
/* Multi-GPU, one process per GPU: the frame renders only the 16x16-pixel bins that `rank` of `world` owns; colour / depth
 * of the other bins are untouched.  The sharded colour is exchanged by the caller (RCCL all-gather, see bench.py).
 * Which bins a rank owns is the host's choice, per frame (every rank of a frame must make the same choice):
 *   MTR_OWN_INTERLEAVED  bin b (row-major) -> rank b % world.  Finest balance; every object touches every rank.
 *   MTR_OWN_BANDS        rank r owns the bin rows [band_rows[r], band_rows[r+1]) (band_rows[0] = 0, band_rows[world] =
 *                        ceil(height / 16), non-decreasing; NULL = equal bands).  An object touches the few ranks
 *                        whose bands it crosses, so the geometry a rank must process shrinks with the world.
 *   MTR_OWN_SUPERTILES   squares of (1 << param) x (1 << param) bins (param <= 6) dealt round-robin, row-major.
 * A sharded rank does not process geometry that cannot reach its bins: every geometry wave first tests the object-space
 * bounds of its 62 strip positions (one box per joint that carries weight, transformed by that joint's palette matrix
 * and the view-projection; computed at mtr_model_create) against the rank's bins, and a batch draw first compacts its
 * instance list the same way.  The test is conservative: the pixels of a rank's bins are exactly those of the unsharded
 * frame.  mtr_device_set_culling(dev, 0) turns it off (tests compare both).  mtr_frame_set_shard = INTERLEAVED. */
enum { MTR_OWN_INTERLEAVED = 0, MTR_OWN_BANDS = 1, MTR_OWN_SUPERTILES = 2 };
int32_t mtr_frame_set_shard(mtr_frame *frame, uint32_t rank, uint32_t world);
int32_t mtr_frame_set_shard_map(mtr_frame *frame, uint32_t rank, uint32_t world, uint32_t map, uint32_t param,
                                const uint32_t *band_rows /* world + 1 entries, or NULL */);
/* mode: MTR_GEOM_CULL_OFF; MTR_GEOM_CULL_SHARDED (default: sharded frames with bands / super-tiles); MTR_GEOM_CULL_ALL_FRAMES:
 * unsharded frames too -- the same test against the whole target, i.e. instances and chunks that are off the target (or
 * behind the near plane as a whole) are skipped before any vertex work.  Costs two small kernels per draw (about 30 us
 * on 1024 instances), so it pays when a sizeable part of a batch is out of view; never changes a pixel. */
enum { MTR_GEOM_CULL_OFF = 0, MTR_GEOM_CULL_SHARDED = 1, MTR_GEOM_CULL_ALL_FRAMES = 2 };
int32_t mtr_device_set_culling(mtr_device *dev, int32_t mode);
/* Model::render (src/model.rs:299-363) with transform = view_proj (src/bin/modelviewer.rs:217-221) */
int32_t mtr_frame_draw_model(mtr_frame *frame, mtr_model *model, const float view_proj[16]);
int32_t mtr_frame_draw_batch(mtr_frame *frame, mtr_batch *batch, const float view_proj[16]);
/* convenience: host arrays, builds a temporary batch (npal palettes per instance, may be 0) */
int32_t mtr_frame_draw_instances(mtr_frame *frame, mtr_model *model, const float *model_mats,
                                 const float *palettes, size_t npal, size_t n,
                                 const float view_proj[16]);
/* The per-joint cubes Model::render adds to the debug overlay every frame (src/model.rs:309-315): one cube per joint at
 * joint_position * 0.01 with scale 0.005 (from_scale_rotation_translation, src/debug_overlay.rs:227-231), drawn like
 * mtr_frame_draw_overlay_cubes.  The positions are JointInfo::offset of every joint (src/model.rs:283-291), given with
 * mtr_model_set_joint_positions (mtr_model_create_from_files sets them).  A model without joints draws nothing. */
int32_t mtr_model_set_joint_positions(mtr_model *model, const float *xyz, size_t njoints);
int32_t mtr_frame_draw_model_joints(mtr_frame *frame, mtr_model *model, const float camera[16]);
/* DebugOverlay::render (src/debug_overlay.rs:202-221): n instanced cubes, no blend, constant colour */
int32_t mtr_frame_draw_overlay_cubes(mtr_frame *frame, const float camera[16], const float *inst_mats,
                                     size_t n);
/* enqueue all kernels; returns without waiting.  A frame that is submitted and then destroyed (or consumed through its
 * device pointers) without mtr_frame_wait cannot be re-run if a bounded bin queue overflows: its tile kernels then
 * leave every bin at the clear colour instead of rendering from incomplete queues, and the NEXT mtr_frame_begin /
 * mtr_frame_submit / mtr_device_synchronize returns MTR_E_OVERFLOW once (the bound has been raised by then). */
int32_t mtr_frame_submit(mtr_frame *frame);
/* framebuffer complete in HBM; a frame whose bin queues overflowed is transparently re-run first (exact two-pass queues) */
int32_t mtr_frame_wait(mtr_frame *frame);
int32_t mtr_frame_end(mtr_frame *frame);    /* submit + wait */
int32_t mtr_frame_read_color(mtr_frame *frame, void *rgba8, size_t len);  /* width*height*4 */
int32_t mtr_frame_read_depth(mtr_frame *frame, float *depth, size_t count); /* width*height */
void *mtr_frame_color_devptr(mtr_frame *frame); /* RGBA8 in HBM, row-major */
void *mtr_frame_depth_devptr(mtr_frame *frame); /* f32 in HBM, row-major */
/* multi-GPU exchange helpers (device pointers, enqueued on the device's stream):
 * pack: this frame's own bins (bin % world == rank), bin-major, 16x16 RGBA8 each, into dst
 *       (mtr_shard_bytes(width,height,world) bytes) = the all-gather send buffer;
 * unpack: gathered = world such blocks in rank order -> linear RGBA8 width*height at dst. */
size_t mtr_shard_bytes(uint32_t width, uint32_t height, uint32_t world); /* INTERLEAVED */
/* all-gather send size of any map = 1 KiB x the largest share of bins (0: bad arguments); pack zero-fills past a rank's own share */
size_t mtr_shard_bytes_map(uint32_t width, uint32_t height, uint32_t world, uint32_t map, uint32_t param, const uint32_t *band_rows);
size_t mtr_frame_shard_bytes(mtr_frame *frame); /* of this frame's map */
int32_t mtr_frame_pack_color_shard(mtr_frame *frame, void *dst_dev, size_t dst_bytes);
/* gathered (world blocks of mtr_frame_shard_bytes each, rank order) -> linear RGBA8 at dst_dev, by this frame's map;
 * hip_stream NULL = the device's public stream */
int32_t mtr_frame_unpack_color_shards_on_stream(mtr_frame *frame, const void *gathered_dev, void *dst_dev, void *hip_stream);
int32_t mtr_device_unpack_color_shards(mtr_device *dev, const void *gathered_dev, uint32_t world,
                                       uint32_t width, uint32_t height, void *dst_dev);
/* the same two steps on a caller-chosen hipStream_t instead of the device's public stream (the pack waits, on that
 * stream, for the frame's completion).  One in-order stream makes the exchange chain of frame k+1 (pack -> all-gather
 * -> unpack, with a cross-stream hand-over before and after the collective) wait for that of frame k; a host that
 * rotates a few exchange streams, each with its own send / receive buffers, overlaps them (bench.py). */
int32_t mtr_frame_pack_color_shard_on_stream(mtr_frame *frame, void *dst_dev, size_t dst_bytes, void *hip_stream);
int32_t mtr_device_unpack_color_shards_on_stream(mtr_device *dev, const void *gathered_dev, uint32_t world,
                                                 uint32_t width, uint32_t height, void *dst_dev, void *hip_stream);
/* The exchange of every sharded frame issued by a second host thread, owned by the device.  all-gather is the host's:
 * `fn` has ncclAllGather's signature (sendbuff, recvbuff, sendcount, datatype, comm, stream) and is called with
 * (send_dev, gathered_dev, send_bytes, dtype_u8, comm, hip_stream), so an RCCL host passes &ncclAllGather, its
 * communicator and ncclUint8; the library links no collective library itself.  Per frame the thread runs, on hip_stream:
 * pack (after the frame completes) -> fn -> unpack into dst_dev, then destroys the frame.
 *   (a frame whose bin queues overflowed is re-run by the thread before it is packed: the gathered frame is never missing
 *   triangles; the all-gather count is mtr_shard_bytes(frame width, height, world), which send_bytes must cover)
 *   mtr_frame_submit_exchange: submits the frame if it was not yet, hands it to the thread and CONSUMES the handle
 *       (blocks while 8 frames are waiting; on an error return the handle is NOT consumed and stays the caller's);   mtr_device_exchange_drain: returns once every handed-over frame has been
 *       issued (not: finished on the GPU -- synchronise hip_stream for that) with the first error of the thread, if any;
 *   mtr_device_exchange_stop: drain + join (also done by mtr_device_destroy).
 *   mtr_device_exchange_add_lane (optional, while the thread is idle, up to 4 lanes): one more (communicator, stream, send /
 *       gathered / destination buffers) set; frames are dealt to the lanes in turn (the i-th frame handed over goes to
 *       lane i % lanes, lane 0 being the one given to _start).  A lane is an in-order stream and completes one pack +
 *       all-gather + unpack latency per frame; two lanes keep two collectives in flight.  Every rank must use the same
 *       number of lanes, and each lane needs a communicator of its own.
 * Frames of one device are still begun / drawn / submitted by ONE thread; only these calls cross threads. */
typedef int (*mtr_allgather_fn)(const void *send, void *recv, size_t count, int datatype, void *comm, void *stream);
int32_t mtr_device_exchange_start(mtr_device *dev, mtr_allgather_fn fn, void *comm, int dtype_u8, void *send_dev,
                                  size_t send_bytes, void *gathered_dev, void *dst_dev, uint32_t world, void *hip_stream);
int32_t mtr_device_exchange_add_lane(mtr_device *dev, void *comm, void *send_dev, void *gathered_dev, void *dst_dev,
                                     void *hip_stream);
int32_t mtr_frame_submit_exchange(mtr_frame *frame);
int32_t mtr_device_exchange_drain(mtr_device *dev);
int32_t mtr_device_exchange_stop(mtr_device *dev);
/* ---- one host thread, N devices ("mtr_group_create(const int* devices, int n, mtr_group**) + same frame calls") ----
 * The reference has one event loop and one wgpu::Device (src/renderer_app_manager.rs:202-272).  A host that keeps that shape
 * and owns several GPUs of one node drives them through a group: rank r of the group is an mtr_device on hip_devices[r]
 * (an index may repeat: several ranks on one card), a group frame is one sharded frame per rank under one ownership map
 * (mtr_frame_set_shard_map's arguments), and ending it gathers the colour of every part into one linear RGBA8 image on
 * the device of rank 0: pack on each device, one peer copy per rank (xGMI where the devices are peers), unpack.
 *   resources are per device: create the model / textures / batches on mtr_group_device(group, r) for every r;
 *   drawing is "the same frame calls": mtr_frame_draw_* into mtr_group_frame_part(gf, r) with rank r's objects
 *       (the parts are owned by the group frame: never submit, wait for or destroy them yourself);
 *   mtr_group_frame_end submits every part, waits for all of them (a part whose bin queues overflowed is re-run first)
 *       and returns with the gathered image complete; it stays readable until the next group frame of the group ends;
 *   mtr_group_destroy destroys the group's devices: destroy their models, textures, batches and group frames first.
 * A group is driven by one thread and ends one frame at a time; the throughput path for N GPUs is one process (or host
 * thread) per device with the exchange thread above.  Errors: mtr_group_last_error(group)
 * (NULL: the last mtr_group_create failure). */
typedef struct mtr_group mtr_group;
typedef struct mtr_group_frame mtr_group_frame;
int32_t mtr_group_create(const int32_t *hip_devices, int32_t n, mtr_group **out); /* 1 <= n <= 64 */
void mtr_group_destroy(mtr_group *group);
int32_t mtr_group_size(const mtr_group *group);
mtr_device *mtr_group_device(mtr_group *group, int32_t rank);
const char *mtr_group_last_error(const mtr_group *group);
int32_t mtr_group_frame_begin(mtr_group *group, uint32_t width, uint32_t height, const float clear_rgba[4], float clear_depth,
                              uint32_t map, uint32_t param, const uint32_t *band_rows, mtr_group_frame **out);
mtr_frame *mtr_group_frame_part(mtr_group_frame *gframe, int32_t rank);
int32_t mtr_group_frame_end(mtr_group_frame *gframe);
int32_t mtr_group_frame_read_color(mtr_group_frame *gframe, void *rgba8, size_t len); /* width*height*4 */
void *mtr_group_frame_color_devptr(mtr_group_frame *gframe); /* on rank 0's device; NULL once a later group frame has ended */
void mtr_group_frame_destroy(mtr_group_frame *gframe);
int32_t mtr_frame_get_stats(mtr_frame *frame, mtr_frame_stats *out);
int32_t mtr_frame_get_timings(mtr_frame *frame, float ms[MTR_STAGE_COUNT]);
/* tuning / test hook: per-bin queue sizes of the frame just rendered (valid until the next frame is submitted on
 * this device): entries[b] = (triangle, bin) pairs of 16x16 bin b, segments[b] = ordered runs; nbins each.  A sharded
 * frame reports its own bins; the bins of the other ranks read 0. */
int32_t mtr_frame_read_bin_counts(mtr_frame *frame, uint32_t *entries, uint32_t *segments, size_t nbins);
void mtr_frame_destroy(mtr_frame *frame);

/* ---- unit-test hooks: one stage at a time through the same kernels ---- */
/* vertex stage of primitive `prim`: clip = M * (skin(position),1) and decoded texcoord for every
 * vertex in [0, vertex_num); out_clip vertex_num*4 f32, out_uv vertex_num*2 f32 (host memory) */
int32_t mtr_model_vertex_stage(mtr_model *model, size_t prim, const float M[16], float *out_clip,
                               float *out_uv);
/* MT crc32 (src/util/crc.rs:36-50), host side: material-name -> material lookups */
uint32_t mtr_crc32(const uint8_t *bytes, size_t len, uint32_t init);

#ifdef __cplusplus
}
#endif
#endif
