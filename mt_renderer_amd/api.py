"""ctypes binding of libmtr.so (include/mtr.h) + a host-side mirror of the reference's interface.

The classes keep the reference's names and argument roles -- ``Texture.new`` (src/texture.rs:11),
``Model.new`` / ``Model.set_parts_disp`` / ``Model.render`` (src/model.rs:36-45, :295, :299-305) --
with ``wgpu::Device`` / ``wgpu::RenderPass`` replaced by :class:`Device` / :class:`Frame`.

There is NO CPU fallback here: if libmtr.so is missing, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

from .scene import ModelData, TextureData

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MTR_LIB_PATH") or os.path.join(_PKG, "libmtr.so")  # MTR_LIB_PATH: A/B runs of two builds on one box

MTR_OK, MTR_E_INVALID, MTR_E_UNSUPPORTED, MTR_E_NOMEM, MTR_E_HIP, MTR_E_OVERFLOW = range(6)
TILE_AUTO, TILE_ORDERED, TILE_VISIBILITY, TILE_MIXED = 0, 1, 2, 3
OWN_INTERLEAVED, OWN_BANDS, OWN_SUPERTILES = 0, 1, 2
TEXRES_DECODED, TEXRES_BLOCKS = 0, 1
GEOM_CULL_OFF, GEOM_CULL_SHARDED, GEOM_CULL_ALL_FRAMES = 0, 1, 2
STAGE_NAMES = ("geom", "scan", "fill", "tile")

# every symbol include/mtr.h declares (tests check that the library exports each one)
EXPORTED_SYMBOLS = [
    "mtr_abi_version", "mtr_device_create", "mtr_device_create_on_stream", "mtr_device_destroy", "mtr_last_error",
    "mtr_device_set_profiling", "mtr_texture_create", "mtr_texture_destroy", "mtr_texture_read_rgba8",
    "mtr_model_create", "mtr_model_destroy", "mtr_model_set_parts_disp", "mtr_model_set_palette",
    "mtr_batch_create", "mtr_batch_destroy", "mtr_frame_begin", "mtr_frame_set_shard", "mtr_frame_draw_model",
    "mtr_frame_draw_batch", "mtr_frame_draw_instances", "mtr_frame_draw_overlay_cubes", "mtr_frame_submit",
    "mtr_frame_wait", "mtr_frame_end", "mtr_frame_read_color", "mtr_frame_read_depth", "mtr_frame_color_devptr",
    "mtr_frame_depth_devptr", "mtr_frame_get_stats", "mtr_frame_get_timings", "mtr_frame_destroy",
    "mtr_model_vertex_stage", "mtr_crc32", "mtr_shard_bytes", "mtr_frame_pack_color_shard",
    "mtr_device_unpack_color_shards", "mtr_frame_read_bin_counts", "mtr_device_set_tile_mode", "mtr_device_set_binning",
    "mtr_frame_pack_color_shard_on_stream", "mtr_device_unpack_color_shards_on_stream",
    "mtr_device_synchronize", "mtr_model_set_joint_positions", "mtr_frame_draw_model_joints", "mtr_model_set_prim_states", "mtr_texture_create_mips", "mtr_frame_set_shard_map", "mtr_device_set_culling", "mtr_device_set_texture_residency", "mtr_shard_bytes_map", "mtr_frame_shard_bytes",
    "mtr_frame_unpack_color_shards_on_stream", "mtr_device_exchange_start", "mtr_device_exchange_add_lane", "mtr_frame_submit_exchange", "mtr_device_exchange_drain", "mtr_device_exchange_stop",
    "mtr_group_create", "mtr_group_destroy", "mtr_group_size", "mtr_group_device", "mtr_group_last_error", "mtr_group_frame_begin",
    "mtr_group_frame_part", "mtr_group_frame_end", "mtr_group_frame_read_color", "mtr_group_frame_color_devptr", "mtr_group_frame_destroy",
    "mtr_model_set_skeleton", "mtr_model_set_pose", "mtr_batch_update", "mtr_batch_set_poses", "mtr_batch_set_poses_device",
    "mtr_batch_read_palettes",
    "mtr_anim_create", "mtr_anim_destroy", "mtr_model_animate", "mtr_batch_animate", "mtr_batch_animate_device", "mtr_anim_sample",
    "mtr_anim_create_tracks",
    "mtr_anim_masks_create", "mtr_anim_masks_destroy", "mtr_model_animate_layers", "mtr_batch_animate_layers",
    "mtr_batch_animate_layers_device", "mtr_anim_sample_layers",
    "mtr_anim_ik_create", "mtr_anim_ik_destroy", "mtr_model_animate_ik", "mtr_batch_animate_ik", "mtr_batch_animate_ik_device",
    "mtr_anim_sample_ik",
    "mtr_anim_spring_create", "mtr_anim_spring_destroy", "mtr_batch_animate_spring_device", "mtr_anim_sample_spring",
    "mtr_batch_attach", "mtr_batch_attach_device", "mtr_batch_sockets", "mtr_batch_sockets_device", "mtr_batch_read_model_mats",
    "mtr_anim_root_create", "mtr_anim_root_destroy", "mtr_batch_root_motion", "mtr_batch_root_motion_device", "mtr_anim_root_deltas",
    "mtr_anim_root_deltas_device",
    "mtr_anim_player_create", "mtr_anim_player_destroy", "mtr_anim_player_advance_device", "mtr_anim_player_advance_device_cmds",
    "mtr_anim_player_advance_host",
    "mtr_anim_ctrl_create", "mtr_anim_ctrl_destroy", "mtr_anim_ctrl_step_device", "mtr_anim_ctrl_step_host",
    "mtr_anim_events_create", "mtr_anim_events_destroy", "mtr_anim_events_collect_device", "mtr_anim_events_collect_host",
    "mtr_anim_blend_create", "mtr_anim_blend_destroy", "mtr_anim_blend_advance_device", "mtr_anim_blend_advance_host",
    "mtr_anim_match_create", "mtr_anim_match_destroy", "mtr_anim_match_search_device", "mtr_anim_match_search_host",
    "mtr_anim_match_scores_host",
]

CLIP_LOOP = 1
# mtr_anim_key / mtr_anim_state (include/mtr.h; SPEC.md section 14)
ANIM_KEY = np.dtype([("t", "<f4", 3), ("pad0", "<f4"), ("q", "<f4", 4), ("s", "<f4", 3), ("pad1", "<f4")])
ANIM_STATE = np.dtype([("clip_a", "<u4"), ("clip_b", "<u4"), ("x_a", "<f4"), ("x_b", "<f4"), ("w", "<f4"), ("pad", "<u4")])
# mtr_anim_track (SPEC.md section 15)
ANIM_TRACK = np.dtype([("first", "<u4"), ("count", "<u4"), ("lo", "<f4", 3), ("step", "<f4", 3)])
# mtr_anim_layer (SPEC.md section 16)
ANIM_LAYER = np.dtype([("clip", "<u4"), ("x", "<f4"), ("w", "<f4"), ("mask", "<u2"), ("mode", "<u2")])
ANIM_MAX_LAYERS = 8
LAYER_OVERRIDE = 0
LAYER_ADDITIVE = 1
# mtr_ik_chain / mtr_ik_target (SPEC.md section 17)
ANIM_IK_CHAIN = np.dtype([("kind", "<u4"), ("joint", "<u4", 3), ("axis", "<f4", 3), ("flags", "<u4")])
ANIM_IK_TARGET = np.dtype([("pos", "<f4", 3), ("w", "<f4"), ("pole", "<f4", 3), ("pad", "<u4")])
ANIM_MAX_IK = 4
# mtr_spring / mtr_spring_state (SPEC.md section 24)
SPRING = np.dtype([("joint", "<u4"), ("flags", "<u4"), ("stiffness", "<f4"), ("drag", "<f4"), ("tail", "<f4", 3), ("pad0", "<f4"),
                   ("gravity", "<f4", 3), ("pad1", "<f4")])
SPRING_STATE = np.dtype([("cur", "<f4", 3), ("live", "<u4"), ("prev", "<f4", 3), ("pad", "<u4")])
ANIM_MAX_SPRINGS = 16
IK_TWO_BONE = 0
IK_AIM = 1
IK_POLE = 1
# mtr_attach (SPEC.md section 18): one attached instance
ATTACH = np.dtype([("src_instance", "<u4"), ("joint", "<u4"), ("flags", "<u4"), ("pad", "<u4"), ("offset", "<f4", 16)])
ATTACH_NO_JOINT = 0xFFFFFFFF
ATTACH_POSITION_ONLY = 1
# mtr_root_step (SPEC.md section 19): one step of an instance's root motion
ROOT_STEP = np.dtype([("clip", "<u4"), ("x", "<f4"), ("dx", "<f4"), ("w", "<f4")])
ROOT_MAX_STEPS = 8
ROOT_CYCLIC = 1
# mtr_play_state, mtr_play_cmd (SPEC.md section 20): what a player keeps per instance on the device, and a command to it
PLAY_STATE = np.dtype([("clip_a", "<u4"), ("clip_b", "<u4"), ("x_a", "<f4"), ("x_b", "<f4"), ("w", "<f4"), ("fade", "<f4"), ("speed", "<f4"),
                       ("flags", "<u4")])
PLAY_CMD = np.dtype([("instance", "<u4"), ("clip", "<u4"), ("x", "<f4"), ("seconds", "<f4")])
PLAY_ENDED = 1
# mtr_ctrl_node, mtr_ctrl_trans, mtr_ctrl_state (SPEC.md section 21): the tables of a controller and what it keeps per instance
CTRL_NODE = np.dtype([("clip", "<u4"), ("first", "<u4"), ("count", "<u4"), ("pad", "<u4")])
CTRL_COND = np.dtype([("param", "<u2"), ("op", "<u2"), ("value", "<f4")])
CTRL_TRANS = np.dtype([("target", "<u4"), ("flags", "<u4"), ("seconds", "<f4"), ("x", "<f4"), ("ncond", "<u4"), ("pad", "<u4"), ("cond", CTRL_COND, (3,))])
CTRL_STATE = np.dtype([("node", "<u4"), ("t", "<f4"), ("fired", "<u4"), ("user", "<u4")])
CTRL_MAX_COND = 3
OP_LT, OP_LE, OP_GT, OP_GE, OP_EQ, OP_NE = range(6)
TR_INTERRUPT, TR_SELF, TR_SYNC, TR_CONSUME = 1, 2, 4, 8
CTRL_TIME, CTRL_POS, CTRL_PHASE, CTRL_ENDED, CTRL_FADING = 0xFFFF, 0xFFFE, 0xFFFD, 0xFFFC, 0xFFFB
CTRL_NONE = 0xFFFFFFFF
# mtr_event_marker, mtr_anim_event (SPEC.md section 22): a marker on a clip, and one record of the list a collect call writes
EVENT_MARKER = np.dtype([("x", "<f4"), ("id", "<u4")])
EVENT = np.dtype([("instance", "<u4"), ("id", "<u4"), ("where", "<u4"), ("w", "<f4")])
EVENT_BACKWARD = 0x80000000
# mtr_blend_sample, mtr_blend_tri, mtr_blend_state (SPEC.md section 23): a sample point with its clip, a triangle of sample
# indices, and what one instance of a blend space keeps on the GPU
BLEND_SAMPLE = np.dtype([("clip", "<u4"), ("px", "<f4"), ("py", "<f4"), ("pad", "<u4")])
BLEND_TRI = np.dtype([("v", "<u4", (3,)), ("pad", "<u4")])
BLEND_STATE = np.dtype([("phase", "<f4"), ("px", "<f4"), ("py", "<f4"), ("speed", "<f4")])
# mtr_match_row, mtr_match_filter, mtr_match_result (SPEC.md section 25): a row of a match set, what an instance admits, what a search found
MATCH_ROW = np.dtype([("clip", "<u4"), ("x", "<f4"), ("bias", "<f4"), ("tags", "<u4")])
MATCH_FILTER = np.dtype([("require", "<u4"), ("exclude", "<u4")])
MATCH_RESULT = np.dtype([("row", "<u4"), ("cur", "<u4"), ("score", "<f4"), ("cur_score", "<f4")])
MATCH_INTERRUPT = 1
MATCH_NONE = 0xFFFFFFFF
MATCH_MAX_DIMS = 64


class MtrError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mtr error {code}: {msg}")
        self.code = code


class _Primitive(C.Structure):
    _fields_ = [("w", C.c_uint32 * 14)]


class _Element(C.Structure):
    _fields_ = [("semantic", C.c_uint8), ("format", C.c_uint8), ("count", C.c_uint8), ("flags", C.c_uint8),
                ("offset", C.c_uint16), ("pad1", C.c_uint16)]


class _Layout(C.Structure):
    _fields_ = [("num_elements", C.c_uint32), ("elements", _Element * 8)]


class FrameStats(C.Structure):
    _fields_ = [("tris_in", C.c_uint64), ("tris_setup", C.c_uint64), ("bin_entries", C.c_uint64),
                ("segments", C.c_uint64), ("width", C.c_uint32), ("height", C.c_uint32), ("nbins", C.c_uint32),
                ("ndraws", C.c_uint32), ("tile_kernel", C.c_uint32), ("binning", C.c_uint32),
                ("chunks", C.c_uint64), ("chunks_culled", C.c_uint64), ("shard_map", C.c_uint32), ("shard_bins", C.c_uint32)]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback for the HIP draw path)")
    # PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64.  If libmtr.so maps the system runtime
    # first and torch is imported later, the process ends up with two HSA runtimes and torch reports "No HIP GPUs
    # are available"; with torch mapped first, libmtr.so binds to the runtime that is already there.  So: when
    # torch is installed, load it before the library (MTR_NO_TORCH_PRELOAD=1 skips this).
    if os.environ.get("MTR_NO_TORCH_PRELOAD") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(LIB_PATH)
    vp, i32, u32, sz = C.c_void_p, C.c_int32, C.c_uint32, C.c_size_t
    sig = {
        "mtr_abi_version": (i32, []),
        "mtr_device_create": (i32, [i32, C.POINTER(vp)]),
        "mtr_device_create_on_stream": (i32, [i32, vp, C.POINTER(vp)]),
        "mtr_device_destroy": (None, [vp]),
        "mtr_last_error": (C.c_char_p, [vp]),
        "mtr_device_set_profiling": (i32, [vp, i32]),
        "mtr_device_synchronize": (i32, [vp]),
        "mtr_texture_create": (i32, [vp, u32, u32, u32, vp, sz, C.POINTER(vp)]),
        "mtr_texture_create_mips": (i32, [vp, u32, u32, u32, u32, vp, sz, C.POINTER(vp)]),
        "mtr_model_set_prim_states": (i32, [vp, vp, sz]),
        "mtr_model_set_joint_positions": (i32, [vp, vp, sz]),
        "mtr_frame_draw_model_joints": (i32, [vp, vp, vp]),
        "mtr_texture_destroy": (None, [vp]),
        "mtr_texture_read_rgba8": (i32, [vp, vp, sz]),
        "mtr_model_create": (i32, [vp, vp, sz, vp, sz, vp, sz, vp, vp, vp, sz, vp, C.POINTER(vp)]),
        "mtr_model_destroy": (None, [vp]),
        "mtr_model_set_parts_disp": (i32, [vp, vp, sz]),
        "mtr_model_set_palette": (i32, [vp, vp, sz]),
        "mtr_batch_create": (i32, [vp, vp, sz, vp, vp, sz, vp, C.POINTER(vp)]),
        "mtr_batch_destroy": (None, [vp]),
        "mtr_frame_begin": (i32, [vp, u32, u32, vp, C.c_float, C.POINTER(vp)]),
        "mtr_frame_set_shard": (i32, [vp, u32, u32]),
        "mtr_frame_set_shard_map": (i32, [vp, u32, u32, u32, u32, vp]),
        "mtr_device_set_culling": (i32, [vp, i32]),
        "mtr_device_set_texture_residency": (i32, [vp, u32]),
        "mtr_shard_bytes_map": (sz, [u32, u32, u32, u32, u32, vp]),
        "mtr_frame_shard_bytes": (sz, [vp]),
        "mtr_frame_unpack_color_shards_on_stream": (i32, [vp, vp, vp, vp]),
        "mtr_frame_draw_model": (i32, [vp, vp, vp]),
        "mtr_frame_draw_batch": (i32, [vp, vp, vp]),
        "mtr_frame_draw_instances": (i32, [vp, vp, vp, vp, sz, sz, vp]),
        "mtr_frame_draw_overlay_cubes": (i32, [vp, vp, vp, sz]),
        "mtr_frame_submit": (i32, [vp]),
        "mtr_frame_wait": (i32, [vp]),
        "mtr_frame_end": (i32, [vp]),
        "mtr_frame_read_color": (i32, [vp, vp, sz]),
        "mtr_frame_read_depth": (i32, [vp, vp, sz]),
        "mtr_frame_color_devptr": (vp, [vp]),
        "mtr_frame_depth_devptr": (vp, [vp]),
        "mtr_frame_get_stats": (i32, [vp, C.POINTER(FrameStats)]),
        "mtr_frame_get_timings": (i32, [vp, C.POINTER(C.c_float * 4)]),
        "mtr_frame_destroy": (None, [vp]),
        "mtr_model_vertex_stage": (i32, [vp, sz, vp, vp, vp]),
        "mtr_crc32": (u32, [vp, sz, u32]),
        "mtr_shard_bytes": (sz, [u32, u32, u32]),
        "mtr_frame_pack_color_shard": (i32, [vp, vp, sz]),
        "mtr_device_unpack_color_shards": (i32, [vp, vp, u32, u32, u32, vp]),
        "mtr_frame_pack_color_shard_on_stream": (i32, [vp, vp, sz, vp]),
        "mtr_device_unpack_color_shards_on_stream": (i32, [vp, vp, u32, u32, u32, vp, vp]),
        "mtr_device_exchange_start": (i32, [vp, vp, vp, i32, vp, sz, vp, vp, u32, vp]),
        "mtr_device_exchange_add_lane": (i32, [vp, vp, vp, vp, vp, vp]),
        "mtr_frame_submit_exchange": (i32, [vp]),
        "mtr_device_exchange_drain": (i32, [vp]),
        "mtr_device_exchange_stop": (i32, [vp]),
        "mtr_frame_read_bin_counts": (i32, [vp, vp, vp, sz]),
        "mtr_device_set_tile_mode": (i32, [vp, i32]),
        "mtr_device_set_binning": (i32, [vp, i32, u32]),
        "mtr_group_create": (i32, [vp, i32, C.POINTER(vp)]),
        "mtr_group_destroy": (None, [vp]),
        "mtr_group_size": (i32, [vp]),
        "mtr_group_device": (vp, [vp, i32]),
        "mtr_group_last_error": (C.c_char_p, [vp]),
        "mtr_group_frame_begin": (i32, [vp, u32, u32, vp, C.c_float, u32, u32, vp, C.POINTER(vp)]),
        "mtr_group_frame_part": (vp, [vp, i32]),
        "mtr_group_frame_end": (i32, [vp]),
        "mtr_group_frame_read_color": (i32, [vp, vp, sz]),
        "mtr_group_frame_color_devptr": (vp, [vp]),
        "mtr_group_frame_destroy": (None, [vp]),
        "mtr_model_set_skeleton": (i32, [vp, vp, vp, sz]),
        "mtr_model_set_pose": (i32, [vp, vp, sz]),
        "mtr_batch_update": (i32, [vp, vp, vp, sz]),
        "mtr_batch_set_poses": (i32, [vp, vp, sz]),
        "mtr_batch_set_poses_device": (i32, [vp, vp, sz, vp]),
        "mtr_batch_read_palettes": (i32, [vp, vp, sz]),
        "mtr_anim_create": (i32, [vp, sz, sz, vp, vp, vp, vp]),
        "mtr_anim_destroy": (None, [vp]),
        "mtr_model_animate": (i32, [vp, vp, vp]),
        "mtr_batch_animate": (i32, [vp, vp, vp]),
        "mtr_batch_animate_device": (i32, [vp, vp, vp, vp]),
        "mtr_anim_sample": (i32, [vp, vp, sz, vp, sz]),
        "mtr_anim_create_tracks": (i32, [vp, sz, sz, vp, vp, vp, vp, vp, sz, vp]),
        "mtr_anim_masks_create": (i32, [vp, sz, sz, vp, vp]),
        "mtr_anim_masks_destroy": (None, [vp]),
        "mtr_model_animate_layers": (i32, [vp, vp, vp, vp, sz]),
        "mtr_batch_animate_layers": (i32, [vp, vp, vp, vp, sz]),
        "mtr_batch_animate_layers_device": (i32, [vp, vp, vp, vp, sz, vp]),
        "mtr_anim_sample_layers": (i32, [vp, vp, vp, sz, sz, vp, sz]),
        "mtr_anim_ik_create": (i32, [vp, sz, vp, sz, vp, vp]),
        "mtr_anim_ik_destroy": (None, [vp]),
        "mtr_model_animate_ik": (i32, [vp, vp, vp, vp, sz, vp, vp]),
        "mtr_batch_animate_ik": (i32, [vp, vp, vp, vp, sz, vp, vp]),
        "mtr_batch_animate_ik_device": (i32, [vp, vp, vp, vp, sz, vp, vp, vp]),
        "mtr_anim_sample_ik": (i32, [vp, vp, vp, vp, sz, vp, sz, vp, sz]),
        "mtr_anim_spring_create": (i32, [vp, sz, vp, sz, vp, vp]),
        "mtr_anim_spring_destroy": (None, [vp]),
        "mtr_batch_animate_spring_device": (i32, [vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, C.c_float, vp]),
        "mtr_anim_sample_spring": (i32, [vp, vp, vp, vp, vp, sz, vp, vp, vp, C.c_float, sz, vp, sz]),
        "mtr_batch_attach": (i32, [vp, vp, vp]),
        "mtr_batch_attach_device": (i32, [vp, vp, vp, vp]),
        "mtr_batch_sockets": (i32, [vp, vp, sz, vp, sz]),
        "mtr_batch_sockets_device": (i32, [vp, vp, sz, vp, vp]),
        "mtr_batch_read_model_mats": (i32, [vp, vp, sz]),
        "mtr_anim_root_create": (i32, [vp, sz, sz, C.c_uint32, vp, vp]),
        "mtr_anim_root_destroy": (None, [vp]),
        "mtr_batch_root_motion": (i32, [vp, vp, vp, vp, sz]),
        "mtr_batch_root_motion_device": (i32, [vp, vp, vp, vp, sz, vp]),
        "mtr_anim_root_deltas": (i32, [vp, vp, vp, sz, sz, vp, sz]),
        "mtr_anim_root_deltas_device": (i32, [vp, vp, vp, sz, sz, vp, vp]),
        "mtr_anim_player_create": (i32, [vp, sz, vp, vp, vp, sz, vp]),
        "mtr_anim_player_destroy": (None, [vp]),
        "mtr_anim_player_advance_device": (i32, [vp, vp, sz, C.c_float, vp, sz, vp, vp, sz, vp, vp]),
        "mtr_anim_player_advance_device_cmds": (i32, [vp, vp, sz, C.c_float, vp, sz, vp, vp, sz, vp, vp]),
        "mtr_anim_player_advance_host": (i32, [vp, vp, sz, C.c_float, vp, sz, vp, vp, sz, vp]),
        "mtr_anim_ctrl_create": (i32, [vp, sz, vp, vp, vp, sz, vp, sz, sz, sz, vp]),
        "mtr_anim_ctrl_destroy": (None, [vp]),
        "mtr_anim_ctrl_step_device": (i32, [vp, vp, vp, vp, sz, C.c_float, vp, vp, vp]),
        "mtr_anim_ctrl_step_host": (i32, [vp, vp, vp, vp, sz, C.c_float, vp, vp]),
        "mtr_anim_events_create": (i32, [vp, sz, vp, vp, vp, vp, sz, vp]),
        "mtr_anim_events_destroy": (None, [vp]),
        "mtr_anim_events_collect_device": (i32, [vp, vp, sz, sz, C.c_float, vp, sz, vp, vp, vp]),
        "mtr_anim_events_collect_host": (i32, [vp, vp, sz, sz, C.c_float, vp, sz, vp, vp]),
        "mtr_anim_blend_create": (i32, [vp, sz, vp, vp, vp, vp, sz, vp, sz, sz, C.c_uint32, C.c_uint32, C.c_float, sz, vp]),
        "mtr_anim_blend_destroy": (None, [vp]),
        "mtr_anim_blend_advance_device": (i32, [vp, vp, vp, sz, C.c_float, vp, sz, vp, vp, vp]),
        "mtr_anim_blend_advance_host": (i32, [vp, vp, vp, sz, C.c_float, vp, sz, vp, vp]),
        "mtr_anim_match_create": (i32, [vp, sz, vp, vp, sz, C.c_uint64, u32, C.c_float, C.c_float, C.c_float, vp, sz, vp, vp, vp, sz, vp]),
        "mtr_anim_match_destroy": (None, [vp]),
        "mtr_anim_match_search_device": (i32, [vp, vp, vp, vp, sz, u32, vp, vp, vp]),
        "mtr_anim_match_search_host": (i32, [vp, vp, vp, vp, sz, u32, vp, vp]),
        "mtr_anim_match_scores_host": (i32, [vp, vp, vp, sz, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


lib = _load()


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a, shape=None) -> np.ndarray:
    r = np.ascontiguousarray(a, dtype=np.float32)
    return r if shape is None else r.reshape(shape)


def shard_bytes_map(width: int, height: int, world: int, own_map: int = OWN_INTERLEAVED, param: int = 0, band_rows=None) -> int:
    br = None if band_rows is None else np.ascontiguousarray(band_rows, dtype=np.uint32)
    return int(lib.mtr_shard_bytes_map(width, height, world, own_map, param, _p(br)))


def crc32(data: bytes, init: int = 0xFFFFFFFF) -> int:
    buf = np.frombuffer(data + b"\0", dtype=np.uint8)
    return int(lib.mtr_crc32(_p(buf), len(data), init))


class Device:
    """Stands where ``wgpu::Device`` + ``wgpu::Queue`` do (src/renderer_app_manager.rs:103-115)."""

    def __init__(self, hip_device: int = 0, stream: Optional[int] = None):
        h = C.c_void_p()
        rc = lib.mtr_device_create_on_stream(hip_device, C.c_void_p(stream) if stream else None, C.byref(h))
        if rc:
            raise MtrError(rc, (lib.mtr_last_error(None) or b"").decode())
        self._h = h
        self.hip_device = hip_device

    def check(self, rc: int):
        if rc:
            raise MtrError(rc, (lib.mtr_last_error(self._h) or b"").decode())

    def unpack_color_shards(self, gathered_devptr: int, world: int, width: int, height: int, dst_devptr: int,
                            stream: Optional[int] = None):
        """gathered [rank][k][16][16] RGBA8 blocks (device) -> linear RGBA8 framebuffer (device); on the device's public
        stream, or on `stream` (a hipStream_t handle)."""
        if stream is None:
            self.check(lib.mtr_device_unpack_color_shards(self._h, C.c_void_p(gathered_devptr), world, width, height,
                                                          C.c_void_p(dst_devptr)))
        else:
            self.check(lib.mtr_device_unpack_color_shards_on_stream(self._h, C.c_void_p(gathered_devptr), world, width, height,
                                                                    C.c_void_p(dst_devptr), C.c_void_p(stream)))

    def exchange_start(self, allgather_fn_addr: int, comm: int, dtype_u8: int, send_devptr: int, send_bytes: int,
                       gathered_devptr: int, dst_devptr: int, world: int, stream: int):
        """start the device's exchange thread (include/mtr.h): per handed-over frame, on `stream`, pack -> all-gather
        (a C function with ncclAllGather's signature, e.g. rccl.Rccl().allgather_addr) -> unpack into dst -> destroy."""
        self.check(lib.mtr_device_exchange_start(self._h, C.c_void_p(allgather_fn_addr), C.c_void_p(comm), dtype_u8,
                                                 C.c_void_p(send_devptr), send_bytes, C.c_void_p(gathered_devptr),
                                                 C.c_void_p(dst_devptr), world, C.c_void_p(stream)))

    def exchange_add_lane(self, comm: int, send_devptr: int, gathered_devptr: int, dst_devptr: int, stream: int):
        """one more (communicator, buffers, stream) set for the exchange thread; frames go to the lanes in turn"""
        self.check(lib.mtr_device_exchange_add_lane(self._h, C.c_void_p(comm), C.c_void_p(send_devptr), C.c_void_p(gathered_devptr),
                                                    C.c_void_p(dst_devptr), C.c_void_p(stream)))

    def exchange_drain(self):
        """returns once every frame handed to the exchange thread has been issued; raises its first error"""
        self.check(lib.mtr_device_exchange_drain(self._h))

    def exchange_stop(self):
        self.check(lib.mtr_device_exchange_stop(self._h))

    def set_culling(self, mode):
        """skip geometry whose bounds cannot reach the rank's bins: False / True (sharded frames, default) or
        GEOM_CULL_ALL_FRAMES (unsharded frames too: what is off the target is skipped; include/mtr.h)"""
        self.check(lib.mtr_device_set_culling(self._h, int(mode)))

    def set_texture_residency(self, mode: int):
        """what BC textures created from now on keep in HBM: TEXRES_DECODED (RGBA8, default) or TEXRES_BLOCKS (include/mtr.h)"""
        self.check(lib.mtr_device_set_texture_residency(self._h, mode))

    def set_tile_mode(self, mode: int):
        """0 auto, 1 force the ordered tile kernel, 2 visibility-key kernel when eligible (include/mtr.h)."""
        self.check(lib.mtr_device_set_tile_mode(self._h, mode))

    def set_binning(self, single_pass: bool, queue_capacity: int = 0):
        """single-pass bounded bin queues (default) or the exact two-pass queues; see include/mtr.h."""
        self.check(lib.mtr_device_set_binning(self._h, 1 if single_pass else 0, queue_capacity))

    def synchronize(self):
        """every submitted frame has left the GPU; raises if one that was never waited for dropped triangles"""
        self.check(lib.mtr_device_synchronize(self._h))

    def set_profiling(self, on: bool):
        self.check(lib.mtr_device_set_profiling(self._h, 1 if on else 0))

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):  # a group's device is destroyed with the group
                lib.mtr_device_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Texture:
    def __init__(self, dev: Device, h):
        self.dev, self._h = dev, h

    @staticmethod
    def new(dev: Device, resource: TextureData) -> "Texture":
        """Texture::new(device, queue, resource) -- src/texture.rs:11."""
        h = C.c_void_p()
        buf = np.frombuffer(resource.data, dtype=np.uint8)
        dev.check(lib.mtr_texture_create_mips(dev._h, resource.width, resource.height, resource.fmt, getattr(resource, "levels", 1),
                                              _p(buf), buf.size, C.byref(h)))
        t = Texture(dev, h)
        t.width, t.height = resource.width, resource.height
        return t

    def read_rgba8(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self.dev.check(lib.mtr_texture_read_rgba8(self._h, _p(out), out.size))
        return out

    def close(self):
        if self._h:
            lib.mtr_texture_destroy(self._h)
            self._h = None


class Model:
    def __init__(self, dev: Device, h, textures: List[Texture], md: ModelData):
        self.dev, self._h, self.textures, self.md = dev, h, textures, md

    @staticmethod
    def new(dev: Device, md: ModelData) -> "Model":
        """Model::new(model_file, material_file, shader2, ...) -- src/model.rs:36-45.  ``md`` carries what
        those three parsed files contribute to the draw path."""
        textures = [Texture.new(dev, t) for t in md.textures]
        vb = np.ascontiguousarray(md.vertex_buf, dtype=np.uint8)
        ib = np.ascontiguousarray(md.index_buf, dtype=np.uint16)
        pr = np.ascontiguousarray(md.prims, dtype=np.uint8).reshape(-1, 0x38)
        lays = (_Layout * len(md.layouts))()
        for i, els in enumerate(md.layouts):
            if len(els) > 8:
                raise MtrError(MTR_E_INVALID, "more than 8 layout elements")
            lays[i].num_elements = len(els)
            for j, el in enumerate(els):  # (semantic, format, count, offset[, flags])
                e = lays[i].elements[j]
                e.semantic, e.format, e.count, e.offset = el[:4]
                e.flags = el[4] if len(el) > 4 else 0
        p2t = np.ascontiguousarray(md.prim_to_texture, dtype=np.int32)
        did = np.ascontiguousarray(md.prim_debug_id, dtype=np.uint32)
        th = (C.c_void_p * max(1, len(textures)))(*[t._h for t in textures])
        h = C.c_void_p()
        dev.check(lib.mtr_model_create(dev._h, _p(vb), vb.size, _p(ib), ib.size, _p(pr), pr.shape[0], C.cast(lays, C.c_void_p),
                                       _p(p2t), C.cast(th, C.c_void_p), len(textures), _p(did), C.byref(h)))
        m = Model(dev, h, textures, md)
        pd = np.ascontiguousarray(md.parts_disp, dtype=np.uint8)
        if pd.size != pr.shape[0] or not pd.all():
            m.set_parts_disp(pd)
        if getattr(md, "prim_states", None) is not None:
            m.set_prim_states(md.prim_states)
        return m

    def set_prim_states(self, states):
        """material state per primitive: uint8 [nprims, 4] = blend, depth write, depth test, cull (include/mtr.h), or None"""
        if states is None:
            self.dev.check(lib.mtr_model_set_prim_states(self._h, None, 0))
        else:
            st = np.ascontiguousarray(states, dtype=np.uint8).reshape(-1, 4)
            self.dev.check(lib.mtr_model_set_prim_states(self._h, _p(st), st.shape[0]))

    def set_parts_disp(self, parts_disp: Sequence[bool]):
        """Model::set_parts_disp -- src/model.rs:295."""
        pd = np.ascontiguousarray(parts_disp, dtype=np.uint8)
        self.dev.check(lib.mtr_model_set_parts_disp(self._h, _p(pd), pd.size))

    def set_palette(self, mats: Optional[np.ndarray]):
        if mats is None:
            self.dev.check(lib.mtr_model_set_palette(self._h, None, 0))
        else:
            m = _f32(mats, (-1, 16))
            self.dev.check(lib.mtr_model_set_palette(self._h, _p(m), m.shape[0]))

    def set_skeleton(self, parents: Optional[Sequence[int]], imats: Optional[np.ndarray] = None):
        """skeleton for set_pose / Batch.set_poses (include/mtr.h): parents[j] = 255 or j for a root, else its parent;
        imats [njoints, 16] inverse bind matrices.  None clears it."""
        if parents is None:
            self.dev.check(lib.mtr_model_set_skeleton(self._h, None, None, 0))
            return
        par = np.ascontiguousarray(parents, dtype=np.uint8)
        im = _f32(imats, (-1, 16))
        if im.shape[0] != par.size:
            raise MtrError(MTR_E_INVALID, "one inverse bind matrix per joint")
        n = par.size
        if n == 0:  # not NULL (which clears the skeleton): the library rejects a skeleton of no joints
            par, im = np.zeros(1, dtype=np.uint8), np.zeros((1, 16), dtype=np.float32)
        self.dev.check(lib.mtr_model_set_skeleton(self._h, _p(par), _p(im), n))

    def set_pose(self, local_mats: np.ndarray):
        """palette formed on the GPU from one local matrix per joint of the skeleton ([njoints, 16])"""
        lm = _f32(local_mats, (-1, 16))
        self.dev.check(lib.mtr_model_set_pose(self._h, _p(lm), lm.shape[0]))

    def animate(self, anim: "Anim", state):
        """palette formed on the GPU (k_anim) from one animation state (an ANIM_STATE record or a dict of its fields)"""
        st = anim_states(state, 1)
        self.dev.check(lib.mtr_model_animate(self._h, anim._h, _p(st)))

    def animate_layers(self, anim: "Anim", layers, masks: Optional["AnimMasks"] = None):
        """palette formed on the GPU (k_anim_layers) from one layer stack: an ANIM_LAYER array [L] or a dict of its fields"""
        ly = anim_layers(layers, 1)
        self.dev.check(lib.mtr_model_animate_layers(self._h, anim._h, masks._h if masks is not None else None, _p(ly), ly.shape[1]))

    def animate_ik(self, anim: "Anim", layers, ik: "AnimIK", targets, masks: Optional["AnimMasks"] = None):
        """palette formed on the GPU (k_anim_ik) from one layer stack and one target per chain of ``ik`` (an ANIM_IK_TARGET
        array [K] or a dict of its fields; SPEC.md section 17)"""
        ly = anim_layers(layers, 1)
        tg = ik_targets(targets, 1, ik.nchains)
        self.dev.check(lib.mtr_model_animate_ik(self._h, anim._h, masks._h if masks is not None else None, _p(ly), ly.shape[1], ik._h, _p(tg)))

    def render(self, frame: "Frame", view_proj: np.ndarray, joints: bool = False):
        """Model::render(rpass, queue, transform_bind_group, debug_overlay) -- src/model.rs:299-305; the
        transform uniform (src/bin/modelviewer.rs:217-221) is passed directly.  joints: also the per-joint debug cubes the
        reference adds to its overlay every frame (src/model.rs:309-315)."""
        frame.draw_model(self, view_proj)
        if joints:
            vp = _f32(view_proj, 16)
            self.dev.check(lib.mtr_frame_draw_model_joints(frame._h, self._h, _p(vp)))

    def set_joint_positions(self, xyz: np.ndarray):
        """JointInfo::offset of every joint (src/model.rs:283-291)"""
        a = _f32(xyz).reshape(-1, 3)
        self.dev.check(lib.mtr_model_set_joint_positions(self._h, _p(a), a.shape[0]))

    def vertex_stage(self, prim: int, M: np.ndarray):
        from .scene import unpack_primitive
        nv = unpack_primitive(self.md.prims[prim])["vertex_num"]
        clip = np.zeros((nv, 4), dtype=np.float32)
        uv = np.zeros((nv, 2), dtype=np.float32)
        Mf = _f32(M, 16)
        self.dev.check(lib.mtr_model_vertex_stage(self._h, prim, _p(Mf), _p(clip), _p(uv)))
        return clip, uv

    def close(self):
        if self._h:
            lib.mtr_model_destroy(self._h)
            self._h = None
        for t in self.textures:
            t.close()
        self.textures = []


def anim_states(states, n: Optional[int] = None) -> np.ndarray:
    """animation states as a contiguous ANIM_STATE array: from a structured array of that dtype, or from a dict of
    clip_a, clip_b, x_a, x_b, w (arrays or scalars; a missing clip_b / x_b / w is 0)"""
    if isinstance(states, dict):
        unknown = set(states) - set(ANIM_STATE.names)
        if unknown or "clip_a" not in states or "x_a" not in states:
            raise MtrError(MTR_E_INVALID, "animation states: clip_a and x_a, optionally clip_b, x_b and w")
        cols = {k: np.atleast_1d(np.asarray(v)) for k, v in states.items()}
        st = np.zeros(max(c.size for c in cols.values()) if n is None else n, dtype=ANIM_STATE)
        for k, v in cols.items():
            st[k] = v
    else:
        a = np.asarray(states)
        if a.dtype != ANIM_STATE:
            raise MtrError(MTR_E_INVALID, "animation states: an array of dtype ANIM_STATE or a dict of its fields")
        st = np.ascontiguousarray(a).reshape(-1)
    if n is not None and st.size != n:
        raise MtrError(MTR_E_INVALID, f"animation states: {n} expected, {st.size} given")
    return st


def anim_layers(layers, n: Optional[int] = None, L: Optional[int] = None) -> np.ndarray:
    """layer stacks as a contiguous ANIM_LAYER array [n, L] (SPEC.md section 16): from a structured array of that dtype
    ([n, L], or flat with n or L given), or from a dict of clip and x, optionally w, mask and mode (arrays [n, L], or
    anything that broadcasts to it; a missing w is 1, a missing mask / mode 0)"""
    if isinstance(layers, dict):
        unknown = set(layers) - set(ANIM_LAYER.names)
        if unknown or "clip" not in layers or "x" not in layers:
            raise MtrError(MTR_E_INVALID, "animation layers: clip and x, optionally w, mask and mode")
        cols = {k: np.asarray(v) for k, v in layers.items()}
        shape = np.broadcast_shapes(*[c.shape for c in cols.values()])
        if len(shape) > 2:
            raise MtrError(MTR_E_INVALID, "animation layers: fields of shape [n, L]")
        shape = (1,) * (2 - len(shape)) + tuple(shape)
        shape = (n if n is not None and shape[0] == 1 else shape[0], L if L is not None and shape[1] == 1 else shape[1])
        ly = np.zeros(shape, dtype=ANIM_LAYER)
        ly["w"] = 1.0
        for k, v in cols.items():
            ly[k] = v
    else:
        a = np.asarray(layers)
        if a.dtype != ANIM_LAYER:
            raise MtrError(MTR_E_INVALID, "animation layers: an array of dtype ANIM_LAYER or a dict of its fields")
        a = np.ascontiguousarray(a)
        if a.ndim == 2:
            ly = a
        elif n is not None and n and a.size % n == 0:
            ly = a.reshape(n, a.size // n)
        elif L is not None and L and a.size % L == 0:
            ly = a.reshape(a.size // L, L)
        else:
            raise MtrError(MTR_E_INVALID, "animation layers: an [n, L] array")
    if (n is not None and ly.shape[0] != n) or (L is not None and ly.shape[1] != L):
        raise MtrError(MTR_E_INVALID, f"animation layers: [{n}, {L}] expected, {list(ly.shape)} given")
    return ly


def ik_targets(targets, n: Optional[int], K: int) -> np.ndarray:
    """IK targets as a contiguous ANIM_IK_TARGET array [n, K] (SPEC.md section 17): from a structured array of that dtype
    ([n, K] or flat), or from a dict of pos ([n, K, 3]), optionally w ([n, K], missing = 1) and pole ([n, K, 3])"""
    if isinstance(targets, dict):
        unknown = set(targets) - {"pos", "w", "pole"}
        if unknown or "pos" not in targets:
            raise MtrError(MTR_E_INVALID, "ik targets: pos, optionally w and pole")
        pos = _f32(targets["pos"]).reshape(-1, K, 3)
        tg = np.zeros((pos.shape[0], K), dtype=ANIM_IK_TARGET)
        tg["pos"], tg["w"] = pos, 1.0
        if "w" in targets:
            tg["w"] = np.asarray(targets["w"], dtype=np.float32).reshape(-1, K)
        if "pole" in targets:
            tg["pole"] = _f32(targets["pole"]).reshape(-1, K, 3)
    else:
        a = np.asarray(targets)
        if a.dtype != ANIM_IK_TARGET or a.size == 0 or a.size % K:
            raise MtrError(MTR_E_INVALID, "ik targets: an [n, nchains] array of dtype ANIM_IK_TARGET or a dict of its fields")
        tg = np.ascontiguousarray(a).reshape(-1, K)
    if n is not None and tg.shape[0] != n:
        raise MtrError(MTR_E_INVALID, f"ik targets: [{n}, {K}] expected, {list(tg.shape)} given")
    return tg


def attach_records(recs, n: Optional[int]) -> np.ndarray:
    """attachment records as a contiguous flat ATTACH array (SPEC.md section 18): from a structured array of that dtype, or
    from a dict of src_instance ([n]), optionally joint ([n], missing = ATTACH_NO_JOINT), flags ([n], missing = 0) and
    offset ([n, 16], column-major, missing = the identity)"""
    if isinstance(recs, dict):
        unknown = set(recs) - {"src_instance", "joint", "flags", "offset"}
        if unknown or "src_instance" not in recs:
            raise MtrError(MTR_E_INVALID, "attach records: src_instance, optionally joint, flags and offset")
        si = np.asarray(recs["src_instance"], dtype=np.uint32).reshape(-1)
        rc = np.zeros(si.shape[0], dtype=ATTACH)
        rc["src_instance"], rc["joint"] = si, ATTACH_NO_JOINT
        rc["offset"] = np.eye(4, dtype=np.float32).reshape(16)
        if "joint" in recs:
            rc["joint"] = np.asarray(recs["joint"], dtype=np.uint32).reshape(-1)
        if "flags" in recs:
            rc["flags"] = np.asarray(recs["flags"], dtype=np.uint32).reshape(-1)
        if "offset" in recs:
            rc["offset"] = _f32(recs["offset"]).reshape(-1, 16)
    else:
        a = np.asarray(recs)
        if a.dtype != ATTACH or a.size == 0:
            raise MtrError(MTR_E_INVALID, "attach records: an array of dtype ATTACH or a dict of its fields")
        rc = np.ascontiguousarray(a).reshape(-1)
    if n is not None and rc.shape[0] != n:
        raise MtrError(MTR_E_INVALID, f"attach records: {n} expected, {rc.shape[0]} given")
    return rc


def root_steps(steps, n: Optional[int]) -> np.ndarray:
    """root-motion steps as a contiguous ROOT_STEP array [n, S] (SPEC.md section 19): from a structured array [n, S] or [n]
    of that dtype, or from a dict of its fields (clip, x, dx, optionally w; each [n, S] or [n])"""
    if isinstance(steps, dict):
        if set(steps) - set(ROOT_STEP.names) or not {"clip", "x", "dx"} <= set(steps):
            raise MtrError(MTR_E_INVALID, "root steps: clip, x and dx, optionally w")
        x = np.asarray(steps["x"], dtype=np.float32)
        st = np.zeros(x.shape if x.ndim == 2 else (x.size, 1), dtype=ROOT_STEP)
        for k, v in steps.items():
            st[k] = np.asarray(v).reshape(st.shape)
    else:
        st = np.asarray(steps)
        if st.dtype != ROOT_STEP or st.ndim not in (1, 2):
            raise MtrError(MTR_E_INVALID, "root steps: an array [n, S] of dtype ROOT_STEP or a dict of its fields")
        st = st.reshape(st.shape[0], -1)
    if n is not None and st.shape[0] != n:
        raise MtrError(MTR_E_INVALID, f"root steps: {n} instances expected, {st.shape[0]} given")
    return np.ascontiguousarray(st)


class _Set:
    """What the animation set classes share: the device ``dev``, the library's handle ``_h`` and the name of the library
    function that destroys it."""
    _destroy = ""

    def close(self):
        if self._h:
            getattr(lib, self._destroy)(self._h)
            self._h = None


def _clip_arrays(size_msg: str, nkeys, flags, *rates):
    """The per-clip arrays of a set's create as contiguous arrays: (uint32 key counts, uint32 flag words or None), and the
    float32 rates behind them for a set that has rates.  ``size_msg``: what to say when they do not hold one entry per clip."""
    nk = np.ascontiguousarray(np.asarray(nkeys, dtype=np.uint32).reshape(-1))
    rt = [np.ascontiguousarray(np.asarray(r, dtype=np.float32).reshape(-1)) for r in rates]
    fl = None if flags is None else np.ascontiguousarray(np.asarray(flags, dtype=np.uint32).reshape(-1))
    if any(r.size != nk.size for r in rt) or (fl is not None and fl.size != nk.size):
        raise MtrError(MTR_E_INVALID, size_msg)
    return (nk, fl, *rt)


class AnimRoot(_Set):
    """A root set (include/mtr.h, SPEC.md section 19) for trajectory sets of ``njoints`` joints and ``nclips`` clips: the
    trajectory joint and one flag word per clip (0 or ROOT_CYCLIC; None: all 0)."""
    _destroy = "mtr_anim_root_destroy"

    def __init__(self, dev: Device, njoints: int, nclips: int, joint: int = 0, flags=None):
        fl = None if flags is None else np.ascontiguousarray(np.asarray(flags, dtype=np.uint32).reshape(-1))
        if fl is not None and fl.size != nclips:
            raise MtrError(MTR_E_INVALID, "anim root: one flag word per clip")
        if not 0 <= joint <= 0xFFFFFFFF:
            raise MtrError(MTR_E_INVALID, "anim root: the trajectory joint lies past the set's joints")
        h = C.c_void_p()
        dev.check(lib.mtr_anim_root_create(dev._h, njoints, nclips, joint, _p(fl), C.byref(h)))
        self.dev, self._h, self.njoints, self.nclips, self.joint = dev, h, njoints, nclips, joint

    def deltas(self, traj: "Anim", steps) -> np.ndarray:
        """the delta matrices alone, [n, 16], of the given steps ([n, S]) on the trajectory set ``traj`` (character controllers,
        collision).  A numpy ROOT_STEP array or a dict is copied in and the result waited for; a torch uint8 [n, S, 16] /
        int32 / float32 [n, S, 4] tensor on the GPU is read in stream order on torch.cuda.current_stream() and a float32
        tensor [n, 16] on the GPU is returned without a wait."""
        if isinstance(steps, (np.ndarray, dict)):
            st = root_steps(steps, None)
            out = np.zeros((st.shape[0], 16), dtype=np.float32)
            self.dev.check(lib.mtr_anim_root_deltas(traj._h, self._h, _p(st), st.shape[1], st.shape[0], _p(out), out.size))
            return out
        import torch
        t, cur = _root_tensor(steps, self.dev, "root deltas", None, None)
        with torch.cuda.stream(cur):
            out = torch.empty((t.shape[0], 16), dtype=torch.float32, device=t.device)
        _on_stream(self.dev, cur, lib.mtr_anim_root_deltas_device,
                   (traj._h, self._h, C.c_void_p(t.data_ptr()), t.shape[1], t.shape[0], C.c_void_p(out.data_ptr())), (t, out))
        return out


def _root_tensor(t, dev: "Device", what: str, n: Optional[int], stream):
    """ROOT_STEP records [n, S] on the GPU (n None: any count) as _device_records returns them"""
    t, cur = _device_records(t, dev, what, "a numpy ROOT_STEP array, a dict, or a uint8 / int32 / float32 tensor on the GPU", _U8_I32_F32,
                             size_ok=lambda t: t.dim() >= 2 and t.shape[-1] * t.element_size() == ROOT_STEP.itemsize,
                             size_msg="steps of 16 bytes, [n, S, 16] uint8 or [n, S, 4] int32 / float32", stream=stream, owner="device is")
    if t.dim() != 3 or (n is not None and t.shape[0] != n):
        raise MtrError(MTR_E_INVALID, f"{what}: a tensor [n, S, 16 bytes]")
    return t, cur


def play_cmds(cmds) -> np.ndarray:
    """player commands as a contiguous PLAY_CMD array [m] (SPEC.md section 20): from a structured array of that dtype, a dict
    of its fields (instance, clip, optionally x and seconds) or None (no commands)"""
    if cmds is None:
        return np.zeros(0, dtype=PLAY_CMD)
    if isinstance(cmds, dict):
        if set(cmds) - set(PLAY_CMD.names) or not {"instance", "clip"} <= set(cmds):
            raise MtrError(MTR_E_INVALID, "player commands: instance and clip, optionally x and seconds")
        c = np.zeros(np.asarray(cmds["instance"]).size, dtype=PLAY_CMD)
        for k, v in cmds.items():
            c[k] = np.asarray(v).reshape(-1)
        return c
    c = np.asarray(cmds)
    if c.dtype != PLAY_CMD or c.ndim != 1:
        raise MtrError(MTR_E_INVALID, "player commands: an array [m] of dtype PLAY_CMD or a dict of its fields")
    return np.ascontiguousarray(c)


def _play_tensor(t, dev: "Device", what: str, record: int, align: int, count: Optional[int]):
    """a tensor the player reads or writes IN PLACE: on the device, contiguous, aligned, count records of `record` bytes"""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.uint8, torch.int32, torch.float32):
        raise MtrError(MTR_E_INVALID, f"{what}: a uint8 / int32 / float32 tensor on the GPU")
    if t.get_device() != dev.hip_device:
        raise MtrError(MTR_E_INVALID, f"{what}: the tensor is on cuda:{t.get_device()}, the device is cuda:{dev.hip_device}")
    if not t.is_contiguous() or t.data_ptr() % align:
        raise MtrError(MTR_E_INVALID, f"{what}: contiguous and {align}-byte aligned (it is used in place)")
    nbytes = t.numel() * t.element_size()
    if nbytes == 0 or nbytes % record or (count is not None and nbytes != count * record):
        raise MtrError(MTR_E_INVALID, f"{what}: records of {record} bytes" + ("" if count is None else f", {count} of them"))
    return nbytes // record


def _want_dtype(t, dtype, msg: str):
    if getattr(t, "dtype", None) != dtype:
        raise MtrError(MTR_E_INVALID, msg)


class _InPlaceArgs:
    """The tensors that one device call of a player, controller, event set or blend set reads or writes IN PLACE: each is
    checked as it is added (_play_tensor, after its dtype where one is required) and kept, so that the call can tell the
    allocator which stream uses them."""

    def __init__(self, dev: "Device"):
        self.dev, self.used = dev, []

    def add(self, t, what: str, record: int, align: int, count: Optional[int], dtype=None, dtype_msg: str = "") -> int:
        """checks ``t`` and returns the number of records it holds"""
        if dtype is not None:
            _want_dtype(t, dtype, dtype_msg)
        k = _play_tensor(t, self.dev, what, record, align, count)
        self.used.append(t)
        return k

    def layers(self, t, what: str, n: int) -> int:
        """``t``: None or n x L ANIM_LAYER records; returns L, 0 for None"""
        if t is None:
            return 0
        nl = self.add(t, what, ANIM_LAYER.itemsize, 16, None)
        if nl % n:
            raise MtrError(MTR_E_INVALID, f"{what}: n x L layers of 16 bytes")
        return nl // n

    @staticmethod
    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def call(self, fn, args, stream):
        """``fn(*args, stream handle)`` in stream order on ``stream`` (None: the current stream of the first tensor's device)"""
        import torch
        cur = stream if stream is not None else torch.cuda.current_stream(self.used[0].device)
        _on_stream(self.dev, cur, fn, args, self.used)


def _layers_in(n: int, nlayers: int, layers) -> Optional[np.ndarray]:
    """the ANIM_LAYER stacks [n, nlayers] a host hook sends in and gets back: a copy of ``layers``, zeroes, or None (no layers)"""
    if not nlayers:
        return None
    return np.zeros((n, nlayers), dtype=ANIM_LAYER) if layers is None else np.ascontiguousarray(layers).copy().reshape(n, nlayers)


class AnimPlayer(_Set):
    """A player set (include/mtr.h, SPEC.md section 20), the library's clock: per clip the key count (ticks for a track set),
    the flag word (0 or CLIP_LOOP; None: all 0) and the rate in positions per second, for up to ``max_instances`` play states
    that live in a tensor of the caller's on the GPU."""
    _destroy = "mtr_anim_player_destroy"

    def __init__(self, dev: Device, nkeys, rates, flags=None, max_instances: int = 1):
        nk, fl, rt = _clip_arrays("anim player: one key count, one rate and one flag word per clip", nkeys, flags, rates)
        h = C.c_void_p()
        dev.check(lib.mtr_anim_player_create(dev._h, nk.size, _p(nk), _p(fl), _p(rt), max_instances, C.byref(h)))
        self.dev, self._h, self.nclips, self.max_instances = dev, h, nk.size, max_instances

    def advance(self, states, dt: float, cmds=None, out_states=None, out_layers=None, out_steps=None, stream=None):
        """advances the n PLAY_STATE records of ``states`` (a torch uint8 [n, 32] / int32 / float32 [n, 8] tensor on the GPU,
        16-byte aligned) by ``dt`` seconds IN PLACE and writes, where given, ANIM_STATE records into ``out_states`` ([n, 24]
        bytes), layers 0 and 1 of the ANIM_LAYER stacks of ``out_layers`` ([n, L, 16] bytes, L from its size) and two
        ROOT_STEP records per instance into ``out_steps`` ([n, 2, 16] bytes), in stream order on ``stream`` (a torch stream;
        None: torch.cuda.current_stream()).  cmds: None, a PLAY_CMD array or a dict (host memory, copied before the call
        returns), or a tensor of PLAY_CMD records on the GPU (read in stream order)."""
        import torch
        a = _InPlaceArgs(self.dev)
        n = a.add(states, "player states", PLAY_STATE.itemsize, 16, None)
        if out_states is not None:
            a.add(out_states, "player out_states", ANIM_STATE.itemsize, 8, n)
        nl = a.layers(out_layers, "player out_layers", n)
        if out_steps is not None:
            a.add(out_steps, "player out_steps", ROOT_STEP.itemsize, 16, 2 * n)
        if isinstance(cmds, torch.Tensor):
            m = a.add(cmds, "player commands", PLAY_CMD.itemsize, 16, None)
            fn, cp, keep = lib.mtr_anim_player_advance_device_cmds, a.ptr(cmds), None
        else:
            keep = play_cmds(cmds)
            m, fn, cp = keep.size, lib.mtr_anim_player_advance_device, (_p(keep) if keep.size else None)
        a.call(fn, (self._h, a.ptr(states), n, float(dt), cp, m, a.ptr(out_states), a.ptr(out_layers), nl, a.ptr(out_steps)), stream)

    def advance_host(self, states: np.ndarray, dt: float, cmds=None, nlayers: int = 0, layers: Optional[np.ndarray] = None, want_states: bool = True,
                     want_steps: bool = True):
        """the test and debug hook: PLAY_STATE records [n] in host memory through the same kernel; waits.  Returns (states,
        out_states or None, out_layers or None, out_steps or None); ``layers`` ([n, nlayers] ANIM_LAYER) is what layers 2..
        hold going in."""
        st = np.ascontiguousarray(np.asarray(states)).copy()
        if st.dtype != PLAY_STATE or st.ndim != 1:
            raise MtrError(MTR_E_INVALID, "player states: an array [n] of dtype PLAY_STATE")
        n = st.size
        cm = play_cmds(cmds)
        oa = np.zeros(n, dtype=ANIM_STATE) if want_states else None
        ol = _layers_in(n, nlayers, layers)
        os_ = np.zeros((n, 2), dtype=ROOT_STEP) if want_steps else None
        self.dev.check(lib.mtr_anim_player_advance_host(self._h, _p(st), n, float(dt), _p(cm) if cm.size else None, cm.size, _p(oa), _p(ol), nlayers, _p(os_)))
        return st, oa, ol, os_


class AnimCtrl(_Set):
    """A controller (include/mtr.h, SPEC.md section 21): per-instance state machines that write a player's commands on the
    GPU.  ``nkeys`` and ``clip_flags`` are what the AnimPlayer was given; ``nodes`` a CTRL_NODE array, ``trans`` a CTRL_TRANS
    array whose first ``nany`` entries are the any-state transitions (``anim_ctrl.build`` makes the three from a readable
    description), ``nparams`` the floats per instance that conditions may name."""

    _destroy = "mtr_anim_ctrl_destroy"

    def __init__(self, dev: Device, nkeys, clip_flags, nodes, trans, nany: int = 0, nparams: int = 0):
        msg = "anim ctrl: one flag word per clip, nodes of dtype CTRL_NODE [S] and transitions of dtype CTRL_TRANS [T]"
        nk, fl = _clip_arrays(msg, nkeys, clip_flags)
        nd, tr = np.asarray(nodes), np.asarray(trans)
        if nd.dtype != CTRL_NODE or tr.dtype != CTRL_TRANS or nd.ndim != 1 or tr.ndim != 1:
            raise MtrError(MTR_E_INVALID, msg)
        nd, tr = np.ascontiguousarray(nd), np.ascontiguousarray(tr)
        h = C.c_void_p()
        dev.check(lib.mtr_anim_ctrl_create(dev._h, nk.size, _p(nk), _p(fl), _p(nd), nd.size, _p(tr) if tr.size else None, tr.size, nany, nparams, C.byref(h)))
        self.dev, self._h, self.nclips, self.nnodes, self.ntrans, self.nany, self.nparams = dev, h, nk.size, nd.size, tr.size, nany, nparams

    def step(self, states, play, params, dt: float, cmds_out, counts=None, stream=None):
        """one step of the n CTRL_STATE records of ``states`` ([n, 16] bytes on the GPU, 16-byte aligned) IN PLACE against the
        PLAY_STATE records of ``play`` ([n, 32] bytes, read only) and the rows of ``params`` (float32 [n, nparams], None when
        nparams == 0; CONSUME writes it); writes PLAY_CMD slot i of ``cmds_out`` (at least n slots of 16 bytes; a longer
        tensor leaves room for the host's own commands behind slot n - 1) and adds to ``counts`` (int32 [ntrans]) where
        given, in stream order on ``stream`` (a torch stream; None: torch.cuda.current_stream())."""
        import torch
        a = _InPlaceArgs(self.dev)
        n = a.add(states, "ctrl states", CTRL_STATE.itemsize, 16, None)
        a.add(play, "ctrl play states", PLAY_STATE.itemsize, 16, n)
        if a.add(cmds_out, "ctrl commands", PLAY_CMD.itemsize, 16, None) < n:
            raise MtrError(MTR_E_INVALID, "ctrl commands: at least n slots of 16 bytes")
        if self.nparams:
            a.add(params, "ctrl params", 4 * self.nparams, 4, n, torch.float32, "ctrl params: a float32 tensor [n, nparams] on the GPU")
        else:
            params = None
        if counts is not None:
            _want_dtype(counts, torch.int32, "ctrl counts: an int32 tensor [ntrans] on the GPU")
            if self.ntrans == 0 or a.add(counts, "ctrl counts", 4, 4, None) < self.ntrans:
                raise MtrError(MTR_E_INVALID, "ctrl counts: one word per transition")
        a.call(lib.mtr_anim_ctrl_step_device, (self._h, a.ptr(states), a.ptr(play), a.ptr(params), n, float(dt), a.ptr(cmds_out), a.ptr(counts)), stream)

    def step_host(self, states: np.ndarray, play: np.ndarray, params, dt: float, counts: Optional[np.ndarray] = None):
        """the test and debug hook: CTRL_STATE [n], PLAY_STATE [n] and float32 [n, nparams] in host memory through the same
        kernel; waits.  Returns (states, params or None, PLAY_CMD [n], counts or None); ``counts`` (uint32 [ntrans]) is added to."""
        st = np.ascontiguousarray(np.asarray(states)).copy()
        pl = np.ascontiguousarray(np.asarray(play))
        if st.dtype != CTRL_STATE or st.ndim != 1 or pl.dtype != PLAY_STATE or pl.shape != st.shape:
            raise MtrError(MTR_E_INVALID, "ctrl states: arrays [n] of dtype CTRL_STATE and PLAY_STATE")
        n = st.size
        pr = None
        if self.nparams:
            pr = np.ascontiguousarray(np.asarray(params, dtype=np.float32)).copy()
            if pr.shape != (n, self.nparams):
                raise MtrError(MTR_E_INVALID, "ctrl params: float32 [n, nparams]")
        ct = None
        if counts is not None:
            ct = np.ascontiguousarray(np.asarray(counts, dtype=np.uint32)).copy()
            if ct.shape != (self.ntrans,):
                raise MtrError(MTR_E_INVALID, "ctrl counts: uint32 [ntrans]")
        cm = np.zeros(n, dtype=PLAY_CMD)
        self.dev.check(lib.mtr_anim_ctrl_step_host(self._h, _p(st), _p(pl), _p(pr), n, float(dt), _p(cm), _p(ct) if ct is not None and ct.size else None))
        return st, pr, cm, ct


class AnimEvents(_Set):
    """An event set (include/mtr.h, SPEC.md section 22): markers on clips that fire into a list on the GPU.  ``nkeys`` and
    ``clip_flags`` are what the AnimPlayer was given; ``counts`` holds the markers per clip and ``markers`` an EVENT_MARKER
    array of them, clip after clip, sorted by x within a clip (``anim_events.build`` makes the two from a dict), for calls of
    up to ``max_instances`` instances."""

    _destroy = "mtr_anim_events_destroy"

    def __init__(self, dev: Device, nkeys, clip_flags, counts, markers, max_instances: int = 1):
        msg = "anim events: one flag word and one marker count per clip, markers of dtype EVENT_MARKER [sum of counts]"
        nk, fl = _clip_arrays(msg, nkeys, clip_flags)
        ct = np.ascontiguousarray(np.asarray(counts, dtype=np.uint32).reshape(-1))
        mk = np.asarray(markers)
        if ct.size != nk.size or mk.dtype != EVENT_MARKER or mk.ndim != 1 or mk.size != int(ct.sum(dtype=np.uint64)):
            raise MtrError(MTR_E_INVALID, msg)
        mk = np.ascontiguousarray(mk)
        h = C.c_void_p()
        dev.check(lib.mtr_anim_events_create(dev._h, nk.size, _p(nk), _p(fl), _p(ct), _p(mk) if mk.size else None, max_instances, C.byref(h)))
        self.dev, self._h, self.nclips, self.nmarkers, self.max_instances = dev, h, nk.size, mk.size, max_instances

    def collect(self, steps, min_weight: float, out, count, bits=None, stream=None):
        """the markers that the S steps of each of n instances arrived at or passed: ``steps`` holds ROOT_STEP records ([n, S,
        16] bytes on the GPU, 16-byte aligned: a player's out_steps), ``out`` takes up to its size of EVENT records (16 bytes
        each, 16-byte aligned; None: capacity 0), ``count`` (int32 [2]) the number fired and the number written, ``bits``
        (int32 [n], optional) the mask of each instance, in stream order on ``stream`` (a torch stream; None:
        torch.cuda.current_stream())."""
        import torch
        if not isinstance(steps, torch.Tensor) or steps.dim() != 3 or steps.shape[1] < 1 or steps.shape[2] * steps.element_size() != ROOT_STEP.itemsize:
            raise MtrError(MTR_E_INVALID, "events steps: a tensor [n, S, 16 bytes] on the GPU")
        n, S = steps.shape[0], steps.shape[1]
        a = _InPlaceArgs(self.dev)
        a.add(steps, "events steps", ROOT_STEP.itemsize, 16, n * S)
        cap = a.add(out, "events list", EVENT.itemsize, 16, None) if out is not None else 0
        a.add(count, "events count", 4, 4, 2, torch.int32, "events count: an int32 tensor [2] on the GPU")
        if bits is not None:
            a.add(bits, "events bits", 4, 4, n, torch.int32, "events bits: an int32 tensor [n] on the GPU")
        a.call(lib.mtr_anim_events_collect_device, (self._h, a.ptr(steps), S, n, float(min_weight), a.ptr(out), cap, a.ptr(count), a.ptr(bits)), stream)

    def collect_host(self, steps: np.ndarray, min_weight: float, capacity: int, out: Optional[np.ndarray] = None, bits: Optional[np.ndarray] = None,
                     want_bits: bool = True):
        """the test and debug hook: ROOT_STEP [n, S] in host memory through the same kernels; waits.  Returns (EVENT [capacity],
        uint32 [2], uint32 [n] or None); ``out`` and ``bits`` are what the list and the masks hold going in."""
        sp = np.ascontiguousarray(np.asarray(steps))
        if sp.dtype != ROOT_STEP or sp.ndim != 2 or sp.shape[1] < 1:
            raise MtrError(MTR_E_INVALID, "events steps: an array [n, S] of dtype ROOT_STEP")
        n, S = sp.shape
        ol = np.zeros(capacity, dtype=EVENT) if out is None else np.ascontiguousarray(np.asarray(out)).copy()
        if ol.dtype != EVENT or ol.shape != (capacity,):
            raise MtrError(MTR_E_INVALID, "events list: EVENT [capacity]")
        bt = None
        if want_bits:
            bt = np.zeros(n, dtype=np.uint32) if bits is None else np.ascontiguousarray(np.asarray(bits, dtype=np.uint32)).copy()
            if bt.shape != (n,):
                raise MtrError(MTR_E_INVALID, "events bits: uint32 [n]")
        ct = np.zeros(2, dtype=np.uint32)
        self.dev.check(lib.mtr_anim_events_collect_host(self._h, _p(sp), S, n, float(min_weight), _p(ol) if capacity else None, capacity, _p(ct), _p(bt)))
        return ol, ct, bt


class AnimBlend(_Set):
    """A blend set (include/mtr.h, SPEC.md section 23): sample points in a 1-D or 2-D parameter space that each carry a LOOP
    clip.  ``nkeys``, ``rates`` and ``clip_flags`` are what an AnimPlayer takes; ``samples`` a BLEND_SAMPLE array, ``tris`` a
    BLEND_TRI array or None for a 1-D space (``anim_blend.build_1d`` / ``build_2d`` make them from points); ``param_x`` and
    ``param_y`` name the floats of an instance's row of ``nparams`` parameters, ``damp`` is the smoothing rate in 1/seconds
    (inf: none), for calls of up to ``max_instances`` instances."""
    _destroy = "mtr_anim_blend_destroy"

    def __init__(self, dev: Device, nkeys, rates, clip_flags, samples, tris=None, nparams: int = 1, param_x: int = 0, param_y: int = 0,
                 damp: float = float("inf"), max_instances: int = 1):
        msg = "anim blend: one key count, rate and flag word per clip, samples of dtype BLEND_SAMPLE [K], triangles of dtype BLEND_TRI [T]"
        nk, fl, rt = _clip_arrays(msg, nkeys, clip_flags, rates)
        sm = np.asarray(samples)
        tr = np.zeros(0, dtype=BLEND_TRI) if tris is None else np.asarray(tris)
        if sm.dtype != BLEND_SAMPLE or sm.ndim != 1 or tr.dtype != BLEND_TRI or tr.ndim != 1:
            raise MtrError(MTR_E_INVALID, msg)
        if not (0 <= param_x < 1 << 32 and 0 <= param_y < 1 << 32):
            raise MtrError(MTR_E_INVALID, "anim blend: param_x and param_y are parameter indices")
        sm, tr = np.ascontiguousarray(sm), np.ascontiguousarray(tr)
        h = C.c_void_p()
        dev.check(lib.mtr_anim_blend_create(dev._h, nk.size, _p(nk), _p(fl), _p(rt), _p(sm) if sm.size else None, sm.size, _p(tr) if tr.size else None, tr.size,
                                            nparams, param_x, param_y, float(damp), max_instances, C.byref(h)))
        self.dev, self._h, self.nclips, self.nsamples, self.ntris, self.nparams, self.max_instances = dev, h, nk.size, sm.size, tr.size, nparams, max_instances

    def advance(self, states, params, dt: float, out_layers=None, out_steps=None, out_shares=None, stream=None):
        """advances the n BLEND_STATE records of ``states`` (a torch uint8 [n, 16] / int32 / float32 [n, 4] tensor on the GPU,
        16-byte aligned) by ``dt`` seconds IN PLACE against the rows of ``params`` (float32 [n, nparams], read only) and writes,
        where given, layers 0 to 2 of the ANIM_LAYER stacks of ``out_layers`` ([n, L, 16] bytes, L from its size), three
        ROOT_STEP records per instance into ``out_steps`` ([n, 3, 16] bytes) and the three shares into ``out_shares`` (float32
        [n, 3]), in stream order on ``stream`` (a torch stream; None: torch.cuda.current_stream())."""
        import torch
        a = _InPlaceArgs(self.dev)
        n = a.add(states, "blend states", BLEND_STATE.itemsize, 16, None)
        a.add(params, "blend params", 4, 4, n * self.nparams, torch.float32, "blend params: a float32 tensor [n, nparams] on the GPU")
        nl = a.layers(out_layers, "blend out_layers", n)
        if out_steps is not None:
            a.add(out_steps, "blend out_steps", ROOT_STEP.itemsize, 16, 3 * n)
        if out_shares is not None:
            a.add(out_shares, "blend out_shares", 4, 4, 3 * n, torch.float32, "blend out_shares: a float32 tensor [n, 3] on the GPU")
        a.call(lib.mtr_anim_blend_advance_device,
               (self._h, a.ptr(states), a.ptr(params), n, float(dt), a.ptr(out_layers), nl, a.ptr(out_steps), a.ptr(out_shares)), stream)

    def advance_host(self, states: np.ndarray, params: np.ndarray, dt: float, nlayers: int = 0, layers: Optional[np.ndarray] = None, want_steps: bool = True,
                     want_shares: bool = True):
        """the test and debug hook: BLEND_STATE records [n] and float32 rows [n, nparams] in host memory through the same kernel;
        waits.  Returns (states, out_layers or None, out_steps or None, out_shares or None); ``layers`` ([n, nlayers]
        ANIM_LAYER) is what layers 3.. hold going in."""
        st = np.ascontiguousarray(np.asarray(states)).copy()
        if st.dtype != BLEND_STATE or st.ndim != 1:
            raise MtrError(MTR_E_INVALID, "blend states: an array [n] of dtype BLEND_STATE")
        n = st.size
        pr = np.ascontiguousarray(np.asarray(params, dtype=np.float32))
        if pr.shape != (n, self.nparams):
            raise MtrError(MTR_E_INVALID, "blend params: float32 [n, nparams]")
        ol = _layers_in(n, nlayers, layers)
        os_ = np.zeros((n, 3), dtype=ROOT_STEP) if want_steps else None
        sh = np.zeros((n, 3), dtype=np.float32) if want_shares else None
        self.dev.check(lib.mtr_anim_blend_advance_host(self._h, _p(st), _p(pr), n, float(dt), _p(ol), nlayers, _p(os_), _p(sh)))
        return st, ol, os_, sh


class AnimMatch(_Set):
    """A match set (include/mtr.h, SPEC.md section 25): nearest-pose search per instance that writes a player's commands on the
    GPU.  ``nkeys`` and ``clip_flags`` are what the AnimPlayer was given; ``rows`` a MATCH_ROW array [R] sorted by clip and by x
    within a clip, ``features`` float32 [R, D], already normalised and weighted (``anim_match.normalise`` and ``rows_of`` make
    them); ``pose_dims`` has bit d set where dimension d is taken from the pose being played, ``mean`` and ``scale`` (float32
    [D], None: 0 and 1) normalise the raw query; ``seconds`` is the fade of a jump, ``near`` and ``margin`` say when a winner is
    not worth one; for calls of up to ``max_instances`` instances."""

    _destroy = "mtr_anim_match_destroy"

    def __init__(self, dev: Device, nkeys, clip_flags, rows, features, pose_dims: int = 0, flags: int = 0, seconds: float = 0.2, near: float = 0.0,
                 margin: float = 0.0, mean=None, scale=None, max_instances: int = 1):
        msg = "anim match: one flag word per clip, rows of dtype MATCH_ROW [R], features float32 [R, D], mean and scale float32 [D]"
        nk, fl = _clip_arrays(msg, nkeys, clip_flags)
        rw, ft = np.asarray(rows), np.ascontiguousarray(np.asarray(features, dtype=np.float32))
        if rw.dtype != MATCH_ROW or rw.ndim != 1 or ft.ndim != 2 or ft.shape[0] != rw.size:
            raise MtrError(MTR_E_INVALID, msg)
        D = ft.shape[1]
        mn, sc = (None if v is None else np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1)) for v in (mean, scale))
        if any(v is not None and v.size != D for v in (mn, sc)):
            raise MtrError(MTR_E_INVALID, msg)
        if not (0 <= pose_dims < 1 << 64 and 0 <= flags < 1 << 32):
            raise MtrError(MTR_E_INVALID, "anim match: pose_dims is a 64-bit and flags a 32-bit word")
        rw = np.ascontiguousarray(rw)
        h = C.c_void_p()
        dev.check(lib.mtr_anim_match_create(dev._h, nk.size, _p(nk), _p(fl), D, pose_dims, flags, float(seconds), float(near), float(margin),
                                            _p(rw) if rw.size else None, rw.size, _p(ft) if ft.size else None, _p(mn), _p(sc), max_instances, C.byref(h)))
        self.dev, self._h, self.nclips, self.nrows, self.D, self.pose_dims, self.max_instances = dev, h, nk.size, rw.size, D, pose_dims, max_instances

    @property
    def needs_query(self) -> bool:
        return self.pose_dims != (1 << self.D) - 1

    def search(self, play, query, cmds_out, filters=None, results=None, instance_base: int = 0, stream=None):
        """one search for the n PLAY_STATE records of ``play`` ([n, 32] bytes on the GPU, 16-byte aligned, read only) against
        the raw queries of ``query`` (float32 [n, D]; None when every dimension is a pose dimension) and, where given, the
        MATCH_FILTER records of ``filters`` ([n, 8] bytes); writes PLAY_CMD slot i of ``cmds_out`` (at least n slots of 16
        bytes; a longer tensor leaves room for the host's own commands behind slot n - 1) as {instance_base + i, ...} and,
        where given, the MATCH_RESULT records of ``results`` ([n, 16] bytes), in stream order on ``stream`` (a torch stream;
        None: torch.cuda.current_stream()).  A slice of a crowd: play[k:k + m], query[k:k + m], cmds[k:k + m], instance_base=k."""
        import torch
        a = _InPlaceArgs(self.dev)
        n = a.add(play, "match play states", PLAY_STATE.itemsize, 16, None)
        if a.add(cmds_out, "match commands", PLAY_CMD.itemsize, 16, None) < n:
            raise MtrError(MTR_E_INVALID, "match commands: at least n slots of 16 bytes")
        if query is not None:
            a.add(query, "match query", 4 * self.D, 16, n, torch.float32, "match query: a float32 tensor [n, D] on the GPU")
        elif self.needs_query:
            raise MtrError(MTR_E_INVALID, "match query: the set has dimensions that are not pose dimensions and no query is given")
        if filters is not None:
            a.add(filters, "match filters", MATCH_FILTER.itemsize, 8, n)
        if results is not None:
            a.add(results, "match results", MATCH_RESULT.itemsize, 16, n)
        if not 0 <= instance_base <= 0xFFFFFFFF:
            raise MtrError(MTR_E_INVALID, "match search: instance_base is a 32-bit index")
        a.call(lib.mtr_anim_match_search_device, (self._h, a.ptr(play), a.ptr(query), a.ptr(filters), n, instance_base, a.ptr(cmds_out), a.ptr(results)), stream)

    def _host_in(self, play, query):
        pl = np.ascontiguousarray(np.asarray(play))
        if pl.dtype != PLAY_STATE or pl.ndim != 1:
            raise MtrError(MTR_E_INVALID, "match play states: an array [n] of dtype PLAY_STATE")
        qr = None
        if query is not None:
            qr = np.ascontiguousarray(np.asarray(query, dtype=np.float32))
            if qr.shape != (pl.size, self.D):
                raise MtrError(MTR_E_INVALID, "match query: float32 [n, D]")
        return pl, qr

    def search_host(self, play: np.ndarray, query, filters: Optional[np.ndarray] = None, instance_base: int = 0, want_results: bool = True):
        """the test and debug hook: PLAY_STATE [n], float32 [n, D] (or None) and MATCH_FILTER [n] (or None) in host memory
        through the same kernels; waits.  Returns (PLAY_CMD [n], MATCH_RESULT [n] or None)."""
        pl, qr = self._host_in(play, query)
        n = pl.size
        fl = None
        if filters is not None:
            fl = np.ascontiguousarray(np.asarray(filters))
            if fl.dtype != MATCH_FILTER or fl.shape != (n,):
                raise MtrError(MTR_E_INVALID, "match filters: an array [n] of dtype MATCH_FILTER")
        cm = np.zeros(n, dtype=PLAY_CMD)
        rs = np.zeros(n, dtype=MATCH_RESULT) if want_results else None
        self.dev.check(lib.mtr_anim_match_search_host(self._h, _p(pl), _p(qr), _p(fl), n, instance_base, _p(cm), _p(rs)))
        return cm, rs

    def scores_host(self, play: np.ndarray, query) -> np.ndarray:
        """the test and debug hook: every score, float32 [n, R], from the search kernel itself; waits"""
        pl, qr = self._host_in(play, query)
        out = np.zeros((pl.size, self.nrows), dtype=np.float32)
        self.dev.check(lib.mtr_anim_match_scores_host(self._h, _p(pl), _p(qr), pl.size, _p(out)))
        return out


class AnimIK(_Set):
    """An IK set (include/mtr.h, SPEC.md section 17): the parents of a skeleton of ``njoints`` joints (a root: 255 or itself)
    and 1 to 4 chains, an ANIM_IK_CHAIN array or a list of dicts of its fields (kind, joint, optionally axis and flags)."""
    _destroy = "mtr_anim_ik_destroy"

    def __init__(self, dev: Device, parents, chains):
        par = np.ascontiguousarray(np.asarray(parents, dtype=np.uint8).reshape(-1))
        if isinstance(chains, np.ndarray):
            if chains.dtype != ANIM_IK_CHAIN:
                raise MtrError(MTR_E_INVALID, "anim ik: chains of dtype ANIM_IK_CHAIN or a list of dicts of its fields")
            ch = np.ascontiguousarray(chains).reshape(-1)
        else:
            ch = np.zeros(len(chains), dtype=ANIM_IK_CHAIN)
            for k, c in enumerate(chains):
                if set(c) - set(ANIM_IK_CHAIN.names) or "kind" not in c or "joint" not in c:
                    raise MtrError(MTR_E_INVALID, "anim ik: a chain has kind and joint, optionally axis and flags")
                jt = np.atleast_1d(np.asarray(c["joint"], dtype=np.uint32))
                ch["kind"][k], ch["flags"][k] = c["kind"], c.get("flags", 0)
                ch["joint"][k, :jt.size] = jt[:3]
                ch["axis"][k] = c.get("axis", (0.0, 0.0, 0.0))
        h = C.c_void_p()
        dev.check(lib.mtr_anim_ik_create(dev._h, par.size, _p(par), ch.size, _p(ch) if ch.size else None, C.byref(h)))
        self.dev, self._h, self.njoints, self.nchains = dev, h, par.size, ch.size

class AnimSpring(_Set):
    """A spring set (include/mtr.h, SPEC.md section 24): the parents of a skeleton of ``njoints`` joints (a root: 255 or itself)
    and 1 to 16 springs, a SPRING array or a list of dicts of its fields (joint and tail, optionally stiffness, drag and
    gravity).  mt_renderer_amd.anim_spring.chain makes the records of a chain of joints."""
    _destroy = "mtr_anim_spring_destroy"

    def __init__(self, dev: Device, parents, springs):
        par = np.ascontiguousarray(np.asarray(parents, dtype=np.uint8).reshape(-1))
        if isinstance(springs, np.ndarray):
            if springs.dtype != SPRING:
                raise MtrError(MTR_E_INVALID, "anim spring: springs of dtype SPRING or a list of dicts of its fields")
            sp = np.ascontiguousarray(springs).reshape(-1)
        else:
            sp = np.zeros(len(springs), dtype=SPRING)
            for k, c in enumerate(springs):
                if set(c) - set(SPRING.names) or "joint" not in c or "tail" not in c:
                    raise MtrError(MTR_E_INVALID, "anim spring: a spring has joint and tail, optionally stiffness, drag, gravity and flags")
                for name, v in c.items():
                    sp[name][k] = v
        h = C.c_void_p()
        dev.check(lib.mtr_anim_spring_create(dev._h, par.size, _p(par), sp.size, _p(sp) if sp.size else None, C.byref(h)))
        self.dev, self._h, self.njoints, self.nsprings = dev, h, par.size, sp.size

class AnimMasks(_Set):
    """A mask set for animation layers (include/mtr.h, SPEC.md section 16): weights [nmasks, njoints] in [0, 1], resident
    in HBM.  A layer's mask index 0 is the built-in mask of ones, index k >= 1 is weights[k - 1]."""
    _destroy = "mtr_anim_masks_destroy"

    def __init__(self, dev: Device, njoints: int, weights):
        w = _f32(weights)
        if njoints < 1 or w.size == 0 or w.size % njoints:
            raise MtrError(MTR_E_INVALID, "anim masks: weights are [nmasks, njoints] float32, at least one mask")
        w = np.ascontiguousarray(w).reshape(-1, njoints)
        h = C.c_void_p()
        dev.check(lib.mtr_anim_masks_create(dev._h, njoints, w.shape[0], _p(w), C.byref(h)))
        self.dev, self._h, self.njoints, self.nmasks = dev, h, njoints, w.shape[0]

class Anim(_Set):
    """An animation set (include/mtr.h, SPEC.md section 14): clips of uniformly spaced keys for ``njoints`` joints, resident
    in HBM.  clips: a list of (keys, flags); keys is [nkeys, njoints, 12] float32 (t.xyz 0 | q.xyzw | s.xyz 0) or an
    ANIM_KEY array [nkeys, njoints]; flags 0 or CLIP_LOOP."""
    _destroy = "mtr_anim_destroy"

    def __init__(self, dev: Device, njoints: int, clips, _handle=None):
        if _handle is not None:  # AnimTracks: created already
            self.dev, self._h, self.njoints, self.nclips = dev, _handle, njoints, len(clips)
            return
        if not 1 <= njoints <= 256:
            raise MtrError(MTR_E_INVALID, "anim: 1 to 256 joints")
        blocks, nkeys, flags = [], [], []
        for keys, fl in clips:
            k = np.asarray(keys)
            k = k.view(np.float32) if k.dtype == ANIM_KEY else _f32(k)
            if k.size % (njoints * 12):
                raise MtrError(MTR_E_INVALID, "anim: keys are [nkeys, njoints, 12] float32")
            k = np.ascontiguousarray(k).reshape(k.size // (njoints * 12), njoints, 12)
            blocks.append(k.reshape(-1, 12))
            nkeys.append(k.shape[0])
            flags.append(int(fl))
        allk = np.ascontiguousarray(np.concatenate(blocks)) if blocks else np.zeros((1, 12), dtype=np.float32)
        nk = np.asarray(nkeys if nkeys else [0], dtype=np.uint32)
        fl = np.asarray(flags if flags else [0], dtype=np.uint32)
        h = C.c_void_p()
        dev.check(lib.mtr_anim_create(dev._h, njoints, len(nkeys), _p(nk), _p(fl), _p(allk), C.byref(h)))
        self.dev, self._h, self.njoints, self.nclips = dev, h, njoints, len(nkeys)

    def sample(self, states) -> np.ndarray:
        """the local matrices [n, njoints, 16] of the given states, formed on the GPU (test / debug hook)"""
        st = anim_states(states)
        out = np.zeros((st.size, self.njoints, 16), dtype=np.float32)
        self.dev.check(lib.mtr_anim_sample(self._h, _p(st), st.size, _p(out), out.size))
        return out

    def sample_layers(self, layers, masks: Optional[AnimMasks] = None) -> np.ndarray:
        """the local matrices [n, njoints, 16] of the given layer stacks ([n, L], SPEC.md section 16), formed on the GPU"""
        ly = anim_layers(layers)
        out = np.zeros((ly.shape[0], self.njoints, 16), dtype=np.float32)
        self.dev.check(lib.mtr_anim_sample_layers(self._h, masks._h if masks is not None else None, _p(ly), ly.shape[1], ly.shape[0], _p(out), out.size))
        return out

    def sample_ik(self, layers, ik: "AnimIK", targets, masks: Optional[AnimMasks] = None) -> np.ndarray:
        """the local matrices [n, njoints, 16] of the given layer stacks ([n, L]) after the chains of ``ik`` have been
        evaluated against ``targets`` ([n, K], SPEC.md section 17), formed on the GPU"""
        ly = anim_layers(layers)
        tg = ik_targets(targets, ly.shape[0], ik.nchains)
        out = np.zeros((ly.shape[0], self.njoints, 16), dtype=np.float32)
        self.dev.check(lib.mtr_anim_sample_ik(self._h, masks._h if masks is not None else None, ik._h, _p(ly), ly.shape[1], _p(tg), ly.shape[0],
                                              _p(out), out.size))
        return out

    def sample_spring(self, layers, spring: "AnimSpring", states, dt: float, ik: Optional["AnimIK"] = None, targets=None, motion=None,
                      masks: Optional[AnimMasks] = None):
        """one step of the springs of ``spring`` (SPEC.md section 24) over the given layer stacks ([n, L]) after the chains of
        ``ik`` (or None), everything in host memory: (the local matrices [n, njoints, 16], the new SPRING_STATE [n, nsprings]).
        states: a SPRING_STATE array [n, nsprings], left as it is; motion: [n, 16] float32 or None"""
        ly = anim_layers(layers)
        n = ly.shape[0]
        st = np.array(states, dtype=SPRING_STATE, copy=True).reshape(n, spring.nsprings)
        tg = ik_targets(targets, n, ik.nchains) if ik is not None and targets is not None else None
        mo = _f32(motion, (n, 16)) if motion is not None else None
        out = np.zeros((n, self.njoints, 16), dtype=np.float32)
        self.dev.check(lib.mtr_anim_sample_spring(self._h, masks._h if masks is not None else None, ik._h if ik is not None else None, spring._h,
                                                  _p(ly), ly.shape[1], _p(tg) if tg is not None else None, _p(st), _p(mo) if mo is not None else None,
                                                  float(dt), n, _p(out), out.size))
        return out, st

def anim_track_arrays(njoints: int, clips):
    """The arrays of mtr_anim_create_tracks from a list of track clips (nticks, flags, tracks, times, values): tracks an
    ANIM_TRACK array [njoints, 3] whose ``first`` counts inside the clip's own times (u16 [nkeys]) and values (u16
    [nkeys, 4]).  The clips are concatenated and ``first`` rebased.  Returns nticks, flags, tracks, times, values."""
    nticks, flags, tracks, times, values, base = [], [], [], [], [], 0
    for nt, fl, tr, tm, va in clips:
        tr = np.array(tr, dtype=ANIM_TRACK).reshape(-1)
        tm = np.ascontiguousarray(tm, dtype=np.uint16).reshape(-1)
        va = np.ascontiguousarray(va, dtype=np.uint16).reshape(-1, 4)
        if tr.size != njoints * 3 or va.shape[0] != tm.size:
            raise MtrError(MTR_E_INVALID, "anim tracks: [njoints, 3] descriptors per clip, four value words per key time")
        tr["first"] = np.minimum(tr["first"].astype(np.uint64) + np.uint64(base), np.uint64(0xFFFFFFFF))  # no wrap: an invalid first stays invalid
        base += tm.size
        nticks.append(int(nt))
        flags.append(int(fl))
        tracks.append(tr)
        times.append(tm)
        values.append(va)
    if not clips:
        raise MtrError(MTR_E_INVALID, "anim tracks: at least one clip")
    return (np.asarray(nticks, dtype=np.uint32), np.asarray(flags, dtype=np.uint32), np.ascontiguousarray(np.concatenate(tracks)),
            np.ascontiguousarray(np.concatenate(times)), np.ascontiguousarray(np.concatenate(values)))


def AnimTracks(dev: Device, njoints: int, clips) -> Anim:
    """A track set (include/mtr.h, SPEC.md section 15) as an Anim: per clip, joint and channel a track with its own key
    times and 16-bit keys.  clips: a list of (nticks, flags, tracks, times, values) as anim_track_arrays describes
    (mt_renderer_amd.anim_tracks.compress makes one from uniformly spaced keys).  The library validates every track."""
    nt, fl, tr, tm, va = anim_track_arrays(njoints, clips)
    h = C.c_void_p()
    dev.check(lib.mtr_anim_create_tracks(dev._h, njoints, nt.size, _p(nt), _p(fl), _p(tr), _p(tm), _p(va), tm.size, C.byref(h)))
    return Anim(dev, njoints, clips, _handle=h)


_POSE_STREAMS = {}


def _pose_stream(device):
    """per device: the torch stream Batch.set_poses orders a pose on when the current stream is the legacy default one"""
    import torch
    if device.index not in _POSE_STREAMS:
        _POSE_STREAMS[device.index] = torch.cuda.Stream(device)
    return _POSE_STREAMS[device.index]


def _nbytes(t) -> int:
    return t.numel() * t.element_size()


_U8_I32, _U8_I32_F32 = ("uint8", "int32"), ("uint8", "int32", "float32")  # names of the torch dtypes a record tensor may have


def _device_records(t, dev: "Device", what: str, expect: str, dtypes, *, size_ok=None, size_msg: str = "", align: int = 16, stream=None,
                    owner: str = "batch on"):
    """A tensor of records that a library call reads in stream order: its type (``dtypes``: names of torch dtypes), its
    device and, where ``size_ok`` is given, its size (``size_ok(t)``) are checked in that order.  Returns (tensor, stream):
    ``stream`` or torch.cuda.current_stream(), and the tensor contiguous and ``align``-byte aligned -- a copy made on that
    stream where the caller's is not.  ``owner``: the words of the device message, which the root-motion calls word otherwise."""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in [getattr(torch, name) for name in dtypes]:
        raise MtrError(MTR_E_INVALID, f"{what}: {expect}")
    if t.get_device() != dev.hip_device:
        raise MtrError(MTR_E_INVALID, f"{what}: the tensor is on cuda:{t.get_device()}, the {owner} cuda:{dev.hip_device}")
    if size_ok is not None and not size_ok(t):
        raise MtrError(MTR_E_INVALID, f"{what}: {size_msg}")
    cur = stream if stream is not None else torch.cuda.current_stream(t.device)
    if not t.is_contiguous() or t.data_ptr() % align:
        with torch.cuda.stream(cur):
            t = t.contiguous().clone()
    return t, cur


def _on_stream(dev: "Device", cur, fn, args, tensors):
    """Runs the library call ``fn(*args, stream handle)`` in stream order on the torch stream ``cur`` and tells the allocator
    that ``tensors`` are in use on the stream the call was given.  torch's legacy default stream: its handle, 0, would name the
    device's own stream to the library (include/mtr.h), which is not ordered with it; the call runs on a helper stream that
    follows the current one, and the current one waits for it."""
    run, handle = cur, cur.cuda_stream
    if handle == 0:
        run = _pose_stream(cur.device)
        run.wait_stream(cur)
        handle = run.cuda_stream
    dev.check(fn(*args, C.c_void_p(handle)))
    for t in tensors:
        t.record_stream(run)
    if run is not cur:
        cur.wait_stream(run)


class Batch:
    """n instances of one Model resident in HBM (the build's scheduler submission)."""

    def __init__(self, dev: Device, model: Model, model_mats: np.ndarray, palettes: Optional[np.ndarray] = None,
                 texture_override: Optional[Sequence[int]] = None):
        mm = _f32(model_mats, (-1, 16))
        n = mm.shape[0]
        pal, npal = None, 0
        if palettes is not None:
            pal = _f32(palettes).reshape(n, -1, 16)
            npal = pal.shape[1]
        to = None if texture_override is None else np.ascontiguousarray(texture_override, dtype=np.int32)
        h = C.c_void_p()
        dev.check(lib.mtr_batch_create(dev._h, model._h, n, _p(mm), _p(pal), npal, _p(to), C.byref(h)))
        self.dev, self._h, self.n, self.model, self.npal = dev, h, n, model, npal

    def update(self, model_mats: Optional[np.ndarray] = None, palettes: Optional[np.ndarray] = None):
        """new instance matrices [n, 16] and / or palettes [n, npal, 16] for frames drawn afterwards; None keeps that part"""
        mm = None if model_mats is None else _f32(model_mats, (self.n, 16))
        pal, npal = None, 0
        if palettes is not None:
            pal = _f32(palettes).reshape(self.n, -1, 16)
            npal = pal.shape[1]
        self.dev.check(lib.mtr_batch_update(self._h, _p(mm), _p(pal), npal))
        if pal is not None:
            self.npal = npal

    def set_poses(self, local_mats):
        """one pose per instance, [n, njoints, 16] local matrices, through the model's skeleton (k_pose).  A numpy array is
        copied in; a torch tensor on the batch's device is read in stream order on torch.cuda.current_stream()."""
        if isinstance(local_mats, np.ndarray):
            lm = _f32(local_mats).reshape(self.n, -1, 16)
            self.dev.check(lib.mtr_batch_set_poses(self._h, _p(lm), lm.shape[1]))
            self.npal = lm.shape[1]
            return
        t, cur = _device_records(local_mats, self.dev, "set_poses", "a numpy array or a float32 tensor on the GPU", ("float32",),
                                 size_ok=lambda t: t.numel() % (self.n * 16) == 0, size_msg="n x njoints x 16 local matrices")
        nj = t.numel() // (self.n * 16)
        _on_stream(self.dev, cur, lib.mtr_batch_set_poses_device, (self._h, C.c_void_p(t.data_ptr()), nj), (t,))
        self.npal = nj

    def animate(self, anim: Anim, states):
        """one animation state per instance through ``anim`` and the model's skeleton (k_anim).  A structured numpy array
        (ANIM_STATE) or a dict of its fields is copied in; a torch uint8 [n, 24] / int32 [n, 6] tensor on the batch's device
        holding ANIM_STATE records is read in stream order on torch.cuda.current_stream()."""
        if isinstance(states, (np.ndarray, dict)):
            st = anim_states(states, self.n)
            self.dev.check(lib.mtr_batch_animate(self._h, anim._h, _p(st)))
            self.npal = anim.njoints
            return
        t, cur = _device_records(states, self.dev, "animate", "a numpy ANIM_STATE array, a dict, or a uint8 / int32 tensor on the GPU", _U8_I32,
                                 size_ok=lambda t: _nbytes(t) == self.n * ANIM_STATE.itemsize, size_msg="n states of 24 bytes", align=8)
        _on_stream(self.dev, cur, lib.mtr_batch_animate_device, (self._h, anim._h, C.c_void_p(t.data_ptr())), (t,))
        self.npal = anim.njoints

    def animate_layers(self, anim: Anim, layers, masks: Optional[AnimMasks] = None, L: Optional[int] = None):
        """one layer stack per instance through ``anim``, ``masks`` (or None) and the model's skeleton (k_anim_layers, SPEC.md
        section 16).  A structured numpy array (ANIM_LAYER, [n, L]) or a dict of its fields is copied in; a torch uint8
        [n, L * 16] / int32 [n, L * 4] tensor on the batch's device holding ANIM_LAYER records is read in stream order on
        torch.cuda.current_stream()."""
        mh = masks._h if masks is not None else None
        if isinstance(layers, (np.ndarray, dict)):
            ly = anim_layers(layers, self.n, L)
            self.dev.check(lib.mtr_batch_animate_layers(self._h, anim._h, mh, _p(ly), ly.shape[1]))
            self.npal = anim.njoints
            return
        t, cur = _device_records(layers, self.dev, "animate_layers", "a numpy ANIM_LAYER array, a dict, or a uint8 / int32 tensor on the GPU", _U8_I32,
                                 size_ok=lambda t: self._layer_stacks(t, L), size_msg="n x L layers of 16 bytes")
        nl = _nbytes(t) // (self.n * ANIM_LAYER.itemsize)
        _on_stream(self.dev, cur, lib.mtr_batch_animate_layers_device, (self._h, anim._h, mh, C.c_void_p(t.data_ptr()), nl), (t,))
        self.npal = anim.njoints

    def _layer_stacks(self, t, L: Optional[int]) -> bool:
        """t holds n stacks of whole ANIM_LAYER records, of L each where L is given"""
        nbytes = _nbytes(t)
        return nbytes != 0 and nbytes % (self.n * ANIM_LAYER.itemsize) == 0 and (L is None or nbytes == self.n * L * ANIM_LAYER.itemsize)

    def animate_ik(self, anim: Anim, layers, ik: AnimIK, targets, masks: Optional[AnimMasks] = None, L: Optional[int] = None):
        """one layer stack and one target per chain of ``ik`` per instance (k_anim_ik, SPEC.md section 17).  Numpy arrays
        (ANIM_LAYER [n, L], ANIM_IK_TARGET [n, K]) or dicts of their fields are copied in.  Where either is a torch uint8 /
        int32 / float32 tensor on the batch's device holding the records, both are read from device memory in stream order
        on torch.cuda.current_stream() (a numpy one of the pair is uploaded on that stream first)."""
        mh = masks._h if masks is not None else None
        host = (np.ndarray, dict)
        if isinstance(layers, host) and isinstance(targets, host):
            ly = anim_layers(layers, self.n, L)
            tg = ik_targets(targets, self.n, ik.nchains)
            self.dev.check(lib.mtr_batch_animate_ik(self._h, anim._h, mh, _p(ly), ly.shape[1], ik._h, _p(tg)))
            self.npal = anim.njoints
            return
        import torch
        device = torch.device("cuda", self.dev.hip_device)

        def on_device(t, what, make):
            if isinstance(t, host):
                raw = np.ascontiguousarray(make(t)).view(np.uint8).reshape(self.n, -1)
                return torch.from_numpy(raw.copy()).to(device)
            # the sizes of the pair are checked below, once both are tensors
            return _device_records(t, self.dev, "animate_ik", f"{what} as a numpy array, a dict, or a uint8 / int32 / float32 tensor on the GPU",
                                   _U8_I32_F32)[0]
        tl = on_device(layers, "layers", lambda a: anim_layers(a, self.n, L))
        tt = on_device(targets, "targets", lambda a: ik_targets(a, self.n, ik.nchains))
        if not self._layer_stacks(tl, L):
            raise MtrError(MTR_E_INVALID, "animate_ik: n x L layers of 16 bytes")
        if _nbytes(tt) != self.n * ik.nchains * ANIM_IK_TARGET.itemsize:
            raise MtrError(MTR_E_INVALID, "animate_ik: n x nchains targets of 32 bytes")
        nl = _nbytes(tl) // (self.n * ANIM_LAYER.itemsize)
        _on_stream(self.dev, torch.cuda.current_stream(device), lib.mtr_batch_animate_ik_device,
                   (self._h, anim._h, mh, C.c_void_p(tl.data_ptr()), nl, ik._h, C.c_void_p(tt.data_ptr())), (tl, tt))
        self.npal = anim.njoints

    def animate_spring(self, anim: Anim, layers, spring: "AnimSpring", states, dt: float, ik: Optional[AnimIK] = None, targets=None, motion=None,
                       masks: Optional[AnimMasks] = None, L: Optional[int] = None):
        """one layer stack per instance, the chains of ``ik`` (or None) against ``targets``, then one step of ``dt`` seconds of
        the springs of ``spring`` (k_anim_spring, SPEC.md section 24).  states: a torch uint8 / int32 / float32 tensor on the
        batch's device holding n x nsprings SPRING_STATE records, contiguous and 16-byte aligned; it is read AND written in
        stream order on torch.cuda.current_stream(), so no copy is made of it.  motion: None, or such a float32 tensor
        [n, 16] as Anim.root_deltas_device gives.  layers and targets: numpy arrays or dicts (uploaded on that stream first)
        or record tensors on the device."""
        import torch
        mh = masks._h if masks is not None else None
        host = (np.ndarray, dict)
        device = torch.device("cuda", self.dev.hip_device)
        what = "animate_spring"

        def on_device(t, name, make):
            if isinstance(t, host):
                raw = np.ascontiguousarray(make(t)).view(np.uint8).reshape(self.n, -1)
                return torch.from_numpy(raw.copy()).to(device)
            return _device_records(t, self.dev, what, f"{name} as a numpy array, a dict, or a uint8 / int32 / float32 tensor on the GPU", _U8_I32_F32)[0]
        if (ik is None) != (targets is None):
            raise MtrError(MTR_E_INVALID, f"{what}: targets go with an IK set, and an IK set with targets")
        tl = on_device(layers, "layers", lambda a: anim_layers(a, self.n, L))
        if not self._layer_stacks(tl, L):
            raise MtrError(MTR_E_INVALID, f"{what}: n x L layers of 16 bytes")
        keep = [tl]
        tt = None
        if ik is not None:
            tt = on_device(targets, "targets", lambda a: ik_targets(a, self.n, ik.nchains))
            if _nbytes(tt) != self.n * ik.nchains * ANIM_IK_TARGET.itemsize:
                raise MtrError(MTR_E_INVALID, f"{what}: n x nchains targets of 32 bytes")
            keep.append(tt)
        # the states are written: the caller's own memory or nothing
        st = _device_records(states, self.dev, what, "spring states as a uint8 / int32 / float32 tensor on the GPU", _U8_I32_F32,
                             size_ok=lambda t: _nbytes(t) == self.n * spring.nsprings * SPRING_STATE.itemsize and t.is_contiguous() and t.data_ptr() % 16 == 0,
                             size_msg="n x nsprings states of 32 bytes, contiguous and 16-byte aligned")[0]
        keep.append(st)
        mo = None
        if motion is not None:
            mo = _device_records(motion, self.dev, what, "motion as a float32 tensor on the GPU", ("float32",),
                                 size_ok=lambda t: t.numel() == self.n * 16, size_msg="n x 16 floats")[0]
            keep.append(mo)
        nl = _nbytes(tl) // (self.n * ANIM_LAYER.itemsize)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        _on_stream(self.dev, torch.cuda.current_stream(device), lib.mtr_batch_animate_spring_device,
                   (self._h, anim._h, mh, ptr(tl), nl, ik._h if ik is not None else None, ptr(tt), spring._h, ptr(st), ptr(mo), float(dt)), keep)
        self.npal = anim.njoints

    def attach(self, src: "Batch", recs, stream=None):
        """instance matrices from the joints of ``src``'s current version (k_attach, SPEC.md section 18): one ATTACH record
        per instance.  One shot: animate ``src`` again, attach again.  A structured numpy array (or a dict of ATTACH's
        fields) is copied in; a torch uint8 [n, 80] / int32 / float32 [n, 20] tensor on the batch's device holding ATTACH
        records is read in stream order on ``stream`` (a torch stream; None: torch.cuda.current_stream()).  The batch's
        palettes and npal are kept; ``src`` may be the batch itself."""
        if isinstance(recs, (np.ndarray, dict)):
            rc = attach_records(recs, self.n)
            self.dev.check(lib.mtr_batch_attach(self._h, src._h, _p(rc)))
            return
        t, cur = _device_records(recs, self.dev, "attach", "a numpy ATTACH array, a dict, or a uint8 / int32 / float32 tensor on the GPU", _U8_I32_F32,
                                 size_ok=lambda t: _nbytes(t) == self.n * ATTACH.itemsize, size_msg="n records of 80 bytes", stream=stream)
        _on_stream(self.dev, cur, lib.mtr_batch_attach_device, (self._h, src._h, C.c_void_p(t.data_ptr())), (t,))

    def root_motion(self, traj: "Anim", root: "AnimRoot", steps):
        """moves every instance by the blended delta of its steps on the trajectory set ``traj`` (k_root, SPEC.md section 19):
        M := M . D into a fresh version; palettes and npal are kept.  One shot; the host advances the positions itself.
        steps: a ROOT_STEP array [n, S] (or [n]: one step each) or a dict of its fields, host memory."""
        st = root_steps(steps, self.n)
        self.dev.check(lib.mtr_batch_root_motion(self._h, traj._h, root._h, _p(st), st.shape[1]))

    def root_motion_device(self, traj: "Anim", root: "AnimRoot", steps, stream=None):
        """the same from a torch uint8 [n, S, 16] / int32 / float32 [n, S, 4] tensor on the batch's device holding ROOT_STEP
        records, read in stream order on ``stream`` (a torch stream; None: torch.cuda.current_stream())."""
        t, cur = _root_tensor(steps, self.dev, "root motion", self.n, stream)
        _on_stream(self.dev, cur, lib.mtr_batch_root_motion_device, (self._h, traj._h, root._h, C.c_void_p(t.data_ptr()), t.shape[1]), (t,))

    def sockets(self, recs) -> np.ndarray:
        """the matrices alone, [len(recs), 16]: ATTACH records (a numpy array or a dict) against THIS batch's current
        version, for the host's own use (emitters, hit boxes).  Waits for the result."""
        rc = attach_records(recs, None)
        out = np.zeros((rc.shape[0], 16), dtype=np.float32)
        self.dev.check(lib.mtr_batch_sockets(self._h, _p(rc), rc.shape[0], _p(out), out.size))
        return out

    def read_model_mats(self) -> np.ndarray:
        """the batch's current instance matrices [n, 16], after its pending update has completed"""
        out = np.zeros((self.n, 16), dtype=np.float32)
        self.dev.check(lib.mtr_batch_read_model_mats(self._h, _p(out), out.size))
        return out

    def read_palettes(self) -> np.ndarray:
        """the batch's current palettes [n, npal, 16], after its pending update has completed"""
        out = np.zeros((self.n, self.npal, 16), dtype=np.float32)
        self.dev.check(lib.mtr_batch_read_palettes(self._h, _p(out), out.size))
        return out

    def close(self):
        if self._h:
            lib.mtr_batch_destroy(self._h)
            self._h = None


class FrameLoop:
    """A render loop body with every argument converted once: begin -> [set_shard] -> draw model / batch -> submit
    [-> exchange] -> destroy, as five or six bare C calls per frame.  The classes above convert numpy arrays and build
    ctypes objects on every call (about 20 us of interpreter time per frame, more than a sharded rank's GPU share of a
    small frame); a native host of the C ABI pays about 10 us per frame (tools/probe/host_cost.cpp).  Same calls, same
    order, same error checks -- only the argument marshalling is hoisted out of the loop."""

    def __init__(self, dev: Device, width: int, height: int, *, model: Optional[Model] = None, batch: Optional[Batch] = None,
                 view_proj: np.ndarray, clear_rgba=(1.0, 1.0, 1.0, 1.0), clear_depth: float = 1.0, shard=None, exchange: bool = False):
        assert (model is None) != (batch is None)
        self.dev = dev
        self._clear = _f32(clear_rgba, 4)
        self._vp = _f32(view_proj, 16)
        self._keep = (model, batch)
        self._begin_args = (dev._h, C.c_uint32(width), C.c_uint32(height), _p(self._clear), C.c_float(clear_depth))
        self._draw = lib.mtr_frame_draw_model if model is not None else lib.mtr_frame_draw_batch
        self._obj = (model or batch)._h
        self._vp_p = _p(self._vp)
        self._shard = None
        if shard is not None:
            sh = tuple(shard)
            rank, world, own_map, param, bands = sh + (OWN_INTERLEAVED, 0, None)[len(sh) - 2:]
            self._bands = None if bands is None else np.ascontiguousarray(bands, dtype=np.uint32)
            self._shard = (C.c_uint32(rank), C.c_uint32(world), C.c_uint32(own_map), C.c_uint32(param), _p(self._bands))
        self._exchange = exchange
        self._h = C.c_void_p()
        self._href = C.byref(self._h)

    def run(self, n: int = 1):
        """n frames: submitted, not waited for (dev.synchronize() / exchange_drain() afterwards reports any error)"""
        begin, draw, submit, destroy, shard_fn = lib.mtr_frame_begin, self._draw, lib.mtr_frame_submit, lib.mtr_frame_destroy, lib.mtr_frame_set_shard_map
        xchg = lib.mtr_frame_submit_exchange
        h, href, ba, obj, vp, sh, check = self._h, self._href, self._begin_args, self._obj, self._vp_p, self._shard, self.dev.check
        for _ in range(n):
            rc = begin(*ba, href)
            if rc:
                check(rc)
            if sh is not None:
                rc = shard_fn(h, *sh)
            rc = rc or draw(h, obj, vp)
            if not rc:
                if self._exchange:
                    rc = xchg(h)
                    if not rc:
                        continue  # the exchange thread owns the frame now
                else:
                    rc = submit(h)
            destroy(h)
            if rc:
                check(rc)


class Frame:
    """One render pass: clear colour / depth as in src/bin/modelviewer.rs:190-210 (white, 1.0)."""

    def __init__(self, dev: Device, width: int, height: int, clear_rgba=(1.0, 1.0, 1.0, 1.0), clear_depth: float = 1.0):
        c = _f32(clear_rgba, 4)
        h = C.c_void_p()
        dev.check(lib.mtr_frame_begin(dev._h, width, height, _p(c), clear_depth, C.byref(h)))
        self.dev, self._h, self.w, self.h = dev, h, width, height

    def set_shard(self, rank: int, world: int, own_map: int = OWN_INTERLEAVED, param: int = 0, band_rows=None):
        """render only the bins `rank` of `world` owns under the ownership map (include/mtr.h: MTR_OWN_*)"""
        br = None if band_rows is None else np.ascontiguousarray(band_rows, dtype=np.uint32)
        if br is not None and br.size != world + 1:
            raise MtrError(MTR_E_INVALID, "band_rows needs world + 1 entries")
        self.dev.check(lib.mtr_frame_set_shard_map(self._h, rank, world, own_map, param, _p(br)))

    def shard_bytes(self) -> int:
        return int(lib.mtr_frame_shard_bytes(self._h))

    def unpack_color_shards(self, gathered_devptr: int, dst_devptr: int, stream: Optional[int] = None):
        """gathered blocks (this frame's ownership map) -> linear RGBA8 at dst_devptr"""
        self.dev.check(lib.mtr_frame_unpack_color_shards_on_stream(self._h, C.c_void_p(gathered_devptr), C.c_void_p(dst_devptr),
                                                                   C.c_void_p(stream) if stream else None))

    def draw_model(self, model: Model, view_proj: np.ndarray):
        vp = _f32(view_proj, 16)
        self.dev.check(lib.mtr_frame_draw_model(self._h, model._h, _p(vp)))

    def draw_batch(self, batch: Batch, view_proj: np.ndarray):
        vp = _f32(view_proj, 16)
        self.dev.check(lib.mtr_frame_draw_batch(self._h, batch._h, _p(vp)))

    def draw_instances(self, model: Model, view_proj: np.ndarray, model_mats: np.ndarray,
                       palettes: Optional[np.ndarray] = None):
        vp = _f32(view_proj, 16)
        mm = _f32(model_mats, (-1, 16))
        pal, npal = None, 0
        if palettes is not None:
            pal = _f32(palettes).reshape(mm.shape[0], -1, 16)
            npal = pal.shape[1]
        self.dev.check(lib.mtr_frame_draw_instances(self._h, model._h, _p(mm), _p(pal), npal, mm.shape[0], _p(vp)))

    def draw_overlay_cubes(self, camera: np.ndarray, inst_mats: np.ndarray):
        cam = _f32(camera, 16)
        im = _f32(inst_mats, (-1, 16))
        self.dev.check(lib.mtr_frame_draw_overlay_cubes(self._h, _p(cam), _p(im), im.shape[0]))

    def submit(self):
        self.dev.check(lib.mtr_frame_submit(self._h))

    def submit_exchange(self):
        """submit (if not yet) and hand the frame to the device's exchange thread, which owns it from here on"""
        self.dev.check(lib.mtr_frame_submit_exchange(self._h))
        self._h = None

    def wait(self):
        self.dev.check(lib.mtr_frame_wait(self._h))

    def end(self):
        self.dev.check(lib.mtr_frame_end(self._h))

    def color(self) -> np.ndarray:
        out = np.zeros((self.h, self.w, 4), dtype=np.uint8)
        self.dev.check(lib.mtr_frame_read_color(self._h, _p(out), out.size))
        return out

    def depth(self) -> np.ndarray:
        out = np.zeros((self.h, self.w), dtype=np.float32)
        self.dev.check(lib.mtr_frame_read_depth(self._h, _p(out), out.size))
        return out

    def pack_color_shard(self, dst_devptr: int, dst_bytes: int, stream: Optional[int] = None):
        """this rank's bins, bin-major, into the all-gather send buffer (device pointer); on the device's public stream,
        or on `stream` (a hipStream_t handle; the pack then waits there for this frame's completion)."""
        if stream is None:
            self.dev.check(lib.mtr_frame_pack_color_shard(self._h, C.c_void_p(dst_devptr), dst_bytes))
        else:
            self.dev.check(lib.mtr_frame_pack_color_shard_on_stream(self._h, C.c_void_p(dst_devptr), dst_bytes, C.c_void_p(stream)))

    def color_devptr(self) -> int:
        return int(lib.mtr_frame_color_devptr(self._h) or 0)

    def stats(self) -> dict:
        s = FrameStats()
        self.dev.check(lib.mtr_frame_get_stats(self._h, C.byref(s)))
        return s.as_dict()

    def bin_counts(self):
        """(entries, segments) per 16x16 bin of the frame just rendered (tuning / test hook)."""
        n = self.stats()["nbins"]
        e = np.zeros(n, dtype=np.uint32)
        s = np.zeros(n, dtype=np.uint32)
        self.dev.check(lib.mtr_frame_read_bin_counts(self._h, _p(e), _p(s), n))
        return e, s

    def timings_ms(self) -> dict:
        ms = (C.c_float * 4)()
        self.dev.check(lib.mtr_frame_get_timings(self._h, C.byref(ms)))
        return {STAGE_NAMES[i]: float(ms[i]) for i in range(4)}

    def close(self):
        if self._h:
            lib.mtr_frame_destroy(self._h)
            self._h = None


class Group:
    """One host thread, N devices (include/mtr.h: mtr_group_*): rank r is a Device on hip_devices[r]; a group frame is one
    sharded Frame per rank, and ending it gathers every part's colour into one image on rank 0's device."""

    def __init__(self, hip_devices: Sequence[int]):
        ids = np.ascontiguousarray(hip_devices, dtype=np.int32)
        h = C.c_void_p()
        rc = lib.mtr_group_create(_p(ids), ids.size, C.byref(h))
        if rc:
            raise MtrError(rc, (lib.mtr_group_last_error(None) or b"").decode())
        self._h = h
        self.devices = []
        for r in range(lib.mtr_group_size(h)):
            d = Device.__new__(Device)
            d._h, d._borrowed, d.hip_device = C.c_void_p(lib.mtr_group_device(h, r)), True, int(ids[r])
            self.devices.append(d)

    def __len__(self):
        return len(self.devices)

    def device(self, rank: int) -> Device:
        return self.devices[rank]

    def check(self, rc: int):
        if rc:
            raise MtrError(rc, (lib.mtr_group_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            lib.mtr_group_destroy(self._h)
            self._h = None
            for d in self.devices:
                d._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class GroupFrame:
    """begin -> draw into part(r) with rank r's models / batches -> end() -> color()"""

    def __init__(self, group: Group, width: int, height: int, clear_rgba=(1.0, 1.0, 1.0, 1.0), clear_depth: float = 1.0,
                 own_map: int = OWN_INTERLEAVED, param: int = 0, band_rows=None):
        c = _f32(clear_rgba, 4)
        br = None if band_rows is None else np.ascontiguousarray(band_rows, dtype=np.uint32)
        if br is not None and br.size != len(group) + 1:
            raise MtrError(MTR_E_INVALID, "band_rows needs world + 1 entries")
        h = C.c_void_p()
        group.check(lib.mtr_group_frame_begin(group._h, width, height, _p(c), clear_depth, own_map, param, _p(br), C.byref(h)))
        self.group, self._h, self.w, self.h = group, h, width, height
        self.parts = []
        for r in range(len(group)):
            f = Frame.__new__(Frame)
            f.dev, f._h, f.w, f.h = group.device(r), None, width, height  # _h None: Frame.close() never destroys a part
            f._part = C.c_void_p(lib.mtr_group_frame_part(h, r))
            self.parts.append(f)

    def part(self, rank: int) -> "Frame":
        """rank's frame with its handle live for the draw calls (owned by the group frame)"""
        f = self.parts[rank]
        f._h = f._part
        return f

    def end(self):
        self.group.check(lib.mtr_group_frame_end(self._h))

    def color(self) -> np.ndarray:
        out = np.zeros((self.h, self.w, 4), dtype=np.uint8)
        self.group.check(lib.mtr_group_frame_read_color(self._h, _p(out), out.size))
        return out

    def color_devptr(self) -> int:
        return int(lib.mtr_group_frame_color_devptr(self._h) or 0)

    def close(self):
        if self._h:
            for f in self.parts:
                f._h = None
            lib.mtr_group_frame_destroy(self._h)
            self._h = None
