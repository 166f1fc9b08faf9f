"""libmtr.so as ctypes sees it: where it lies, the error codes and MtrError, the structs and the one table of signatures of
include/mtr.h that the library is bound from, and what every owner of a library handle shares.

There is NO CPU fallback here: if libmtr.so is missing, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MTR_LIB_PATH") or os.path.join(_PKG, "libmtr.so")  # MTR_LIB_PATH: A/B runs of two builds on one box

MTR_OK, MTR_E_INVALID, MTR_E_UNSUPPORTED, MTR_E_NOMEM, MTR_E_HIP, MTR_E_OVERFLOW = range(6)


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


vp, i32, u32, u64, sz, f32, out = C.c_void_p, C.c_int32, C.c_uint32, C.c_uint64, C.c_size_t, C.c_float, C.POINTER(C.c_void_p)
# every function include/mtr.h declares: name -> (restype, argtypes).  The library is bound from this table, and the tests hold
# it to the header: the same names, the argument count and the return type of every prototype.
SIGNATURES = {
    "mtr_abi_version": (i32, []),
    "mtr_device_create": (i32, [i32, out]),
    "mtr_device_create_on_stream": (i32, [i32, vp, out]),
    "mtr_device_destroy": (None, [vp]),
    "mtr_last_error": (C.c_char_p, [vp]),
    "mtr_device_set_profiling": (i32, [vp, i32]),
    "mtr_device_synchronize": (i32, [vp]),
    "mtr_texture_create": (i32, [vp, u32, u32, u32, vp, sz, out]),
    "mtr_texture_create_mips": (i32, [vp, u32, u32, u32, u32, vp, sz, out]),
    "mtr_model_set_prim_states": (i32, [vp, vp, sz]),
    "mtr_model_set_joint_positions": (i32, [vp, vp, sz]),
    "mtr_frame_draw_model_joints": (i32, [vp, vp, vp]),
    "mtr_texture_destroy": (None, [vp]),
    "mtr_texture_read_rgba8": (i32, [vp, vp, sz]),
    "mtr_model_create": (i32, [vp, vp, sz, vp, sz, vp, sz, vp, vp, vp, sz, vp, out]),
    "mtr_model_destroy": (None, [vp]),
    "mtr_model_set_parts_disp": (i32, [vp, vp, sz]),
    "mtr_model_set_palette": (i32, [vp, vp, sz]),
    "mtr_batch_create": (i32, [vp, vp, sz, vp, vp, sz, vp, out]),
    "mtr_batch_destroy": (None, [vp]),
    "mtr_frame_begin": (i32, [vp, u32, u32, vp, f32, out]),
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
    "mtr_group_create": (i32, [vp, i32, out]),
    "mtr_group_destroy": (None, [vp]),
    "mtr_group_size": (i32, [vp]),
    "mtr_group_device": (vp, [vp, i32]),
    "mtr_group_last_error": (C.c_char_p, [vp]),
    "mtr_group_frame_begin": (i32, [vp, u32, u32, vp, f32, u32, u32, vp, out]),
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
    "mtr_batch_animate_spring_device": (i32, [vp, vp, vp, vp, sz, vp, vp, vp, vp, vp, f32, vp]),
    "mtr_anim_sample_spring": (i32, [vp, vp, vp, vp, vp, sz, vp, vp, vp, f32, sz, vp, sz]),
    "mtr_batch_attach": (i32, [vp, vp, vp]),
    "mtr_batch_attach_device": (i32, [vp, vp, vp, vp]),
    "mtr_batch_sockets": (i32, [vp, vp, sz, vp, sz]),
    "mtr_batch_sockets_device": (i32, [vp, vp, sz, vp, vp]),
    "mtr_batch_read_model_mats": (i32, [vp, vp, sz]),
    "mtr_anim_root_create": (i32, [vp, sz, sz, u32, vp, vp]),
    "mtr_anim_root_destroy": (None, [vp]),
    "mtr_batch_root_motion": (i32, [vp, vp, vp, vp, sz]),
    "mtr_batch_root_motion_device": (i32, [vp, vp, vp, vp, sz, vp]),
    "mtr_anim_root_deltas": (i32, [vp, vp, vp, sz, sz, vp, sz]),
    "mtr_anim_root_deltas_device": (i32, [vp, vp, vp, sz, sz, vp, vp]),
    "mtr_anim_player_create": (i32, [vp, sz, vp, vp, vp, sz, vp]),
    "mtr_anim_player_destroy": (None, [vp]),
    "mtr_anim_player_advance_device": (i32, [vp, vp, sz, f32, vp, sz, vp, vp, sz, vp, vp]),
    "mtr_anim_player_advance_device_cmds": (i32, [vp, vp, sz, f32, vp, sz, vp, vp, sz, vp, vp]),
    "mtr_anim_player_advance_host": (i32, [vp, vp, sz, f32, vp, sz, vp, vp, sz, vp]),
    "mtr_anim_ctrl_create": (i32, [vp, sz, vp, vp, vp, sz, vp, sz, sz, sz, vp]),
    "mtr_anim_ctrl_destroy": (None, [vp]),
    "mtr_anim_ctrl_step_device": (i32, [vp, vp, vp, vp, sz, f32, vp, vp, vp]),
    "mtr_anim_ctrl_step_host": (i32, [vp, vp, vp, vp, sz, f32, vp, vp]),
    "mtr_anim_events_create": (i32, [vp, sz, vp, vp, vp, vp, sz, vp]),
    "mtr_anim_events_destroy": (None, [vp]),
    "mtr_anim_events_collect_device": (i32, [vp, vp, sz, sz, f32, vp, sz, vp, vp, vp]),
    "mtr_anim_events_collect_host": (i32, [vp, vp, sz, sz, f32, vp, sz, vp, vp]),
    "mtr_anim_blend_create": (i32, [vp, sz, vp, vp, vp, vp, sz, vp, sz, sz, u32, u32, f32, sz, vp]),
    "mtr_anim_blend_destroy": (None, [vp]),
    "mtr_anim_blend_advance_device": (i32, [vp, vp, vp, sz, f32, vp, sz, vp, vp, vp]),
    "mtr_anim_blend_advance_host": (i32, [vp, vp, vp, sz, f32, vp, sz, vp, vp]),
    "mtr_anim_match_create": (i32, [vp, sz, vp, vp, sz, u64, u32, f32, f32, f32, vp, sz, vp, vp, vp, sz, vp]),
    "mtr_anim_match_destroy": (None, [vp]),
    "mtr_anim_match_search_device": (i32, [vp, vp, vp, vp, sz, u32, vp, vp, vp]),
    "mtr_anim_match_search_host": (i32, [vp, vp, vp, vp, sz, u32, vp, vp]),
    "mtr_anim_match_scores_host": (i32, [vp, vp, vp, sz, vp]),
}
del vp, i32, u32, u64, sz, f32, out
EXPORTED_SYMBOLS = list(SIGNATURES)


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
    for name, (res, args) in SIGNATURES.items():
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


def _create(owner, fn, *args):
    """The handle that the library's create function ``fn(*args, &handle)`` returns; ``owner`` (a Device or a Group) raises
    what the library says where it fails."""
    h = C.c_void_p()
    owner.check(fn(*args, C.byref(h)))
    return h


class _Handle:
    """What the classes that own one object of the library share: its handle ``_h``, and the name of the library function
    that destroys it, which close() calls once."""
    _destroy = ""

    def close(self):
        if self._h:
            getattr(lib, self._destroy)(self._h)
            self._h = None
