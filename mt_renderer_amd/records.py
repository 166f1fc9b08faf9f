"""The records and constants of include/mtr.h as numpy dtypes, and the builders that make contiguous arrays of them from a
structured array or from a dict of its fields.  numpy on the host; nothing here touches the library."""
from __future__ import annotations

from typing import Optional

import numpy as np

from ._lib import MTR_E_INVALID, MtrError, _f32

TILE_AUTO, TILE_ORDERED, TILE_VISIBILITY, TILE_MIXED = 0, 1, 2, 3
OWN_INTERLEAVED, OWN_BANDS, OWN_SUPERTILES = 0, 1, 2
TEXRES_DECODED, TEXRES_BLOCKS = 0, 1
GEOM_CULL_OFF, GEOM_CULL_SHARDED, GEOM_CULL_ALL_FRAMES = 0, 1, 2
STAGE_NAMES = ("geom", "scan", "fill", "tile")

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


def _bad(msg: str) -> MtrError:
    return MtrError(MTR_E_INVALID, msg)


def _dict_form(d: dict, allowed, required, msg: str):
    """the dict form of a record: no key but the ``allowed`` ones and every ``required`` one, else MtrError ``msg``"""
    if set(d) - set(allowed) or not set(required) <= set(d):
        raise _bad(msg)


def _array_form(a, dtype, msg: str, shape_ok=None) -> np.ndarray:
    """the array form of a record: ``a`` as a contiguous array, which must have ``dtype`` (and, where given, a shape that
    ``shape_ok(a)`` accepts), else MtrError ``msg``"""
    a = np.asarray(a)
    if a.dtype != dtype or (shape_ok is not None and not shape_ok(a)):
        raise _bad(msg)
    return np.ascontiguousarray(a)


def _count(n: Optional[int], got: int, msg: str):
    """``got`` where ``n`` are expected (None: any count), else MtrError ``msg``"""
    if n is not None and got != n:
        raise _bad(msg)


def anim_states(states, n: Optional[int] = None) -> np.ndarray:
    """animation states as a contiguous ANIM_STATE array: from a structured array of that dtype, or from a dict of
    clip_a, clip_b, x_a, x_b, w (arrays or scalars; a missing clip_b / x_b / w is 0)"""
    if isinstance(states, dict):
        _dict_form(states, ANIM_STATE.names, ("clip_a", "x_a"), "animation states: clip_a and x_a, optionally clip_b, x_b and w")
        cols = {k: np.atleast_1d(np.asarray(v)) for k, v in states.items()}
        st = np.zeros(max(c.size for c in cols.values()) if n is None else n, dtype=ANIM_STATE)
        for k, v in cols.items():
            st[k] = v
    else:
        st = _array_form(states, ANIM_STATE, "animation states: an array of dtype ANIM_STATE or a dict of its fields").reshape(-1)
    _count(n, st.size, f"animation states: {n} expected, {st.size} given")
    return st


def anim_layers(layers, n: Optional[int] = None, L: Optional[int] = None) -> np.ndarray:
    """layer stacks as a contiguous ANIM_LAYER array [n, L] (SPEC.md section 16): from a structured array of that dtype
    ([n, L], or flat with n or L given), or from a dict of clip and x, optionally w, mask and mode (arrays [n, L], or
    anything that broadcasts to it; a missing w is 1, a missing mask / mode 0)"""
    if isinstance(layers, dict):
        _dict_form(layers, ANIM_LAYER.names, ("clip", "x"), "animation layers: clip and x, optionally w, mask and mode")
        cols = {k: np.asarray(v) for k, v in layers.items()}
        shape = np.broadcast_shapes(*[c.shape for c in cols.values()])
        if len(shape) > 2:
            raise _bad("animation layers: fields of shape [n, L]")
        shape = (1,) * (2 - len(shape)) + tuple(shape)
        shape = (n if n is not None and shape[0] == 1 else shape[0], L if L is not None and shape[1] == 1 else shape[1])
        ly = np.zeros(shape, dtype=ANIM_LAYER)
        ly["w"] = 1.0
        for k, v in cols.items():
            ly[k] = v
    else:
        a = _array_form(layers, ANIM_LAYER, "animation layers: an array of dtype ANIM_LAYER or a dict of its fields")
        if a.ndim == 2:
            ly = a
        elif n is not None and n and a.size % n == 0:
            ly = a.reshape(n, a.size // n)
        elif L is not None and L and a.size % L == 0:
            ly = a.reshape(a.size // L, L)
        else:
            raise _bad("animation layers: an [n, L] array")
    msg = f"animation layers: [{n}, {L}] expected, {list(ly.shape)} given"
    _count(n, ly.shape[0], msg)
    _count(L, ly.shape[1], msg)
    return ly


def ik_targets(targets, n: Optional[int], K: int) -> np.ndarray:
    """IK targets as a contiguous ANIM_IK_TARGET array [n, K] (SPEC.md section 17): from a structured array of that dtype
    ([n, K] or flat), or from a dict of pos ([n, K, 3]), optionally w ([n, K], missing = 1) and pole ([n, K, 3])"""
    if isinstance(targets, dict):
        _dict_form(targets, ("pos", "w", "pole"), ("pos",), "ik targets: pos, optionally w and pole")
        pos = _f32(targets["pos"]).reshape(-1, K, 3)
        tg = np.zeros((pos.shape[0], K), dtype=ANIM_IK_TARGET)
        tg["pos"], tg["w"] = pos, 1.0
        if "w" in targets:
            tg["w"] = np.asarray(targets["w"], dtype=np.float32).reshape(-1, K)
        if "pole" in targets:
            tg["pole"] = _f32(targets["pole"]).reshape(-1, K, 3)
    else:
        tg = _array_form(targets, ANIM_IK_TARGET, "ik targets: an [n, nchains] array of dtype ANIM_IK_TARGET or a dict of its fields",
                         lambda a: a.size != 0 and a.size % K == 0).reshape(-1, K)
    _count(n, tg.shape[0], f"ik targets: [{n}, {K}] expected, {list(tg.shape)} given")
    return tg


def attach_records(recs, n: Optional[int]) -> np.ndarray:
    """attachment records as a contiguous flat ATTACH array (SPEC.md section 18): from a structured array of that dtype, or
    from a dict of src_instance ([n]), optionally joint ([n], missing = ATTACH_NO_JOINT), flags ([n], missing = 0) and
    offset ([n, 16], column-major, missing = the identity)"""
    if isinstance(recs, dict):
        _dict_form(recs, ("src_instance", "joint", "flags", "offset"), ("src_instance",), "attach records: src_instance, optionally joint, flags and offset")
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
        rc = _array_form(recs, ATTACH, "attach records: an array of dtype ATTACH or a dict of its fields", lambda a: a.size != 0).reshape(-1)
    _count(n, rc.shape[0], f"attach records: {n} expected, {rc.shape[0]} given")
    return rc


def root_steps(steps, n: Optional[int]) -> np.ndarray:
    """root-motion steps as a contiguous ROOT_STEP array [n, S] (SPEC.md section 19): from a structured array [n, S] or [n]
    of that dtype, or from a dict of its fields (clip, x, dx, optionally w; each [n, S] or [n])"""
    if isinstance(steps, dict):
        _dict_form(steps, ROOT_STEP.names, ("clip", "x", "dx"), "root steps: clip, x and dx, optionally w")
        x = np.asarray(steps["x"], dtype=np.float32)
        st = np.zeros(x.shape if x.ndim == 2 else (x.size, 1), dtype=ROOT_STEP)
        for k, v in steps.items():
            st[k] = np.asarray(v).reshape(st.shape)
    else:
        st = _array_form(steps, ROOT_STEP, "root steps: an array [n, S] of dtype ROOT_STEP or a dict of its fields", lambda a: a.ndim in (1, 2))
        st = st.reshape(st.shape[0], -1)
    _count(n, st.shape[0], f"root steps: {n} instances expected, {st.shape[0]} given")
    return st


def play_cmds(cmds) -> np.ndarray:
    """player commands as a contiguous PLAY_CMD array [m] (SPEC.md section 20): from a structured array of that dtype, a dict
    of its fields (instance, clip, optionally x and seconds) or None (no commands)"""
    if cmds is None:
        return np.zeros(0, dtype=PLAY_CMD)
    if isinstance(cmds, dict):
        _dict_form(cmds, PLAY_CMD.names, ("instance", "clip"), "player commands: instance and clip, optionally x and seconds")
        c = np.zeros(np.asarray(cmds["instance"]).size, dtype=PLAY_CMD)
        for k, v in cmds.items():
            c[k] = np.asarray(v).reshape(-1)
        return c
    return _array_form(cmds, PLAY_CMD, "player commands: an array [m] of dtype PLAY_CMD or a dict of its fields", lambda a: a.ndim == 1)


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
            raise _bad("anim tracks: [njoints, 3] descriptors per clip, four value words per key time")
        tr["first"] = np.minimum(tr["first"].astype(np.uint64) + np.uint64(base), np.uint64(0xFFFFFFFF))  # no wrap: an invalid first stays invalid
        base += tm.size
        nticks.append(int(nt))
        flags.append(int(fl))
        tracks.append(tr)
        times.append(tm)
        values.append(va)
    if not clips:
        raise _bad("anim tracks: at least one clip")
    return (np.asarray(nticks, dtype=np.uint32), np.asarray(flags, dtype=np.uint32), np.ascontiguousarray(np.concatenate(tracks)),
            np.ascontiguousarray(np.concatenate(times)), np.ascontiguousarray(np.concatenate(values)))


def _host_array(a, dtype, msg: str, shape=None, copy: bool = False) -> np.ndarray:
    """An input of a host hook as a contiguous array of ``dtype`` -- records must have it, numbers are converted to it -- that
    is [n], or of ``shape`` where one is given, else MtrError ``msg``; a copy where the call writes it."""
    dtype = np.dtype(dtype)
    r = np.ascontiguousarray(np.asarray(a, dtype=None if dtype.names else dtype))
    if r.dtype != dtype or (r.ndim != 1 if shape is None else r.shape != shape):
        raise _bad(msg)
    return r.copy() if copy else r


def _host_out(want, shape, dtype, given=None, msg: str = "") -> Optional[np.ndarray]:
    """An optional output of a host hook: None unless ``want``; else zeroes of ``shape`` and ``dtype``, or a copy of what
    ``given`` holds going in (checked as _host_array checks it)."""
    if not want:
        return None
    return np.zeros(shape, dtype=dtype) if given is None else _host_array(given, dtype, msg, shape, copy=True)
