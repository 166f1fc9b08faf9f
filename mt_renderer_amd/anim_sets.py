"""The animation sets of include/mtr.h: clips and tracks (Anim, AnimTracks), masks, IK and spring sets, root sets, and the
five clock sets that keep their states in tensors of the caller's on the GPU (AnimPlayer, AnimCtrl, AnimEvents, AnimBlend,
AnimMatch), each with its device call and its host hook."""
from __future__ import annotations

from typing import Optional

import numpy as np

from ._lib import MTR_E_INVALID, MtrError, _create, _f32, _Handle, _p, lib
from ._tensors import _DeviceArgs
from .records import (ANIM_IK_CHAIN, ANIM_KEY, ANIM_LAYER, ANIM_STATE, BLEND_SAMPLE, BLEND_STATE, BLEND_TRI, CTRL_NODE, CTRL_STATE, CTRL_TRANS, EVENT,
                      EVENT_MARKER, MATCH_FILTER, MATCH_RESULT, MATCH_ROW, PLAY_CMD, PLAY_STATE, ROOT_STEP, SPRING, SPRING_STATE, _array_form, _dict_form,
                      _host_array, _host_out, anim_layers, anim_states, anim_track_arrays, ik_targets, play_cmds, root_steps)


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))


def _clip_arrays(size_msg: str, nkeys, flags, *rates):
    """The per-clip arrays of a set's create as contiguous arrays: (uint32 key counts, uint32 flag words or None), and the
    float32 rates behind them for a set that has rates.  ``size_msg``: what to say when they do not hold one entry per clip."""
    nk = _u32(nkeys)
    rt = [np.ascontiguousarray(np.asarray(r, dtype=np.float32).reshape(-1)) for r in rates]
    fl = None if flags is None else _u32(flags)
    if any(r.size != nk.size for r in rt) or (fl is not None and fl.size != nk.size):
        raise MtrError(MTR_E_INVALID, size_msg)
    return (nk, fl, *rt)


def _flat(a: np.ndarray) -> bool:
    return a.ndim == 1


def _some(a: np.ndarray):
    """the pointer of an array that may be empty, for which the library takes NULL"""
    return _p(a) if a.size else None


def _handle_of(s: Optional[_Handle]):
    return s._h if s is not None else None


class AnimRoot(_Handle):
    """A root set (include/mtr.h, SPEC.md section 19) for trajectory sets of ``njoints`` joints and ``nclips`` clips: the
    trajectory joint and one flag word per clip (0 or ROOT_CYCLIC; None: all 0)."""
    _destroy = "mtr_anim_root_destroy"

    def __init__(self, dev: "Device", njoints: int, nclips: int, joint: int = 0, flags=None):
        fl = None if flags is None else _u32(flags)
        if fl is not None and fl.size != nclips:
            raise MtrError(MTR_E_INVALID, "anim root: one flag word per clip")
        if not 0 <= joint <= 0xFFFFFFFF:
            raise MtrError(MTR_E_INVALID, "anim root: the trajectory joint lies past the set's joints")
        self._h = _create(dev, lib.mtr_anim_root_create, dev._h, njoints, nclips, joint, _p(fl))
        self.dev, self.njoints, self.nclips, self.joint = dev, njoints, nclips, joint

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
        a = _DeviceArgs(self.dev)
        t = a.root_steps(steps, "root deltas", None)
        with torch.cuda.stream(a.stream()):
            out = torch.empty((t.shape[0], 16), dtype=torch.float32, device=t.device)
        a.used.append(out)
        a.call(lib.mtr_anim_root_deltas_device, (traj._h, self._h, a.ptr(t), t.shape[1], t.shape[0], a.ptr(out)))
        return out


def _layers_in(n: int, nlayers: int, layers) -> Optional[np.ndarray]:
    """the ANIM_LAYER stacks [n, nlayers] a host hook sends in and gets back: a copy of ``layers``, zeroes, or None (no layers)"""
    if not nlayers:
        return None
    return np.zeros((n, nlayers), dtype=ANIM_LAYER) if layers is None else np.ascontiguousarray(layers).copy().reshape(n, nlayers)


class AnimPlayer(_Handle):
    """A player set (include/mtr.h, SPEC.md section 20), the library's clock: per clip the key count (ticks for a track set),
    the flag word (0 or CLIP_LOOP; None: all 0) and the rate in positions per second, for up to ``max_instances`` play states
    that live in a tensor of the caller's on the GPU."""
    _destroy = "mtr_anim_player_destroy"

    def __init__(self, dev: "Device", nkeys, rates, flags=None, max_instances: int = 1):
        nk, fl, rt = _clip_arrays("anim player: one key count, one rate and one flag word per clip", nkeys, flags, rates)
        self._h = _create(dev, lib.mtr_anim_player_create, dev._h, nk.size, _p(nk), _p(fl), _p(rt), max_instances)
        self.dev, self.nclips, self.max_instances = dev, nk.size, max_instances

    def advance(self, states, dt: float, cmds=None, out_states=None, out_layers=None, out_steps=None, stream=None):
        """advances the n PLAY_STATE records of ``states`` (a torch uint8 [n, 32] / int32 / float32 [n, 8] tensor on the GPU,
        16-byte aligned) by ``dt`` seconds IN PLACE and writes, where given, ANIM_STATE records into ``out_states`` ([n, 24]
        bytes), layers 0 and 1 of the ANIM_LAYER stacks of ``out_layers`` ([n, L, 16] bytes, L from its size) and two
        ROOT_STEP records per instance into ``out_steps`` ([n, 2, 16] bytes), in stream order on ``stream`` (a torch stream;
        None: torch.cuda.current_stream()).  cmds: None, a PLAY_CMD array or a dict (host memory, copied before the call
        returns), or a tensor of PLAY_CMD records on the GPU (read in stream order)."""
        import torch
        a = _DeviceArgs(self.dev, stream)
        n = a.in_place(states, "player states", PLAY_STATE.itemsize, 16, None)
        if out_states is not None:
            a.in_place(out_states, "player out_states", ANIM_STATE.itemsize, 8, n)
        nl = a.layers_in_place(out_layers, "player out_layers", n)
        if out_steps is not None:
            a.in_place(out_steps, "player out_steps", ROOT_STEP.itemsize, 16, 2 * n)
        if isinstance(cmds, torch.Tensor):
            m = a.in_place(cmds, "player commands", PLAY_CMD.itemsize, 16, None)
            fn, cp, keep = lib.mtr_anim_player_advance_device_cmds, a.ptr(cmds), None
        else:
            keep = play_cmds(cmds)
            m, fn, cp = keep.size, lib.mtr_anim_player_advance_device, _some(keep)
        a.call(fn, (self._h, a.ptr(states), n, float(dt), cp, m, a.ptr(out_states), a.ptr(out_layers), nl, a.ptr(out_steps)))

    def advance_host(self, states: np.ndarray, dt: float, cmds=None, nlayers: int = 0, layers: Optional[np.ndarray] = None, want_states: bool = True,
                     want_steps: bool = True):
        """the test and debug hook: PLAY_STATE records [n] in host memory through the same kernel; waits.  Returns (states,
        out_states or None, out_layers or None, out_steps or None); ``layers`` ([n, nlayers] ANIM_LAYER) is what layers 2..
        hold going in."""
        st = _host_array(states, PLAY_STATE, "player states: an array [n] of dtype PLAY_STATE", copy=True)
        n = st.size
        cm = play_cmds(cmds)
        oa = _host_out(want_states, n, ANIM_STATE)
        ol = _layers_in(n, nlayers, layers)
        os_ = _host_out(want_steps, (n, 2), ROOT_STEP)
        self.dev.check(lib.mtr_anim_player_advance_host(self._h, _p(st), n, float(dt), _some(cm), cm.size, _p(oa), _p(ol), nlayers, _p(os_)))
        return st, oa, ol, os_


class AnimCtrl(_Handle):
    """A controller (include/mtr.h, SPEC.md section 21): per-instance state machines that write a player's commands on the
    GPU.  ``nkeys`` and ``clip_flags`` are what the AnimPlayer was given; ``nodes`` a CTRL_NODE array, ``trans`` a CTRL_TRANS
    array whose first ``nany`` entries are the any-state transitions (``anim_ctrl.build`` makes the three from a readable
    description), ``nparams`` the floats per instance that conditions may name."""

    _destroy = "mtr_anim_ctrl_destroy"

    def __init__(self, dev: "Device", nkeys, clip_flags, nodes, trans, nany: int = 0, nparams: int = 0):
        msg = "anim ctrl: one flag word per clip, nodes of dtype CTRL_NODE [S] and transitions of dtype CTRL_TRANS [T]"
        nk, fl = _clip_arrays(msg, nkeys, clip_flags)
        nd, tr = _array_form(nodes, CTRL_NODE, msg, _flat), _array_form(trans, CTRL_TRANS, msg, _flat)
        self._h = _create(dev, lib.mtr_anim_ctrl_create, dev._h, nk.size, _p(nk), _p(fl), _p(nd), nd.size, _some(tr), tr.size, nany, nparams)
        self.dev, self.nclips, self.nnodes, self.ntrans, self.nany, self.nparams = dev, nk.size, nd.size, tr.size, nany, nparams

    def step(self, states, play, params, dt: float, cmds_out, counts=None, stream=None):
        """one step of the n CTRL_STATE records of ``states`` ([n, 16] bytes on the GPU, 16-byte aligned) IN PLACE against the
        PLAY_STATE records of ``play`` ([n, 32] bytes, read only) and the rows of ``params`` (float32 [n, nparams], None when
        nparams == 0; CONSUME writes it); writes PLAY_CMD slot i of ``cmds_out`` (at least n slots of 16 bytes; a longer
        tensor leaves room for the host's own commands behind slot n - 1) and adds to ``counts`` (int32 [ntrans]) where
        given, in stream order on ``stream`` (a torch stream; None: torch.cuda.current_stream())."""
        import torch
        a = _DeviceArgs(self.dev, stream)
        n = a.in_place(states, "ctrl states", CTRL_STATE.itemsize, 16, None)
        a.in_place(play, "ctrl play states", PLAY_STATE.itemsize, 16, n)
        if a.in_place(cmds_out, "ctrl commands", PLAY_CMD.itemsize, 16, None) < n:
            raise MtrError(MTR_E_INVALID, "ctrl commands: at least n slots of 16 bytes")
        if self.nparams:
            a.in_place(params, "ctrl params", 4 * self.nparams, 4, n, torch.float32, "ctrl params: a float32 tensor [n, nparams] on the GPU")
        else:
            params = None
        if counts is not None:
            a.of_dtype(counts, torch.int32, "ctrl counts: an int32 tensor [ntrans] on the GPU")
            if self.ntrans == 0 or a.in_place(counts, "ctrl counts", 4, 4, None) < self.ntrans:
                raise MtrError(MTR_E_INVALID, "ctrl counts: one word per transition")
        a.call(lib.mtr_anim_ctrl_step_device, (self._h, a.ptr(states), a.ptr(play), a.ptr(params), n, float(dt), a.ptr(cmds_out), a.ptr(counts)))

    def step_host(self, states: np.ndarray, play: np.ndarray, params, dt: float, counts: Optional[np.ndarray] = None):
        """the test and debug hook: CTRL_STATE [n], PLAY_STATE [n] and float32 [n, nparams] in host memory through the same
        kernel; waits.  Returns (states, params or None, PLAY_CMD [n], counts or None); ``counts`` (uint32 [ntrans]) is added to."""
        msg = "ctrl states: arrays [n] of dtype CTRL_STATE and PLAY_STATE"
        st = _host_array(states, CTRL_STATE, msg, copy=True)
        pl = _host_array(play, PLAY_STATE, msg, st.shape)
        n = st.size
        pr = _host_array(params, np.float32, "ctrl params: float32 [n, nparams]", (n, self.nparams), copy=True) if self.nparams else None
        ct = _host_out(counts is not None, (self.ntrans,), np.uint32, counts, "ctrl counts: uint32 [ntrans]")
        cm = np.zeros(n, dtype=PLAY_CMD)
        self.dev.check(lib.mtr_anim_ctrl_step_host(self._h, _p(st), _p(pl), _p(pr), n, float(dt), _p(cm), _some(ct) if ct is not None else None))
        return st, pr, cm, ct


class AnimEvents(_Handle):
    """An event set (include/mtr.h, SPEC.md section 22): markers on clips that fire into a list on the GPU.  ``nkeys`` and
    ``clip_flags`` are what the AnimPlayer was given; ``counts`` holds the markers per clip and ``markers`` an EVENT_MARKER
    array of them, clip after clip, sorted by x within a clip (``anim_events.build`` makes the two from a dict), for calls of
    up to ``max_instances`` instances."""

    _destroy = "mtr_anim_events_destroy"

    def __init__(self, dev: "Device", nkeys, clip_flags, counts, markers, max_instances: int = 1):
        msg = "anim events: one flag word and one marker count per clip, markers of dtype EVENT_MARKER [sum of counts]"
        nk, fl = _clip_arrays(msg, nkeys, clip_flags)
        ct = _u32(counts)
        mk = _array_form(markers, EVENT_MARKER, msg, lambda mk: ct.size == nk.size and mk.ndim == 1 and mk.size == int(ct.sum(dtype=np.uint64)))
        self._h = _create(dev, lib.mtr_anim_events_create, dev._h, nk.size, _p(nk), _p(fl), _p(ct), _some(mk), max_instances)
        self.dev, self.nclips, self.nmarkers, self.max_instances = dev, nk.size, mk.size, max_instances

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
        a = _DeviceArgs(self.dev, stream)
        a.in_place(steps, "events steps", ROOT_STEP.itemsize, 16, n * S)
        cap = a.in_place(out, "events list", EVENT.itemsize, 16, None) if out is not None else 0
        a.in_place(count, "events count", 4, 4, 2, torch.int32, "events count: an int32 tensor [2] on the GPU")
        if bits is not None:
            a.in_place(bits, "events bits", 4, 4, n, torch.int32, "events bits: an int32 tensor [n] on the GPU")
        a.call(lib.mtr_anim_events_collect_device, (self._h, a.ptr(steps), S, n, float(min_weight), a.ptr(out), cap, a.ptr(count), a.ptr(bits)))

    def collect_host(self, steps: np.ndarray, min_weight: float, capacity: int, out: Optional[np.ndarray] = None, bits: Optional[np.ndarray] = None,
                     want_bits: bool = True):
        """the test and debug hook: ROOT_STEP [n, S] in host memory through the same kernels; waits.  Returns (EVENT [capacity],
        uint32 [2], uint32 [n] or None); ``out`` and ``bits`` are what the list and the masks hold going in."""
        sp = np.ascontiguousarray(np.asarray(steps))
        if sp.dtype != ROOT_STEP or sp.ndim != 2 or sp.shape[1] < 1:
            raise MtrError(MTR_E_INVALID, "events steps: an array [n, S] of dtype ROOT_STEP")
        n, S = sp.shape
        ol = _host_out(True, (capacity,), EVENT, out, "events list: EVENT [capacity]")
        bt = _host_out(want_bits, (n,), np.uint32, bits, "events bits: uint32 [n]")
        ct = np.zeros(2, dtype=np.uint32)
        self.dev.check(lib.mtr_anim_events_collect_host(self._h, _p(sp), S, n, float(min_weight), _p(ol) if capacity else None, capacity, _p(ct), _p(bt)))
        return ol, ct, bt


class AnimBlend(_Handle):
    """A blend set (include/mtr.h, SPEC.md section 23): sample points in a 1-D or 2-D parameter space that each carry a LOOP
    clip.  ``nkeys``, ``rates`` and ``clip_flags`` are what an AnimPlayer takes; ``samples`` a BLEND_SAMPLE array, ``tris`` a
    BLEND_TRI array or None for a 1-D space (``anim_blend.build_1d`` / ``build_2d`` make them from points); ``param_x`` and
    ``param_y`` name the floats of an instance's row of ``nparams`` parameters, ``damp`` is the smoothing rate in 1/seconds
    (inf: none), for calls of up to ``max_instances`` instances."""
    _destroy = "mtr_anim_blend_destroy"

    def __init__(self, dev: "Device", nkeys, rates, clip_flags, samples, tris=None, nparams: int = 1, param_x: int = 0, param_y: int = 0,
                 damp: float = float("inf"), max_instances: int = 1):
        msg = "anim blend: one key count, rate and flag word per clip, samples of dtype BLEND_SAMPLE [K], triangles of dtype BLEND_TRI [T]"
        nk, fl, rt = _clip_arrays(msg, nkeys, clip_flags, rates)
        sm = _array_form(samples, BLEND_SAMPLE, msg, _flat)
        tr = _array_form(np.zeros(0, dtype=BLEND_TRI) if tris is None else tris, BLEND_TRI, msg, _flat)
        if not (0 <= param_x < 1 << 32 and 0 <= param_y < 1 << 32):
            raise MtrError(MTR_E_INVALID, "anim blend: param_x and param_y are parameter indices")
        self._h = _create(dev, lib.mtr_anim_blend_create, dev._h, nk.size, _p(nk), _p(fl), _p(rt), _some(sm), sm.size, _some(tr), tr.size,
                          nparams, param_x, param_y, float(damp), max_instances)
        self.dev, self.nclips, self.nsamples, self.ntris, self.nparams, self.max_instances = dev, nk.size, sm.size, tr.size, nparams, max_instances

    def advance(self, states, params, dt: float, out_layers=None, out_steps=None, out_shares=None, stream=None):
        """advances the n BLEND_STATE records of ``states`` (a torch uint8 [n, 16] / int32 / float32 [n, 4] tensor on the GPU,
        16-byte aligned) by ``dt`` seconds IN PLACE against the rows of ``params`` (float32 [n, nparams], read only) and writes,
        where given, layers 0 to 2 of the ANIM_LAYER stacks of ``out_layers`` ([n, L, 16] bytes, L from its size), three
        ROOT_STEP records per instance into ``out_steps`` ([n, 3, 16] bytes) and the three shares into ``out_shares`` (float32
        [n, 3]), in stream order on ``stream`` (a torch stream; None: torch.cuda.current_stream())."""
        import torch
        a = _DeviceArgs(self.dev, stream)
        n = a.in_place(states, "blend states", BLEND_STATE.itemsize, 16, None)
        a.in_place(params, "blend params", 4, 4, n * self.nparams, torch.float32, "blend params: a float32 tensor [n, nparams] on the GPU")
        nl = a.layers_in_place(out_layers, "blend out_layers", n)
        if out_steps is not None:
            a.in_place(out_steps, "blend out_steps", ROOT_STEP.itemsize, 16, 3 * n)
        if out_shares is not None:
            a.in_place(out_shares, "blend out_shares", 4, 4, 3 * n, torch.float32, "blend out_shares: a float32 tensor [n, 3] on the GPU")
        a.call(lib.mtr_anim_blend_advance_device,
               (self._h, a.ptr(states), a.ptr(params), n, float(dt), a.ptr(out_layers), nl, a.ptr(out_steps), a.ptr(out_shares)))

    def advance_host(self, states: np.ndarray, params: np.ndarray, dt: float, nlayers: int = 0, layers: Optional[np.ndarray] = None, want_steps: bool = True,
                     want_shares: bool = True):
        """the test and debug hook: BLEND_STATE records [n] and float32 rows [n, nparams] in host memory through the same kernel;
        waits.  Returns (states, out_layers or None, out_steps or None, out_shares or None); ``layers`` ([n, nlayers]
        ANIM_LAYER) is what layers 3.. hold going in."""
        st = _host_array(states, BLEND_STATE, "blend states: an array [n] of dtype BLEND_STATE", copy=True)
        n = st.size
        pr = _host_array(params, np.float32, "blend params: float32 [n, nparams]", (n, self.nparams))
        ol = _layers_in(n, nlayers, layers)
        os_ = _host_out(want_steps, (n, 3), ROOT_STEP)
        sh = _host_out(want_shares, (n, 3), np.float32)
        self.dev.check(lib.mtr_anim_blend_advance_host(self._h, _p(st), _p(pr), n, float(dt), _p(ol), nlayers, _p(os_), _p(sh)))
        return st, ol, os_, sh


class AnimMatch(_Handle):
    """A match set (include/mtr.h, SPEC.md section 25): nearest-pose search per instance that writes a player's commands on the
    GPU.  ``nkeys`` and ``clip_flags`` are what the AnimPlayer was given; ``rows`` a MATCH_ROW array [R] sorted by clip and by x
    within a clip, ``features`` float32 [R, D], already normalised and weighted (``anim_match.normalise`` and ``rows_of`` make
    them); ``pose_dims`` has bit d set where dimension d is taken from the pose being played, ``mean`` and ``scale`` (float32
    [D], None: 0 and 1) normalise the raw query; ``seconds`` is the fade of a jump, ``near`` and ``margin`` say when a winner is
    not worth one; for calls of up to ``max_instances`` instances."""

    _destroy = "mtr_anim_match_destroy"

    def __init__(self, dev: "Device", nkeys, clip_flags, rows, features, pose_dims: int = 0, flags: int = 0, seconds: float = 0.2, near: float = 0.0,
                 margin: float = 0.0, mean=None, scale=None, max_instances: int = 1):
        msg = "anim match: one flag word per clip, rows of dtype MATCH_ROW [R], features float32 [R, D], mean and scale float32 [D]"
        nk, fl = _clip_arrays(msg, nkeys, clip_flags)
        ft = np.ascontiguousarray(np.asarray(features, dtype=np.float32))
        rw = _array_form(rows, MATCH_ROW, msg, lambda rw: rw.ndim == 1 and ft.ndim == 2 and ft.shape[0] == rw.size)
        D = ft.shape[1]
        mn, sc = (None if v is None else np.ascontiguousarray(np.asarray(v, dtype=np.float32).reshape(-1)) for v in (mean, scale))
        if any(v is not None and v.size != D for v in (mn, sc)):
            raise MtrError(MTR_E_INVALID, msg)
        if not (0 <= pose_dims < 1 << 64 and 0 <= flags < 1 << 32):
            raise MtrError(MTR_E_INVALID, "anim match: pose_dims is a 64-bit and flags a 32-bit word")
        self._h = _create(dev, lib.mtr_anim_match_create, dev._h, nk.size, _p(nk), _p(fl), D, pose_dims, flags, float(seconds), float(near), float(margin),
                          _some(rw), rw.size, _some(ft), _p(mn), _p(sc), max_instances)
        self.dev, self.nclips, self.nrows, self.D, self.pose_dims, self.max_instances = dev, nk.size, rw.size, D, pose_dims, max_instances

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
        a = _DeviceArgs(self.dev, stream)
        n = a.in_place(play, "match play states", PLAY_STATE.itemsize, 16, None)
        if a.in_place(cmds_out, "match commands", PLAY_CMD.itemsize, 16, None) < n:
            raise MtrError(MTR_E_INVALID, "match commands: at least n slots of 16 bytes")
        if query is not None:
            a.in_place(query, "match query", 4 * self.D, 16, n, torch.float32, "match query: a float32 tensor [n, D] on the GPU")
        elif self.needs_query:
            raise MtrError(MTR_E_INVALID, "match query: the set has dimensions that are not pose dimensions and no query is given")
        if filters is not None:
            a.in_place(filters, "match filters", MATCH_FILTER.itemsize, 8, n)
        if results is not None:
            a.in_place(results, "match results", MATCH_RESULT.itemsize, 16, n)
        if not 0 <= instance_base <= 0xFFFFFFFF:
            raise MtrError(MTR_E_INVALID, "match search: instance_base is a 32-bit index")
        a.call(lib.mtr_anim_match_search_device, (self._h, a.ptr(play), a.ptr(query), a.ptr(filters), n, instance_base, a.ptr(cmds_out), a.ptr(results)))

    def _host_in(self, play, query):
        pl = _host_array(play, PLAY_STATE, "match play states: an array [n] of dtype PLAY_STATE")
        return pl, None if query is None else _host_array(query, np.float32, "match query: float32 [n, D]", (pl.size, self.D))

    def search_host(self, play: np.ndarray, query, filters: Optional[np.ndarray] = None, instance_base: int = 0, want_results: bool = True):
        """the test and debug hook: PLAY_STATE [n], float32 [n, D] (or None) and MATCH_FILTER [n] (or None) in host memory
        through the same kernels; waits.  Returns (PLAY_CMD [n], MATCH_RESULT [n] or None)."""
        pl, qr = self._host_in(play, query)
        n = pl.size
        fl = None if filters is None else _host_array(filters, MATCH_FILTER, "match filters: an array [n] of dtype MATCH_FILTER", (n,))
        cm = np.zeros(n, dtype=PLAY_CMD)
        rs = _host_out(want_results, n, MATCH_RESULT)
        self.dev.check(lib.mtr_anim_match_search_host(self._h, _p(pl), _p(qr), _p(fl), n, instance_base, _p(cm), _p(rs)))
        return cm, rs

    def scores_host(self, play: np.ndarray, query) -> np.ndarray:
        """the test and debug hook: every score, float32 [n, R], from the search kernel itself; waits"""
        pl, qr = self._host_in(play, query)
        out = np.zeros((pl.size, self.nrows), dtype=np.float32)
        self.dev.check(lib.mtr_anim_match_scores_host(self._h, _p(pl), _p(qr), pl.size, _p(out)))
        return out


class AnimIK(_Handle):
    """An IK set (include/mtr.h, SPEC.md section 17): the parents of a skeleton of ``njoints`` joints (a root: 255 or itself)
    and 1 to 4 chains, an ANIM_IK_CHAIN array or a list of dicts of its fields (kind, joint, optionally axis and flags)."""
    _destroy = "mtr_anim_ik_destroy"

    def __init__(self, dev: "Device", parents, chains):
        par = np.ascontiguousarray(np.asarray(parents, dtype=np.uint8).reshape(-1))
        if isinstance(chains, np.ndarray):
            ch = _array_form(chains, ANIM_IK_CHAIN, "anim ik: chains of dtype ANIM_IK_CHAIN or a list of dicts of its fields").reshape(-1)
        else:
            ch = np.zeros(len(chains), dtype=ANIM_IK_CHAIN)
            for k, c in enumerate(chains):
                _dict_form(c, ANIM_IK_CHAIN.names, ("kind", "joint"), "anim ik: a chain has kind and joint, optionally axis and flags")
                jt = np.atleast_1d(np.asarray(c["joint"], dtype=np.uint32))
                ch["kind"][k], ch["flags"][k] = c["kind"], c.get("flags", 0)
                ch["joint"][k, :jt.size] = jt[:3]
                ch["axis"][k] = c.get("axis", (0.0, 0.0, 0.0))
        self._h = _create(dev, lib.mtr_anim_ik_create, dev._h, par.size, _p(par), ch.size, _some(ch))
        self.dev, self.njoints, self.nchains = dev, par.size, ch.size


class AnimSpring(_Handle):
    """A spring set (include/mtr.h, SPEC.md section 24): the parents of a skeleton of ``njoints`` joints (a root: 255 or itself)
    and 1 to 16 springs, a SPRING array or a list of dicts of its fields (joint and tail, optionally stiffness, drag and
    gravity).  mt_renderer_amd.anim_spring.chain makes the records of a chain of joints."""
    _destroy = "mtr_anim_spring_destroy"

    def __init__(self, dev: "Device", parents, springs):
        par = np.ascontiguousarray(np.asarray(parents, dtype=np.uint8).reshape(-1))
        if isinstance(springs, np.ndarray):
            sp = _array_form(springs, SPRING, "anim spring: springs of dtype SPRING or a list of dicts of its fields").reshape(-1)
        else:
            sp = np.zeros(len(springs), dtype=SPRING)
            for k, c in enumerate(springs):
                _dict_form(c, SPRING.names, ("joint", "tail"), "anim spring: a spring has joint and tail, optionally stiffness, drag, gravity and flags")
                for name, v in c.items():
                    sp[name][k] = v
        self._h = _create(dev, lib.mtr_anim_spring_create, dev._h, par.size, _p(par), sp.size, _some(sp))
        self.dev, self.njoints, self.nsprings = dev, par.size, sp.size


class AnimMasks(_Handle):
    """A mask set for animation layers (include/mtr.h, SPEC.md section 16): weights [nmasks, njoints] in [0, 1], resident
    in HBM.  A layer's mask index 0 is the built-in mask of ones, index k >= 1 is weights[k - 1]."""
    _destroy = "mtr_anim_masks_destroy"

    def __init__(self, dev: "Device", njoints: int, weights):
        w = _f32(weights)
        if njoints < 1 or w.size == 0 or w.size % njoints:
            raise MtrError(MTR_E_INVALID, "anim masks: weights are [nmasks, njoints] float32, at least one mask")
        w = np.ascontiguousarray(w).reshape(-1, njoints)
        self._h = _create(dev, lib.mtr_anim_masks_create, dev._h, njoints, w.shape[0], _p(w))
        self.dev, self.njoints, self.nmasks = dev, njoints, w.shape[0]


class Anim(_Handle):
    """An animation set (include/mtr.h, SPEC.md section 14): clips of uniformly spaced keys for ``njoints`` joints, resident
    in HBM.  clips: a list of (keys, flags); keys is [nkeys, njoints, 12] float32 (t.xyz 0 | q.xyzw | s.xyz 0) or an
    ANIM_KEY array [nkeys, njoints]; flags 0 or CLIP_LOOP."""
    _destroy = "mtr_anim_destroy"

    def __init__(self, dev: "Device", njoints: int, clips):
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
        self._h = _create(dev, lib.mtr_anim_create, dev._h, njoints, len(nkeys), _p(nk), _p(fl), _p(allk))
        self.dev, self.njoints, self.nclips = dev, njoints, len(nkeys)

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
        self.dev.check(lib.mtr_anim_sample_layers(self._h, _handle_of(masks), _p(ly), ly.shape[1], ly.shape[0], _p(out), out.size))
        return out

    def sample_ik(self, layers, ik: "AnimIK", targets, masks: Optional[AnimMasks] = None) -> np.ndarray:
        """the local matrices [n, njoints, 16] of the given layer stacks ([n, L]) after the chains of ``ik`` have been
        evaluated against ``targets`` ([n, K], SPEC.md section 17), formed on the GPU"""
        ly = anim_layers(layers)
        tg = ik_targets(targets, ly.shape[0], ik.nchains)
        out = np.zeros((ly.shape[0], self.njoints, 16), dtype=np.float32)
        self.dev.check(lib.mtr_anim_sample_ik(self._h, _handle_of(masks), ik._h, _p(ly), ly.shape[1], _p(tg), ly.shape[0], _p(out), out.size))
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
        self.dev.check(lib.mtr_anim_sample_spring(self._h, _handle_of(masks), _handle_of(ik), spring._h, _p(ly), ly.shape[1], _p(tg), _p(st), _p(mo),
                                                  float(dt), n, _p(out), out.size))
        return out, st


def AnimTracks(dev: "Device", njoints: int, clips) -> Anim:
    """A track set (include/mtr.h, SPEC.md section 15) as an Anim: per clip, joint and channel a track with its own key
    times and 16-bit keys.  clips: a list of (nticks, flags, tracks, times, values) as anim_track_arrays describes
    (mt_renderer_amd.anim_tracks.compress makes one from uniformly spaced keys).  The library validates every track."""
    nt, fl, tr, tm, va = anim_track_arrays(njoints, clips)
    a = Anim.__new__(Anim)
    a._h = _create(dev, lib.mtr_anim_create_tracks, dev._h, njoints, nt.size, _p(nt), _p(fl), _p(tr), _p(tm), _p(va), tm.size)
    a.dev, a.njoints, a.nclips = dev, njoints, len(clips)
    return a
