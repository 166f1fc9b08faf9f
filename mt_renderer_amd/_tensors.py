"""Tensors of records on the GPU that a library call uses in stream order: the one object that checks them, and the one place
where such a call is put on a torch stream.  torch is imported inside the functions that need it: the binding loads without."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from ._lib import MTR_E_INVALID, MtrError
from .records import ANIM_LAYER, ROOT_STEP

_POSE_STREAMS = {}


def _pose_stream(device):
    """per device: the torch stream Batch.set_poses orders a pose on when the current stream is the legacy default one"""
    import torch
    if device.index not in _POSE_STREAMS:
        _POSE_STREAMS[device.index] = torch.cuda.Stream(device)
    return _POSE_STREAMS[device.index]


def _on_stream(dev, cur, fn, args, tensors):
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


def _nbytes(t) -> int:
    return t.numel() * t.element_size()


def _layer_stacks(t, n: int, L: Optional[int]) -> bool:
    """t holds n stacks of whole ANIM_LAYER records, of L each where L is given"""
    nbytes = _nbytes(t)
    return nbytes != 0 and nbytes % (n * ANIM_LAYER.itemsize) == 0 and (L is None or nbytes == n * L * ANIM_LAYER.itemsize)


_U8_I32, _U8_I32_F32 = ("uint8", "int32"), ("uint8", "int32", "float32")  # names of the torch dtypes a record tensor may have
_RECORDS = "a uint8 / int32 / float32 tensor on the GPU"


class _DeviceArgs:
    """The tensors that one library call uses in stream order on ``stream`` (a torch stream; None: the current stream of the
    device): each is checked as it is added -- its type, then its device, then its size -- and kept, so that the call can tell
    the allocator which stream uses them.  A tensor the call only reads (read) may be replaced by a contiguous, aligned copy
    made on that stream; one it reads or writes IN PLACE (in_place) is refused unless it is contiguous and aligned.
    ``owner``: the words of the device message, which the calls of a batch word otherwise."""

    def __init__(self, dev, stream=None, owner: str = "device is"):
        self.dev, self._stream, self.owner, self.used = dev, stream, owner, []

    def stream(self):
        import torch
        if self._stream is None:
            self._stream = torch.cuda.current_stream(torch.device("cuda", self.dev.hip_device))
        return self._stream

    def _type_then_device(self, t, what: str, expect: str, dtypes):
        import torch
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in [getattr(torch, name) for name in dtypes]:
            raise MtrError(MTR_E_INVALID, f"{what}: {expect}")
        if t.get_device() != self.dev.hip_device:
            raise MtrError(MTR_E_INVALID, f"{what}: the tensor is on cuda:{t.get_device()}, the {self.owner} cuda:{self.dev.hip_device}")

    def read(self, t, what: str, expect: str, dtypes, size_ok=None, size_msg: str = "", align: int = 16):
        """checks ``t`` (``dtypes``: names of torch dtypes; ``size_ok(t)`` where given) and returns it contiguous and
        ``align``-byte aligned: a copy made on the call's stream where the caller's is not"""
        import torch
        self._type_then_device(t, what, expect, dtypes)
        if size_ok is not None and not size_ok(t):
            raise MtrError(MTR_E_INVALID, f"{what}: {size_msg}")
        if not t.is_contiguous() or t.data_ptr() % align:
            with torch.cuda.stream(self.stream()):
                t = t.contiguous().clone()
        self.used.append(t)
        return t

    def records(self, t, what: str, name: str, make, rows: int):
        """one of the layers and targets of a call that takes the pair from device memory: host records (a numpy array or a
        dict, through ``make``) are uploaded on the call's stream as uint8 [rows, bytes]; a tensor is checked, its size by
        the caller once both are there"""
        if not isinstance(t, (np.ndarray, dict)):
            return self.read(t, what, f"{name} as a numpy array, a dict, or {_RECORDS}", _U8_I32_F32)
        import torch
        raw = np.ascontiguousarray(make(t)).view(np.uint8).reshape(rows, -1)
        with torch.cuda.stream(self.stream()):
            t = torch.from_numpy(raw.copy()).to(torch.device("cuda", self.dev.hip_device))
        self.used.append(t)
        return t

    def root_steps(self, t, what: str, n: Optional[int]):
        """ROOT_STEP records [n, S] (n None: any count) that the call reads"""
        t = self.read(t, what, f"a numpy ROOT_STEP array, a dict, or {_RECORDS}", _U8_I32_F32,
                      size_ok=lambda t: t.dim() >= 2 and t.shape[-1] * t.element_size() == ROOT_STEP.itemsize,
                      size_msg="steps of 16 bytes, [n, S, 16] uint8 or [n, S, 4] int32 / float32")
        if t.dim() != 3 or (n is not None and t.shape[0] != n):
            raise MtrError(MTR_E_INVALID, f"{what}: a tensor [n, S, 16 bytes]")
        return t

    @staticmethod
    def of_dtype(t, dtype, msg: str):
        if getattr(t, "dtype", None) != dtype:
            raise MtrError(MTR_E_INVALID, msg)

    def in_place(self, t, what: str, record: int, align: int, count: Optional[int], dtype=None, dtype_msg: str = "") -> int:
        """checks ``t``, used IN PLACE: ``count`` records (None: any number) of ``record`` bytes, of ``dtype`` where one is
        required; returns the number of records it holds"""
        if dtype is not None:
            self.of_dtype(t, dtype, dtype_msg)
        self._type_then_device(t, what, _RECORDS, _U8_I32_F32)
        if not t.is_contiguous() or t.data_ptr() % align:
            raise MtrError(MTR_E_INVALID, f"{what}: contiguous and {align}-byte aligned (it is used in place)")
        nbytes = _nbytes(t)
        if nbytes == 0 or nbytes % record or (count is not None and nbytes != count * record):
            raise MtrError(MTR_E_INVALID, f"{what}: records of {record} bytes" + ("" if count is None else f", {count} of them"))
        self.used.append(t)
        return nbytes // record

    def layers_in_place(self, t, what: str, n: int) -> int:
        """``t``: None or n x L ANIM_LAYER records; returns L, 0 for None"""
        if t is None:
            return 0
        nl = self.in_place(t, what, ANIM_LAYER.itemsize, 16, None)
        if nl % n:
            raise MtrError(MTR_E_INVALID, f"{what}: n x L layers of 16 bytes")
        return nl // n

    @staticmethod
    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def call(self, fn, args):
        """``fn(*args, stream handle)`` in stream order on the call's stream"""
        _on_stream(self.dev, self.stream(), fn, args, self.used)
