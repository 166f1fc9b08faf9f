"""The binding of libmtr.so (include/mtr.h) as its users see it: a host-side mirror of the reference's interface, and every
name of the modules it is made of -- _lib (the library, its errors and its signatures), records (dtypes, constants and record
builders), _tensors (tensor arguments on a torch stream) and anim_sets (the animation sets).

The classes keep the reference's names and argument roles -- ``Texture.new`` (src/texture.rs:11),
``Model.new`` / ``Model.set_parts_disp`` / ``Model.render`` (src/model.rs:36-45, :295, :299-305) --
with ``wgpu::Device`` / ``wgpu::RenderPass`` replaced by :class:`Device` / :class:`Frame`.

There is NO CPU fallback here: if libmtr.so is missing, importing this module raises.
"""
from __future__ import annotations

import ctypes as C
import os  # noqa: F401  (api.os, like every public name this module has had, stays reachable)
from typing import List, Optional, Sequence

import numpy as np

from ._lib import (EXPORTED_SYMBOLS, LIB_PATH, MTR_E_HIP, MTR_E_INVALID, MTR_E_NOMEM, MTR_E_OVERFLOW, MTR_E_UNSUPPORTED, MTR_OK,  # noqa: F401
                   FrameStats, MtrError, _create, _f32, _Handle, _Layout, _p, lib)
from ._tensors import _U8_I32, _U8_I32_F32, _DeviceArgs, _layer_stacks, _nbytes
from .anim_sets import (Anim, AnimBlend, AnimCtrl, AnimEvents, AnimIK, AnimMasks, AnimMatch, AnimPlayer, AnimRoot, AnimSpring, AnimTracks,  # noqa: F401
                        _handle_of)
from .records import *  # noqa: F401,F403  (the dtypes, the constants and the record builders)
from .records import (ANIM_IK_TARGET, ANIM_LAYER, ANIM_STATE, ATTACH, OWN_INTERLEAVED, SPRING_STATE, STAGE_NAMES, anim_layers, anim_states, attach_records,
                      ik_targets, root_steps)
from .scene import ModelData, TextureData


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


class Texture(_Handle):
    _destroy = "mtr_texture_destroy"

    def __init__(self, dev: Device, h):
        self.dev, self._h = dev, h

    @staticmethod
    def new(dev: Device, resource: TextureData) -> "Texture":
        """Texture::new(device, queue, resource) -- src/texture.rs:11."""
        buf = np.frombuffer(resource.data, dtype=np.uint8)
        t = Texture(dev, _create(dev, lib.mtr_texture_create_mips, dev._h, resource.width, resource.height, resource.fmt,
                                 getattr(resource, "levels", 1), _p(buf), buf.size))
        t.width, t.height = resource.width, resource.height
        return t

    def read_rgba8(self) -> np.ndarray:
        out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self.dev.check(lib.mtr_texture_read_rgba8(self._h, _p(out), out.size))
        return out


class Model(_Handle):
    _destroy = "mtr_model_destroy"

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
        h = _create(dev, lib.mtr_model_create, dev._h, _p(vb), vb.size, _p(ib), ib.size, _p(pr), pr.shape[0], C.cast(lays, C.c_void_p),
                    _p(p2t), C.cast(th, C.c_void_p), len(textures), _p(did))
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
        self.dev.check(lib.mtr_model_animate_layers(self._h, anim._h, _handle_of(masks), _p(ly), ly.shape[1]))

    def animate_ik(self, anim: "Anim", layers, ik: "AnimIK", targets, masks: Optional["AnimMasks"] = None):
        """palette formed on the GPU (k_anim_ik) from one layer stack and one target per chain of ``ik`` (an ANIM_IK_TARGET
        array [K] or a dict of its fields; SPEC.md section 17)"""
        ly = anim_layers(layers, 1)
        tg = ik_targets(targets, 1, ik.nchains)
        self.dev.check(lib.mtr_model_animate_ik(self._h, anim._h, _handle_of(masks), _p(ly), ly.shape[1], ik._h, _p(tg)))

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
        super().close()
        for t in self.textures:
            t.close()
        self.textures = []


class Batch(_Handle):
    """n instances of one Model resident in HBM (the build's scheduler submission)."""
    _destroy = "mtr_batch_destroy"

    def __init__(self, dev: Device, model: Model, model_mats: np.ndarray, palettes: Optional[np.ndarray] = None,
                 texture_override: Optional[Sequence[int]] = None):
        mm = _f32(model_mats, (-1, 16))
        n = mm.shape[0]
        pal, npal = None, 0
        if palettes is not None:
            pal = _f32(palettes).reshape(n, -1, 16)
            npal = pal.shape[1]
        to = None if texture_override is None else np.ascontiguousarray(texture_override, dtype=np.int32)
        self._h = _create(dev, lib.mtr_batch_create, dev._h, model._h, n, _p(mm), _p(pal), npal, _p(to))
        self.dev, self.n, self.model, self.npal = dev, n, model, npal

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

    def _args(self, stream=None) -> _DeviceArgs:
        """the tensors of one device call of this batch, whose device message names the batch"""
        return _DeviceArgs(self.dev, stream, "batch on")

    def set_poses(self, local_mats):
        """one pose per instance, [n, njoints, 16] local matrices, through the model's skeleton (k_pose).  A numpy array is
        copied in; a torch tensor on the batch's device is read in stream order on torch.cuda.current_stream()."""
        if isinstance(local_mats, np.ndarray):
            lm = _f32(local_mats).reshape(self.n, -1, 16)
            self.dev.check(lib.mtr_batch_set_poses(self._h, _p(lm), lm.shape[1]))
            self.npal = lm.shape[1]
            return
        a = self._args()
        t = a.read(local_mats, "set_poses", "a numpy array or a float32 tensor on the GPU", ("float32",),
                   size_ok=lambda t: t.numel() % (self.n * 16) == 0, size_msg="n x njoints x 16 local matrices")
        nj = t.numel() // (self.n * 16)
        a.call(lib.mtr_batch_set_poses_device, (self._h, a.ptr(t), nj))
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
        a = self._args()
        t = a.read(states, "animate", "a numpy ANIM_STATE array, a dict, or a uint8 / int32 tensor on the GPU", _U8_I32,
                   size_ok=lambda t: _nbytes(t) == self.n * ANIM_STATE.itemsize, size_msg="n states of 24 bytes", align=8)
        a.call(lib.mtr_batch_animate_device, (self._h, anim._h, a.ptr(t)))
        self.npal = anim.njoints

    def animate_layers(self, anim: Anim, layers, masks: Optional[AnimMasks] = None, L: Optional[int] = None):
        """one layer stack per instance through ``anim``, ``masks`` (or None) and the model's skeleton (k_anim_layers, SPEC.md
        section 16).  A structured numpy array (ANIM_LAYER, [n, L]) or a dict of its fields is copied in; a torch uint8
        [n, L * 16] / int32 [n, L * 4] tensor on the batch's device holding ANIM_LAYER records is read in stream order on
        torch.cuda.current_stream()."""
        mh = _handle_of(masks)
        if isinstance(layers, (np.ndarray, dict)):
            ly = anim_layers(layers, self.n, L)
            self.dev.check(lib.mtr_batch_animate_layers(self._h, anim._h, mh, _p(ly), ly.shape[1]))
            self.npal = anim.njoints
            return
        a = self._args()
        t = a.read(layers, "animate_layers", "a numpy ANIM_LAYER array, a dict, or a uint8 / int32 tensor on the GPU", _U8_I32,
                   size_ok=lambda t: _layer_stacks(t, self.n, L), size_msg="n x L layers of 16 bytes")
        a.call(lib.mtr_batch_animate_layers_device, (self._h, anim._h, mh, a.ptr(t), self._nlayers(t)))
        self.npal = anim.njoints

    def _nlayers(self, t) -> int:
        return _nbytes(t) // (self.n * ANIM_LAYER.itemsize)

    def _layers(self, a: _DeviceArgs, what: str, layers, L: Optional[int]):
        return a.records(layers, what, "layers", lambda r: anim_layers(r, self.n, L), self.n)

    def _targets(self, a: _DeviceArgs, what: str, targets, ik: AnimIK):
        return a.records(targets, what, "targets", lambda r: ik_targets(r, self.n, ik.nchains), self.n)

    def _sized_layers(self, what: str, tl, L: Optional[int]):
        if not _layer_stacks(tl, self.n, L):
            raise MtrError(MTR_E_INVALID, f"{what}: n x L layers of 16 bytes")

    def _sized_targets(self, what: str, tt, ik: AnimIK):
        if _nbytes(tt) != self.n * ik.nchains * ANIM_IK_TARGET.itemsize:
            raise MtrError(MTR_E_INVALID, f"{what}: n x nchains targets of 32 bytes")

    def animate_ik(self, anim: Anim, layers, ik: AnimIK, targets, masks: Optional[AnimMasks] = None, L: Optional[int] = None):
        """one layer stack and one target per chain of ``ik`` per instance (k_anim_ik, SPEC.md section 17).  Numpy arrays
        (ANIM_LAYER [n, L], ANIM_IK_TARGET [n, K]) or dicts of their fields are copied in.  Where either is a torch uint8 /
        int32 / float32 tensor on the batch's device holding the records, both are read from device memory in stream order
        on torch.cuda.current_stream() (a numpy one of the pair is uploaded on that stream first)."""
        mh = _handle_of(masks)
        host = (np.ndarray, dict)
        if isinstance(layers, host) and isinstance(targets, host):
            ly = anim_layers(layers, self.n, L)
            tg = ik_targets(targets, self.n, ik.nchains)
            self.dev.check(lib.mtr_batch_animate_ik(self._h, anim._h, mh, _p(ly), ly.shape[1], ik._h, _p(tg)))
            self.npal = anim.njoints
            return
        a, what = self._args(), "animate_ik"
        tl, tt = self._layers(a, what, layers, L), self._targets(a, what, targets, ik)
        self._sized_layers(what, tl, L)  # the sizes of the pair are checked once both are tensors
        self._sized_targets(what, tt, ik)
        a.call(lib.mtr_batch_animate_ik_device, (self._h, anim._h, mh, a.ptr(tl), self._nlayers(tl), ik._h, a.ptr(tt)))
        self.npal = anim.njoints

    def animate_spring(self, anim: Anim, layers, spring: "AnimSpring", states, dt: float, ik: Optional[AnimIK] = None, targets=None, motion=None,
                       masks: Optional[AnimMasks] = None, L: Optional[int] = None):
        """one layer stack per instance, the chains of ``ik`` (or None) against ``targets``, then one step of ``dt`` seconds of
        the springs of ``spring`` (k_anim_spring, SPEC.md section 24).  states: a torch uint8 / int32 / float32 tensor on the
        batch's device holding n x nsprings SPRING_STATE records, contiguous and 16-byte aligned; it is read AND written in
        stream order on torch.cuda.current_stream(), so no copy is made of it.  motion: None, or such a float32 tensor
        [n, 16] as Anim.root_deltas_device gives.  layers and targets: numpy arrays or dicts (uploaded on that stream first)
        or record tensors on the device."""
        a, what = self._args(), "animate_spring"
        if (ik is None) != (targets is None):
            raise MtrError(MTR_E_INVALID, f"{what}: targets go with an IK set, and an IK set with targets")
        tl = self._layers(a, what, layers, L)
        self._sized_layers(what, tl, L)
        tt = None
        if ik is not None:
            tt = self._targets(a, what, targets, ik)
            self._sized_targets(what, tt, ik)
        # the states are written: the caller's own memory or nothing
        st = a.read(states, what, "spring states as a uint8 / int32 / float32 tensor on the GPU", _U8_I32_F32,
                    size_ok=lambda t: _nbytes(t) == self.n * spring.nsprings * SPRING_STATE.itemsize and t.is_contiguous() and t.data_ptr() % 16 == 0,
                    size_msg="n x nsprings states of 32 bytes, contiguous and 16-byte aligned")
        mo = None
        if motion is not None:
            mo = a.read(motion, what, "motion as a float32 tensor on the GPU", ("float32",), size_ok=lambda t: t.numel() == self.n * 16, size_msg="n x 16 floats")
        a.call(lib.mtr_batch_animate_spring_device,
               (self._h, anim._h, _handle_of(masks), a.ptr(tl), self._nlayers(tl), _handle_of(ik), a.ptr(tt), spring._h, a.ptr(st), a.ptr(mo), float(dt)))
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
        a = self._args(stream)
        t = a.read(recs, "attach", "a numpy ATTACH array, a dict, or a uint8 / int32 / float32 tensor on the GPU", _U8_I32_F32,
                   size_ok=lambda t: _nbytes(t) == self.n * ATTACH.itemsize, size_msg="n records of 80 bytes")
        a.call(lib.mtr_batch_attach_device, (self._h, src._h, a.ptr(t)))

    def root_motion(self, traj: "Anim", root: "AnimRoot", steps):
        """moves every instance by the blended delta of its steps on the trajectory set ``traj`` (k_root, SPEC.md section 19):
        M := M . D into a fresh version; palettes and npal are kept.  One shot; the host advances the positions itself.
        steps: a ROOT_STEP array [n, S] (or [n]: one step each) or a dict of its fields, host memory."""
        st = root_steps(steps, self.n)
        self.dev.check(lib.mtr_batch_root_motion(self._h, traj._h, root._h, _p(st), st.shape[1]))

    def root_motion_device(self, traj: "Anim", root: "AnimRoot", steps, stream=None):
        """the same from a torch uint8 [n, S, 16] / int32 / float32 [n, S, 4] tensor on the batch's device holding ROOT_STEP
        records, read in stream order on ``stream`` (a torch stream; None: torch.cuda.current_stream())."""
        a = _DeviceArgs(self.dev, stream)  # the root-motion calls word the device message as the root set's do
        t = a.root_steps(steps, "root motion", self.n)
        a.call(lib.mtr_batch_root_motion_device, (self._h, traj._h, root._h, a.ptr(t), t.shape[1]))

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



class Group(_Handle):
    """One host thread, N devices (include/mtr.h: mtr_group_*): rank r is a Device on hip_devices[r]; a group frame is one
    sharded Frame per rank, and ending it gathers every part's colour into one image on rank 0's device."""
    _destroy = "mtr_group_destroy"

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
            super().close()
            for d in self.devices:
                d._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class GroupFrame(_Handle):
    """begin -> draw into part(r) with rank r's models / batches -> end() -> color()"""
    _destroy = "mtr_group_frame_destroy"

    def __init__(self, group: Group, width: int, height: int, clear_rgba=(1.0, 1.0, 1.0, 1.0), clear_depth: float = 1.0,
                 own_map: int = OWN_INTERLEAVED, param: int = 0, band_rows=None):
        c = _f32(clear_rgba, 4)
        br = None if band_rows is None else np.ascontiguousarray(band_rows, dtype=np.uint32)
        if br is not None and br.size != len(group) + 1:
            raise MtrError(MTR_E_INVALID, "band_rows needs world + 1 entries")
        h = _create(group, lib.mtr_group_frame_begin, group._h, width, height, _p(c), clear_depth, own_map, param, _p(br))
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
            super().close()
