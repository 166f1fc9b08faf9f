"""GPU: what the binding says when it refuses a tensor argument of a call that reads records in stream order (Batch.set_poses,
animate, animate_layers, animate_ik, animate_spring, attach, root_motion_device and AnimRoot.deltas), text for text and in the
order type, device, size; and the one policy such a call has for a read-only tensor that is not contiguous or not 16-byte
aligned: a copy made on the call's stream, so the palettes and matrices equal those of the contiguous, aligned tensor bit for
bit.  Every refusal is made in Python, before any library call."""
import numpy as np
import pytest

from mt_renderer_amd import api
from tests import anim_ik_model as ik
from tests import anim_model as am
from tests import spring_model as sm
from tests.test_gpu_anim import CHAIN64, _bits_equal, _small_md
from tests.test_gpu_player import _raises_saying

pytestmark = pytest.mark.gpu

N, J = 2, 64
REC3 = "a uint8 / int32 / float32 tensor on the GPU"


def _placements(torch, rows, row_bytes):
    """uint8 [rows, row_bytes] tensors on cuda:0: contiguous and aligned, a view of every other half row, and one that begins
    8 bytes into its allocation"""
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device="cuda:0")
    off = u8(rows * row_bytes + 16)[8:8 + rows * row_bytes].view(rows, row_bytes)
    wide = u8(rows * 2 * row_bytes).view(rows, 2 * row_bytes)[:, :row_bytes]
    assert off.is_contiguous() and off.data_ptr() % 16 == 8 and not wide.is_contiguous() and wide.data_ptr() % 16 == 0
    return [("contiguous and aligned", u8(rows * row_bytes).view(rows, row_bytes)), ("non-contiguous", wide), ("offset by 8 bytes", off)]


def _behind_a_long_operation(torch, t, good, junk, call):
    """``t`` holds ``good`` only on a side stream, between a long GPU operation and a write of ``junk``: the call reads it there"""
    t.copy_(junk)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        torch.cuda._sleep(2_000_000)
        t.copy_(good)
        call(t)
        t.copy_(junk)
    torch.cuda.synchronize()


def test_tensor_arguments_are_refused_in_the_same_words_and_copied_on_the_stream(gpu_device):
    import torch
    dev = gpu_device
    rng = np.random.default_rng(5)
    clips, traj_clips = am.random_clips(rng, J), am.random_clips(rng, 1)
    eye = np.tile(np.eye(4, dtype=np.float32).reshape(16), (J, 1))
    m = api.Model.new(dev, _small_md())
    m.set_skeleton(CHAIN64, eye)
    mats = np.tile(np.eye(4, dtype=np.float32).reshape(16), (N, 1))
    b, tgt = api.Batch(dev, m, mats), api.Batch(dev, m, mats)
    anim, traj = api.Anim(dev, J, clips), api.Anim(dev, 1, traj_clips)
    masks = api.AnimMasks(dev, J, np.linspace(0.0, 1.0, J, dtype=np.float32))
    iks = api.AnimIK(dev, ik.skeleton(J), ik.default_chains(ik.skeleton(J), 1).astype(api.ANIM_IK_CHAIN))
    spring = api.AnimSpring(dev, ik.skeleton(J), sm.make_springs([1], [(0.0, 1.0, 0.0)], dtype=api.SPRING))
    root = api.AnimRoot(dev, 1, len(traj_clips), 0)
    assert iks.nchains == 1 and spring.nsprings == 1
    u8 = lambda *shape: torch.zeros(shape, dtype=torch.uint8, device="cuda:0")
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda:0")
    f64 = lambda *shape: torch.zeros(shape, dtype=torch.float64, device="cuda:0")
    ly, tg, st, mo = u8(N, 16), u8(N, 32), u8(N, 32), f32(N, 16)  # a valid layers, targets, spring states and motion tensor
    spr = lambda layers=ly, states=st, **kw: b.animate_spring(anim, layers, spring, states, 1.0 / 60.0, **kw)
    try:
        poses = "set_poses: a numpy array or a float32 tensor on the GPU"
        states = "animate: a numpy ANIM_STATE array, a dict, or a uint8 / int32 tensor on the GPU"
        layers = "animate_layers: a numpy ANIM_LAYER array, a dict, or a uint8 / int32 tensor on the GPU"
        pair = lambda what, name: f"{what}: {name} as a numpy array, a dict, or {REC3}"
        recs = f"attach: a numpy ATTACH array, a dict, or {REC3}"
        steps = lambda what: f"{what}: a numpy ROOT_STEP array, a dict, or {REC3}"
        step_size = lambda what: f"{what}: steps of 16 bytes, [n, S, 16] uint8 or [n, S, 4] int32 / float32"
        cases = [
            # per caller: a CPU tensor, a wrong dtype, a wrong size
            (lambda: b.set_poses(f32(N, J, 16).cpu()), poses),
            (lambda: b.set_poses(u8(N, J, 16)), poses),
            (lambda: b.set_poses([[0.0] * 16] * (N * J)), poses),
            (lambda: b.set_poses(f32(N * J * 16 + 1)), "set_poses: n x njoints x 16 local matrices"),
            (lambda: b.animate(anim, u8(N, 24).cpu()), states),
            (lambda: b.animate(anim, f32(N, 6)), states),
            (lambda: b.animate(anim, [1, 2, 3]), states),
            (lambda: b.animate(anim, u8(N + 1, 24)), "animate: n states of 24 bytes"),
            (lambda: b.animate_layers(anim, ly.cpu()), layers),
            (lambda: b.animate_layers(anim, f32(N, 4)), layers),
            (lambda: b.animate_layers(anim, u8(N * 16 + 8)), "animate_layers: n x L layers of 16 bytes"),
            (lambda: b.animate_layers(anim, u8(0)), "animate_layers: n x L layers of 16 bytes"),
            (lambda: b.animate_layers(anim, ly, masks, L=2), "animate_layers: n x L layers of 16 bytes"),
            (lambda: b.animate_ik(anim, ly.cpu(), iks, tg), pair("animate_ik", "layers")),
            (lambda: b.animate_ik(anim, f64(N, 2), iks, tg), pair("animate_ik", "layers")),
            (lambda: b.animate_ik(anim, u8(N * 16 + 8), iks, tg), "animate_ik: n x L layers of 16 bytes"),
            (lambda: b.animate_ik(anim, ly, iks, tg.cpu()), pair("animate_ik", "targets")),
            (lambda: b.animate_ik(anim, ly, iks, f64(N, 4)), pair("animate_ik", "targets")),
            (lambda: b.animate_ik(anim, ly, iks, u8(N + 1, 32)), "animate_ik: n x nchains targets of 32 bytes"),
            # the layers speak before the targets, a type before a size
            (lambda: b.animate_ik(anim, ly.cpu(), iks, tg.cpu()), pair("animate_ik", "layers")),
            (lambda: b.animate_ik(anim, u8(N * 16 + 8), iks, tg.cpu()), pair("animate_ik", "targets")),
            (lambda: b.animate_ik(anim, u8(N * 16 + 8), iks, u8(N + 1, 32)), "animate_ik: n x L layers of 16 bytes"),
            (lambda: spr(targets=tg), "animate_spring: targets go with an IK set, and an IK set with targets"),
            (lambda: spr(ik=iks), "animate_spring: targets go with an IK set, and an IK set with targets"),
            (lambda: spr(ly.cpu(), targets=tg), "animate_spring: targets go with an IK set, and an IK set with targets"),
            (lambda: spr(ly.cpu()), pair("animate_spring", "layers")),
            (lambda: spr(f64(N, 2)), pair("animate_spring", "layers")),
            (lambda: spr(u8(N * 16 + 8)), "animate_spring: n x L layers of 16 bytes"),
            (lambda: spr(ik=iks, targets=tg.cpu()), pair("animate_spring", "targets")),
            (lambda: spr(ik=iks, targets=f64(N, 4)), pair("animate_spring", "targets")),
            (lambda: spr(ik=iks, targets=u8(N + 1, 32)), "animate_spring: n x nchains targets of 32 bytes"),
            (lambda: spr(states=st.cpu()), f"animate_spring: spring states as {REC3}"),
            (lambda: spr(states=f64(N, 4)), f"animate_spring: spring states as {REC3}"),
            (lambda: spr(states=u8(N + 1, 32)), "animate_spring: n x nsprings states of 32 bytes, contiguous and 16-byte aligned"),
            (lambda: spr(states=u8(N, 64)[:, :32]), "animate_spring: n x nsprings states of 32 bytes, contiguous and 16-byte aligned"),
            (lambda: spr(states=u8(N * 32 + 16)[8:8 + N * 32]), "animate_spring: n x nsprings states of 32 bytes, contiguous and 16-byte aligned"),
            (lambda: spr(motion=mo.cpu()), "animate_spring: motion as a float32 tensor on the GPU"),
            (lambda: spr(motion=u8(N, 64)), "animate_spring: motion as a float32 tensor on the GPU"),
            (lambda: spr(motion=f32(N, 15)), "animate_spring: n x 16 floats"),
            # the layers before the targets, the targets before the states, the states before the motion
            (lambda: spr(u8(N * 16 + 8), st.cpu(), ik=iks, targets=tg.cpu()), "animate_spring: n x L layers of 16 bytes"),
            (lambda: spr(states=st.cpu(), ik=iks, targets=u8(N + 1, 32), motion=mo.cpu()), "animate_spring: n x nchains targets of 32 bytes"),
            (lambda: spr(states=u8(N + 1, 32), motion=mo.cpu()), "animate_spring: n x nsprings states of 32 bytes, contiguous and 16-byte aligned"),
            (lambda: tgt.attach(b, u8(N, 80).cpu()), recs),
            (lambda: tgt.attach(b, f64(N, 10)), recs),
            (lambda: tgt.attach(b, u8(N + 1, 80)), "attach: n records of 80 bytes"),
            (lambda: b.root_motion_device(traj, root, u8(N, 1, 16).cpu()), steps("root motion")),
            (lambda: b.root_motion_device(traj, root, f64(N, 1, 2)), steps("root motion")),
            (lambda: b.root_motion_device(traj, root, u8(N, 1, 15)), step_size("root motion")),
            (lambda: b.root_motion_device(traj, root, u8(N * 16)), step_size("root motion")),
            (lambda: b.root_motion_device(traj, root, u8(N, 16)), "root motion: a tensor [n, S, 16 bytes]"),
            (lambda: b.root_motion_device(traj, root, f32(N + 1, 2, 4)), "root motion: a tensor [n, S, 16 bytes]"),
            (lambda: root.deltas(traj, u8(N, 1, 16).cpu()), steps("root deltas")),
            (lambda: root.deltas(traj, f64(N, 1, 2)), steps("root deltas")),
            (lambda: root.deltas(traj, [0, 1]), steps("root deltas")),
            (lambda: root.deltas(traj, f32(N, 2, 3)), step_size("root deltas")),
            (lambda: root.deltas(traj, u8(N, 16)), "root deltas: a tensor [n, S, 16 bytes]"),
        ]
        if torch.cuda.device_count() > 1:  # the device after the type, before the size
            on1 = lambda shape, dtype=torch.uint8: torch.zeros(shape, dtype=dtype, device="cuda:1")
            batch, device = "the tensor is on cuda:1, the batch on cuda:0", "the tensor is on cuda:1, the device is cuda:0"
            cases += [
                (lambda: b.set_poses(on1(N * J * 16 + 1, torch.float32)), f"set_poses: {batch}"),
                (lambda: b.animate(anim, on1((N + 1, 24))), f"animate: {batch}"),
                (lambda: b.animate_layers(anim, on1(N * 16 + 8)), f"animate_layers: {batch}"),
                (lambda: b.animate_ik(anim, on1((N, 16)), iks, tg), f"animate_ik: {batch}"),
                (lambda: b.animate_ik(anim, ly, iks, on1((N, 32))), f"animate_ik: {batch}"),
                (lambda: spr(on1((N, 16))), f"animate_spring: {batch}"),
                (lambda: spr(ik=iks, targets=on1((N, 32))), f"animate_spring: {batch}"),
                (lambda: spr(states=on1((N + 1, 32))), f"animate_spring: {batch}"),
                (lambda: spr(motion=on1((N, 15), torch.float32)), f"animate_spring: {batch}"),
                (lambda: tgt.attach(b, on1((N + 1, 80))), f"attach: {batch}"),
                (lambda: b.root_motion_device(traj, root, on1((N, 1, 15))), f"root motion: {device}"),
                (lambda: root.deltas(traj, on1((N, 16))), f"root deltas: {device}"),
                (lambda: b.animate(anim, on1((N, 6), torch.float32)), states),
            ]
        _raises_saying(cases)
        torch.cuda.synchronize()
        assert b.npal == 0 and _bits_equal(b.read_model_mats(), mats) and _bits_equal(tgt.read_model_mats(), mats), "nothing ran"
        assert not st.any().item() and not ly.any().item() and not tg.any().item() and not mo.any().item()

        # accepted: a layers tensor that is not contiguous, or not aligned, gives the palettes of the contiguous, aligned one
        good = api.anim_layers(dict(clip=[[0, 1], [2, 0]], x=[[0.5, 3.25], [7.75, 1.0]], w=[[1.0, 0.5], [1.0, 0.25]], mask=[[0, 1], [0, 0]]), N, 2)
        junk = good.copy()
        junk["x"] += np.float32(1.5)
        as_u8 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(N, -1).copy()).to("cuda:0")
        b.animate_layers(anim, junk, masks)
        pal_junk = b.read_palettes()
        pals = {}
        for name, t in _placements(torch, N, 2 * api.ANIM_LAYER.itemsize):
            _behind_a_long_operation(torch, t, as_u8(good), as_u8(junk), lambda t: b.animate_layers(anim, t, masks))
            pals[name] = b.read_palettes()
            assert b.npal == J and pals[name].shape == (N, J, 16) and np.isfinite(pals[name]).all()
            assert _bits_equal(pals[name], pals["contiguous and aligned"]), f"animate_layers, {name}"
        assert not _bits_equal(pal_junk, pals["contiguous and aligned"]), "the two inputs can be told apart"
        b.animate_layers(anim, good, masks)
        assert _bits_equal(b.read_palettes(), pals["contiguous and aligned"]), "the records of the tensor are the host's"

        # the same for attachment records, against the palettes just formed
        off = rng.standard_normal((N, 16)).astype(np.float32)
        good = api.attach_records(dict(src_instance=[1, 0], joint=[3, 40], offset=off), N)
        junk = good.copy()
        junk["offset"] = np.nan
        out = {}
        for name, t in _placements(torch, N, api.ATTACH.itemsize):
            tgt.update(model_mats=np.zeros((N, 16), dtype=np.float32))
            _behind_a_long_operation(torch, t, as_u8(good), as_u8(junk), lambda t: tgt.attach(b, t))
            out[name] = tgt.read_model_mats()
            assert np.isfinite(out[name]).all() and out[name].any()
            assert _bits_equal(out[name], out["contiguous and aligned"]), f"attach, {name}"
        tgt.attach(b, good)
        assert _bits_equal(tgt.read_model_mats(), out["contiguous and aligned"]), "the records of the tensor are the host's"
    finally:
        for h in (tgt, b, root, spring, iks, masks, traj, anim, m):
            h.close()
