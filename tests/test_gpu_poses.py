"""GPU: skeletal poses (SPEC.md section 12).  k_pose forms palettes bit for bit as mtr_rmodel_palette does on the host
(files.ModelFile.palette over a synthetic rModel); posed models and batches render bit-exact against the oracle given those
palettes; batch updates keep the frame semantics of recorded draws (frames in flight, overflow re-runs by mtr_frame_wait
and by the exchange thread, sharded culling); poses from device memory; invalid calls change nothing; no memory growth."""
import ctypes as C

import numpy as np
import pytest

from mt_renderer_amd import api, files, scene
from oracle import oracle as orc
from tests import mt_files
from tests.helpers import assert_same, render_oracle

pytestmark = pytest.mark.gpu

CHAIN64 = [255] + list(range(63))


def _skeletons():
    rng = np.random.default_rng(11)
    tree = [int(rng.integers(j + 1, 64)) for j in range(63)] + [255]  # every parent listed after its child
    multi = []
    for j in range(40):
        if j in (0, 25):
            multi.append(255)
        elif j in (10, 30):
            multi.append(j)  # its own parent: a root
        else:
            multi.append(int(rng.integers(0, 40)) if j > 30 else int(rng.integers(0, j)))
    big = [j + 1 if j % 3 else int(rng.integers(j + 1, 256)) for j in range(255)] + [255]
    # multi: joints past 30 pick any parent; keep only choices that form no cycle
    for j in range(31, 40):
        while True:
            p, seen, k = multi[j], set(), j
            while k not in seen and multi[k] not in (255, k):
                seen.add(k)
                k = multi[k]
            if k not in seen:
                break
            multi[j] = int(rng.integers(0, 31))
    return {"chain64": CHAIN64, "tree_parents_after": tree, "multi_root": multi, "j256": big}


SKELETONS = _skeletons()


def _rot(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _trs(rng, n, scale=(0.95, 1.05), trans=10.0, angle=None):
    """n column-major f32 matrices: a random rotation (or one about z by at most `angle`), per-axis scale, translation"""
    out = np.zeros((n, 16), dtype=np.float32)
    for i in range(n):
        if angle is None:
            R = _rot(rng)
        else:
            a = rng.uniform(-angle, angle)
            R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        M = np.eye(4)
        M[:3, :3] = R * rng.uniform(*scale, size=3)[None, :]
        M[:3, 3] = rng.uniform(-trans, trans, size=3)
        out[i] = M.T.reshape(16)
    return out


def _small_md():
    return scene.skinned_capsule_model([((0.0, 0.0, 0.0), 0.35, 1.6)], rows=2, cols=3)


def _model_file(parents, imats):
    md = _small_md()
    n = len(parents)
    joints = [(j, int(p), (0.0, 0.0, 0.0)) for j, p in enumerate(parents)]
    lm = np.tile(np.eye(4, dtype=np.float32).reshape(16), (n, 1))
    return files.ModelFile(mt_files.write_rmodel(md, [0] * md.nprims, ["m"], [0] * md.nprims, joints=joints, lmats=lm, imats=imats))


def _ref_palettes(mf, poses):
    return np.stack([mf.palette(p) for p in poses]).astype(np.float32)


def _np_palettes(parents, poses, imats, reverse):
    """the rule with float32 products and sums (no fma); reverse: local * world_parent instead of world_parent * local"""
    def mul(A, B):  # column-major [n, 16] x [n, 16]
        out = np.zeros_like(A)
        for c in range(4):
            for i in range(4):
                s = np.zeros(A.shape[0], dtype=np.float32)
                for k in range(4):
                    s = (s + A[:, k * 4 + i] * B[:, c * 4 + k]).astype(np.float32)
                out[:, c * 4 + i] = s
        return out
    J = len(parents)
    world = [None] * J

    def get(j):
        if world[j] is None:
            p = parents[j]
            L = poses[:, j]
            world[j] = L.copy() if p in (255, j) else (mul(L, get(p)) if reverse else mul(get(p), L))
        return world[j]
    return np.stack([mul(get(j), np.broadcast_to(imats[j], poses[:, j].shape).copy()) for j in range(J)], axis=1)


def _bits_equal(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


@pytest.mark.parametrize("kind", list(SKELETONS))
def test_pose_palettes_are_bit_exact(gpu_device, kind):
    parents = SKELETONS[kind]
    J, n = len(parents), 8
    rng = np.random.default_rng(J * 7 + len(kind))
    imats = _trs(rng, J, scale=(0.5, 2.0), trans=20.0)
    poses = _trs(rng, n * J, trans=10.0).reshape(n, J, 16)
    ref = _ref_palettes(_model_file(parents, imats), poses)
    assert np.isfinite(ref).all()
    m = api.Model.new(gpu_device, _small_md())
    b = None
    try:
        m.set_skeleton(parents, imats)
        b = api.Batch(gpu_device, m, np.tile(np.eye(4, dtype=np.float32).reshape(16), (n, 1)))
        b.set_poses(poses)
        got = b.read_palettes()
        assert got.shape == (n, J, 16)
        assert _bits_equal(got, ref), f"{int((got != ref).sum())} of {ref.size} palette elements differ"
        if kind == "chain64":
            # the poses are strong enough that the other product order, or products without fma, change bits: a kernel
            # that multiplied in the other order (or lost an fma) would fail the comparison above
            assert not _bits_equal(_np_palettes(parents, poses, imats, reverse=True), ref)
            assert not _bits_equal(_np_palettes(parents, poses, imats, reverse=False), ref)
    finally:
        if b:
            b.close()
        m.close()


def _render(dev, W, H, draw):
    fr = api.Frame(dev, W, H)
    try:
        draw(fr)
        fr.end()
        return fr.color(), fr.depth(), fr.stats()
    finally:
        fr.close()


def _bend(rng, n, angle=0.04, trans=0.02):
    return _trs(rng, n, scale=(0.99, 1.01), trans=trans, angle=angle)


@pytest.mark.parametrize("textured", [False, True])
def test_model_pose_renders_like_the_oracle(gpu_device, textured):
    W, H = 160, 96
    tex = [scene.checker_rgba8_texture(64, 64)] if textured else None
    md = scene.mesh50k(textured=textured, textures=tex, rows=12, cols=20)
    rng = np.random.default_rng(21 + textured)
    imats = _bend(rng, 64, angle=0.05)
    local = _bend(rng, 64)
    pal = _model_file(CHAIN64, imats).palette(local)
    M = scene.to_f32_colmajor(scene.headline_transform(W, H))
    ref = render_oracle(W, H, [dict(md=md, M=M, palette=pal)])
    m = api.Model.new(gpu_device, md)
    try:
        m.set_skeleton(CHAIN64, imats)
        m.set_pose(local)
        for mode in (api.TILE_ORDERED, api.TILE_AUTO):
            gpu_device.set_tile_mode(mode)
            assert_same(_render(gpu_device, W, H, lambda fr: m.render(fr, M)), ref, f"model pose, tile mode {mode}")
        om = orc.OracleModel(md)
        for p in range(md.nprims):
            gc, gu = m.vertex_stage(p, M)
            rc_, ru = om.vertex_stage(p, M, pal)
            assert _bits_equal(gc, rc_) and _bits_equal(gu, ru), "vertex stage"
    finally:
        gpu_device.set_tile_mode(api.TILE_AUTO)
        m.close()


def _batch_setup(dev, n_side=4, rows=10, cols=16):
    md = scene.skinned_capsule_model([((0.0, 0.0, 0.0), 0.35, 1.6)], rows=rows, cols=cols)
    rng = np.random.default_rng(5)
    imats = _bend(rng, 64, angle=0.05)
    mf = _model_file(CHAIN64, imats)
    m = api.Model.new(dev, md)
    m.set_skeleton(CHAIN64, imats)
    return md, mf, m, rng


@pytest.mark.parametrize("cull", [True, False])
def test_batch_poses_and_updates_unsharded_and_sharded(gpu_device, cull):
    W, H = 192, 112
    md, mf, m, rng = _batch_setup(gpu_device)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats0, _ = scene.instance_lattice(4, 4, seed=300)
    b = api.Batch(gpu_device, m, mats0)
    gpu_device.set_culling(cull)
    try:
        for step in range(3):
            mats, _ = scene.instance_lattice(4, 4, seed=301 + step)
            poses = _bend(rng, 16 * 64, angle=0.08, trans=0.03).reshape(16, 64, 16)
            pals = _ref_palettes(mf, poses)
            if step == 1:
                b.update(model_mats=mats, palettes=pals)  # host palettes through mtr_batch_update
            else:
                b.set_poses(poses)
                b.update(model_mats=mats)
            assert _bits_equal(b.read_palettes(), pals)
            ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=mats, palettes=pals)])
            assert_same(_render(gpu_device, W, H, lambda fr: fr.draw_batch(b, vp)), ref, f"unsharded step {step}")
            nby = (H + 15) // 16
            for world in (2, 4):
                bands = np.round(np.linspace(0, nby, world + 1)).astype(np.uint32)
                for r in range(world):
                    def draw(fr):
                        fr.set_shard(r, world, api.OWN_BANDS, 0, bands)
                        fr.draw_batch(b, vp)
                    c, d, _ = _render(gpu_device, W, H, draw)
                    y0, y1 = int(bands[r]) * 16, min(int(bands[r + 1]) * 16, H)
                    assert (c[y0:y1] == ref[0][y0:y1]).all(), f"step {step}, rank {r} of {world}: colour"
                    assert _bits_equal(d[y0:y1], ref[1][y0:y1]), f"step {step}, rank {r} of {world}: depth"
    finally:
        gpu_device.set_culling(api.GEOM_CULL_SHARDED)
        b.close()
        m.close()


def test_frames_in_flight_each_with_its_own_pose(gpu_device):
    W, H = 160, 96
    md, mf, m, rng = _batch_setup(gpu_device, rows=6, cols=10)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    b = api.Batch(gpu_device, m, scene.instance_lattice(4, 4)[0])
    frames, args = [], []
    try:
        for k in range(40):
            mats, _ = scene.instance_lattice(4, 4, seed=500 + k)
            poses = _bend(rng, 16 * 64, angle=0.08).reshape(16, 64, 16)
            if k == 20:  # ring churn: many updates between two frames
                for c in range(30):
                    b.set_poses(_bend(rng, 16 * 64, angle=0.3).reshape(16, 64, 16))
                    b.update(model_mats=scene.instance_lattice(4, 4, seed=900 + c)[0])
            b.set_poses(poses)
            b.update(model_mats=mats)
            fr = api.Frame(gpu_device, W, H)
            fr.draw_batch(b, vp)
            fr.submit()
            frames.append(fr)
            args.append((mats, poses))
        for k in reversed(range(40)):
            fr = frames[k]
            fr.wait()
            if k % 4 == 0:
                mats, poses = args[k]
                ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=mats, palettes=_ref_palettes(mf, poses))])
                assert_same((fr.color(), fr.depth(), fr.stats()), ref, f"frame {k}")
    finally:
        for fr in frames:
            fr.close()
        b.close()
        m.close()


def _overflow_scene(dev, W):
    md, mf, m, rng = _batch_setup(dev, rows=10, cols=16)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, W))
    mats, _ = scene.instance_lattice(4, 4, seed=41)
    poses = _bend(rng, 16 * 64, angle=0.08).reshape(16, 64, 16)
    ref = render_oracle(W, W, [dict(md=md, vp=vp, model_mats=mats, palettes=_ref_palettes(mf, poses))])
    return m, rng, vp, mats, poses, ref


def _churn(b, rng, k):
    for c in range(k):
        b.set_poses(_bend(rng, 16 * 64, angle=0.5, trans=0.2).reshape(16, 64, 16))
        b.update(model_mats=scene.instance_lattice(4, 4, seed=700 + c)[0])


def test_overflow_rerun_by_wait_draws_the_recorded_pose():
    W = 48
    with api.Device(0) as dev:
        m, rng, vp, mats, poses, ref = _overflow_scene(dev, W)
        dev.set_binning(True, 64)
        b = api.Batch(dev, m, mats)
        b.set_poses(poses)
        fr = api.Frame(dev, W, W)
        fr.draw_batch(b, vp)
        fr.submit()
        _churn(b, rng, 40)  # updated after submit: the re-run must still draw what was recorded
        fr.wait()
        st = fr.stats()
        assert st["binning"] == 2, "the frame overflowed its 64-entry queues and was re-run through the exact queues"
        assert_same((fr.color(), fr.depth(), st), ref, "re-run after mtr_frame_wait")
        fr.close()
        b.close()
        m.close()


def test_overflow_rerun_by_the_exchange_thread_draws_the_recorded_pose():
    """One rank (the scene is dense enough to overflow every time only as a whole frame): the frame overflows its 64-entry
    queues when waited for, so the same frame handed to the exchange thread at the same bound overflows too and shows its
    recorded pose only if the thread re-ran it (otherwise its bins stay at the clear colour and the next call reports
    MTR_E_OVERFLOW)."""
    import torch
    W = 48
    xs = torch.cuda.Stream()
    with api.Device(0) as dev:
        m, rng, vp, mats, poses, ref = _overflow_scene(dev, W)
        b = api.Batch(dev, m, mats)
        b.set_poses(poses)
        dev.set_binning(True, 64)
        fr = api.Frame(dev, W, W)
        fr.draw_batch(b, vp)
        fr.submit()
        fr.wait()
        assert fr.stats()["binning"] == 2, "the frame must overflow its 64-entry queues"
        fr.close()
        world = 1
        nbytes = int(api.lib.mtr_shard_bytes(W, W, world))
        shard = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        gathered = torch.zeros(nbytes * world, dtype=torch.uint8, device="cuda")
        final = torch.zeros(W * W * 4, dtype=torch.uint8, device="cuda")

        @C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p)
        def fake_allgather(send, recv, count, dtype, comm, stream):
            with torch.cuda.stream(xs):
                gathered[:count].copy_(shard[:count], non_blocking=True)
            return 0

        dev.exchange_start(C.cast(fake_allgather, C.c_void_p).value, 0, 1, shard.data_ptr(), shard.numel(), gathered.data_ptr(),
                           final.data_ptr(), world, xs.cuda_stream)
        dev.set_binning(True, 64)
        fr = api.Frame(dev, W, W)
        fr.draw_batch(b, vp)
        fr.submit_exchange()
        _churn(b, rng, 20)  # updated after the hand-over: the re-run must still draw what was recorded
        dev.exchange_drain()
        torch.cuda.synchronize()
        got = final.cpu().numpy().reshape(W, W, 4)
        assert (got == ref[0]).all(), "the exchanged frame must show the pose it recorded"
        dev.synchronize()  # nothing latched: the exchange thread re-ran the overflowed frame itself
        dev.exchange_stop()
        b.close()
        m.close()


@pytest.mark.parametrize("stream", ["default", "side"])
def test_device_poses_follow_the_current_stream(gpu_device, stream):
    """The input tensor is written by torch work queued behind a long GPU op, and overwritten by work queued right after
    the frame is submitted, with no synchronisation in between: the frame shows the pose only if k_pose ran in stream order
    between the two (on torch's legacy default stream, whose handle is 0, as well as on a side stream)."""
    import torch
    W, H = 160, 96
    md, mf, m, rng = _batch_setup(gpu_device, rows=6, cols=10)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats, _ = scene.instance_lattice(4, 4, seed=61)
    poses = _bend(rng, 16 * 64, angle=0.08).reshape(16, 64, 16)
    pals = _ref_palettes(mf, poses)
    ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=mats, palettes=pals)])
    b = api.Batch(gpu_device, m, mats)
    fr = None
    try:
        src = torch.tensor(poses, device="cuda:0")
        nan = torch.full_like(src, float("nan"))
        t = torch.full_like(src, float("nan"))
        torch.cuda.synchronize()
        s = torch.cuda.current_stream() if stream == "default" else torch.cuda.Stream()
        with torch.cuda.stream(s):
            if stream == "default":
                assert torch.cuda.current_stream().cuda_stream == 0, "the legacy default stream"
            torch.cuda._sleep(50_000_000)  # a long GPU op in front of the producer
            t.copy_(src)                   # the input exists only after it
            b.set_poses(t)
            fr = api.Frame(gpu_device, W, H)
            fr.draw_batch(b, vp)
            fr.submit()
            t.copy_(nan)                   # later work on the stream overwrites the input
        fr.wait()
        assert_same((fr.color(), fr.depth(), fr.stats()), ref, f"device poses, {stream} stream")
        torch.cuda.synchronize()
        assert _bits_equal(b.read_palettes(), pals)
    finally:
        if fr:
            fr.close()
        b.close()
        m.close()


def test_device_poses_equal_host_poses(gpu_device):
    import torch
    md, mf, m, rng = _batch_setup(gpu_device, rows=6, cols=10)
    poses = _bend(rng, 16 * 64, angle=0.08).reshape(16, 64, 16)
    b = api.Batch(gpu_device, m, scene.instance_lattice(4, 4, seed=62)[0])
    try:
        b.set_poses(poses)
        host = b.read_palettes()
        assert _bits_equal(host, _ref_palettes(mf, poses))
        b.update(palettes=np.zeros((16, 64, 16), dtype=np.float32))
        t = torch.tensor(poses, device="cuda:0")
        b.set_poses(t[:, :, :].transpose(1, 2).contiguous().transpose(1, 2))  # not contiguous: copied first
        assert _bits_equal(b.read_palettes(), host)
        b.update(palettes=np.zeros((16, 64, 16), dtype=np.float32))
        b.set_poses(t)
        assert _bits_equal(b.read_palettes(), host)
    finally:
        b.close()
        m.close()


def test_invalid_calls_change_nothing(gpu_device):
    W, H = 160, 96
    md, mf, m, rng = _batch_setup(gpu_device, rows=6, cols=10)
    bare = api.Model.new(gpu_device, md)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats, _ = scene.instance_lattice(4, 4, seed=81)
    poses = _bend(rng, 16 * 64, angle=0.08).reshape(16, 64, 16)
    local = _bend(rng, 64)
    pals = _ref_palettes(mf, poses)
    b = api.Batch(gpu_device, m, mats)
    bb = api.Batch(gpu_device, bare, mats)
    try:
        def invalid(fn):
            with pytest.raises(api.MtrError) as e:
                fn()
            assert e.value.code == api.MTR_E_INVALID
        invalid(lambda: bare.set_pose(local))          # no skeleton
        invalid(lambda: bb.set_poses(poses))
        b.set_poses(poses)
        m.set_pose(local)
        im2 = np.tile(np.eye(4, dtype=np.float32).reshape(16), (2, 1))
        invalid(lambda: b.set_poses(poses[:, :63].copy()))  # njoints not the skeleton's
        invalid(lambda: m.set_pose(local[:63]))
        invalid(lambda: m.set_skeleton([1, 0], im2))        # a cycle
        invalid(lambda: m.set_skeleton([5, 255], im2))      # a parent out of range
        invalid(lambda: m.set_skeleton(np.zeros(0, np.uint8), np.zeros((0, 16), np.float32)))  # no joints
        invalid(lambda: m.set_skeleton([255] * 257, np.tile(im2[:1], (257, 1))))  # more than 256
        invalid(lambda: b.update(palettes=np.zeros((16, 257, 16), dtype=np.float32)))
        assert _bits_equal(b.read_palettes(), pals)
        ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=mats, palettes=pals)])
        assert_same(_render(gpu_device, W, H, lambda fr: fr.draw_batch(b, vp)), ref, "batch after invalid calls")
        M = scene.to_f32_colmajor(scene.headline_transform(W, H))
        ref = render_oracle(W, H, [dict(md=md, M=M, palette=mf.palette(local))])
        assert_same(_render(gpu_device, W, H, lambda fr: m.render(fr, M)), ref, "model after invalid calls")
        m.set_pose(local)  # the skeleton is still the one set first
        m.set_skeleton(None)
        invalid(lambda: m.set_pose(local))
    finally:
        b.close()
        bb.close()
        bare.close()
        m.close()


def _files_model(dev, md, joints, lm, im):
    rmodel, rshader2, rmaterial, _ = mt_files.files_from_model_data(md)
    names = [f"mat_{p}" for p in range(md.nprims)]
    rmodel = mt_files.write_rmodel(md, [mt_files.handle_of("IATest0", low=p) for p in range(md.nprims)], names, list(range(md.nprims)),
                                   joints=joints, lmats=lm, imats=im)
    sh = files.Shader2File(rshader2)
    mat = files.MaterialFile(rmaterial, sh)
    mf = files.ModelFile(rmodel)
    return files.model_from_files(dev, mf, sh, mat, []), mf, (sh, mat)


def test_create_from_files_sets_the_file_skeleton_or_none(gpu_device):
    W, H = 160, 96
    md = scene.mesh50k(rows=6, cols=10)
    rng = np.random.default_rng(91)
    lm = _bend(rng, 64)
    im = _bend(rng, 64, angle=0.05)
    M = scene.to_f32_colmajor(scene.headline_transform(W, H))
    good = [(j, CHAIN64[j], (0.0, 0.01 * j, 0.0)) for j in range(64)]
    model, mf, keep = _files_model(gpu_device, md, good, lm, im)
    try:
        parents, imats = mf.skeleton()
        assert list(parents) == CHAIN64
        model.set_pose(lm)
        ref = render_oracle(W, H, [dict(md=md, M=M, palette=mf.palette(lm))])
        assert_same(_render(gpu_device, W, H, lambda fr: model.render(fr, M)), ref, "pose through the file's skeleton")
    finally:
        model.close()
        for k in keep:
            k.close()
    cyclic = [(j, (j + 1) % 64, (0.0, 0.0, 0.0)) for j in range(64)]
    model, mf, keep = _files_model(gpu_device, md, cyclic, lm, im)
    try:
        ref = render_oracle(W, H, [dict(md=md, M=M, palette=None)])
        assert_same(_render(gpu_device, W, H, lambda fr: model.render(fr, M)), ref, "cyclic skeleton: created as without one")
        with pytest.raises(api.MtrError) as e:
            model.set_pose(lm)
        assert e.value.code == api.MTR_E_INVALID
    finally:
        model.close()
        for k in keep:
            k.close()


def test_batch_lifetime_and_no_memory_growth(gpu_device):
    import torch
    W, H = 160, 96
    md, mf, m, rng = _batch_setup(gpu_device, rows=6, cols=10)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats, _ = scene.instance_lattice(4, 4, seed=71)
    poses = _bend(rng, 16 * 64, angle=0.08).reshape(16, 64, 16)
    try:
        b = api.Batch(gpu_device, m, mats)
        b.set_poses(poses)
        b.close()  # straight after set_poses, no draw
        b = api.Batch(gpu_device, m, mats)
        b.set_poses(poses)
        fr = api.Frame(gpu_device, W, H)
        fr.draw_batch(b, vp)
        fr.submit()
        b.close()  # straight after a submit
        fr.wait()
        ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=mats, palettes=_ref_palettes(mf, poses))])
        assert_same((fr.color(), fr.depth(), fr.stats()), ref, "batch destroyed after submit")
        fr.close()
        # 1 000 updates (256 instances: 1 MiB of palettes per version) with a frame now and then: no growth
        big_mats = np.tile(mats, (16, 1))
        big = api.Batch(gpu_device, m, big_mats)
        host_poses = [_bend(rng, 256 * 64, angle=0.1).reshape(256, 64, 16) for _ in range(4)]
        dev_poses = [torch.tensor(p, device="cuda:0") for p in host_poses]

        def run(k0, count):
            for k in range(k0, k0 + count):
                if k % 2:
                    big.set_poses(dev_poses[k % 4])
                else:
                    big.set_poses(host_poses[k % 4])
                if k % 3 == 0:
                    big.update(model_mats=big_mats)
                if k % 10 == 0:
                    fr = api.Frame(gpu_device, W, H)
                    fr.draw_batch(big, vp)
                    fr.submit()
                    fr.close()
        run(0, 100)
        gpu_device.synchronize()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        run(100, 1000)
        gpu_device.synchronize()
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        assert free0 - free1 < 64 << 20, f"device memory grew by {(free0 - free1) >> 20} MiB over 1000 updates"
        big.close()
    finally:
        m.close()
