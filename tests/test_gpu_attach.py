"""GPU: attachments (SPEC.md section 18).  The matrices of k_attach (Batch.sockets, Batch.attach + read_model_mats) equal the
binary32 numpy model (tests/attach_model.py) bit for bit on every case of the generator, from host records and from device
records on the default and on a side stream, against a source whose write is still pending; the attached batch keeps its
palettes; a scene with attached cubes renders bit-exact against the oracle, unsharded through every tile path and bin
builder and as rank 1 of 2 with culling; frames in flight with the source destroyed before anyone waits; chains of
attachments and a batch attached to itself; invalid calls change nothing."""
import ctypes as C

import numpy as np
import pytest

from mt_renderer_amd import api, scene
from tests import anim_model as anm
from tests import attach_model as am
from tests.helpers import assert_same, render_oracle
from tests.test_gpu_anim import _bits_equal, _render, _small_md
from tests.test_gpu_anim_ik import _dev_targets, _ik64, _reach
from tests.test_gpu_anim_layers import _dev_layers, _setup, _stack

pytestmark = pytest.mark.gpu

CASES = am.cases()


def _dev_recs(recs, dtype="uint8"):
    import torch
    raw = np.ascontiguousarray(recs).view(np.uint8).reshape(recs.shape[0], -1)
    t = torch.from_numpy(raw.copy()).to("cuda:0")
    return t if dtype == "uint8" else t.view(torch.float32)


def _same(got, want, what):
    bad = ~am.same_bits(got, want)
    assert got.shape == want.shape and not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} matrix elements differ, first at {np.argwhere(bad)[0]}"


# ---- 1. the matrices, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_src,npal", [(s, p) for s in am.N_SRC for p in am.NPAL])
def test_matrices_are_bit_exact(gpu_device, n_src, npal):
    """every record count of the generator against one source: host records, device records on the default stream and on a
    side stream (written behind a long GPU operation and overwritten right after the call)"""
    import torch
    assert api.ATTACH == am.ATTACH
    m = api.Model.new(gpu_device, _small_md())
    cases = [c for c in CASES if c["n_src"] == n_src and c["npal"] == npal]
    src = tgt = None
    try:
        for k, c in enumerate(cases):
            n, recs = c["n"], c["recs"]
            want = am.attach(c["M_src"], c["P_src"], recs)
            if k % 2 == 0 or not npal:
                src = api.Batch(gpu_device, m, c["M_src"], c["P_src"])
            else:  # the palettes from mtr_batch_update: the source's current version is a later one of its ring
                src = api.Batch(gpu_device, m, c["M_src"], np.zeros_like(c["P_src"]))
                src.update(palettes=c["P_src"])
            _same(src.sockets(recs), want, f"{c['name']} sockets")
            rng = np.random.default_rng(n)
            keep = am.trs(rng, n * 3).reshape(n, 3, 16)
            tgt = api.Batch(gpu_device, m, am.trs(rng, n), keep)
            tgt.attach(src, recs)
            _same(tgt.read_model_mats(), want, f"{c['name']} host records")
            assert tgt.npal == 3 and _bits_equal(tgt.read_palettes(), keep), "the attached batch keeps its palettes"
            junk = recs.copy()
            junk["offset"] = np.nan
            for s in (torch.cuda.current_stream(), torch.cuda.Stream()):
                tgt.update(model_mats=np.zeros((n, 16), dtype=np.float32))
                good, bad = _dev_recs(recs, "float32" if k % 2 else "uint8"), _dev_recs(junk, "float32" if k % 2 else "uint8")
                t = bad.clone()
                torch.cuda.synchronize()
                with torch.cuda.stream(s):
                    if n == 257:
                        torch.cuda._sleep(2_000_000)
                    t.copy_(good)
                    tgt.attach(src, t, stream=s if k % 2 else None)  # None: torch's current stream, which is s
                    t.copy_(bad)
                got = tgt.read_model_mats()
                torch.cuda.synchronize()
                _same(got, want, f"{c['name']} device records on stream {s.cuda_stream:#x}")
            assert _bits_equal(tgt.read_palettes(), keep)
            tgt.close()
            src.close()
            src = tgt = None
    finally:
        for h in (tgt, src, m):
            if h:
                h.close()


def test_source_animated_on_the_device_with_its_write_pending(gpu_device):
    """the source's palettes come from mtr_batch_animate_ik_device on a side stream behind a long GPU operation: k_attach
    reads a version whose write has not run when the attach call returns"""
    import torch
    md, mf, m, rng, clips, masks = _setup(gpu_device, "uniform", rows=2, cols=3)
    anim = api.Anim(gpu_device, 64, clips)
    mk = api.AnimMasks(gpu_device, 64, masks)
    parents, chains, iks = _ik64(gpu_device)
    n_src, n = 7, 65
    mats = am.trs(rng, n_src)
    src = api.Batch(gpu_device, m, mats)
    cube = api.Model.new(gpu_device, scene.cube_model())
    tgt = api.Batch(gpu_device, cube, am.trs(rng, n))
    try:
        for rnd in range(2):
            ly = _stack(rng, n_src)
            tg, locals_ = _reach(rng, clips, ly, masks, parents, chains)
            pals = anm.palettes(mf, locals_)
            recs = am.records(rng, n, n_src, 64)
            want = am.attach(mats, pals, recs)
            dly, dtg, drec = _dev_layers(ly), _dev_targets(tg), _dev_recs(recs)
            side = torch.cuda.Stream()
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                torch.cuda._sleep(20_000_000)
                src.animate_ik(anim, dly, iks, dtg, mk)
            if rnd == 0:
                tgt.attach(src, recs)              # host records: the library's copy stream waits for the side stream's write
            else:
                tgt.attach(src, drec)              # device records on torch's default stream
            _same(tgt.read_model_mats(), want, f"round {rnd}")
            _same(src.sockets(recs), want, f"round {rnd} sockets")
            assert _bits_equal(src.read_palettes(), pals)
            torch.cuda.synchronize()
    finally:
        for h in (tgt, cube, src, iks, mk, anim, m):
            h.close()


# ---- 2. pixels ---------------------------------------------------------------------------------------------------------
def _cube_records(rng, n, n_src, position_only=()):
    """cubes of edge 0.12 placed around the capsule's surface in its bind space, each on a joint of some source instance"""
    r = np.zeros(n, dtype=api.ATTACH)
    r["src_instance"] = np.arange(n) % n_src
    r["joint"] = rng.integers(0, 64, size=n)
    for k in range(n):
        a = rng.uniform(0, 2 * np.pi)
        o = scene.mat_translate(0.42 * np.cos(a), rng.uniform(-0.7, 0.7), 0.42 * np.sin(a)) @ scene.mat_rot_y(a) @ scene.mat_scale(0.06, 0.06, 0.06)
        r["offset"][k] = scene.to_f32_colmajor(o)
        if k in position_only:
            r["flags"][k] = api.ATTACH_POSITION_ONLY
            r["offset"][k] = scene.to_f32_colmajor(scene.mat_scale(0.22, 0.22, 0.22))
    return r


def _scene(gpu_device):
    md, mf, m, rng, clips, masks = _setup(gpu_device, "uniform", rows=6, cols=10)
    return md, mf, m, rng, clips, scene.cube_model(debug_id=3)


def test_attached_cubes_render_like_the_oracle_unsharded_and_sharded(gpu_device):
    W, H = 160, 96
    md, mf, m, rng, clips, cmd = _scene(gpu_device)
    cube = api.Model.new(gpu_device, cmd)
    anim = api.Anim(gpu_device, 64, clips)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats = scene.instance_lattice(3, 2, seed=300)[0][:5]
    src = api.Batch(gpu_device, m, mats)
    cubes = api.Batch(gpu_device, cube, np.zeros((12, 16), dtype=np.float32))
    try:
        st = anm.random_states(rng, 5, api.ANIM_STATE)
        pals = anm.palettes(mf, anm.sample(clips, st, 64))
        recs = _cube_records(rng, 12, 5, position_only=(4, 9))
        cmats = am.attach(mats, pals, recs)
        src.animate(anim, st)
        cubes.attach(src, recs)
        _same(cubes.read_model_mats(), cmats, "cubes")
        both = [dict(md=md, vp=vp, model_mats=mats, palettes=pals), dict(md=cmd, vp=vp, model_mats=cmats)]
        ref = render_oracle(W, H, both)
        alone = render_oracle(W, H, both[:1])
        assert ref[2]["tris_setup"] > alone[2]["tris_setup"] + 12 and (ref[0] != alone[0]).any(), "the cubes are on screen"

        def draw(fr):
            fr.draw_batch(src, vp)
            fr.draw_batch(cubes, vp)
        for single_pass, mode in ((False, api.TILE_ORDERED), (True, api.TILE_ORDERED), (True, api.TILE_AUTO)):
            gpu_device.set_binning(single_pass)
            gpu_device.set_tile_mode(mode)
            assert_same(_render(gpu_device, W, H, draw), ref, f"single pass {single_pass}, tile mode {mode}")
        # rank 1 of 2, bands, culling on (the default for sharded frames): culling reads the attached matrices
        nby = (H + 15) // 16
        bands = np.round(np.linspace(0, nby, 3)).astype(np.uint32)

        def draw_sharded(fr):
            fr.set_shard(1, 2, api.OWN_BANDS, 0, bands)
            draw(fr)
        c, d, _ = _render(gpu_device, W, H, draw_sharded)
        y0, y1 = int(bands[1]) * 16, min(int(bands[2]) * 16, H)
        assert (ref[0][y0:y1] != alone[0][y0:y1]).any(), "a cube lies in the rank's band"
        assert (c[y0:y1] == ref[0][y0:y1]).all(), "rank 1 of 2: colour"
        assert _bits_equal(d[y0:y1], ref[1][y0:y1]), "rank 1 of 2: depth"
    finally:
        gpu_device.set_binning(True)
        gpu_device.set_tile_mode(api.TILE_AUTO)
        for h in (cubes, src, anim, cube, m):
            h.close()


# ---- 3. frames in flight, the source destroyed before anyone waits ---------------------------------------------------------
def test_frames_in_flight_and_the_source_destroyed_before_the_wait(gpu_device):
    import torch
    W, H = 160, 96
    md, mf, m, rng, clips, cmd = _scene(gpu_device)
    cube = api.Model.new(gpu_device, cmd)
    anim = api.Anim(gpu_device, 64, clips)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    cubes = api.Batch(gpu_device, cube, np.zeros((12, 16), dtype=np.float32))
    free = []
    try:
        for rnd in range(8):
            mats = scene.instance_lattice(3, 2, seed=500 + rnd)[0][:5]
            src = api.Batch(gpu_device, m, mats)
            frames, want = [], []
            for half in range(2):
                st = anm.random_states(rng, 5, api.ANIM_STATE)
                pals = anm.palettes(mf, anm.sample(clips, st, 64))
                recs = _cube_records(rng, 12, 5, position_only=(rnd % 12,))
                src.animate(anim, st)
                cubes.attach(src, _dev_recs(recs) if (rnd + half) % 2 else recs)
                fr = api.Frame(gpu_device, W, H)
                fr.draw_batch(src, vp)
                fr.draw_batch(cubes, vp)
                fr.submit()
                frames.append(fr)
                want.append([dict(md=md, vp=vp, model_mats=mats, palettes=pals), dict(md=cmd, vp=vp, model_mats=am.attach(mats, pals, recs))])
            src.close()  # before either frame has been waited for
            for half in (1, 0):
                fr = frames[half]
                fr.wait()
                assert_same((fr.color(), fr.depth(), fr.stats()), render_oracle(W, H, want[half]), f"round {rnd}, frame {'AB'[half]}")
                fr.close()
            gpu_device.synchronize()
            torch.cuda.synchronize()
            free.append(torch.cuda.mem_get_info()[0])
        assert free[2] - free[7] < 64 << 20, f"device memory grew by {(free[2] - free[7]) >> 20} MiB after round 2: {free}"
    finally:
        for h in (cubes, anim, cube, m):
            h.close()


# ---- 4. chains of attachments, and a batch attached to itself ----------------------------------------------------------------
@pytest.mark.parametrize("animate_first", [False, True])
def test_mount_rider_sword(gpu_device, animate_first):
    md, mf, m, rng, clips, masks = _setup(gpu_device, "uniform", rows=2, cols=3)
    anim = api.Anim(gpu_device, 64, clips)
    cube = api.Model.new(gpu_device, scene.cube_model())
    m_mats = am.trs(rng, 3)
    mount = api.Batch(gpu_device, m, m_mats)
    rider = api.Batch(gpu_device, m, am.trs(rng, 4))
    sword = api.Batch(gpu_device, cube, am.trs(rng, 6))
    try:
        st_m, st_r = anm.random_states(rng, 3, api.ANIM_STATE), anm.random_states(rng, 4, api.ANIM_STATE)
        p_m, p_r = anm.palettes(mf, anm.sample(clips, st_m, 64)), anm.palettes(mf, anm.sample(clips, st_r, 64))
        rec_r, rec_s = am.records(rng, 4, 3, 64), am.records(rng, 6, 4, 64)
        mount.animate(anim, st_m)
        if animate_first:
            rider.animate(anim, st_r)
            rider.attach(mount, rec_r)
        else:
            rider.attach(mount, _dev_recs(rec_r))
            rider.animate(anim, st_r)
        sword.attach(rider, rec_s)
        r_mats = am.attach(m_mats, p_m, rec_r)
        _same(rider.read_model_mats(), r_mats, "rider")
        assert rider.npal == 64 and _bits_equal(rider.read_palettes(), p_r), "the rider's own animation"
        _same(sword.read_model_mats(), am.attach(r_mats, p_r, rec_s), "sword")
    finally:
        for h in (sword, rider, mount, cube, anim, m):
            h.close()


def test_a_batch_attached_to_itself(gpu_device):
    md, mf, m, rng, clips, masks = _setup(gpu_device, "uniform", rows=2, cols=3)
    anim = api.Anim(gpu_device, 64, clips)
    mats = am.trs(rng, 5)
    b = api.Batch(gpu_device, m, mats)
    try:
        st = anm.random_states(rng, 5, api.ANIM_STATE)
        pals = anm.palettes(mf, anm.sample(clips, st, 64))
        b.animate(anim, st)
        recs = am.records(rng, 5, 5, 64)
        recs["src_instance"] = 0
        for step in range(3):  # each call reads the version the call before wrote
            b.attach(b, _dev_recs(recs) if step == 1 else recs)
            mats = am.attach(mats, pals, recs)
            _same(b.read_model_mats(), mats, f"step {step}")
            assert _bits_equal(b.read_palettes(), pals)
    finally:
        for h in (b, anim, m):
            h.close()


# ---- 5. invalid calls change nothing ----------------------------------------------------------------------------------------
def test_invalid_calls_change_nothing(gpu_device):
    import torch
    W, H = 160, 96
    md, mf, m, rng, clips, cmd = _scene(gpu_device)
    cube = api.Model.new(gpu_device, cmd)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats, pals = scene.instance_lattice(3, 2, seed=300)
    mats, pals = mats[:5], np.ascontiguousarray(pals[:5])
    src = api.Batch(gpu_device, m, mats, pals)
    cubes = api.Batch(gpu_device, cube, np.zeros((12, 16), dtype=np.float32))
    dev2 = api.Device(0)
    m2 = api.Model.new(dev2, cmd)
    other = api.Batch(dev2, m2, np.zeros((12, 16), dtype=np.float32))
    L = api.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    try:
        recs = _cube_records(rng, 12, 5, position_only=(2,))
        cubes.attach(src, recs)
        cmats = am.attach(mats, pals, recs)
        bad = _cube_records(rng, 12, 5)
        dbad, drecs = _dev_recs(bad), _dev_recs(recs)
        pad = torch.zeros(12 * 80 + 16, dtype=torch.uint8, device="cuda:0")
        out = np.full((12, 16), 7.0, dtype=np.float32)
        dout = torch.zeros(12 * 16 + 4, dtype=torch.float32, device="cuda:0")
        inv = api.MTR_E_INVALID
        assert L.mtr_batch_attach(None, src._h, p(bad)) == inv
        assert L.mtr_batch_attach(cubes._h, None, p(bad)) == inv
        assert L.mtr_batch_attach(cubes._h, src._h, None) == inv
        assert L.mtr_batch_attach(cubes._h, other._h, p(bad)) == inv          # another device
        assert L.mtr_batch_attach(other._h, src._h, p(bad)) == inv
        assert L.mtr_batch_attach_device(cubes._h, None, C.c_void_p(dbad.data_ptr()), None) == inv
        assert L.mtr_batch_attach_device(cubes._h, src._h, None, None) == inv
        assert L.mtr_batch_attach_device(cubes._h, src._h, C.c_void_p(pad.data_ptr() + 8), None) == inv
        assert L.mtr_batch_attach_device(cubes._h, other._h, C.c_void_p(dbad.data_ptr()), None) == inv
        assert L.mtr_batch_sockets(None, p(bad), 12, p(out), out.size) == inv
        assert L.mtr_batch_sockets(src._h, None, 12, p(out), out.size) == inv
        assert L.mtr_batch_sockets(src._h, p(bad), 12, None, out.size) == inv
        assert L.mtr_batch_sockets(src._h, p(bad), 0, p(out), out.size) == inv
        assert L.mtr_batch_sockets(src._h, p(bad), 12, p(out), out.size - 1) == inv
        assert L.mtr_batch_sockets_device(src._h, C.c_void_p(dbad.data_ptr()), 0, C.c_void_p(dout.data_ptr()), None) == inv
        assert L.mtr_batch_sockets_device(src._h, C.c_void_p(pad.data_ptr() + 8), 12, C.c_void_p(dout.data_ptr()), None) == inv
        assert L.mtr_batch_sockets_device(src._h, C.c_void_p(dbad.data_ptr()), 12, C.c_void_p(dout.data_ptr() + 4), None) == inv
        assert L.mtr_batch_sockets_device(src._h, C.c_void_p(dbad.data_ptr()), 12, None, None) == inv
        assert L.mtr_batch_read_model_mats(cubes._h, p(out), out.size - 1) == inv
        assert L.mtr_batch_read_model_mats(cubes._h, None, out.size) == inv
        assert L.mtr_batch_read_model_mats(None, p(out), out.size) == inv
        for fn in (lambda: cubes.attach(src, bad[:11]), lambda: cubes.attach(src, dbad[:11]), lambda: cubes.attach(src, np.zeros(12, dtype=api.ANIM_LAYER)),
                   lambda: cubes.attach(src, dict(joint=np.zeros(12))), lambda: src.sockets(np.zeros(0, dtype=api.ATTACH))):
            with pytest.raises(api.MtrError) as e:
                fn()
            assert e.value.code == inv
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (dout == 0).all().item(), "nothing was written"
        # the valid socket call on device memory, for contrast
        gpu_device.check(L.mtr_batch_sockets_device(src._h, C.c_void_p(drecs.data_ptr()), 12, C.c_void_p(dout.data_ptr()), None))
        gpu_device.synchronize()
        _same(dout[:192].cpu().numpy().reshape(12, 16), cmats, "sockets_device")
        _same(cubes.read_model_mats(), cmats, "after invalid calls")
        assert _bits_equal(src.read_model_mats(), mats) and _bits_equal(src.read_palettes(), pals)
        ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=mats, palettes=pals), dict(md=cmd, vp=vp, model_mats=cmats)])

        def draw(fr):
            fr.draw_batch(src, vp)
            fr.draw_batch(cubes, vp)
        assert_same(_render(gpu_device, W, H, draw), ref, "after invalid calls")
    finally:
        for h in (other, m2):
            h.close()
        dev2.close()
        for h in (cubes, src, cube, m):
            h.close()
