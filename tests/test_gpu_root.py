"""GPU: root motion (SPEC.md section 19).  The deltas of k_root (AnimRoot.deltas) and the matrices it leaves in a batch
(Batch.root_motion + read_model_mats) equal the binary32 numpy model (tests/root_model.py) bit for bit on every case of the
generator -- uniform keys and tracks, 1, 2 and 8 steps, 1, 5, 17 and 257 instances, host steps and device steps on a side
stream whose buffer is overwritten right after the call; calls accumulate; palettes and npal are kept; a draw recorded before
the call renders the old matrices and one after it the new ones, bit-exact against the oracle; a mount moved this way
carries its attached rider; the trajectory set and the root set are destroyed right after the call; invalid calls change
nothing."""
import ctypes as C

import numpy as np
import pytest

from mt_renderer_amd import api, scene
from tests import anim_model as anm
from tests import attach_model as am
from tests import root_model as rm
from tests.helpers import assert_same, render_oracle
from tests.test_gpu_anim import _bits_equal, _render, _small_md
from tests.test_gpu_anim_layers import _setup

pytestmark = pytest.mark.gpu

CASES = rm.cases()


def _dev_steps(st, dtype="uint8"):
    import torch
    raw = np.ascontiguousarray(st).view(np.uint8).reshape(st.shape[0], st.shape[1], 16)
    t = torch.from_numpy(raw.copy()).to("cuda:0")
    return t if dtype == "uint8" else t.view(torch.float32)


def _same(got, want, what):
    bad = ~rm.same_bits(got, want)
    assert got.shape == want.shape and not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} matrix elements differ, first at {np.argwhere(bad)[0]}"


def _make(dev, kind, J, traj):
    return api.Anim(dev, J, traj) if kind == "uniform" else api.AnimTracks(dev, J, traj)


def _walk(dev):
    traj = rm.walk_clip()
    return traj, (0, np.array([rm.CYCLIC], dtype=np.uint32)), api.Anim(dev, 1, traj), api.AnimRoot(dev, 1, 1, 0, [api.ROOT_CYCLIC])


def _walk_steps(rng, n, S=2):
    st = np.zeros((n, S), dtype=api.ROOT_STEP)
    st["x"] = rng.uniform(0.0, 30.0, size=(n, S))
    st["dx"] = rng.uniform(1.0, 6.0, size=(n, S))
    st["w"] = rng.uniform(0.0, 1.0, size=(n, S))
    return st


# ---- 1. the deltas and the matrices, bit for bit --------------------------------------------------------------------------
@pytest.mark.parametrize("kind,J,joint", rm.SETS)
def test_deltas_and_matrices_are_bit_exact(gpu_device, kind, J, joint):
    import torch
    assert api.ROOT_STEP == rm.STEP
    cases = [c for c in CASES if c["kind"] == kind and c["J"] == J]
    traj = _make(gpu_device, kind, J, cases[0]["traj"])
    root = api.AnimRoot(gpu_device, J, len(rm.LENGTHS), joint, rm.ROOT_FLAGS)
    plain = api.Model.new(gpu_device, scene.cube_model())  # no skeleton
    skinned = api.Model.new(gpu_device, _small_md())
    b = None
    nan_seen = False
    try:
        for k, c in enumerate(cases):
            n, st, M = c["n"], c["steps"], c["M"]
            want_d = rm.deltas(c["traj"], c["root"], st)
            want_m = rm.root_motion(M, c["traj"], c["root"], st)
            nan_seen |= bool(np.isnan(want_m).any())
            _same(root.deltas(traj, st), want_d, f"{c['name']} deltas")
            _same(root.deltas(traj, _dev_steps(st, "float32" if k % 2 else "uint8")).cpu().numpy(), want_d, f"{c['name']} deltas from device steps")
            keep = am.trs(np.random.default_rng(n), n * 64).reshape(n, 64, 16) if k % 2 else None
            b = api.Batch(gpu_device, skinned if k % 2 else plain, M, keep)
            b.root_motion(traj, root, st)
            _same(b.read_model_mats(), want_m, f"{c['name']} host steps")
            assert b.npal == (64 if k % 2 else 0)
            if k % 2:
                assert _bits_equal(b.read_palettes(), keep), "the batch keeps its palettes"
            junk = st.copy()
            junk["x"], junk["dx"], junk["clip"] = 3.0, 1.0, 5
            for s in (torch.cuda.current_stream(), torch.cuda.Stream()):
                b.update(model_mats=M)
                good, bad = _dev_steps(st), _dev_steps(junk)
                t = bad.clone()
                torch.cuda.synchronize()
                with torch.cuda.stream(s):
                    if n == 257:
                        torch.cuda._sleep(2_000_000)
                    t.copy_(good)
                    b.root_motion_device(traj, root, t, stream=s if k % 2 else None)
                    t.copy_(bad)
                got = b.read_model_mats()
                torch.cuda.synchronize()
                _same(got, want_m, f"{c['name']} device steps on stream {s.cuda_stream:#x}")
            if k % 2:
                assert _bits_equal(b.read_palettes(), keep)
            b.close()
            b = None
        assert nan_seen, "the special steps reach the comparison"
    finally:
        for h in (b, skinned, plain, root, traj):
            if h:
                h.close()


def test_three_calls_accumulate(gpu_device):
    c = next(c for c in CASES if c["name"] == "tracks_J3_n17_S2")
    traj = _make(gpu_device, c["kind"], c["J"], c["traj"])
    root = api.AnimRoot(gpu_device, c["J"], len(rm.LENGTHS), c["root"][0], rm.ROOT_FLAGS)
    m = api.Model.new(gpu_device, scene.cube_model())
    b = api.Batch(gpu_device, m, c["M"])
    try:
        mats, rng = c["M"], np.random.default_rng(3)
        for call in range(3):  # each call reads the version the call before wrote
            st = rm.make_steps(rng, c["n"], c["S"], off=call)
            finite = ~np.isnan(rm.deltas(c["traj"], c["root"], st)).any(axis=1)
            st[~finite] = st[np.argmax(finite)]
            if call == 1:
                b.root_motion_device(traj, root, _dev_steps(st))
            else:
                b.root_motion(traj, root, st)
            mats = rm.root_motion(mats, c["traj"], c["root"], st)
            _same(b.read_model_mats(), mats, f"call {call}")
        assert np.isfinite(mats).all()
    finally:
        for h in (b, m, root, traj):
            h.close()


# ---- 2. pixels: a draw uses what was current when it was recorded ----------------------------------------------------------
def test_draws_before_and_after_the_call_render_like_the_oracle(gpu_device):
    W, H = 160, 96
    md, mf, m, rng, clips, masks = _setup(gpu_device, "uniform", rows=6, cols=10)
    tr, rt, traj, root = _walk(gpu_device)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats, pals = scene.instance_lattice(3, 2, seed=300)
    mats, pals = mats[:5], np.ascontiguousarray(pals[:5])
    b = api.Batch(gpu_device, m, mats, pals)
    try:
        st = _walk_steps(rng, 5)
        new = rm.root_motion(mats, tr, rt, st)
        before = api.Frame(gpu_device, W, H)
        before.draw_batch(b, vp)
        b.root_motion(traj, root, st)
        before.end()
        old_ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=mats, palettes=pals)])
        new_ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=new, palettes=pals)])
        assert (old_ref[0] != new_ref[0]).any() and new_ref[2]["tris_setup"] > 0, "the instances moved, on screen"
        assert_same((before.color(), before.depth(), before.stats()), old_ref, "the draw recorded before the call")
        before.close()
        assert_same(_render(gpu_device, W, H, lambda fr: fr.draw_batch(b, vp)), new_ref, "the draw recorded after the call")
        _same(b.read_model_mats(), new, "matrices")
        assert _bits_equal(b.read_palettes(), pals)
    finally:
        for h in (b, root, traj, m):
            h.close()


# ---- 3. a mount moved by root motion carries its rider ------------------------------------------------------------------------
def test_mount_moves_and_carries_its_rider(gpu_device):
    md, mf, m, rng, clips, masks = _setup(gpu_device, "uniform", rows=2, cols=3)
    anim = api.Anim(gpu_device, 64, clips)
    tr, rt, traj, root = _walk(gpu_device)
    m_mats = am.trs(rng, 3)
    mount = api.Batch(gpu_device, m, m_mats)
    rider = api.Batch(gpu_device, m, am.trs(rng, 4))
    try:
        st_m = anm.random_states(rng, 3, api.ANIM_STATE)
        p_m = anm.palettes(mf, anm.sample(clips, st_m, 64))
        mount.animate(anim, st_m)
        st = _walk_steps(rng, 3)
        mount.root_motion_device(traj, root, _dev_steps(st))
        recs = am.records(rng, 4, 3, 64)
        rider.attach(mount, recs)
        moved = rm.root_motion(m_mats, tr, rt, st)
        _same(mount.read_model_mats(), moved, "mount")
        assert mount.npal == 64 and _bits_equal(mount.read_palettes(), p_m), "the mount's own animation"
        _same(rider.read_model_mats(), am.attach(moved, p_m, recs), "rider = M_new . palette_j . O")
    finally:
        for h in (rider, mount, root, traj, anim, m):
            h.close()


# ---- 4. the sets destroyed right after the call, no host wait -----------------------------------------------------------------
def test_sets_destroyed_right_after_the_call(gpu_device):
    import torch
    c = next(c for c in CASES if c["name"] == "uniform_J3_n257_S8")
    m = api.Model.new(gpu_device, scene.cube_model())
    b = api.Batch(gpu_device, m, c["M"])
    try:
        want = rm.root_motion(c["M"], c["traj"], c["root"], c["steps"])
        for rnd in range(3):
            b.update(model_mats=c["M"])
            traj = _make(gpu_device, c["kind"], c["J"], c["traj"])
            root = api.AnimRoot(gpu_device, c["J"], len(rm.LENGTHS), c["root"][0], rm.ROOT_FLAGS)
            t = _dev_steps(c["steps"])
            side = torch.cuda.Stream()
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                torch.cuda._sleep(20_000_000)
                b.root_motion_device(traj, root, t)
                d = root.deltas(traj, t)
            traj.close()
            root.close()
            _same(b.read_model_mats(), want, f"round {rnd}")
            torch.cuda.synchronize()
            _same(d.cpu().numpy(), rm.deltas(c["traj"], c["root"], c["steps"]), f"round {rnd} deltas")
    finally:
        for h in (b, m):
            h.close()


# ---- 5. invalid calls change nothing ----------------------------------------------------------------------------------------
def test_invalid_calls_change_nothing(gpu_device):
    import torch
    tr, rt, traj, root = _walk(gpu_device)
    rng = np.random.default_rng(9)
    m = api.Model.new(gpu_device, scene.cube_model())
    mats = am.trs(rng, 6)
    b = api.Batch(gpu_device, m, mats)
    loop = api.Anim(gpu_device, 1, [(tr[0][0], api.CLIP_LOOP)])
    two = api.Anim(gpu_device, 1, [tr[0], tr[0]])
    dev2 = api.Device(0)
    root2 = api.AnimRoot(dev2, 1, 1)
    L = api.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    try:
        st = _walk_steps(rng, 6)
        dst = _dev_steps(st)
        pad = torch.zeros(6 * 32 + 16, dtype=torch.uint8, device="cuda:0")
        out = np.full((6, 16), 7.0, dtype=np.float32)
        dout = torch.zeros(6 * 16 + 4, dtype=torch.float32, device="cuda:0")
        inv, h = api.MTR_E_INVALID, C.c_void_p()
        fl = np.array([2], dtype=np.uint32)
        assert L.mtr_anim_root_create(gpu_device._h, 1, 1, 1, None, C.byref(h)) == inv and not h          # joint >= njoints
        assert L.mtr_anim_root_create(gpu_device._h, 1, 1, 0, p(fl), C.byref(h)) == inv and not h         # unknown flag bits
        assert b"clip 0" in L.mtr_last_error(gpu_device._h)
        assert L.mtr_anim_root_create(gpu_device._h, 1, 1, 0, None, None) == inv
        assert L.mtr_batch_root_motion(None, traj._h, root._h, p(st), 2) == inv
        assert L.mtr_batch_root_motion(b._h, None, root._h, p(st), 2) == inv
        assert L.mtr_batch_root_motion(b._h, traj._h, None, p(st), 2) == inv
        assert L.mtr_batch_root_motion(b._h, traj._h, root._h, None, 2) == inv
        assert L.mtr_batch_root_motion(b._h, traj._h, root._h, p(st), 0) == inv
        assert L.mtr_batch_root_motion(b._h, traj._h, root._h, p(st), 9) == inv
        assert L.mtr_batch_root_motion(b._h, loop._h, root._h, p(st), 2) == inv                        # a LOOP clip
        assert L.mtr_batch_root_motion(b._h, two._h, root._h, p(st), 2) == inv                         # another clip count
        assert L.mtr_batch_root_motion(b._h, traj._h, root2._h, p(st), 2) == inv                       # another device
        assert L.mtr_batch_root_motion_device(b._h, traj._h, root._h, None, 2, None) == inv
        assert L.mtr_batch_root_motion_device(b._h, traj._h, root._h, C.c_void_p(pad.data_ptr() + 8), 2, None) == inv
        assert L.mtr_batch_root_motion_device(b._h, loop._h, root._h, C.c_void_p(dst.data_ptr()), 2, None) == inv
        assert L.mtr_anim_root_deltas(traj._h, root._h, p(st), 2, 0, p(out), out.size) == inv
        assert L.mtr_anim_root_deltas(traj._h, root._h, p(st), 2, 6, p(out), out.size - 1) == inv
        assert L.mtr_anim_root_deltas(traj._h, root._h, p(st), 2, 6, None, out.size) == inv
        assert L.mtr_anim_root_deltas(traj._h, root._h, None, 2, 6, p(out), out.size) == inv
        assert L.mtr_anim_root_deltas(traj._h, root._h, p(st), 2, (1 << 27) + 1, p(out), 1 << 40) == inv
        assert L.mtr_anim_root_deltas(loop._h, root._h, p(st), 2, 6, p(out), out.size) == inv
        assert L.mtr_anim_root_deltas_device(traj._h, root._h, C.c_void_p(dst.data_ptr()), 2, 6, C.c_void_p(dout.data_ptr() + 4), None) == inv
        assert L.mtr_anim_root_deltas_device(traj._h, root._h, C.c_void_p(pad.data_ptr() + 8), 2, 6, C.c_void_p(dout.data_ptr()), None) == inv
        assert L.mtr_anim_root_deltas_device(traj._h, root._h, C.c_void_p(dst.data_ptr()), 9, 6, C.c_void_p(dout.data_ptr()), None) == inv
        for fn in (lambda: b.root_motion(traj, root, st[:5]), lambda: b.root_motion_device(traj, root, dst[:5]),
                   lambda: b.root_motion(traj, root, np.zeros(6, dtype=api.ANIM_LAYER)), lambda: api.AnimRoot(gpu_device, 1, 1, 0, [1, 1])):
            with pytest.raises(api.MtrError) as e:
                fn()
            assert e.value.code == inv
        torch.cuda.synchronize()
        assert (out == 7.0).all() and (dout == 0).all().item(), "nothing was written"
        assert _bits_equal(b.read_model_mats(), mats), "nothing moved"
        # the valid calls, for contrast
        gpu_device.check(L.mtr_anim_root_deltas_device(traj._h, root._h, C.c_void_p(dst.data_ptr()), 2, 6, C.c_void_p(dout.data_ptr()), None))
        gpu_device.synchronize()
        _same(dout[:96].cpu().numpy().reshape(6, 16), rm.deltas(tr, rt, st), "deltas_device")
        b.root_motion(traj, root, st)
        _same(b.read_model_mats(), rm.root_motion(mats, tr, rt, st), "after invalid calls")
    finally:
        root2.close()
        dev2.close()
        for h in (b, m, two, loop, root, traj):
            h.close()
