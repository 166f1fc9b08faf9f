"""GPU: inverse kinematics after the layer stack (SPEC.md section 17).  The local matrices of the k_anim_ik kernels equal
the binary32 numpy model (tests/anim_ik_model.py) bit for bit on both kinds of animation set; with every weight 0 they are
section 16's; the palettes equal mtr_rmodel_palette over the model's local matrices bit for bit (host targets, device
targets on the default and on a side stream); a batch and a model render bit-exact against the oracle; one batch is
animated by every kind of pose call with frames in flight while IK sets come and go; invalid calls change nothing; no memory
growth."""
import ctypes as C
import functools

import numpy as np
import pytest

from mt_renderer_amd import anim_tracks, api, scene
from tests import anim_ik_model as ik
from tests import anim_layers_model as lm
from tests import anim_model as am
from tests import anim_tracks_model as tm
from tests.helpers import assert_same, render_oracle
from tests.test_gpu_anim import CHAIN64, _bits_equal, _model_file, _render, _small_md, _trs
from tests.test_gpu_anim_layers import KINDS, _dev_layers, _inputs, _layers, _lpals, _make, _setup, _stack

pytestmark = pytest.mark.gpu


def _dev_targets(tg, dtype="uint8"):
    import torch
    raw = np.ascontiguousarray(tg).view(np.uint8).reshape(tg.shape[0], -1)
    t = torch.from_numpy(raw.copy()).to("cuda:0")
    return t if dtype == "uint8" else t.view(torch.float32)


@functools.lru_cache(maxsize=None)
def _case(kind, J, K, L):
    """layers, parents, chains, targets, the stack's (T, Q, S) and the model's locals of one case; nobody writes into them"""
    clips, masks = _inputs(kind, J)
    ly = _layers(kind, J, L)
    parents = ik.skeleton(J)
    chains = ik.default_chains(parents, K).astype(api.ANIM_IK_CHAIN)
    tqs = ik.stack_tqs(clips, ly, J, masks)
    tg = ik.make_targets(np.random.default_rng(J * 10 + K), tqs, parents, chains, dtype=api.ANIM_IK_TARGET)
    probe = []
    ref = ik.sample(clips, ly, J, masks, parents, chains, tg, tqs=tqs, probe=probe)
    return ly, parents, chains, tg, tqs, ref, probe


# ---- 1. the local matrices, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("J,K,L", [(J, K, L) for J in (3, 64, 65, 256) for K in (1, 4) for L in (1, 3)])
def test_sampled_locals_are_bit_exact(gpu_device, kind, J, K, L):
    """J = 3: the chain is the whole skeleton, a is a root, its path has one joint.  J = 65: the chains (62, 63, 64) and
    (61, 62, 63) and the aims at 62 and 64 straddle the wave boundary.  J = 256: the chain hangs at depth 210."""
    assert api.ANIM_IK_CHAIN == ik.CHAIN and api.ANIM_IK_TARGET == ik.TARGET
    clips, masks = _inputs(kind, J)
    ly, parents, chains, tg, tqs, ref, probe = _case(kind, J, K, L)
    assert np.isfinite(ref).all() and all(p["hit"].sum() > 100 for p in probe), "most instances are solved"
    if J == 256:
        assert len(ik.paths_of(parents)[int(chains["joint"][0, 0])]) >= 200
    anim = _make(gpu_device, kind, J, clips)
    mk = api.AnimMasks(gpu_device, J, masks)
    iks = api.AnimIK(gpu_device, parents, chains)
    try:
        got = anim.sample_ik(ly, iks, tg, mk)
        assert got.shape == (ly.shape[0], J, 16)
        bad = got.view(np.uint32) != ref.view(np.uint32)
        assert not bad.any(), f"{int(bad.sum())} of {ref.size} local matrix elements differ, first at {np.argwhere(bad)[0]}"
        assert not _bits_equal(got, lm.sample(clips, ly, J, masks)), "the chains show"
    finally:
        iks.close()
        mk.close()
        anim.close()


# ---- 2. every weight 0: section 16 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("J", [3, 65])
def test_all_weights_zero_is_the_layer_stack(gpu_device, kind, J):
    clips, masks = _inputs(kind, J)
    ly, parents, chains, tg, _, _, _ = _case(kind, J, 4, 3)
    tg = tg.copy()
    tg["w"] = np.random.default_rng(5).choice(np.array([0.0, -0.0, -3.0, np.nan, -np.inf], dtype=np.float32), tg["w"].shape)
    tg["pos"][::2] = np.nan  # not read
    anim = _make(gpu_device, kind, J, clips)
    mk = api.AnimMasks(gpu_device, J, masks)
    iks = api.AnimIK(gpu_device, parents, chains)
    try:
        want = anim.sample_layers(ly, mk)
        assert _bits_equal(want, lm.sample(clips, ly, J, masks))
        assert _bits_equal(anim.sample_ik(ly, iks, tg, mk), want)
    finally:
        iks.close()
        mk.close()
        anim.close()


# ---- 3. the palettes, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("J", [64, 256])
def test_palettes_are_bit_exact_host_and_device_targets(gpu_device, kind, J):
    import torch
    n, L, K = 64, 3, 4
    parents = ik.skeleton(J)
    rng = np.random.default_rng(J * 7 + 5)
    imats = _trs(rng, J, scale=(0.5, 2.0), trans=20.0)
    mf = _model_file([int(p) for p in parents], imats)
    clips, masks = _inputs(kind, J)
    chains = ik.default_chains(parents, K).astype(api.ANIM_IK_CHAIN)
    m = api.Model.new(gpu_device, _small_md())
    anim = mk = iks = b = None
    try:
        m.set_skeleton([int(p) for p in parents], imats)
        anim = _make(gpu_device, kind, J, clips)
        mk = api.AnimMasks(gpu_device, J, masks)
        iks = api.AnimIK(gpu_device, parents, chains)
        b = api.Batch(gpu_device, m, np.tile(np.eye(4, dtype=np.float32).reshape(16), (n, 1)))
        zero = np.zeros((n, J, 16), dtype=np.float32)

        def fresh():
            ly = lm.layer_states(rng, clips, n=n, L=L, dtype=api.ANIM_LAYER)
            tqs = ik.stack_tqs(clips, ly, J, masks)
            tg = ik.make_targets(rng, tqs, parents, chains, dtype=api.ANIM_IK_TARGET)
            ref = am.palettes(mf, ik.sample(clips, ly, J, masks, parents, chains, tg, tqs=tqs))
            assert np.isfinite(ref).all()
            return ly, tg, ref

        def check(what, animate):
            ly, tg, ref = fresh()
            b.update(palettes=zero)
            animate(ly, tg)
            got = b.read_palettes()
            assert got.shape == (n, J, 16)
            assert _bits_equal(got, ref), f"{what}: {int((got.view(np.uint32) != ref.view(np.uint32)).sum())} of {ref.size} palette elements differ"

        check("host targets", lambda ly, tg: b.animate_ik(anim, ly, iks, tg, mk))
        check("device targets, host layers", lambda ly, tg: b.animate_ik(anim, ly, iks, _dev_targets(tg, "float32"), mk))

        # device targets written behind a long GPU op and overwritten right after the call, on the default and on a side stream
        for s in (torch.cuda.current_stream(), torch.cuda.Stream()):
            ly, tg, ref = fresh()
            wrong = tg.copy()
            wrong["pos"] = np.nan
            wrong["w"] = 1.0
            src, bad, dly = _dev_targets(tg), _dev_targets(wrong), _dev_layers(ly)
            t = bad.clone()
            b.update(palettes=zero)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                torch.cuda._sleep(20_000_000)
                t.copy_(src)
                b.animate_ik(anim, dly, iks, t, mk)
                t.copy_(bad)
            got = b.read_palettes()
            torch.cuda.synchronize()
            assert _bits_equal(got, ref), f"device targets on stream {s.cuda_stream:#x}"
    finally:
        for h in (b, iks, mk, anim):
            if h:
                h.close()
        m.close()


# ---- 4. rendering ------------------------------------------------------------------------------------------------------
def _ik64(dev, K=4):
    parents = ik.skeleton(64)
    assert [int(p) for p in parents] == CHAIN64
    chains = ik.default_chains(parents, K).astype(api.ANIM_IK_CHAIN)
    return parents, chains, api.AnimIK(dev, parents, chains)


def _reach(rng, clips, ly, masks, parents, chains):
    """targets for the stacks and the model's local matrices"""
    tqs = ik.stack_tqs(clips, ly, 64, masks)
    tg = ik.make_targets(rng, tqs, parents, chains, dtype=api.ANIM_IK_TARGET)
    return tg, ik.sample(clips, ly, 64, masks, parents, chains, tg, tqs=tqs)


@pytest.mark.parametrize("kind", KINDS)
def test_batch_and_model_animated_with_ik_render_like_the_oracle(gpu_device, kind):
    W, H = 192, 112
    md, mf, m, rng, clips, masks = _setup(gpu_device, kind)
    anim = _make(gpu_device, kind, 64, clips)
    mk = api.AnimMasks(gpu_device, 64, masks)
    parents, chains, iks = _ik64(gpu_device)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats, _ = scene.instance_lattice(4, 4, seed=300)
    b = api.Batch(gpu_device, m, mats)
    try:
        ly = _stack(rng, 16)
        tg, locals_ = _reach(rng, clips, ly, masks, parents, chains)
        pals = am.palettes(mf, locals_)
        assert not _bits_equal(pals, _lpals(mf, clips, ly, masks)), "the chains show"
        b.animate_ik(anim, _dev_layers(ly) if kind == "tracks" else ly, iks, tg, mk)
        assert _bits_equal(b.read_palettes(), pals)
        ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=mats, palettes=pals)])
        M = scene.to_f32_colmajor(scene.headline_transform(W, H))
        m.animate_ik(anim, ly[3], iks, tg[3], mk)
        mref = render_oracle(W, H, [dict(md=md, M=M, palette=pals[3])])
        for mode in (api.TILE_ORDERED, api.TILE_AUTO):
            gpu_device.set_tile_mode(mode)
            assert_same(_render(gpu_device, W, H, lambda fr: fr.draw_batch(b, vp)), ref, f"{kind} batch, tile mode {mode}")
            assert_same(_render(gpu_device, W, H, lambda fr: m.render(fr, M)), mref, f"{kind} model, tile mode {mode}")
    finally:
        gpu_device.set_tile_mode(api.TILE_AUTO)
        b.close()
        iks.close()
        mk.close()
        anim.close()
        m.close()


# ---- 5. frames in flight ------------------------------------------------------------------------------------------------
def test_frames_in_flight_from_every_kind_of_pose_call(gpu_device):
    W, H = 160, 96
    md, mf, m, rng, clips, masks = _setup(gpu_device, "uniform", rows=6, cols=10)
    tclips = [anim_tracks.compress(k, fl, tol_t=2e-3, tol_q=2e-3, tol_s=2e-3) for k, fl in clips]
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    sets = [api.Anim(gpu_device, 64, clips), api.AnimTracks(gpu_device, 64, tclips)]
    src = [clips, tclips]
    mk = api.AnimMasks(gpu_device, 64, masks)
    parents, chains, iks = _ik64(gpu_device)
    b = api.Batch(gpu_device, m, scene.instance_lattice(4, 4)[0])
    frames, want = [], []
    try:
        for k in range(12):
            mats, _ = scene.instance_lattice(4, 4, seed=900 + k)
            ly = _stack(rng, 16)
            st = am.random_states(rng, 16, api.ANIM_STATE)
            tmp = None
            which = k % 4
            if which == 0:    # IK over the uniform or the track set; in frame 4 through an IK set destroyed after the submit
                s = (k // 4) % 2
                if k == 4:
                    tmp = api.AnimIK(gpu_device, parents, chains)
                tg, locals_ = _reach(rng, src[s], ly, masks, parents, chains)
                b.animate_ik(sets[s], ly, tmp or iks, _dev_targets(tg) if k == 8 else tg, mk)
            elif which == 1:  # layers
                b.animate_layers(sets[1], ly, mk)
                locals_ = lm.sample(tclips, ly, 64, masks)
            elif which == 2:  # plain states
                b.animate(sets[0], st)
                locals_ = am.sample(clips, st, 64)
            else:             # poses from the host
                locals_ = tm.sample(tclips, st, 64)
                b.set_poses(locals_)
            b.update(model_mats=mats)
            fr = api.Frame(gpu_device, W, H)
            fr.draw_batch(b, vp)
            fr.submit()
            if tmp:
                tmp.close()
            frames.append(fr)
            want.append((mats, locals_))
        for k in reversed(range(12)):
            fr = frames[k]
            fr.wait()
            if k in (0, 1, 3, 4, 6, 8):
                mats, locals_ = want[k]
                ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=mats, palettes=am.palettes(mf, locals_))])
                assert_same((fr.color(), fr.depth(), fr.stats()), ref, f"frame {k}")
    finally:
        for fr in frames:
            fr.close()
        b.close()
        iks.close()
        mk.close()
        for a in sets:
            a.close()
        m.close()


# ---- 6. invalid calls change nothing --------------------------------------------------------------------------------------
def test_invalid_calls_change_nothing(gpu_device):
    import torch
    W, H = 160, 96
    md, mf, m, rng, clips, masks = _setup(gpu_device, "uniform", rows=6, cols=10)
    bare = api.Model.new(gpu_device, md)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats, _ = scene.instance_lattice(4, 4, seed=81)
    anim = api.Anim(gpu_device, 64, clips)
    mk = api.AnimMasks(gpu_device, 64, masks)
    parents, chains, iks = _ik64(gpu_device)
    ly, other = _stack(rng, 16), _stack(rng, 16)
    tg, locals_ = _reach(rng, clips, ly, masks, parents, chains)
    otg, _ = _reach(rng, clips, other, masks, parents, chains)
    pals = am.palettes(mf, locals_)
    b = api.Batch(gpu_device, m, mats)
    bb = api.Batch(gpu_device, bare, mats)
    anim63 = api.Anim(gpu_device, 63, am.gentle_clips(rng, 63))
    ik63 = api.AnimIK(gpu_device, ik.skeleton(63), ik.default_chains(ik.skeleton(63), 4).astype(api.ANIM_IK_CHAIN))
    tree = parents.copy()
    tree[40] = 7  # joint 40 hangs elsewhere: not the model's skeleton (the chains sit at 60..63 and stay valid)
    ik_tree = api.AnimIK(gpu_device, tree, chains)
    ik1 = api.AnimIK(gpu_device, parents, chains[:1])
    dev2 = api.Device(0)
    ik_dev2 = api.AnimIK(dev2, parents, chains)
    closed = api.AnimIK(gpu_device, parents, chains)
    closed.close()
    L = api.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    try:
        def invalid(fn):
            with pytest.raises(api.MtrError) as e:
                fn()
            assert e.value.code == api.MTR_E_INVALID
            return str(e.value)

        def rc_invalid(rc):
            assert rc == api.MTR_E_INVALID
        b.animate_ik(anim, ly, iks, tg, mk)
        m.animate_ik(anim, ly[:1], iks, tg[:1], mk)
        dly, dtg = _dev_layers(other), _dev_targets(otg)
        for bad_ik in (ik63, ik_tree, ik_dev2, closed):
            invalid(lambda: b.animate_ik(anim, other, bad_ik, otg[:, :bad_ik.nchains], mk))
            invalid(lambda: b.animate_ik(anim, dly, bad_ik, dtg, mk))
            invalid(lambda: m.animate_ik(anim, other[:1], bad_ik, otg[:1], mk))
        assert "joint 40" in invalid(lambda: b.animate_ik(anim, other, ik_tree, otg, mk))
        invalid(lambda: b.animate_ik(anim63, other, iks, otg, mk))          # what the layered calls reject
        invalid(lambda: bare.animate_ik(anim, other[:1], iks, otg[:1], mk))
        invalid(lambda: bb.animate_ik(anim, other, iks, otg, None))
        invalid(lambda: b.animate_ik(anim, np.zeros((16, 9), dtype=api.ANIM_LAYER), iks, otg, mk))
        invalid(lambda: b.animate_ik(anim, other, ik1, otg, mk))            # 4 targets per instance for a set of 1 chain
        rc_invalid(L.mtr_batch_animate_ik(b._h, anim._h, mk._h, p(other), 3, None, p(otg)))
        rc_invalid(L.mtr_batch_animate_ik(b._h, anim._h, mk._h, p(other), 3, iks._h, None))
        rc_invalid(L.mtr_batch_animate_ik(b._h, anim._h, mk._h, None, 3, iks._h, p(otg)))
        rc_invalid(L.mtr_batch_animate_ik(None, anim._h, mk._h, p(other), 3, iks._h, p(otg)))
        rc_invalid(L.mtr_model_animate_ik(m._h, anim._h, mk._h, p(other), 3, iks._h, None))
        rc_invalid(L.mtr_model_animate_ik(m._h, anim._h, mk._h, p(other), 3, None, p(otg)))
        rc_invalid(L.mtr_batch_animate_ik_device(b._h, anim._h, mk._h, C.c_void_p(dly.data_ptr()), 3, iks._h, None, None))
        pad = torch.zeros(16 * 128 + 16, dtype=torch.uint8, device="cuda:0")
        pad[8:8 + 16 * 128] = dtg.reshape(-1)
        assert (pad.data_ptr() + 8) % 16 == 8
        rc_invalid(L.mtr_batch_animate_ik_device(b._h, anim._h, mk._h, C.c_void_p(dly.data_ptr()), 3, iks._h, C.c_void_p(pad.data_ptr() + 8), None))
        out = np.zeros((16, 64, 16), dtype=np.float32)
        rc_invalid(L.mtr_anim_sample_ik(anim._h, mk._h, ik63._h, p(other), 3, p(otg), 16, p(out), out.size))
        rc_invalid(L.mtr_anim_sample_ik(anim._h, mk._h, None, p(other), 3, p(otg), 16, p(out), out.size))
        rc_invalid(L.mtr_anim_sample_ik(anim._h, mk._h, iks._h, p(other), 3, None, 16, p(out), out.size))
        rc_invalid(L.mtr_anim_sample_ik(anim._h, mk._h, iks._h, p(other), 3, p(otg), 16, p(out), out.size - 1))

        # creation: every rule of section 17, and the chain is named
        def chain(**kw):
            c = chains[:2].copy()
            for k, v in kw.items():
                c[k][1] = v
            return c
        for bad, word in ((chain(kind=2), "kind"), (chain(flags=2), "flag"), (chain(joint=(64, 0, 0)), "joint"),
                          (chain(axis=(0, 0, 0)), "axis"), (chain(axis=(np.nan, 1, 0)), "axis"), (chain(axis=(np.inf, 1, 0)), "axis"),
                          (chain(kind=0, joint=(61, 62, 62)), "twice"), (chain(kind=0, joint=(60, 62, 63)), "child"),
                          (chain(kind=0, joint=(61, 63, 62)), "child"), (chain(kind=0, joint=(62, 63, 64)), "joint")):
            msg = invalid(lambda: api.AnimIK(gpu_device, parents, bad))
            assert "chain 1" in msg and word in msg, msg
        two_roots = parents.copy()
        two_roots[63] = 255
        assert "root" in invalid(lambda: api.AnimIK(gpu_device, two_roots, chains[:1]))
        invalid(lambda: api.AnimIK(gpu_device, parents, np.zeros(0, dtype=api.ANIM_IK_CHAIN)))
        invalid(lambda: api.AnimIK(gpu_device, parents, np.concatenate([chains, chains[:1]])))
        cyc = parents.copy()
        cyc[0] = 5
        invalid(lambda: api.AnimIK(gpu_device, cyc, chains))
        h = C.c_void_p(1)
        rc_invalid(L.mtr_anim_ik_create(gpu_device._h, 64, None, 4, p(chains), C.byref(h)))
        assert not h.value
        rc_invalid(L.mtr_anim_ik_create(gpu_device._h, 257, p(parents), 4, p(chains), C.byref(h)))
        # nothing changed: the batch and the model still render what the last valid calls set
        assert _bits_equal(b.read_palettes(), pals)
        ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=mats, palettes=pals)])
        assert_same(_render(gpu_device, W, H, lambda fr: fr.draw_batch(b, vp)), ref, "batch after invalid calls")
        M = scene.to_f32_colmajor(scene.headline_transform(W, H))
        ref = render_oracle(W, H, [dict(md=md, M=M, palette=pals[0])])
        assert_same(_render(gpu_device, W, H, lambda fr: m.render(fr, M)), ref, "model after invalid calls")
    finally:
        for h in (b, bb, anim63, ik63, ik_tree, ik1, ik_dev2):
            h.close()
        dev2.close()
        for h in (iks, mk, anim, bare, m):
            h.close()


# ---- 7. no growth ------------------------------------------------------------------------------------------------------
def test_no_memory_growth_over_mixed_calls(gpu_device):
    import torch
    W, H = 160, 96
    md, mf, m, rng, clips, masks = _setup(gpu_device, "uniform", rows=6, cols=10)
    tclips = [anim_tracks.compress(k, fl, tol_t=2e-3, tol_q=2e-3, tol_s=2e-3) for k, fl in clips]
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats = np.tile(scene.instance_lattice(4, 4, seed=71)[0], (16, 1))
    sets = [api.Anim(gpu_device, 64, clips), api.AnimTracks(gpu_device, 64, tclips)]
    mk = api.AnimMasks(gpu_device, 64, masks)
    parents, chains, iks = _ik64(gpu_device)
    big = api.Batch(gpu_device, m, mats)
    host = [_stack(rng, 256) for _ in range(4)]
    devs = [_dev_layers(s) for s in host]
    tgs = [_reach(rng, tclips, s, masks, parents, chains)[0] for s in host]
    dtgs = [_dev_targets(t) for t in tgs]
    states = am.random_states(rng, 256, api.ANIM_STATE)
    poses = am.sample(clips, states, 64)
    try:
        def run(k0, count):
            for k in range(k0, k0 + count):
                if k % 5 == 3:
                    big.animate(sets[k % 2], states)
                elif k % 5 == 4:
                    big.set_poses(poses)
                elif k % 5 == 2:
                    big.animate_layers(sets[k % 2], host[k % 4], mk)
                else:
                    dev = k % 3 == 1
                    big.animate_ik(sets[k % 2], devs[k % 4] if dev else host[k % 4], iks, dtgs[k % 4] if dev else tgs[k % 4], mk if k % 7 else None)
                if k % 10 == 0:
                    fr = api.Frame(gpu_device, W, H)
                    fr.draw_batch(big, vp)
                    fr.submit()
                    fr.close()
                if k % 25 == 5:  # IK sets come and go as well
                    tmp = api.AnimIK(gpu_device, parents, chains[:1 + k % 4])
                    big.animate_ik(sets[k % 2], host[k % 4], tmp, np.ascontiguousarray(tgs[k % 4][:, :tmp.nchains]), mk)
                    tmp.close()
        run(0, 60)
        gpu_device.synchronize()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        run(60, 300)
        gpu_device.synchronize()
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        assert free0 - free1 < 64 << 20, f"device memory grew by {(free0 - free1) >> 20} MiB over 300 calls"
        big.animate_ik(sets[1], host[1], iks, tgs[1], mk)
        want = am.palettes(mf, ik.sample(tclips, host[1], 64, masks, parents, chains, tgs[1]))
        assert _bits_equal(big.read_palettes(), want)
    finally:
        big.close()
        iks.close()
        mk.close()
        for a in sets:
            a.close()
        m.close()
