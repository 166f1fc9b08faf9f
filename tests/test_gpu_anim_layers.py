"""GPU: animation layers (SPEC.md section 16).  The local matrices of k_anim_layers equal the binary32 numpy model
(tests/anim_layers_model.py) bit for bit on both kinds of animation set; two OVERRIDE layers on mask 0 equal the cross-fade
of sections 14 / 15 bit for bit; the palettes equal mtr_rmodel_palette over the model's local matrices bit for bit (host and
device layers); a batch and a model animated from a base, a masked override and an additive layer render bit-exact against
the oracle; one batch is animated by all kinds of call with frames in flight while mask sets come and go; invalid calls
change nothing; every layer step lies within the section's per-step bound; no memory growth."""
import ctypes as C
import functools

import numpy as np
import pytest

from mt_renderer_amd import anim_layers, anim_tracks, api, scene
from tests import anim_layers_model as lm
from tests import anim_model as am
from tests import anim_tracks_model as tm
from tests.helpers import assert_same, render_oracle
from tests.test_gpu_anim import CHAIN64, SKELETONS, _bend, _bits_equal, _dev_states, _model_file, _render, _small_md, _trs

pytestmark = pytest.mark.gpu

PARENTS = {"chain64": SKELETONS["chain64"], "multi_root": SKELETONS["multi_root"], "j256": SKELETONS["j256"], "one": [255]}
KINDS = ["uniform", "tracks"]


def _make(dev, kind, J, clips):
    return api.Anim(dev, J, clips) if kind == "uniform" else api.AnimTracks(dev, J, clips)


def _dev_layers(ly, dtype="uint8"):
    import torch
    raw = np.ascontiguousarray(ly).view(np.uint8).reshape(ly.shape[0], -1)
    t = torch.from_numpy(raw.copy()).to("cuda:0")
    return t if dtype == "uint8" else t.view(torch.int32)


@functools.lru_cache(maxsize=None)
def _inputs(kind, J):
    """clips and masks of one (kind, J), shared by the cases that differ in L only; nobody writes into them"""
    rng = np.random.default_rng(16 + J)
    clips = am.random_clips(rng, J) if kind == "uniform" else tm.random_track_clips(rng, J)
    return clips, lm.random_masks(rng, J)


def _layers(kind, J, L, n=lm.N_STATES):
    clips, _ = _inputs(kind, J)
    return lm.layer_states(np.random.default_rng(1000 * J + L), clips, n=n, L=L, dtype=api.ANIM_LAYER)


# ---- 1. the local matrices, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("J,L", [(J, L) for J in (1, 63, 64, 65, 256) for L in (1, 2, 8)] + [(64, 4)])
def test_sampled_locals_are_bit_exact(gpu_device, kind, J, L):
    assert api.ANIM_LAYER == lm.LAYER
    clips, masks = _inputs(kind, J)
    ly = _layers(kind, J, L)
    ref = lm.sample(clips, ly, J, masks)
    assert np.isfinite(ref).all()
    anim = _make(gpu_device, kind, J, clips)
    mk = api.AnimMasks(gpu_device, J, masks)
    try:
        got = anim.sample_layers(ly, mk)
        assert got.shape == (ly.shape[0], J, 16)
        bad = got.view(np.uint32) != ref.view(np.uint32)
        assert not bad.any(), f"{int(bad.sum())} of {ref.size} local matrix elements differ, first at {np.argwhere(bad)[0]}"
        # without a mask set every mask index means the built-in mask
        bad = anim.sample_layers(ly).view(np.uint32) != lm.sample(clips, ly, J, None).view(np.uint32)
        assert not bad.any(), f"no mask set: {int(bad.sum())} elements differ"
    finally:
        mk.close()
        anim.close()


# ---- 2. two OVERRIDE layers on mask 0 are the cross-fade ------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("J", [64, 65])
def test_two_override_layers_equal_the_cross_fade(gpu_device, kind, J):
    clips, masks = _inputs(kind, J)
    st = am.random_states(np.random.default_rng(2), 256, api.ANIM_STATE)
    anim = _make(gpu_device, kind, J, clips)
    mk = api.AnimMasks(gpu_device, J, masks)
    try:
        want = anim.sample(st)
        assert (st["w"] == 0).any() and _bits_equal(want, (am if kind == "uniform" else tm).sample(clips, st, J))
        ly = lm.crossfade_layers(st, api.ANIM_LAYER)
        assert _bits_equal(anim.sample_layers(ly, mk), want)
        assert _bits_equal(anim.sample_layers(ly), want)
    finally:
        mk.close()
        anim.close()


# ---- 3. the palettes, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("skel", list(PARENTS))
def test_palettes_are_bit_exact_host_and_device_layers(gpu_device, kind, skel):
    import torch
    parents = PARENTS[skel]
    J, n, L = len(parents), 64, 3
    rng = np.random.default_rng(J * 7 + 3)
    imats = _trs(rng, J, scale=(0.5, 2.0), trans=20.0)
    mf = _model_file(parents, imats)
    clips, masks = _inputs(kind, J)
    m = api.Model.new(gpu_device, _small_md())
    anim = mk = b = None
    try:
        m.set_skeleton(parents, imats)
        anim = _make(gpu_device, kind, J, clips)
        mk = api.AnimMasks(gpu_device, J, masks)
        b = api.Batch(gpu_device, m, np.tile(np.eye(4, dtype=np.float32).reshape(16), (n, 1)))
        zero = np.zeros((n, J, 16), dtype=np.float32)

        def check(what, animate):
            ly = lm.layer_states(rng, clips, n=n, L=L, dtype=api.ANIM_LAYER)
            ref = am.palettes(mf, lm.sample(clips, ly, J, masks))
            assert np.isfinite(ref).all()
            b.update(palettes=zero)
            animate(ly)
            got = b.read_palettes()
            assert got.shape == (n, J, 16)
            assert _bits_equal(got, ref), f"{what}: {int((got.view(np.uint32) != ref.view(np.uint32)).sum())} of {ref.size} palette elements differ"

        check("host layers", lambda ly: b.animate_layers(anim, ly, mk))
        assert torch.cuda.current_stream().cuda_stream == 0
        check("device layers, default stream", lambda ly: b.animate_layers(anim, _dev_layers(ly), mk))
        check("device layers as int32", lambda ly: b.animate_layers(anim, _dev_layers(ly, "int32"), mk, L=L))
        side = torch.cuda.Stream()

        def on_side(ly):
            with torch.cuda.stream(side):
                b.animate_layers(anim, _dev_layers(ly), mk)
        check("device layers, side stream", on_side)
        torch.cuda.synchronize()
    finally:
        if b:
            b.close()
        if mk:
            mk.close()
        if anim:
            anim.close()
        m.close()


# ---- 4. rendering ------------------------------------------------------------------------------------------------------
def _gentle(rng, kind, **kw):
    """four gentle clips and, as clip 4, the deltas of the 31-key clip from the first key of the looping clip; two masks"""
    clips = am.gentle_clips(rng, 64, **kw)
    clips.append((anim_layers.delta_clip(clips[1][0], clips[2][0][0]), 0))
    if kind == "tracks":
        clips = [anim_tracks.compress(k, fl, tol_t=2e-3, tol_q=2e-3, tol_s=2e-3) for k, fl in clips]
    masks = np.zeros((2, 64), dtype=np.float32)
    masks[0, 24:] = np.linspace(0.0, 1.0, 40)   # the upper body, faded in
    masks[1] = np.where(np.arange(64) % 3 == 0, 0.0, rng.uniform(0.2, 1.0, 64))
    masks[1, 60:] = 1.0
    return clips, masks


def _stack(rng, n):
    """n stacks of a base, an OVERRIDE on mask 1 and an ADDITIVE layer of the delta clip on mask 2"""
    ly = np.zeros((n, 3), dtype=api.ANIM_LAYER)
    ly["clip"][:, 0], ly["clip"][:, 1], ly["clip"][:, 2] = rng.integers(0, 4, n), rng.integers(0, 4, n), 4
    ly["x"] = rng.uniform(-40.0, 160.0, (n, 3))
    ly["w"][:, 1:] = rng.uniform(0.1, 1.1, (n, 2))
    ly["mask"][:, 1], ly["mask"][:, 2] = 1, 2
    ly["mode"][:, 2] = api.LAYER_ADDITIVE
    return ly


def _setup(dev, kind, rows=10, cols=16, seed=5):
    md = scene.skinned_capsule_model([((0.0, 0.0, 0.0), 0.35, 1.6)], rows=rows, cols=cols)
    rng = np.random.default_rng(seed)
    imats = _bend(rng, 64, angle=0.05)
    mf = _model_file(CHAIN64, imats)
    m = api.Model.new(dev, md)
    m.set_skeleton(CHAIN64, imats)
    clips, masks = _gentle(rng, kind)
    return md, mf, m, rng, clips, masks


def _lpals(mf, clips, ly, masks):
    return am.palettes(mf, lm.sample(clips, ly, 64, masks))


@pytest.mark.parametrize("kind", KINDS)
def test_batch_animated_from_layers_renders_like_the_oracle(gpu_device, kind):
    W, H = 192, 112
    md, mf, m, rng, clips, masks = _setup(gpu_device, kind)
    anim = _make(gpu_device, kind, 64, clips)
    mk = api.AnimMasks(gpu_device, 64, masks)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats, _ = scene.instance_lattice(4, 4, seed=300)
    b = api.Batch(gpu_device, m, mats)
    try:
        for step in range(2):
            ly = _stack(rng, 16)
            pals = _lpals(mf, clips, ly, masks)
            assert not _bits_equal(pals, _lpals(mf, clips, ly[:, :2], masks)), "the additive layer shows"
            assert not _bits_equal(pals, _lpals(mf, clips, ly[:, ::2], masks)), "the override layer shows"
            b.animate_layers(anim, ly if step == 0 else _dev_layers(ly), mk)
            assert _bits_equal(b.read_palettes(), pals)
            ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=mats, palettes=pals)])
            for mode in (api.TILE_ORDERED, api.TILE_AUTO):
                gpu_device.set_tile_mode(mode)
                assert_same(_render(gpu_device, W, H, lambda fr: fr.draw_batch(b, vp)), ref, f"{kind} step {step}, tile mode {mode}")
    finally:
        gpu_device.set_tile_mode(api.TILE_AUTO)
        b.close()
        mk.close()
        anim.close()
        m.close()


@pytest.mark.parametrize("kind", KINDS)
def test_model_animated_from_layers_renders_like_the_oracle(gpu_device, kind):
    W, H = 160, 96
    md = scene.mesh50k(rows=12, cols=20)
    rng = np.random.default_rng(23)
    imats = _bend(rng, 64, angle=0.05)
    mf = _model_file(CHAIN64, imats)
    clips, masks = _gentle(rng, kind, angle=0.04, trans=0.02)
    M = scene.to_f32_colmajor(scene.headline_transform(W, H))
    m = api.Model.new(gpu_device, md)
    anim = _make(gpu_device, kind, 64, clips)
    mk = api.AnimMasks(gpu_device, 64, masks)
    try:
        m.set_skeleton(CHAIN64, imats)
        for ly in (_stack(rng, 1), dict(clip=[[2, 1, 4]], x=[[47.3, 12.5, 3.25]], w=[[1.0, 0.4, 0.8]], mask=[[0, 1, 0]], mode=[[0, 0, 1]])):
            pal = _lpals(mf, clips, api.anim_layers(ly, 1), masks)[0]
            ref = render_oracle(W, H, [dict(md=md, M=M, palette=pal)])
            m.animate_layers(anim, ly, mk)
            for mode in (api.TILE_ORDERED, api.TILE_AUTO):
                gpu_device.set_tile_mode(mode)
                assert_same(_render(gpu_device, W, H, lambda fr: m.render(fr, M)), ref, f"{kind} model layers, tile mode {mode}")
    finally:
        gpu_device.set_tile_mode(api.TILE_AUTO)
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
    b = api.Batch(gpu_device, m, scene.instance_lattice(4, 4)[0])
    frames, want = [], []
    try:
        for k in range(12):
            mats, _ = scene.instance_lattice(4, 4, seed=700 + k)
            ly = _stack(rng, 16)
            st = am.random_states(rng, 16, api.ANIM_STATE)
            tmp = None
            if k == 5:  # ring churn: many calls of every kind between two frames
                for c in range(30):
                    if c % 3 == 2:
                        b.animate(sets[c % 2], am.random_states(rng, 16, api.ANIM_STATE))
                    else:
                        other = _stack(rng, 16)
                        b.animate_layers(sets[c % 2], _dev_layers(other) if c % 4 == 1 else other, mk if c % 5 else None)
            kind = k % 4
            if kind == 0:    # layers over the uniform set
                b.animate_layers(sets[0], _dev_layers(ly) if k == 8 else ly, mk)
                locals_ = lm.sample(clips, ly, 64, masks)
            elif kind == 1:  # plain states
                b.animate(sets[(k // 4) % 2], st)
                locals_ = (am.sample(clips, st, 64) if (k // 4) % 2 == 0 else tm.sample(tclips, st, 64))
            elif kind == 2:  # layers over the track set; in frame 6 through a mask set that is destroyed after the submit
                if k == 6:
                    tmp = api.AnimMasks(gpu_device, 64, masks)
                b.animate_layers(sets[1], ly, tmp or mk)
                locals_ = lm.sample(tclips, ly, 64, masks)
            else:            # poses from the host
                locals_ = am.sample(clips, st, 64)
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
            if k in (0, 2, 3, 5, 6, 8, 9):
                mats, locals_ = want[k]
                ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=mats, palettes=am.palettes(mf, locals_))])
                assert_same((fr.color(), fr.depth(), fr.stats()), ref, f"frame {k}")
    finally:
        for fr in frames:
            fr.close()
        b.close()
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
    ly, other = _stack(rng, 16), _stack(rng, 16)
    one = _stack(rng, 1)
    pals = _lpals(mf, clips, ly, masks)
    anim = api.Anim(gpu_device, 64, clips)
    mk = api.AnimMasks(gpu_device, 64, masks)
    b = api.Batch(gpu_device, m, mats)
    bb = api.Batch(gpu_device, bare, mats)
    anim63 = api.Anim(gpu_device, 63, am.gentle_clips(rng, 63))
    mk63 = api.AnimMasks(gpu_device, 63, np.ones((1, 63), dtype=np.float32))
    dev2 = api.Device(0)
    anim_dev2 = api.Anim(dev2, 64, clips)
    mk_dev2 = api.AnimMasks(dev2, 64, masks)
    closed = api.Anim(gpu_device, 64, clips)
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
        b.animate_layers(anim, ly, mk)
        m.animate_layers(anim, one, mk)
        dly = _dev_layers(other)
        big = np.zeros((16, 9), dtype=api.ANIM_LAYER)
        for bad_anim, bad_mk in ((anim63, mk), (anim, mk63), (anim_dev2, mk), (anim, mk_dev2), (closed, mk)):
            invalid(lambda: b.animate_layers(bad_anim, other, bad_mk))     # joint counts, devices, a NULL handle
            invalid(lambda: b.animate_layers(bad_anim, dly, bad_mk))
            invalid(lambda: m.animate_layers(bad_anim, one, bad_mk))
        invalid(lambda: bare.animate_layers(anim, one, mk))                # no skeleton
        invalid(lambda: bb.animate_layers(anim, other, None))
        invalid(lambda: bb.animate_layers(anim, dly, None))
        invalid(lambda: b.animate_layers(anim, big, mk))                   # 9 layers
        invalid(lambda: b.animate_layers(anim, _dev_layers(big), mk))
        invalid(lambda: m.animate_layers(anim, big[:1], mk))
        rc_invalid(L.mtr_batch_animate_layers(b._h, anim._h, mk._h, p(other), 0))
        rc_invalid(L.mtr_batch_animate_layers(b._h, anim._h, mk._h, None, 3))
        rc_invalid(L.mtr_model_animate_layers(m._h, anim._h, mk._h, None, 3))
        rc_invalid(L.mtr_batch_animate_layers_device(b._h, anim._h, mk._h, None, 3, None))
        rc_invalid(L.mtr_batch_animate_layers(None, anim._h, mk._h, p(other), 3))
        pad = torch.zeros(16 * 48 + 16, dtype=torch.uint8, device="cuda:0")
        pad[8:8 + 16 * 48] = dly.reshape(-1)
        assert (pad.data_ptr() + 8) % 16 == 8
        rc_invalid(L.mtr_batch_animate_layers_device(b._h, anim._h, mk._h, C.c_void_p(pad.data_ptr() + 8), 3, None))  # misaligned
        out = np.zeros((16, 64, 16), dtype=np.float32)
        rc_invalid(L.mtr_anim_sample_layers(anim._h, mk._h, p(other), 9, 16, p(out), out.size))
        rc_invalid(L.mtr_anim_sample_layers(anim._h, mk63._h, p(other), 3, 16, p(out), out.size))
        rc_invalid(L.mtr_anim_sample_layers(anim._h, mk._h, p(other), 3, 16, p(out), out.size - 1))
        # mask sets: njoints outside 1..256, no mask, weights that are NaN or outside [0, 1]
        w1 = np.ones(257, dtype=np.float32)
        for nj, nm in ((0, 1), (257, 1), (64, 0)):
            h = C.c_void_p(1)
            rc_invalid(L.mtr_anim_masks_create(gpu_device._h, nj, nm, p(w1), C.byref(h)))
            assert not h.value
        rc_invalid(L.mtr_anim_masks_create(gpu_device._h, 64, 1, None, C.byref(C.c_void_p())))
        for v in (np.nan, -1e-6, 1.0000001, np.inf):
            w = masks.copy()
            w[1, 37] = v
            msg = invalid(lambda: api.AnimMasks(gpu_device, 64, w))
            assert "mask 2, joint 37" in msg, msg
        with pytest.raises(api.MtrError):
            b.animate_layers(anim, other[:15], mk)                         # not n stacks
        # nothing changed: the batch and the model still render what the last valid calls set
        assert _bits_equal(b.read_palettes(), pals)
        ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=mats, palettes=pals)])
        assert_same(_render(gpu_device, W, H, lambda fr: fr.draw_batch(b, vp)), ref, "batch after invalid calls")
        M = scene.to_f32_colmajor(scene.headline_transform(W, H))
        ref = render_oracle(W, H, [dict(md=md, M=M, palette=_lpals(mf, clips, one, masks)[0])])
        assert_same(_render(gpu_device, W, H, lambda fr: m.render(fr, M)), ref, "model after invalid calls")
    finally:
        b.close()
        bb.close()
        anim63.close()
        mk63.close()
        anim_dev2.close()
        mk_dev2.close()
        dev2.close()
        mk.close()
        anim.close()
        bare.close()
        m.close()


# ---- 7. the per-step bound ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_every_layer_step_lies_within_the_bound_of_the_exact_step(gpu_device, kind):
    """Per layer step, |binary32 - float64 step| <= k u sum|terms| with k of SPEC.md section 16 (21 / 25 on uniform keys,
    23 / 27 on tracks, OVERRIDE / ADDITIVE), nlerp calls with |d| < 8 u left out (under 1 % of the calls).  The GPU's local
    matrices equal the model's bit for bit, so its (T, Q, S) after every step are the model's, which step_exact measures."""
    J, L = 64, 8
    clips, masks = _inputs(kind, J)
    ly = _layers(kind, J, L)
    anim = _make(gpu_device, kind, J, clips)
    mk = api.AnimMasks(gpu_device, J, masks)
    try:
        for upto in (2, 4, 8):  # the stack after its first layers: the (T, Q, S) every later step starts from
            assert _bits_equal(anim.sample_layers(np.ascontiguousarray(ly[:, :upto]), mk), lm.sample(clips, ly[:, :upto], J, masks))
    finally:
        mk.close()
        anim.close()
    res = lm.step_exact(clips, ly, J, masks)
    assert {r["kind"] for r in res} == {lm.OVERRIDE, lm.ADDITIVE}
    for r in res:
        print(f"{kind}, J = {J}, L = {L}, {'ADDITIVE' if r['kind'] else 'OVERRIDE'}: {r['calls']} nlerp calls, {r['left_out']} with |d| < 8 u "
              f"(min |d| {r['min_d']:.3e}); largest |GPU - exact| / ({r['k']} u sum|terms|) = {r['frac']:.4f}")
        assert r["k"] == {("uniform", 0): 21, ("uniform", 1): 25, ("tracks", 0): 23, ("tracks", 1): 27}[(kind, r["kind"])]
        assert r["left_out"] < 0.01 * r["calls"]
        assert r["frac"] <= 1.0


# ---- 8. no growth ------------------------------------------------------------------------------------------------------
def test_no_memory_growth_over_the_three_kinds_of_call(gpu_device):
    import torch
    W, H = 160, 96
    md, mf, m, rng, clips, masks = _setup(gpu_device, "uniform", rows=6, cols=10)
    tclips = [anim_tracks.compress(k, fl, tol_t=2e-3, tol_q=2e-3, tol_s=2e-3) for k, fl in clips]
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats = np.tile(scene.instance_lattice(4, 4, seed=71)[0], (16, 1))
    sets = [api.Anim(gpu_device, 64, clips), api.AnimTracks(gpu_device, 64, tclips)]
    mk = api.AnimMasks(gpu_device, 64, masks)
    big = api.Batch(gpu_device, m, mats)
    host = [_stack(rng, 256) for _ in range(4)]
    devs = [_dev_layers(s) for s in host]
    states = am.random_states(rng, 256, api.ANIM_STATE)
    poses = am.sample(clips, states, 64)
    try:
        def run(k0, count):
            for k in range(k0, k0 + count):
                if k % 5 == 3:
                    big.animate(sets[k % 2], states)
                elif k % 5 == 4:
                    big.set_poses(poses)
                else:
                    big.animate_layers(sets[k % 2], devs[k % 4] if k % 3 == 1 else host[k % 4], mk if k % 7 else None)
                if k % 10 == 0:
                    fr = api.Frame(gpu_device, W, H)
                    fr.draw_batch(big, vp)
                    fr.submit()
                    fr.close()
                if k % 50 == 25:  # clip sets and mask sets come and go as well
                    tmp = api.AnimTracks(gpu_device, 64, tclips) if k % 100 == 25 else api.Anim(gpu_device, 64, clips)
                    tmk = api.AnimMasks(gpu_device, 64, masks)
                    big.animate_layers(tmp, host[k % 4], tmk)
                    tmk.close()
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
        big.animate_layers(sets[1], host[1], mk)
        assert _bits_equal(big.read_palettes(), _lpals(mf, tclips, host[1], masks))
    finally:
        big.close()
        mk.close()
        for a in sets:
            a.close()
        m.close()
