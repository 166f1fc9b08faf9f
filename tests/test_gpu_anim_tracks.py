"""GPU: animation tracks (SPEC.md section 15).  A track set goes through the entry points of section 14 unchanged: k_anim's
local matrices from tracks equal the binary32 numpy model (tests/anim_tracks_model.py) bit for bit, its palettes equal
mtr_rmodel_palette over the model's local matrices bit for bit (host and device states); models and batches animated from
tracks the reference encoder made render bit-exact against the oracle; one batch is animated alternately from a uniform
and a track set with frames in flight; invalid calls change nothing; no memory growth; and the local matrices lie within
the bound of section 15 of the same rules in float64."""
import numpy as np
import pytest

from mt_renderer_amd import anim_tracks, api, scene
from tests import anim_model as am
from tests import anim_tracks_model as tm
from tests.helpers import assert_same, render_oracle
from tests.test_gpu_anim import CHAIN64, SKELETONS, _bend, _bits_equal, _dev_states, _model_file, _render, _small_md, _trs

pytestmark = pytest.mark.gpu

PARENTS = {"chain64": SKELETONS["chain64"], "multi_root": SKELETONS["multi_root"], "j256": SKELETONS["j256"], "one": [255]}
assert {k: len(v) for k, v in PARENTS.items()} == tm.JOINT_COUNTS


def _inputs(J, n=tm.N_STATES, seed=15):
    rng = np.random.default_rng(seed)
    clips = tm.random_track_clips(rng, J)
    return clips, tm.track_states(rng, clips, J, n=n, dtype=api.ANIM_STATE)


# ---- 1. the local matrices, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(tm.JOINT_COUNTS))
def test_sampled_locals_from_tracks_are_bit_exact(gpu_device, kind):
    J = tm.JOINT_COUNTS[kind]
    clips, st = _inputs(J)
    ref = tm.sample(clips, st, J)
    assert np.isfinite(ref).all()
    # what the input must be able to tell apart, on the model alone
    for v in tm.WRONG_VARIANTS:
        inst = float((tm.sample(clips, st, J, variant=v).view(np.uint32) != ref.view(np.uint32)).any(axis=(1, 2)).mean())
        print(f"{kind}: {v} differs in {inst:.3f} of the instances")
        assert inst >= 0.10, f"{v} must be visible"
    anim = api.AnimTracks(gpu_device, J, clips)
    try:
        got = anim.sample(st)
        assert got.shape == (st.size, J, 16)
        bad = got.view(np.uint32) != ref.view(np.uint32)
        assert not bad.any(), f"{int(bad.sum())} of {ref.size} local matrix elements differ, first at {np.argwhere(bad)[0]}"
    finally:
        anim.close()


# ---- 2. the palettes, bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(tm.JOINT_COUNTS))
def test_palettes_from_tracks_are_bit_exact_host_and_device_states(gpu_device, kind):
    import torch
    parents = PARENTS[kind]
    J, n = len(parents), 64
    rng = np.random.default_rng(J * 7 + 1)
    imats = _trs(rng, J, scale=(0.5, 2.0), trans=20.0)
    mf = _model_file(parents, imats)
    clips = tm.random_track_clips(rng, J)
    m = api.Model.new(gpu_device, _small_md())
    anim = b = None
    try:
        m.set_skeleton(parents, imats)
        anim = api.AnimTracks(gpu_device, J, clips)
        b = api.Batch(gpu_device, m, np.tile(np.eye(4, dtype=np.float32).reshape(16), (n, 1)))
        zero = np.zeros((n, J, 16), dtype=np.float32)

        def check(what, animate):
            st = tm.track_states(rng, clips, J, n=n, dtype=api.ANIM_STATE)
            ref = am.palettes(mf, tm.sample(clips, st, J))
            assert np.isfinite(ref).all()
            b.update(palettes=zero)
            animate(st)
            got = b.read_palettes()
            assert got.shape == (n, J, 16)
            assert _bits_equal(got, ref), f"{what}: {int((got.view(np.uint32) != ref.view(np.uint32)).sum())} of {ref.size} palette elements differ"

        check("host states", lambda st: b.animate(anim, st))
        assert torch.cuda.current_stream().cuda_stream == 0
        check("device states, default stream", lambda st: b.animate(anim, _dev_states(st)))
        side = torch.cuda.Stream()

        def on_side(st):
            with torch.cuda.stream(side):
                b.animate(anim, _dev_states(st))
        check("device states, side stream", on_side)
        torch.cuda.synchronize()
    finally:
        if b:
            b.close()
        if anim:
            anim.close()
        m.close()


# ---- 3. rendering: what the encoder made is what gets drawn ---------------------------------------------------------
def _gentle_tracks(rng, **kw):
    clips = am.gentle_clips(rng, 64, **kw)
    return clips, [anim_tracks.compress(k, fl, tol_t=2e-3, tol_q=2e-3, tol_s=2e-3) for k, fl in clips]


def _setup(dev, rows=10, cols=16, seed=5):
    md = scene.skinned_capsule_model([((0.0, 0.0, 0.0), 0.35, 1.6)], rows=rows, cols=cols)
    rng = np.random.default_rng(seed)
    imats = _bend(rng, 64, angle=0.05)
    mf = _model_file(CHAIN64, imats)
    m = api.Model.new(dev, md)
    m.set_skeleton(CHAIN64, imats)
    clips, tclips = _gentle_tracks(rng)
    return md, mf, m, rng, clips, tclips


def _tpals(mf, tclips, st):
    return am.palettes(mf, tm.sample(tclips, st, 64))


def test_batch_animated_from_tracks_renders_like_the_oracle_unsharded_and_sharded(gpu_device):
    W, H = 192, 112
    md, mf, m, rng, clips, tclips = _setup(gpu_device)
    anim = api.AnimTracks(gpu_device, 64, tclips)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats, _ = scene.instance_lattice(4, 4, seed=300)
    b = api.Batch(gpu_device, m, mats)
    try:
        for step in range(2):
            st = am.random_states(rng, 16, api.ANIM_STATE)
            pals = _tpals(mf, tclips, st)
            b.animate(anim, st if step == 0 else _dev_states(st))
            assert _bits_equal(b.read_palettes(), pals)
            ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=mats, palettes=pals)])
            for mode in (api.TILE_ORDERED, api.TILE_AUTO):
                gpu_device.set_tile_mode(mode)
                assert_same(_render(gpu_device, W, H, lambda fr: fr.draw_batch(b, vp)), ref, f"unsharded step {step}, tile mode {mode}")
        nby, world = (H + 15) // 16, 2
        bands = np.round(np.linspace(0, nby, world + 1)).astype(np.uint32)
        for r in range(world):
            def draw(fr):
                fr.set_shard(r, world, api.OWN_BANDS, 0, bands)
                fr.draw_batch(b, vp)
            c, d, _ = _render(gpu_device, W, H, draw)
            y0, y1 = int(bands[r]) * 16, min(int(bands[r + 1]) * 16, H)
            assert (c[y0:y1] == ref[0][y0:y1]).all(), f"rank {r} of {world}: colour"
            assert _bits_equal(d[y0:y1], ref[1][y0:y1]), f"rank {r} of {world}: depth"
    finally:
        gpu_device.set_tile_mode(api.TILE_AUTO)
        b.close()
        anim.close()
        m.close()


def test_model_animated_from_tracks_renders_like_the_oracle(gpu_device):
    W, H = 160, 96
    md = scene.mesh50k(rows=12, cols=20)
    rng = np.random.default_rng(23)
    imats = _bend(rng, 64, angle=0.05)
    mf = _model_file(CHAIN64, imats)
    _, tclips = _gentle_tracks(rng, angle=0.04, trans=0.02)
    M = scene.to_f32_colmajor(scene.headline_transform(W, H))
    m = api.Model.new(gpu_device, md)
    anim = api.AnimTracks(gpu_device, 64, tclips)
    try:
        m.set_skeleton(CHAIN64, imats)
        for st in (dict(clip_a=2, x_a=47.3), dict(clip_a=1, x_a=12.5, clip_b=2, x_b=-3.25, w=0.4)):
            pal = _tpals(mf, tclips, api.anim_states(st, 1))[0]
            ref = render_oracle(W, H, [dict(md=md, M=M, palette=pal)])
            m.animate(anim, st)
            for mode in (api.TILE_ORDERED, api.TILE_AUTO):
                gpu_device.set_tile_mode(mode)
                assert_same(_render(gpu_device, W, H, lambda fr: m.render(fr, M)), ref, f"model animate {st}, tile mode {mode}")
    finally:
        gpu_device.set_tile_mode(api.TILE_AUTO)
        anim.close()
        m.close()


# ---- 4. both kinds of set on one batch -------------------------------------------------------------------------------
def test_one_batch_animated_alternately_from_a_uniform_and_a_track_set(gpu_device):
    W, H = 160, 96
    md, mf, m, rng, clips, tclips = _setup(gpu_device, rows=6, cols=10)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    sets = [api.Anim(gpu_device, 64, clips), api.AnimTracks(gpu_device, 64, tclips)]
    b = api.Batch(gpu_device, m, scene.instance_lattice(4, 4)[0])
    frames, args = [], []
    try:
        for k in range(12):
            mats, _ = scene.instance_lattice(4, 4, seed=700 + k)
            st = am.random_states(rng, 16, api.ANIM_STATE)
            if k == 5:  # ring churn: many animate calls of both kinds between two frames
                for c in range(30):
                    other = am.random_states(rng, 16, api.ANIM_STATE)
                    b.animate(sets[c % 2], _dev_states(other) if c % 3 == 1 else other)
            kind = k % 2
            if k == 9:  # a fresh track set, destroyed straight after the submit
                tmp = api.AnimTracks(gpu_device, 64, tclips)
                b.animate(tmp, st)
            else:
                b.animate(sets[kind], _dev_states(st) if k % 3 == 1 else st)
            b.update(model_mats=mats)
            fr = api.Frame(gpu_device, W, H)
            fr.draw_batch(b, vp)
            fr.submit()
            if k == 9:
                tmp.close()
            frames.append(fr)
            args.append((mats, st, kind))
        for k in reversed(range(12)):
            fr = frames[k]
            fr.wait()
            if k % 4 == 0 or k == 9:
                mats, st, kind = args[k]
                pals = _tpals(mf, tclips, st) if kind else am.palettes(mf, am.sample(clips, st, 64))
                ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=mats, palettes=pals)])
                assert_same((fr.color(), fr.depth(), fr.stats()), ref, f"frame {k}, {'tracks' if kind else 'uniform keys'}")
    finally:
        for fr in frames:
            fr.close()
        b.close()
        for a in sets:
            a.close()
        m.close()


# ---- 5. invalid calls change nothing -------------------------------------------------------------------------------
def test_invalid_calls_change_nothing(gpu_device):
    W, H = 160, 96
    md, mf, m, rng, clips, tclips = _setup(gpu_device, rows=6, cols=10)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats, _ = scene.instance_lattice(4, 4, seed=81)
    st = am.random_states(rng, 16, api.ANIM_STATE)
    other = am.random_states(rng, 16, api.ANIM_STATE)
    one = dict(clip_a=2, x_a=31.5, clip_b=0, x_b=0.25, w=0.5)
    pals = _tpals(mf, tclips, st)
    anim = api.AnimTracks(gpu_device, 64, tclips)
    b = api.Batch(gpu_device, m, mats)
    rng63 = np.random.default_rng(3)
    anim63 = api.AnimTracks(gpu_device, 63, tm.random_track_clips(rng63, 63))
    dev2 = api.Device(0)
    anim_dev2 = api.AnimTracks(dev2, 64, tclips)
    try:
        def invalid(fn):
            with pytest.raises(api.MtrError) as e:
                fn()
            assert e.value.code == api.MTR_E_INVALID
            return str(e.value)

        b.animate(anim, st)
        m.animate(anim, one)
        dst = _dev_states(other)
        invalid(lambda: b.animate(anim63, other))          # njoints not the skeleton's
        invalid(lambda: b.animate(anim63, dst))
        invalid(lambda: m.animate(anim63, one))
        invalid(lambda: b.animate(anim_dev2, other))       # a track set of another device
        invalid(lambda: b.animate(anim_dev2, dst))
        invalid(lambda: m.animate(anim_dev2, one))
        # creation: every violation of "Data", one at a time on an otherwise valid set
        valid = tm.random_track_clips(np.random.default_rng(4), 40)
        api.AnimTracks(gpu_device, 40, valid).close()
        for what, bad, c, j, ch in tm.invalid_sets(valid, 40):
            assert tm.validate(bad, 40) is not None, what
            msg = invalid(lambda: api.AnimTracks(gpu_device, 40, bad))
            assert f"clip {c}" in msg, (what, msg)
            if j is not None:
                assert f"joint {j}, channel {ch}" in msg, (what, msg)
        invalid(lambda: api.AnimTracks(gpu_device, 0, valid))
        invalid(lambda: api.AnimTracks(gpu_device, 257, valid))
        invalid(lambda: api.AnimTracks(gpu_device, 40, []))
        # nothing changed: the batch and the model still render what the last valid calls set
        assert _bits_equal(b.read_palettes(), pals)
        ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=mats, palettes=pals)])
        assert_same(_render(gpu_device, W, H, lambda fr: fr.draw_batch(b, vp)), ref, "batch after invalid calls")
        M = scene.to_f32_colmajor(scene.headline_transform(W, H))
        ref = render_oracle(W, H, [dict(md=md, M=M, palette=_tpals(mf, tclips, api.anim_states(one, 1))[0])])
        assert_same(_render(gpu_device, W, H, lambda fr: m.render(fr, M)), ref, "model after invalid calls")
    finally:
        b.close()
        anim63.close()
        anim_dev2.close()
        dev2.close()
        anim.close()
        m.close()


# ---- 6. accuracy against exact arithmetic --------------------------------------------------------------------------
@pytest.mark.parametrize("J", [64, 256])
def test_locals_lie_within_the_bound_of_the_exact_rules(gpu_device, J):
    """|GPU - float64 model| <= K_LOCALS u sum|terms| (SPEC.md section 15: K_LOCALS = 26 rounded operations on the longest
    path), nlerp calls with |d| < 8 u left out (under 1 % of the calls)."""
    clips, st = _inputs(J)
    tr = am.Trace()
    val, mag = tm.sample_exact(clips, st, J, trace=tr)
    d = tr.all_d()
    near = float((np.abs(d) < 8 * tm.U).mean())
    anim = api.AnimTracks(gpu_device, J, clips)
    try:
        got = anim.sample(st).astype(np.float64)
    finally:
        anim.close()
    keep = ~tr.near
    frac = np.abs(got - val)[keep] / (tm.K_LOCALS * tm.U * mag[keep] + 1e-300)
    print(f"J = {J}: {d.size} nlerp calls, {near:.5f} with |d| < 8 u (min |d| {np.abs(d).min():.3e}); "
          f"largest |GPU - exact| / ({tm.K_LOCALS} u sum|terms|) = {frac.max():.4f}")
    assert near < 0.01
    assert frac.max() <= 1.0


# ---- 7. no growth --------------------------------------------------------------------------------------------------
def test_no_memory_growth_over_both_kinds(gpu_device):
    import torch
    W, H = 160, 96
    md, mf, m, rng, clips, tclips = _setup(gpu_device, rows=6, cols=10)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats = np.tile(scene.instance_lattice(4, 4, seed=71)[0], (16, 1))
    sets = [api.Anim(gpu_device, 64, clips), api.AnimTracks(gpu_device, 64, tclips)]
    big = api.Batch(gpu_device, m, mats)
    host = [am.random_states(rng, 256, api.ANIM_STATE) for _ in range(4)]
    devs = [_dev_states(s) for s in host]
    try:
        def run(k0, count):
            for k in range(k0, k0 + count):
                big.animate(sets[k % 2], devs[k % 4] if k % 3 == 1 else host[k % 4])
                if k % 10 == 0:
                    fr = api.Frame(gpu_device, W, H)
                    fr.draw_batch(big, vp)
                    fr.submit()
                    fr.close()
                if k % 50 == 25:  # sets of both kinds come and go as well
                    tmp = api.AnimTracks(gpu_device, 64, tclips) if k % 100 == 25 else api.Anim(gpu_device, 64, clips)
                    big.animate(tmp, host[k % 4])
                    tmp.close()
        run(0, 60)
        gpu_device.synchronize()
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        run(60, 300)
        gpu_device.synchronize()
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        assert free0 - free1 < 64 << 20, f"device memory grew by {(free0 - free1) >> 20} MiB over 300 animate calls"
        assert _bits_equal(big.read_palettes(), _tpals(mf, tclips, host[359 % 4]))
    finally:
        big.close()
        for a in sets:
            a.close()
        m.close()
