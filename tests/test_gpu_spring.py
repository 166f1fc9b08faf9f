"""GPU: spring bones after the IK chains (SPEC.md section 24).  The k_anim_spring kernels equal the binary32 numpy model
(tests/spring_model.py) bit for bit -- the local matrices through mtr_anim_sample_spring, the palettes through
mtr_batch_read_palettes, and the state records themselves -- on both kinds of animation set, frame after frame with the
states handed on: a strand of three springs (three rounds), two strands listed child first (two rounds, two threads a
round), a spring whose spring parent lies in the other wave, chains on an ancestor of a spring joint (and the same call
without an IK set), motion taken from the root deltas of a player's steps on the same stream, zeroed, NaN and user-written
states, paused calls, 67 instances over 40 frames in place on the device, and rejected calls that change nothing."""
import ctypes as C
import functools

import numpy as np
import pytest

from mt_renderer_amd import api
from tests import anim_ik_model as ik
from tests import anim_model as anm
from tests import player_model as pm
from tests import root_model as rm
from tests import spring_model as sm
from tests.test_gpu_anim import _bits_equal, _model_file, _small_md, _trs
from tests.test_gpu_anim_layers import KINDS, _make

pytestmark = pytest.mark.gpu
F = np.float32
DT = 1.0 / 60.0


def _dev(a):
    """a structured array as a uint8 tensor [records, bytes] on the GPU"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1, a.dtype.itemsize).copy()).to("cuda:0")


def _dev_f32(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=F)).to("cuda:0")


def _host(t, dtype, shape):
    return t.cpu().numpy().reshape(-1).view(dtype).reshape(shape)


def _same_states(got, want, what):
    g, w = (np.ascontiguousarray(a).view(np.uint32).reshape(-1, 8) for a in (got, want))
    bad = g != w
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} state words differ, first at {np.argwhere(bad)[0]}"


def _same_mats(got, want, what):
    assert got.shape == want.shape, what
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} matrix elements differ, first at {np.argwhere(bad)[0]}"


@functools.lru_cache(maxsize=None)
def _case(name, kind, n, h=DT, with_motion=True, seed=7):
    """one case of the model's generator with the library's dtypes; nobody writes into it"""
    assert (api.SPRING, api.SPRING_STATE) == (sm.SPRING, sm.STATE)
    return sm.make_case(name, seed + 13 * n, n=n, h=h, with_motion=with_motion, kind=kind, dtype_spring=api.SPRING, dtype_state=api.SPRING_STATE,
                        dtype_layer=api.ANIM_LAYER, dtype_target=api.ANIM_IK_TARGET)


class _Sets:
    """the library's sets of a case"""

    def __init__(self, dev, c, skeleton=False):
        self.c, self.J = c, c["J"]
        self.anim = _make(dev, c["kind"], c["J"], c["clips"])
        self.mk = api.AnimMasks(dev, c["J"], c["masks"])
        self.sp = api.AnimSpring(dev, c["parents"], c["springs"])
        self.ik = api.AnimIK(dev, c["parents"], c["chains"].astype(api.ANIM_IK_CHAIN)) if c["chains"] is not None else None
        self.m = self.b = self.mf = None
        if skeleton:
            par = [int(p) for p in c["parents"]]
            imats = _trs(np.random.default_rng(c["J"]), c["J"], scale=(0.5, 2.0), trans=20.0)
            self.mf = _model_file(par, imats)
            self.m = api.Model.new(dev, _small_md())
            self.m.set_skeleton(par, imats)
            self.b = api.Batch(dev, self.m, np.tile(np.eye(4, dtype=F).reshape(16), (c["n"], 1)))

    def close(self):
        for h in (self.b, self.ik, self.sp, self.mk, self.anim, self.m):
            if h:
                h.close()


def _frames(c, nframes, seed=3):
    """per frame the layers (the clips move on by a third of a key) and the motion of the case's kind"""
    rng = np.random.default_rng(seed)
    ly = c["layers"]
    for f in range(nframes):
        yield ly, (sm.rigid(rng, c["n"]) if c["motion"] is not None else None)
        ly = ly.copy()
        ly["x"] += F(1.0 / 3.0)


def _model(c, ly, st, motion, h=None, chains="case"):
    ch = c["chains"] if isinstance(chains, str) else chains
    return sm.sample(c["clips"], ly, c["J"], c["masks"], c["parents"], c["springs"].astype(sm.SPRING), st.astype(sm.STATE), c["h"] if h is None else h,
                     motion, ch, c["targets"] if ch is not None else None)


SHAPES = [("chain4", 1), ("chain4", 5), ("strands9", 5), ("waves70", 3), ("ik9", 5)]


# ---- 1. the local matrices and the states through the host hook, 12 frames --------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,n", SHAPES)
def test_sampled_locals_and_states_are_bit_exact(gpu_device, kind, name, n):
    c = _case(name, kind, n)
    rounds = sm.rounds_of(c["parents"], c["springs"])
    assert max(rounds) + 1 == {"chain4": 3, "strands9": 2, "waves70": 3, "ik9": 2}[name]
    if name == "strands9":
        assert rounds == [1, 0, 1, 0], "listed child first"
    if name == "waves70":
        assert int(c["springs"]["joint"][0]) >= 64 > int(c["springs"]["joint"][2]) and rounds[0] == rounds[2] + 1
    s = _Sets(gpu_device, c)
    try:
        st = c["states"]
        for f, (ly, mo) in enumerate(_frames(c, 12)):
            want, want_st = _model(c, ly, st, mo)
            assert np.isfinite(want).all()
            got, got_st = s.anim.sample_spring(ly, s.sp, st, c["h"], s.ik, c["targets"], mo, s.mk)
            _same_mats(got, want, f"frame {f}: locals")
            _same_states(got_st, want_st, f"frame {f}: states")
            if f == 0:
                assert not _bits_equal(got, _model(c, ly, np.zeros_like(st), mo)[0]) or n == 1, "the states show"
            st = got_st
    finally:
        s.close()


# ---- 2. the palettes and the states on the device, in place, 12 frames ------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,n", [("chain4", 1), ("chain4", 5), ("waves70", 3), ("ik9", 5)])
def test_palettes_and_device_states_are_bit_exact(gpu_device, kind, name, n):
    c = _case(name, kind, n)
    s = _Sets(gpu_device, c, skeleton=True)
    try:
        st = c["states"].astype(sm.STATE)
        t_st = _dev(c["states"])
        for f, (ly, mo) in enumerate(_frames(c, 12)):
            locals_, st = _model(c, ly, st, mo)
            s.b.animate_spring(s.anim, ly if f % 2 else _dev(ly).view(n, -1), s.sp, t_st, c["h"], s.ik, c["targets"],
                               _dev_f32(mo), s.mk)
            if f in (0, 1, 5, 11):
                _same_mats(s.b.read_palettes(), anm.palettes(s.mf, locals_), f"frame {f}: palettes")
                _same_states(_host(t_st, sm.STATE, (n, -1)), st, f"frame {f}: states")
    finally:
        s.close()


# ---- 3. the chains come first, and no IK set means no chains ----------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_springs_see_the_solved_rotation_and_no_ik_set_means_no_chains(gpu_device, kind):
    c = _case("ik9", kind, 5)
    s = _Sets(gpu_device, c)
    try:
        ly, st, mo = c["layers"], c["states"], c["motion"]
        with_ik, st_ik = _model(c, ly, st, mo)
        without, st_no = _model(c, ly, st, mo, chains=None)
        assert not _bits_equal(with_ik[:, 2], without[:, 2]), "the chain on joint 1 shows in the spring on joint 2"
        got, got_st = s.anim.sample_spring(ly, s.sp, st, c["h"], s.ik, c["targets"], mo, s.mk)
        _same_mats(got, with_ik, "with the chains")
        _same_states(got_st, st_ik, "with the chains")
        got, got_st = s.anim.sample_spring(ly, s.sp, st, c["h"], None, None, mo, s.mk)
        _same_mats(got, without, "without an IK set")
        _same_states(got_st, st_no, "without an IK set")
    finally:
        s.close()


# ---- 4. zeroed, NaN and user-written states; paused calls ------------------------------------------------------------------------
@pytest.mark.parametrize("with_motion", [True, False])
@pytest.mark.parametrize("h", [DT, 0.0, -DT, float("nan"), float("inf")])
def test_state_patterns_and_paused_calls(gpu_device, h, with_motion):
    c = _case("strands9", "uniform", 8, h=h, with_motion=with_motion)
    s = _Sets(gpu_device, c)
    try:
        ly, st, mo = c["layers"], c["states"], c["motion"]
        probe = []
        want, want_st = sm.sample(c["clips"], ly, c["J"], c["masks"], c["parents"], c["springs"].astype(sm.SPRING), st.astype(sm.STATE), c["h"], mo,
                                  probe=probe)
        assert all(p["dead"][0] and p["nonfinite"][1] and p["nonfinite"][2] and not p["fresh"][3:].any() for p in probe)
        assert st["pad"][3, 0] == 0xDEADBEEF and (want_st["pad"] == 0).all() and (want_st["live"] == 1).all()
        got, got_st = s.anim.sample_spring(ly, s.sp, st, c["h"], None, None, mo, s.mk)
        _same_mats(got, want, "locals")
        _same_states(got_st, want_st, "states")
        if not h > 0 or not np.isfinite(h):
            assert all(p["paused"] for p in probe)
            if not with_motion:  # nothing carried: prev is what went in, bit for bit
                assert (got_st["prev"][3:].view(np.uint32) == st["prev"][3:].view(np.uint32)).all()
                assert any(p["ul_zero"][4] for p in probe), "cur at the joint itself: the rest position"
            else:  # what went in after the carry
                D = mo.astype(F)
                for k in range(st.shape[1]):
                    assert (got_st["prev"][3:, k].view(np.uint32) == sm._carry(D, st["prev"][:, k], None)[3:].view(np.uint32)).all()
        else:
            assert not _bits_equal(got_st["prev"][3:], st["prev"][3:])
    finally:
        s.close()


# ---- 5. motion from the root deltas of a player's steps, 20 frames on one stream ----------------------------------------------
def test_motion_from_root_deltas_chained_with_root_motion(gpu_device):
    import torch
    n, J = 5, 9
    c = _case("strands9", "uniform", n)
    rng = np.random.default_rng(24)
    clips = anm.gentle_clips(rng, J, shape=[(30, anm.CLIP_LOOP), (20, anm.CLIP_LOOP)], angle=0.4, trans=1.0, scale=(1.0, 1.0))
    traj = rm.walk_clip(31, 1) + rm.walk_clip(21, 1)
    rflags = np.array([rm.CYCLIC, rm.CYCLIC], dtype=np.uint32)
    tab = pm.table([30, 20], [pm.LOOP, pm.LOOP], [30.0, 24.0])
    par = [int(p) for p in c["parents"]]
    imats = _trs(rng, J, scale=(0.5, 2.0), trans=20.0)
    mf = _model_file(par, imats)
    m = api.Model.new(gpu_device, _small_md())
    m.set_skeleton(par, imats)
    anim, tset, root = api.Anim(gpu_device, J, clips), api.Anim(gpu_device, 1, traj), api.AnimRoot(gpu_device, 1, 2, 0, rflags)
    pl = api.AnimPlayer(gpu_device, tab[0], tab[2], tab[1], max_instances=n)
    sp = api.AnimSpring(gpu_device, c["parents"], c["springs"])
    mats = _trs(rng, n, scale=(1.0, 1.0), trans=5.0)
    b = api.Batch(gpu_device, m, mats)
    try:
        play = np.zeros(n, dtype=pm.PLAY)
        play["x_a"] = rng.uniform(0, 30, n)
        play["speed"] = rng.uniform(0.5, 1.5, n)
        play["clip_a"] = [0, 1, 0, 1, 0]
        t_pl, t_ly, t_sp = _dev(play), _dev(np.zeros((n, 2), dtype=pm.LAYER)).view(n, 2, 16), _dev(np.zeros((n, 2), dtype=pm.STEP)).view(n, 2, 16)
        zero = np.zeros((n, len(c["springs"])), dtype=api.SPRING_STATE)
        t_st, t_still = _dev(zero), _dev(zero)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        M, st, still = mats, zero.astype(sm.STATE), zero.astype(sm.STATE)
        springs = c["springs"].astype(sm.SPRING)
        for frame in range(1, 21):
            pl.advance(t_pl, pm.DT, None, out_layers=t_ly, out_steps=t_sp, stream=side)
            with torch.cuda.stream(side):
                D = root.deltas(tset, t_sp)
                b.animate_spring(anim, t_ly, sp, t_still, pm.DT)  # the second run: the same frames, motion == NULL
                b.animate_spring(anim, t_ly, sp, t_st, pm.DT, motion=D)
                b.root_motion_device(tset, root, t_sp, stream=side)
            play, _, ly, steps = pm.advance(play, pm.DT, tab, None, 2)
            Dm = rm.deltas(traj, (0, rflags), steps.astype(rm.STEP))
            locals_, st = sm.sample(clips, ly.astype(sm.lm.LAYER), J, None, c["parents"], springs, st, pm.DT, Dm)
            M = rm.root_motion(M, traj, (0, rflags), steps.astype(rm.STEP))
            _, still = sm.sample(clips, ly.astype(sm.lm.LAYER), J, None, c["parents"], springs, still, pm.DT, None)
            if frame in (1, 2, 10, 20):
                _same_mats(b.read_palettes(), anm.palettes(mf, locals_), f"frame {frame}: palettes")
                assert pm.same_bits(b.read_model_mats(), M).all(), f"frame {frame}: instance matrices"
                _same_states(_host(t_st, sm.STATE, (n, -1)), st, f"frame {frame}: states")
        # the same frames without motion: the particles are not carried, and it shows
        _same_states(_host(t_still, sm.STATE, (n, -1)), still, "without motion")
        assert not _bits_equal(_host(t_still, sm.STATE, (n, -1))["cur"], _host(t_st, sm.STATE, (n, -1))["cur"]), "motion shows"
    finally:
        for h in (b, sp, pl, root, tset, anim, m):
            h.close()


# ---- 6. 67 instances over 40 frames, the states in place on the device ---------------------------------------------------------
def test_sixty_seven_instances_forty_frames_in_place(gpu_device):
    n = 67
    c = _case("chain4", "uniform", n)
    s = _Sets(gpu_device, c, skeleton=True)
    try:
        st = c["states"].astype(sm.STATE)
        t_st = _dev(c["states"])
        t_ly = _dev(c["layers"]).view(n, -1)
        for f, (ly, mo) in enumerate(_frames(c, 40)):
            locals_, st = _model(c, ly, st, mo)
            t_ly.copy_(_dev(ly).view(n, -1))
            s.b.animate_spring(s.anim, t_ly, s.sp, t_st, c["h"], motion=_dev_f32(mo), masks=s.mk)
            if f in (0, 19, 39):
                _same_mats(s.b.read_palettes(), anm.palettes(s.mf, locals_), f"frame {f}: palettes")
        _same_states(_host(t_st, sm.STATE, (n, -1)), st, "the states after 40 frames")
        assert np.isfinite(st["cur"]).all()
    finally:
        s.close()


# ---- 7. rejected calls change nothing ----------------------------------------------------------------------------------------
def test_rejected_device_calls_leave_the_states_alone(gpu_device):
    import torch
    n = 5
    c = _case("ik9", "uniform", n)
    s = _Sets(gpu_device, c, skeleton=True)
    other = api.AnimSpring(gpu_device, ik.skeleton(4), sm.make_springs([1], [(0.0, 1.0, 0.0)], dtype=api.SPRING))
    tree = c["parents"].copy()
    tree[8] = 0
    moved = api.AnimSpring(gpu_device, tree, c["springs"])
    try:
        t_st, t_ly, t_tg = _dev(c["states"]), _dev(c["layers"]).view(n, -1), _dev(c["targets"]).view(n, -1)
        t_mo = torch.from_numpy(c["motion"]).to("cuda:0")
        big = torch.zeros(t_st.numel() + 32, dtype=torch.uint8, device="cuda:0")
        s.b.animate_spring(s.anim, t_ly, s.sp, t_st, c["h"], s.ik, t_tg, t_mo, s.mk)
        torch.cuda.synchronize()
        before_st, before_pal = t_st.cpu().numpy().copy(), s.b.read_palettes()
        L, inv = api.lib, api.MTR_E_INVALID
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        ok = (s.b._h, s.anim._h, s.mk._h, p(t_ly), 2, s.ik._h, p(t_tg), s.sp._h, p(t_st), p(t_mo), C.c_float(DT), None)

        def call(**kw):
            names = ("batch", "anim", "masks", "layers", "nlayers", "ik", "targets", "spring", "states", "motion", "dt", "stream")
            args = [kw.get(k, v) for k, v in zip(names, ok)]
            return L.mtr_batch_animate_spring_device(*args)
        unaligned = C.c_void_p(big.data_ptr() + 8)
        for what, kw in [("no batch", dict(batch=None)), ("no set", dict(anim=None)), ("no layers", dict(layers=None)), ("9 layers", dict(nlayers=9)),
                         ("no spring set", dict(spring=None)), ("a spring set of another skeleton", dict(spring=other._h)),
                         ("no states", dict(states=None)),
                         ("misaligned states", dict(states=unaligned)), ("misaligned motion", dict(motion=unaligned)),
                         ("misaligned layers", dict(layers=unaligned)), ("targets without an IK set", dict(ik=None)),
                         ("an IK set without targets", dict(targets=None)), ("misaligned targets", dict(targets=unaligned))]:
            assert call(**kw) == inv, what
        assert call(spring=moved._h) == inv and "joint 8 " in api.lib.mtr_last_error(gpu_device._h).decode(), "a spring set of other parents"
        torch.cuda.synchronize()
        assert (t_st.cpu().numpy() == before_st).all(), "the states' bytes"
        assert _bits_equal(s.b.read_palettes(), before_pal), "the palettes"
        for bad in (lambda: s.b.animate_spring(s.anim, t_ly, s.sp, t_st[:, :31], DT), lambda: s.b.animate_spring(s.anim, t_ly, s.sp, t_st.cpu(), DT),
                    lambda: s.b.animate_spring(s.anim, t_ly, s.sp, t_st, DT, ik=s.ik), lambda: s.b.animate_spring(s.anim, t_ly, s.sp, t_st, DT, motion=t_mo[:4])):
            with pytest.raises(api.MtrError):
                bad()
        # and a valid call still works
        want, want_st = _model(c, c["layers"], _host(t_st, sm.STATE, (n, -1)), c["motion"])
        s.b.animate_spring(s.anim, t_ly, s.sp, t_st, c["h"], s.ik, t_tg, t_mo, s.mk)
        _same_mats(s.b.read_palettes(), anm.palettes(s.mf, want), "after the rejected calls")
        _same_states(_host(t_st, sm.STATE, (n, -1)), want_st, "after the rejected calls")
    finally:
        moved.close()
        other.close()
        s.close()
