"""GPU: players (SPEC.md section 20).  k_play equals the binary32 numpy model (tests/player_model.py) bit for bit on every case
of the generator -- one advance through the host hook and three consecutive device advances, in the stored states and in all
three outputs, with 2 and 8 layers per instance (layers 2.. untouched), each output pointer NULL in turn, 1 to 257 instances;
commands from host and device lists, duplicates in every order, a clean scratch array after every call, a device command
buffer overwritten right after the call; 40 frames of advance -> animate_layers -> root_motion on a side stream with nothing
uploaded in between, palettes and matrices equal to the chained models and the last frame bit-exact against the oracle, a
rider attached after the root call; the player destroyed right after the last advance; invalid calls change nothing."""
import ctypes as C

import numpy as np
import pytest

from mt_renderer_amd import api, scene
from tests import anim_layers_model as lm
from tests import anim_model as anm
from tests import attach_model as am
from tests import player_model as pm
from tests import root_model as rm
from tests.helpers import assert_same, render_oracle
from tests.test_gpu_anim import _bits_equal, _render
from tests.test_gpu_anim_layers import _setup

pytestmark = pytest.mark.gpu

CASES = pm.cases()


def _dev(a):
    """a structured array as a uint8 tensor [records, bytes] on the GPU"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1, a.dtype.itemsize).copy()).to("cuda:0")


def _host(t, dtype, shape=None):
    a = t.cpu().numpy().reshape(-1).view(dtype)
    return a if shape is None else a.reshape(shape)


def _same(got, want, what):
    bad = ~pm.same_bits(got, want)
    assert got.shape == want.shape and not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} records differ, first at {np.argwhere(bad)[0]}"


def _player(dev, tab, n):
    return api.AnimPlayer(dev, tab[0], tab[2], tab[1], max_instances=n)


# ---- 1. bit for bit against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", pm.COUNTS)
def test_states_and_outputs_are_bit_exact(gpu_device, n):
    import torch
    assert (api.PLAY_STATE, api.PLAY_CMD, api.ANIM_STATE, api.ANIM_LAYER, api.ROOT_STEP) == (pm.PLAY, pm.CMD, pm.STATE, pm.LAYER, pm.STEP)
    side = torch.cuda.Stream()
    nan_seen = False
    for k, c in enumerate(c for c in CASES if c["n"] == n):
        want = pm.run_case(c)
        nl, skip = c["nlayers"], (None, "states", "layers", "steps")[k % 4]  # each output pointer NULL in turn
        pl = _player(gpu_device, c["tab"], n if k % 2 else n + 3)
        try:
            # one advance through the host hook
            dt, cm = c["calls"][0]
            st, oa, ol, os_ = pl.advance_host(c["states"], dt, cm, nlayers=0 if skip == "layers" else nl, layers=c["layers"],
                                              want_states=skip != "states", want_steps=skip != "steps")
            _same(st, want[0][0], f"{c['name']} host hook: states")
            for got, ref, name in ((oa, want[0][1], "states"), (ol, want[0][2], "layers"), (os_, want[0][3], "steps")):
                assert (got is None) == (skip == name)
                if got is not None:
                    _same(got, ref, f"{c['name']} host hook: out_{name}")
            # three consecutive device advances, on the current stream or on a side stream, the commands from host or device memory
            t_st, t_oa, t_ol, t_os = _dev(c["states"]), _dev(np.zeros(n, dtype=pm.STATE)), _dev(c["layers"]), _dev(np.zeros((n, 2), dtype=pm.STEP))
            cmds = [(_dev(cm) if (k % 3 == 1 and len(cm)) else (cm if len(cm) else None)) for _, cm in c["calls"]]
            torch.cuda.synchronize()
            s = side if k % 2 else torch.cuda.current_stream()
            for i, (dt, _) in enumerate(c["calls"]):
                pl.advance(t_st, dt, cmds[i], out_states=None if skip == "states" else t_oa, out_layers=None if skip == "layers" else t_ol.view(n, nl, 16),
                           out_steps=None if skip == "steps" else t_os.view(n, 2, 16), stream=s)
                s.synchronize()
                _same(_host(t_st, pm.PLAY), want[i][0], f"{c['name']} call {i}: states")
                if skip != "states":
                    _same(_host(t_oa, pm.STATE), want[i][1], f"{c['name']} call {i}: out_states")
                if skip != "layers":
                    _same(_host(t_ol, pm.LAYER, (n, nl)), want[i][2], f"{c['name']} call {i}: out_layers")
                if skip != "steps":
                    _same(_host(t_os, pm.STEP, (n, 2)), want[i][3], f"{c['name']} call {i}: out_steps")
            if skip == "layers":
                _same(_host(t_ol, pm.LAYER, (n, nl)), c["layers"], f"{c['name']}: layers not asked for")
            nan_seen |= bool(np.isnan(want[2][0]["w"]).any() or np.isnan(want[2][0]["x_b"]).any())
        finally:
            pl.close()
    assert nan_seen or n < 63, "the special values reach the comparison"


# ---- 2. commands ---------------------------------------------------------------------------------------------------------------
def test_commands_from_host_and_device_in_any_order(gpu_device):
    import torch
    c = next(c for c in CASES if c["n"] == 257 and len(c["tab"][0]) == 3)
    n, tab, st0 = c["n"], c["tab"], c["states"]
    rng = np.random.default_rng(21)
    pl = _player(gpu_device, tab, n)
    side = torch.cuda.Stream()
    try:
        # host and device lists; among duplicates the last wins whatever the order of the others; instances >= n are ignored
        last = np.array([(7, 2, 3.0, 0.25), (200, 1, 4.0, 0.0)], dtype=pm.CMD)
        for rnd in range(4):
            others = pm.make_cmds(rng, n, 3, 300, [(7, 0, 9.0, 0.0), (7, 1, 1.0, 0.5), (200, 0, 2.0, 0.1), (n, 1, 1.0, 0.0)])
            cm = np.concatenate([others[rng.permutation(len(others))], last])
            want = pm.advance(st0, pm.DT, tab, cm, 2)
            assert pm.same_bits(want[0][[7, 200]], pm.advance(st0, pm.DT, tab, last)[0][[7, 200]]).all()
            got_h = pl.advance_host(st0, pm.DT, cm, nlayers=2)
            t_st, t_os = _dev(st0), _dev(np.zeros((n, 2), dtype=pm.STEP))
            pl.advance(t_st, pm.DT, _dev(cm) if rnd % 2 else cm, out_steps=t_os.view(n, 2, 16))
            torch.cuda.synchronize()
            for got, ref, name in zip(got_h, want, ("states", "out_states", "out_layers", "out_steps")):
                _same(got, ref, f"round {rnd} host hook {name}")
            _same(_host(t_st, pm.PLAY), want[0], f"round {rnd} device states")
            _same(_host(t_os, pm.STEP, (n, 2)), want[3], f"round {rnd} device steps")
        # a call without commands right after one with commands, then one whose commands have SMALLER indices than the first
        # call's: anything left in the scratch array would win or swallow them.  No wait in between.
        big = pm.make_cmds(rng, n, 3, 500, [(i, 1, 2.0, 0.5) for i in range(n)])
        small = np.array([(i, 2, 1.0, 0.0) for i in range(0, n, 2)], dtype=pm.CMD)
        st, ref = st0, []
        for cm in (big, None, small, None):
            st = pm.advance(st, pm.DT, tab, cm)[0]
            ref.append(st)
        t_st = _dev(st0)
        t_big, t_junk = _dev(big), _dev(pm.make_cmds(rng, n, 3, len(big), []))
        t_cm = t_junk.clone()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(2_000_000)
            t_cm.copy_(t_big)
            pl.advance(t_st, pm.DT, t_cm, stream=side)
            t_cm.copy_(t_junk)  # the device command buffer is overwritten by later stream work without effect
            pl.advance(t_st, pm.DT, None, stream=side)
            pl.advance(t_st, pm.DT, small, stream=side)
            small_copy = small.copy()
            small["clip"], small["x"] = 0, 9.0  # host commands were copied before the call returned
            pl.advance(t_st, pm.DT, None, stream=side)
        side.synchronize()
        _same(_host(t_st, pm.PLAY), ref[3], "four calls in a row")
        assert not pm.same_bits(ref[3], pm.advance(pm.advance(ref[1], pm.DT, tab, small)[0], pm.DT, tab)[0]).all(), "the overwritten list would show"
        # and a different stream takes over the same player: ordered behind the calls before
        other = torch.cuda.Stream()
        t2 = _dev(st0)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(2_000_000)
            pl.advance(t_st, pm.DT, small_copy, stream=side)
        pl.advance(t2, pm.DT, last, stream=other)
        torch.cuda.synchronize()
        _same(_host(t2, pm.PLAY), pm.advance(st0, pm.DT, tab, last)[0], "a second stream")
        _same(_host(t_st, pm.PLAY), pm.advance(ref[3], pm.DT, tab, small_copy)[0], "the first stream")
    finally:
        pl.close()


# ---- 3. end to end: forty frames with nothing uploaded in between ------------------------------------------------------------------
def test_forty_frames_walk_fade_cut_and_stop(gpu_device):
    import torch
    W, H, n, J = 160, 96, 65, 64
    md, mf, m, rng, _, _ = _setup(gpu_device, "uniform", rows=2, cols=3)
    clips = anm.gentle_clips(rng, J, shape=[(30, anm.CLIP_LOOP), (20, anm.CLIP_LOOP), (12, 0)])
    traj = rm.walk_clip(31, 1) + rm.walk_clip(21, 1) + rm.walk_clip(12, 1)
    rflags = np.array([rm.CYCLIC, rm.CYCLIC, 0], dtype=np.uint32)
    tab = pm.table([30, 20, 12], [pm.LOOP, pm.LOOP, 0], [30.0, 24.0, 45.0])
    anim, tset, root = api.Anim(gpu_device, J, clips), api.Anim(gpu_device, 1, traj), api.AnimRoot(gpu_device, 1, 3, 0, rflags)
    pl = _player(gpu_device, tab, n)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats, _ = scene.instance_lattice(9, 8, seed=300)
    mats = np.ascontiguousarray(mats[:n])
    b = api.Batch(gpu_device, m, mats)
    rider = api.Batch(gpu_device, m, am.trs(rng, 7))
    recs = am.records(rng, 7, n, J)
    try:
        st = np.zeros(n, dtype=pm.PLAY)
        st["x_a"] = rng.uniform(0, 30, n)
        st["speed"] = rng.uniform(0.5, 1.5, n)
        st["speed"][[11, 40]] *= -1
        st["flags"] = rng.integers(0, 1 << 31, n) * 2
        third = np.arange(0, n, 3)
        cmds = {5: np.array([(i, 1, 0.5, 0.3) for i in third], dtype=pm.CMD), 12: np.array([(i, 0, 2.0, 0.0) for i in third + 1], dtype=pm.CMD),
                20: np.array([(i, 2, 0.0, 0.1) for i in third], dtype=pm.CMD)}
        t_st, t_ly, t_sp = _dev(st), _dev(np.zeros((n, 2), dtype=pm.LAYER)).view(n, 2, 16), _dev(np.zeros((n, 2), dtype=pm.STEP)).view(n, 2, 16)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        M, ended_seen, fading_seen = mats, False, False
        for frame in range(1, 41):
            pl.advance(t_st, pm.DT, cmds.get(frame), out_layers=t_ly, out_steps=t_sp, stream=side)
            with torch.cuda.stream(side):
                b.animate_layers(anim, t_ly)
                b.root_motion_device(tset, root, t_sp, stream=side)
            st, _, ly, sp = pm.advance(st, pm.DT, tab, cmds.get(frame), 2)
            M = rm.root_motion(M, traj, (0, rflags), sp.astype(rm.STEP))
            fading_seen |= bool(((ly["w"][:, 1] > 0) & (ly["w"][:, 1] < 1)).any())
            if frame in (1, 6, 13, 25, 40):
                pals = anm.palettes(mf, lm.sample(clips, ly.astype(lm.LAYER), J, None))
                assert _bits_equal(b.read_palettes(), pals), f"frame {frame}: palettes"
                assert pm.same_bits(b.read_model_mats(), M).all(), f"frame {frame}: instance matrices"
                _same(_host(t_st, pm.PLAY), st, f"frame {frame}: states")
        # the one-shot clip has stopped at its end where it was started, the others still walk
        assert ((st["flags"][third] & 1) == 1).all() and (st["clip_a"][third] == 2).all() and (st["x_a"][third] == 11).all()
        assert ((st["flags"][third + 1] & 1) == 0).all() and fading_seen and np.isfinite(M).all()
        # a rider attached after the root call follows, and the last frame renders like the oracle from those palettes and matrices
        rider.attach(b, recs)
        assert pm.same_bits(rider.read_model_mats(), am.attach(M, pals, recs)).all(), "the rider"
        ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=M, palettes=pals)])
        assert_same(_render(gpu_device, W, H, lambda fr: fr.draw_batch(b, vp)), ref, "the last frame")
    finally:
        for h in (rider, b, pl, root, tset, anim, m):
            h.close()


# ---- 4. lifetime, and invalid calls ---------------------------------------------------------------------------------------------
def test_player_destroyed_right_after_the_last_advance(gpu_device):
    import torch
    c = next(c for c in CASES if c["n"] == 257 and len(c["tab"][0]) == 3)
    want = pm.run_case(c)
    side = torch.cuda.Stream()
    for rnd in range(3):
        pl = _player(gpu_device, c["tab"], 257)
        t_st, t_os = _dev(c["states"]), _dev(np.zeros((257, 2), dtype=pm.STEP))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)
        for dt, cm in c["calls"]:
            pl.advance(t_st, dt, cm if len(cm) else None, out_steps=t_os.view(257, 2, 16), stream=side)
        pl.close()  # no host wait: the table, the scratch array and the staged commands are parked behind the kernels
        side.synchronize()
        _same(_host(t_st, pm.PLAY), want[2][0], f"round {rnd} states")
        _same(_host(t_os, pm.STEP, (257, 2)), want[2][3], f"round {rnd} steps")


def test_invalid_calls_change_nothing(gpu_device):
    import torch
    c = next(c for c in CASES if c["n"] == 65 and len(c["tab"][0]) == 3)
    n, tab = 65, c["tab"]
    pl = _player(gpu_device, tab, n)
    L, inv, h = api.lib, api.MTR_E_INVALID, C.c_void_p()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    d = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    try:
        nk, fl, rt = np.array([30, 2], dtype=np.uint32), np.array([1, 0], dtype=np.uint32), np.array([30.0, 1.0], dtype=np.float32)
        create = lambda *a: L.mtr_anim_player_create(gpu_device._h, *a, C.byref(h))
        assert create(0, p(nk), p(fl), p(rt), 8) == inv and not h
        assert create(2, p(np.array([30, 0], dtype=np.uint32)), p(fl), p(rt), 8) == inv and b"clip 1" in L.mtr_last_error(gpu_device._h)
        assert create(2, p(np.array([(1 << 24) + 1, 2], dtype=np.uint32)), p(fl), p(rt), 8) == inv and b"clip 0" in L.mtr_last_error(gpu_device._h)
        assert create(2, p(nk), p(np.array([1, 2], dtype=np.uint32)), p(rt), 8) == inv and b"clip 1" in L.mtr_last_error(gpu_device._h)
        for bad in (np.inf, -np.inf, np.nan):
            assert create(2, p(nk), p(fl), p(np.array([30.0, bad], dtype=np.float32)), 8) == inv and b"clip 1" in L.mtr_last_error(gpu_device._h)
        assert create(2, p(nk), p(fl), p(rt), 0) == inv and create(2, p(nk), p(fl), p(rt), (1 << 27) + 1) == inv and not h
        assert create(2, None, p(fl), p(rt), 8) == inv and create(2, p(nk), p(fl), None, 8) == inv
        assert L.mtr_anim_player_create(gpu_device._h, 2, p(nk), p(fl), p(rt), 8, None) == inv
        assert L.mtr_anim_player_create(None, 2, p(nk), p(fl), p(rt), 8, C.byref(h)) == inv
        t_st = _dev(c["states"])
        pad = torch.zeros(n * 64 + 32, dtype=torch.uint8, device="cuda:0")
        t_oa, t_ol, t_os = torch.zeros(n * 24 + 16, dtype=torch.uint8, device="cuda:0"), torch.zeros(n * 8 * 16 + 16, dtype=torch.uint8, device="cuda:0"), torch.zeros(n * 32 + 16, dtype=torch.uint8, device="cuda:0")
        cm = np.array([(0, 1, 1.0, 0.0)], dtype=pm.CMD)
        t_cm = _dev(np.concatenate([cm, cm]))
        for fn in (L.mtr_anim_player_advance_device, L.mtr_anim_player_advance_device_cmds):
            dev_cm = fn is L.mtr_anim_player_advance_device_cmds
            cp = d(t_cm) if dev_cm else p(cm)
            call = lambda pl_=pl._h, st=d(t_st), n_=n, cmds=cp, m=1, oa=d(t_oa), ol=d(t_ol), nl=8, os_=d(t_os): fn(pl_, st, n_, pm.DT, cmds, m, oa, ol, nl, os_, None)
            assert call(pl_=None) == inv and call(st=None) == inv and call(n_=0) == inv and call(n_=n + 1) == inv
            assert call(nl=1) == inv and call(nl=9) == inv and call(cmds=None) == inv
            assert call(st=d(pad, 8)) == inv and call(ol=d(t_ol, 8)) == inv and call(os_=d(t_os, 8)) == inv and call(oa=d(t_oa, 4)) == inv
            if dev_cm:
                assert call(cmds=d(t_cm, 8)) == inv
        hs = c["states"].copy()
        assert L.mtr_anim_player_advance_host(pl._h, None, n, pm.DT, None, 0, None, None, 0, None) == inv
        assert L.mtr_anim_player_advance_host(pl._h, p(hs), n + 1, pm.DT, None, 0, None, None, 0, None) == inv
        assert L.mtr_anim_player_advance_host(pl._h, p(hs), n, pm.DT, None, 3, None, None, 0, None) == inv
        for fn in (lambda: pl.advance(t_st[:, :31], pm.DT), lambda: pl.advance(t_st, pm.DT, out_steps=t_os[:n * 16]), lambda: pl.advance(t_st.cpu(), pm.DT),
                   lambda: pl.advance(t_st, pm.DT, cmds=np.zeros(2, dtype=pm.STEP)), lambda: api.AnimPlayer(gpu_device, [30, 2], [1.0]),
                   lambda: pl.advance(t_st, pm.DT, out_states=t_oa[4:4 + n * 24])):
            with pytest.raises(api.MtrError) as e:
                fn()
            assert e.value.code == inv
        torch.cuda.synchronize()
        _same(_host(t_st, pm.PLAY), c["states"], "the states are untouched")
        assert _bits_equal(hs, c["states"]) and not t_oa.any().item() and not t_ol.any().item() and not t_os.any().item(), "nothing was written"
        # the valid call, for contrast: the scratch array is still clean
        dt, cm0 = c["calls"][0]
        pl.advance(t_st, dt, cm0)
        torch.cuda.synchronize()
        _same(_host(t_st, pm.PLAY), pm.advance(c["states"], dt, tab, cm0)[0], "after invalid calls")
    finally:
        pl.close()


def _raises_saying(cases):
    """each call raises MtrError MTR_E_INVALID with exactly the given text: the binding's own argument checks, before any kernel"""
    for k, (fn, text) in enumerate(cases):
        with pytest.raises(api.MtrError) as e:
            fn()
        assert e.value.code == api.MTR_E_INVALID and str(e.value) == f"mtr error {api.MTR_E_INVALID}: {text}", (k, str(e.value))


def test_argument_errors_of_advance_read_as_before(gpu_device):
    import torch
    n = 3
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device="cuda:0")
    st = u8(n * 32)
    pl = api.AnimPlayer(gpu_device, [30, 2], [30.0, 1.0], [1, 0], max_instances=n)
    try:
        _raises_saying([
            (lambda: pl.advance(st.double(), 0.1), "player states: a uint8 / int32 / float32 tensor on the GPU"),
            (lambda: pl.advance(st.cpu(), 0.1), "player states: a uint8 / int32 / float32 tensor on the GPU"),
            (lambda: pl.advance(u8(n * 32 + 16)[8:8 + n * 32], 0.1), "player states: contiguous and 16-byte aligned (it is used in place)"),
            (lambda: pl.advance(u8(n * 64).view(n, 64)[:, :32], 0.1), "player states: contiguous and 16-byte aligned (it is used in place)"),
            (lambda: pl.advance(u8(n * 32 + 1), 0.1), "player states: records of 32 bytes"),
            (lambda: pl.advance(st, 0.1, out_states=u8((n + 1) * 24)), "player out_states: records of 24 bytes, 3 of them"),
            (lambda: pl.advance(st, 0.1, out_states=u8(n * 24 + 8)[4:4 + n * 24]), "player out_states: contiguous and 8-byte aligned (it is used in place)"),
            (lambda: pl.advance(st, 0.1, out_layers=u8((2 * n + 1) * 16)), "player out_layers: n x L layers of 16 bytes"),
            (lambda: pl.advance(st, 0.1, out_layers=u8(n * 2 * 16).double()), "player out_layers: a uint8 / int32 / float32 tensor on the GPU"),
            (lambda: pl.advance(st, 0.1, out_steps=u8(n * 16)), "player out_steps: records of 16 bytes, 6 of them"),
            (lambda: pl.advance(st, 0.1, cmds=u8(24)), "player commands: records of 16 bytes"),
            (lambda: pl.advance(st, 0.1, cmds=u8(48)[8:40]), "player commands: contiguous and 16-byte aligned (it is used in place)"),
            # the first check that fails speaks: the states before the outputs, an output before the commands
            (lambda: pl.advance(u8(n * 32 + 1), 0.1, out_states=u8(1), cmds=u8(24)), "player states: records of 32 bytes"),
            (lambda: pl.advance(st, 0.1, out_steps=u8(n * 16), cmds=u8(24)), "player out_steps: records of 16 bytes, 6 of them"),
            (lambda: api.AnimPlayer(gpu_device, [30, 2], [1.0]), "anim player: one key count, one rate and one flag word per clip"),
            (lambda: api.AnimPlayer(gpu_device, [30, 2], [1.0, 1.0], [1]), "anim player: one key count, one rate and one flag word per clip"),
        ])
        torch.cuda.synchronize()
        assert not st.any().item(), "nothing ran"
    finally:
        pl.close()
        pl.close()  # a second close does nothing
