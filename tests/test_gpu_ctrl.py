"""GPU: controllers (SPEC.md section 21).  k_ctrl equals the binary32 numpy model (tests/ctrl_model.py) bit for bit on every case
of the generator -- one step through the host hook and three consecutive device steps chained with real AnimPlayer advances, in
the states, the parameters after CONSUME, all n command slots and the counts, on the current stream and a side stream, counts
given and NULL, 1 to 257 instances; 40 frames of step -> advance -> animate_layers -> root_motion for 64 instances of the
locomotion graph on a side stream with nothing uploaded in between, nodes, play states, palettes and matrices equal to the
chained models and the last frame bit-exact against the oracle; a host command appended behind slot n - 1 overrules the
controller's; the controller destroyed right after its last step; invalid calls change nothing."""
import ctypes as C

import numpy as np
import pytest

from mt_renderer_amd import anim_ctrl, api, scene
from tests import anim_layers_model as lm
from tests import anim_model as anm
from tests import ctrl_model as cm
from tests import player_model as pm
from tests import root_model as rm
from tests.helpers import assert_same, render_oracle
from tests.test_gpu_anim import _bits_equal, _render
from tests.test_gpu_anim_layers import _setup
from tests.test_gpu_player import _dev, _host, _player, _same

pytestmark = pytest.mark.gpu

CASES = cm.cases()
F = np.float32


def _ctrl(dev, tab, g):
    return api.AnimCtrl(dev, tab[0], tab[1], g["nodes"], g["trans"], g["nany"], g["nparams"])


def _params(pr):
    """float32 [n, NP] on the GPU, or None when the controller has no parameters"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(pr, dtype=F).copy()).to("cuda:0") if pr.shape[1] else None


def _junk_cmds(n, extra=0):
    return _dev(np.frombuffer(bytes([0x5A]) * ((n + extra) * 16), dtype=pm.CMD))


# ---- 1. bit for bit against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", cm.COUNTS)
def test_states_params_commands_and_counts_are_bit_exact(gpu_device, n):
    import torch
    assert (api.CTRL_NODE, api.CTRL_TRANS, api.CTRL_STATE) == (cm.NODE, cm.TRANS, cm.STATE)
    side = torch.cuda.Stream()
    nan_seen = fired = 0
    for k, c in enumerate(c for c in CASES if c["n"] == n):
        g, tab, T = c["graph"], c["tab"], len(c["graph"]["trans"])
        want = cm.run_case(c)
        ct, pl = _ctrl(gpu_device, tab, g), _player(gpu_device, tab, n)
        try:
            # one step through the host hook
            st, pr, cmds, cnt = ct.step_host(c["states"], c["play"], c["params"], c["dts"][0], counts=np.zeros(T, dtype=np.uint32) if T else None)
            _same(st, want[0][0], f"{c['name']} host hook: states")
            _same(cmds, want[0][2], f"{c['name']} host hook: commands")
            if g["nparams"]:
                _same(pr, want[0][1], f"{c['name']} host hook: params")
            if T:
                assert (cnt == want[0][3]).all(), f"{c['name']} host hook: counts"
            # three consecutive device steps, each consumed by a real advance, on the current stream or on a side stream,
            # counts given or NULL
            t_st, t_pl, t_pr, t_cm = _dev(c["states"]), _dev(c["play"]), _params(c["params"]), _junk_cmds(n)
            t_ct = torch.zeros(T, dtype=torch.int32, device="cuda:0") if T and (k // 2) % 2 == 0 else None
            torch.cuda.synchronize()
            s = side if k % 2 else torch.cuda.current_stream()
            for i, dt in enumerate(c["dts"]):
                ct.step(t_st, t_pl, t_pr, dt, t_cm, counts=t_ct, stream=s)
                pl.advance(t_pl, dt, t_cm, stream=s)
                s.synchronize()
                _same(_host(t_st, cm.STATE), want[i][0], f"{c['name']} step {i}: states")
                _same(_host(t_cm, pm.CMD), want[i][2], f"{c['name']} step {i}: commands")
                if t_pr is not None:
                    _same(t_pr.cpu().numpy(), want[i][1], f"{c['name']} step {i}: params")
                if t_ct is not None:
                    assert (t_ct.cpu().numpy().view(np.uint32) == want[i][3]).all(), f"{c['name']} step {i}: counts"
                _same(_host(t_pl, pm.PLAY), want[i][4], f"{c['name']} step {i}: play states after the advance")
            nan_seen += int(np.isnan(want[2][0]["t"]).any() or any(np.isnan(w[2]["x"]).any() for w in want))
            fired += sum(int((w[0]["fired"] != cm.NONE).sum()) for w in want)
        finally:
            ct.close()
            pl.close()
    assert nan_seen or n < 63, "the special values reach the comparison"
    assert fired, "no transition fires at this size"


def _crowd(n):
    """the start of the forty frames: play states, controller states, parameters (speed, trigger) and what is added to each
    speed every frame -- speeds rise or fall by a constant (a device-side add: nothing is uploaded), triggers are set once"""
    rng = np.random.default_rng(2121)
    play = np.zeros(n, dtype=pm.PLAY)
    play["x_a"] = rng.uniform(0, 30, n)
    play["speed"] = rng.uniform(0.75, 1.25, n)
    st = np.zeros(n, dtype=cm.STATE)
    st["user"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    params = np.zeros((n, 2), dtype=F)
    params[:, cm.SPEED] = rng.uniform(0, 3, n)
    params[::7, cm.TRIGGER] = 1.0
    slope = np.where(np.arange(n) % 2 == 0, F(0.0625), F(-0.0625)).astype(F)
    return play, st, params, slope


# ---- 2. end to end: forty frames with nothing uploaded in between ------------------------------------------------------------------
def test_forty_frames_of_a_crowd_that_decides(gpu_device):
    import torch
    W, H, n, J = 160, 96, 64, 64
    md, mf, m, rng, _, _ = _setup(gpu_device, "uniform", rows=2, cols=3)
    tab = cm.LOCO_TAB
    clips = anm.gentle_clips(rng, J, shape=[(30, anm.CLIP_LOOP), (32, anm.CLIP_LOOP), (16, anm.CLIP_LOOP), (12, 0)])
    traj = rm.walk_clip(31, 1) + rm.walk_clip(33, 1) + rm.walk_clip(17, 1) + rm.walk_clip(12, 1)
    rflags = np.array([rm.CYCLIC, rm.CYCLIC, rm.CYCLIC, 0], dtype=np.uint32)
    # the graph through the readable description: the tables of the model's locomotion graph
    names = [dict(name="idle", clip=0), dict(name="walk", clip=1), dict(name="run", clip=2), dict(name="jump", clip=3)]
    g = anim_ctrl.build(names, [
        dict(src="any", dst="jump", when=[("trigger", ">", 0.5)], flags=("interrupt", "consume")),
        dict(src="idle", dst="walk", when=[("speed", ">", 0.6)], seconds=0.2),
        dict(src="walk", dst="idle", when=[("speed", "<", 0.4)], seconds=0.2),
        dict(src="walk", dst="run", when=[("speed", ">", 2.2)], seconds=0.2, flags=("sync",)),
        dict(src="run", dst="walk", when=[("speed", "<", 1.8)], seconds=0.2, flags=("sync",)),
        dict(src="jump", dst="idle", when=[("ENDED", ">=", 1.0)], seconds=0.1)], params=["speed", "trigger"])
    gm = cm.locomotion()
    assert g["trans"].tobytes() == gm["trans"].tobytes() and g["nodes"].tobytes() == gm["nodes"].tobytes()
    anim, tset, root = api.Anim(gpu_device, J, clips), api.Anim(gpu_device, 1, traj), api.AnimRoot(gpu_device, 1, 4, 0, rflags)
    pl, ct = _player(gpu_device, tab, n), api.AnimCtrl(gpu_device, tab[0], tab[1], g["nodes"], g["trans"], g["nany"], len(g["params"]))
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats, _ = scene.instance_lattice(9, 8, seed=300)
    mats = np.ascontiguousarray(mats[:n])
    b = api.Batch(gpu_device, m, mats)
    try:
        play, st, params, slope = _crowd(n)
        counts = np.zeros(len(gm["trans"]), dtype=np.uint32)
        t_st, t_pl, t_pr, t_cm = _dev(st), _dev(play), _params(params), _junk_cmds(n)
        t_slope = torch.from_numpy(slope).to("cuda:0")
        t_ct = torch.zeros(len(counts), dtype=torch.int32, device="cuda:0")
        t_ly, t_sp = _dev(np.zeros((n, 2), dtype=pm.LAYER)).view(n, 2, 16), _dev(np.zeros((n, 2), dtype=pm.STEP)).view(n, 2, 16)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        M, fading_seen = mats, False
        for frame in range(1, 41):
            with torch.cuda.stream(side):
                t_pr[:, cm.SPEED] += t_slope
            ct.step(t_st, t_pl, t_pr, pm.DT, t_cm, counts=t_ct, stream=side)
            pl.advance(t_pl, pm.DT, t_cm, out_layers=t_ly, out_steps=t_sp, stream=side)
            with torch.cuda.stream(side):
                b.animate_layers(anim, t_ly)
                b.root_motion_device(tset, root, t_sp, stream=side)
            params[:, cm.SPEED] = params[:, cm.SPEED] + slope
            st, params, cmds, counts = cm.step(gm, tab, st, play, params, pm.DT, counts)
            play, _, ly, sp = pm.advance(play, pm.DT, tab, cmds, 2)
            M = rm.root_motion(M, traj, (0, rflags), sp.astype(rm.STEP))
            fading_seen |= bool(((ly["w"][:, 1] > 0) & (ly["w"][:, 1] < 1)).any())
            side.synchronize()
            _same(_host(t_st, cm.STATE), st, f"frame {frame}: controller states")  # 16 bytes each: the frame that goes wrong is named
            if frame in (1, 2, 9, 17, 28, 40):
                pals = anm.palettes(mf, lm.sample(clips, ly.astype(lm.LAYER), J, None))
                _same(_host(t_pl, pm.PLAY), play, f"frame {frame}: play states")
                _same(t_pr.cpu().numpy(), params, f"frame {frame}: params")
                assert _bits_equal(b.read_palettes(), pals), f"frame {frame}: palettes"
                assert pm.same_bits(b.read_model_mats(), M).all(), f"frame {frame}: instance matrices"
        assert (t_ct.cpu().numpy().view(np.uint32) == counts).all() and counts[0] == len(params[::7]) and (counts > 0).all(), counts
        assert fading_seen and np.isfinite(M).all() and len(set(st["node"])) >= 3 and (params[:, cm.TRIGGER] == 0).all()
        # the last frame renders like the oracle from those palettes and matrices
        ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=M, palettes=pals)])
        assert_same(_render(gpu_device, W, H, lambda fr: fr.draw_batch(b, vp)), ref, "the last frame")
    finally:
        for h in (b, ct, pl, root, tset, anim, m):
            h.close()


# ---- 3. the host overrules ---------------------------------------------------------------------------------------------------------
def test_a_host_command_behind_slot_n_minus_1_overrules(gpu_device):
    import torch
    c = next(c for c in CASES if c["n"] == 257 and c["graph"]["nany"] == 2 and c["graph"]["nparams"] == 5)
    n, g, tab, dt = c["n"], c["graph"], c["tab"], c["dts"][0]
    st, pr, cmds, _ = cm.step(g, tab, c["states"], c["play"], c["params"], dt)
    firing, quiet = np.flatnonzero(st["fired"] != cm.NONE), np.flatnonzero(st["fired"] == cm.NONE)
    assert len(firing) >= 2 and len(quiet) >= 1
    host = np.array([(firing[0], 0, 3.0, 0.0), (quiet[0], len(tab[0]) - 1, 1.0, 0.25), (firing[-1], 0, 2.0, 0.5)], dtype=pm.CMD)
    want = pm.advance(c["play"], dt, tab, np.concatenate([cmds, host]))[0]
    assert not pm.same_bits(want, pm.advance(c["play"], dt, tab, cmds)[0]).all(), "the host's commands would show"
    ct, pl = _ctrl(gpu_device, tab, g), _player(gpu_device, tab, n)
    try:
        t_st, t_pl, t_pr, t_cm = _dev(c["states"]), _dev(c["play"]), _params(c["params"]), _junk_cmds(n, len(host))
        t_cm[n:] = _dev(host)  # written once, behind the controller's slots; the step leaves them alone
        torch.cuda.synchronize()
        ct.step(t_st, t_pl, t_pr, dt, t_cm)
        pl.advance(t_pl, dt, t_cm)
        torch.cuda.synchronize()
        _same(_host(t_cm, pm.CMD), np.concatenate([cmds, host]), "the list")
        _same(_host(t_pl, pm.PLAY), want, "play states")
        _same(_host(t_st, cm.STATE), st, "controller states")
    finally:
        ct.close()
        pl.close()


# ---- 4. lifetime, and invalid calls ---------------------------------------------------------------------------------------------
def test_controller_destroyed_right_after_the_last_step(gpu_device):
    import torch
    c = next(c for c in CASES if c["n"] == 257 and c["graph"]["nany"] == 2 and c["graph"]["nparams"] == 16)
    n, g, tab = c["n"], c["graph"], c["tab"]
    st, pr, cmds = c["states"], c["params"], None
    for dt in c["dts"]:  # three steps against the same play states
        st, pr, cmds, _ = cm.step(g, tab, st, c["play"], pr, dt)
    side = torch.cuda.Stream()
    for rnd in range(3):
        ct = _ctrl(gpu_device, tab, g)
        t_st, t_pl, t_pr, t_cm = _dev(c["states"]), _dev(c["play"]), _params(c["params"]), _junk_cmds(n)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)
        for dt in c["dts"]:
            ct.step(t_st, t_pl, t_pr, dt, t_cm, stream=side)
        ct.close()  # no host wait: the tables are parked behind the kernels
        side.synchronize()
        _same(_host(t_st, cm.STATE), st, f"round {rnd} states")
        _same(_host(t_cm, pm.CMD), cmds, f"round {rnd} commands")
        _same(t_pr.cpu().numpy(), pr, f"round {rnd} params")


def test_one_graph_for_crowds_on_two_streams_destroyed_right_after(gpu_device):
    """one controller steps a crowd on a stalled side stream and then another on the current stream; destroyed at once, its
    tables are parked behind BOTH steps (the second stream waited for the controller's event), so a frame that collects the
    garbage and a fresh controller that may take the memory change nothing the first crowd's steps read"""
    import torch
    c = next(c for c in CASES if c["n"] == 257 and c["graph"]["nany"] == 2 and c["graph"]["nparams"] == 16)
    n, g, tab = c["n"], c["graph"], c["tab"]
    st, pr, cmds = c["states"], c["params"], None
    for dt in c["dts"]:
        st, pr, cmds, _ = cm.step(g, tab, st, c["play"], pr, dt)
    st1, _, cmds1, _ = cm.step(g, tab, c["states"], c["play"], c["params"], c["dts"][0])
    side = torch.cuda.Stream()
    ct = _ctrl(gpu_device, tab, g)
    a_st, a_pl, a_pr, a_cm = _dev(c["states"]), _dev(c["play"]), _params(c["params"]), _junk_cmds(n)
    b_st, b_pl, b_pr, b_cm = _dev(c["states"]), _dev(c["play"]), _params(c["params"]), _junk_cmds(n)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
    for dt in c["dts"]:
        ct.step(a_st, a_pl, a_pr, dt, a_cm, stream=side)
    ct.step(b_st, b_pl, b_pr, c["dts"][0], b_cm)
    ct.close()
    _render(gpu_device, 32, 32, lambda fr: None)  # a submit collects what is parked and done
    other = _ctrl(gpu_device, tab, next(x for x in CASES if x["n"] == 257 and x["graph"]["nany"] == 0 and x["graph"]["nparams"] == 16)["graph"])
    torch.cuda.synchronize()
    other.close()
    _same(_host(a_st, cm.STATE), st, "the side stream's crowd: states")
    _same(_host(a_cm, pm.CMD), cmds, "the side stream's crowd: commands")
    _same(_host(b_st, cm.STATE), st1, "the current stream's crowd: states")
    _same(_host(b_cm, pm.CMD), cmds1, "the current stream's crowd: commands")


def test_invalid_calls_change_nothing(gpu_device):
    import torch
    c = next(c for c in CASES if c["n"] == 65 and c["graph"]["nany"] == 2 and c["graph"]["nparams"] == 5)
    n, g, tab = 65, c["graph"], c["tab"]
    T, S, Cn = len(g["trans"]), len(g["nodes"]), len(tab[0])
    ct = _ctrl(gpu_device, tab, g)
    L, inv, h = api.lib, api.MTR_E_INVALID, C.c_void_p()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    d = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    err = lambda: L.mtr_last_error(gpu_device._h)
    try:
        nk, fl = np.asarray(tab[0], dtype=np.uint32), np.asarray(tab[1], dtype=np.uint32)
        nd, tr = g["nodes"], g["trans"]
        create = lambda nclips=Cn, nk_=nk, fl_=fl, nd_=nd, S_=S, tr_=tr, T_=T, nany=2, NP=5: L.mtr_anim_ctrl_create(
            gpu_device._h, nclips, p(nk_), p(fl_), p(nd_), S_, p(tr_), T_, nany, NP, C.byref(h))
        assert create(nclips=0) == inv and create(S_=0) == inv and create(S_=65536) == inv and create(T_=(1 << 20) + 1) == inv and not h
        assert create(nany=T + 1) == inv and create(NP=17) == inv and not h
        bad = nk.copy(); bad[Cn - 1] = 0
        assert create(nk_=bad) == inv and f"clip {Cn - 1} ".encode() in err()
        bad = fl.copy(); bad[0] |= 4
        assert create(fl_=bad) == inv and b"clip 0 " in err()
        for field, value in (("clip", Cn), ("first", T + 1), ("count", T), ("first", 1)):
            bad = nd.copy(); bad[field][2] = value
            assert create(nd_=bad) == inv and b"node 2 " in err(), (field, value)
        bad = nd.copy(); bad["first"][3], bad["count"][3] = 3, 0xFFFFFFFE  # the sum wraps
        assert create(nd_=bad) == inv and b"node 3 " in err()
        for field, value in (("target", S), ("flags", 16), ("ncond", 4)):
            bad = tr.copy(); bad[field][T - 1] = value
            assert create(tr_=bad) == inv and f"transition {T - 1} ".encode() in err(), (field, value)
        for field, value in (("op", 6), ("param", 5), ("param", 0xFFFA)):
            bad = tr.copy(); bad["ncond"][3] = 3; bad["cond"]["op"][3] = 0; bad["cond"]["param"][3] = 0; bad["cond"][field][3, 2] = value
            assert create(tr_=bad) == inv and b"transition 3 " in err(), (field, value)
        assert L.mtr_anim_ctrl_create(gpu_device._h, Cn, p(nk), p(fl), p(nd), S, p(tr), T, 2, 5, None) == inv
        assert L.mtr_anim_ctrl_create(None, Cn, p(nk), p(fl), p(nd), S, p(tr), T, 2, 5, C.byref(h)) == inv and not h
        t_st, t_pl, t_pr = _dev(c["states"]), _dev(c["play"]), _params(c["params"])
        t_cm = torch.zeros(n * 16 + 16, dtype=torch.uint8, device="cuda:0")
        t_ct = torch.zeros(T + 1, dtype=torch.int32, device="cuda:0")
        pad = torch.zeros(n * 32 + 32, dtype=torch.uint8, device="cuda:0")
        call = lambda ct_=ct._h, st=d(t_st), pl=d(t_pl), pr=d(t_pr), n_=n, cm_=d(t_cm), cnt=d(t_ct): L.mtr_anim_ctrl_step_device(ct_, st, pl, pr, n_, pm.DT, cm_, cnt, None)
        assert call(ct_=None) == inv and call(st=None) == inv and call(pl=None) == inv and call(cm_=None) == inv and call(pr=None) == inv
        assert call(n_=0) == inv and call(n_=(1 << 27) + 1) == inv
        assert call(st=d(pad, 8)) == inv and call(pl=d(pad, 8)) == inv and call(cm_=d(t_cm, 8)) == inv and call(pr=d(t_pr, 2)) == inv and call(cnt=d(t_ct, 2)) == inv
        hs, hp = c["states"].copy(), c["params"].copy()
        hc = np.zeros(n, dtype=pm.CMD)
        assert L.mtr_anim_ctrl_step_host(ct._h, None, p(c["play"]), p(hp), n, pm.DT, p(hc), None) == inv
        assert L.mtr_anim_ctrl_step_host(ct._h, p(hs), None, p(hp), n, pm.DT, p(hc), None) == inv
        assert L.mtr_anim_ctrl_step_host(ct._h, p(hs), p(c["play"]), None, n, pm.DT, p(hc), None) == inv
        assert L.mtr_anim_ctrl_step_host(ct._h, p(hs), p(c["play"]), p(hp), n, pm.DT, None, None) == inv
        assert L.mtr_anim_ctrl_step_host(ct._h, p(hs), p(c["play"]), p(hp), 0, pm.DT, p(hc), None) == inv
        cm_ok = t_cm[:n * 16]
        for fn in (lambda: ct.step(t_st[:, :15], t_pl, t_pr, pm.DT, cm_ok), lambda: ct.step(t_st, t_pl[:n - 1], t_pr, pm.DT, cm_ok),
                   lambda: ct.step(t_st, t_pl, None, pm.DT, cm_ok), lambda: ct.step(t_st, t_pl, t_pr[:, :4], pm.DT, cm_ok),
                   lambda: ct.step(t_st, t_pl, t_pr, pm.DT, t_cm[:(n - 1) * 16]), lambda: ct.step(t_st.cpu(), t_pl, t_pr, pm.DT, cm_ok),
                   lambda: ct.step(t_st, t_pl, t_pr, pm.DT, cm_ok, counts=t_ct[:T - 1]), lambda: ct.step(t_st, t_pl, t_pr, pm.DT, cm_ok, counts=t_ct.float()),
                   lambda: api.AnimCtrl(gpu_device, tab[0], tab[1], g["nodes"].view(np.uint8), g["trans"]),
                   lambda: ct.step_host(c["states"], c["play"][:3], c["params"], pm.DT)):
            with pytest.raises(api.MtrError) as e:
                fn()
            assert e.value.code == inv
        torch.cuda.synchronize()
        _same(_host(t_st, cm.STATE), c["states"], "the states are untouched")
        _same(_host(t_pl, pm.PLAY), c["play"], "the play states are untouched")
        _same(t_pr.cpu().numpy(), c["params"], "the parameters are untouched")
        assert _bits_equal(hs, c["states"]) and not hc.view(np.uint8).any() and not t_cm.any().item() and not t_ct.any().item(), "nothing was written"
        # the valid call, for contrast
        ct.step(t_st, t_pl, t_pr, c["dts"][0], cm_ok, counts=t_ct)
        torch.cuda.synchronize()
        want = cm.step(g, tab, c["states"], c["play"], c["params"], c["dts"][0], np.zeros(T, dtype=np.uint32))
        _same(_host(t_st, cm.STATE), want[0], "after invalid calls")
        assert (t_ct.cpu().numpy().view(np.uint32)[:T] == want[3]).all() and t_ct[T].item() == 0
    finally:
        ct.close()


def test_argument_errors_of_step_read_as_before(gpu_device):
    import torch
    from tests.test_gpu_player import _raises_saying
    n = 3
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device="cuda:0")
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda:0")
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device="cuda:0")
    nodes, trans = np.zeros(1, dtype=api.CTRL_NODE), np.zeros(2, dtype=api.CTRL_TRANS)
    nodes["count"] = 2
    create_msg = "anim ctrl: one flag word per clip, nodes of dtype CTRL_NODE [S] and transitions of dtype CTRL_TRANS [T]"
    ct = api.AnimCtrl(gpu_device, [30, 2], [1, 0], nodes, trans, nany=0, nparams=2)
    st, pl, pr, cmds = u8(n * 16), u8(n * 32), f32(n, 2), u8(n * 16)
    try:
        _raises_saying([
            (lambda: ct.step(st.double(), pl, pr, 0.1, cmds), "ctrl states: a uint8 / int32 / float32 tensor on the GPU"),
            (lambda: ct.step(u8(n * 16 + 16)[8:8 + n * 16], pl, pr, 0.1, cmds), "ctrl states: contiguous and 16-byte aligned (it is used in place)"),
            (lambda: ct.step(st, u8((n - 1) * 32), pr, 0.1, cmds), "ctrl play states: records of 32 bytes, 3 of them"),
            (lambda: ct.step(st, pl, pr, 0.1, u8((n - 1) * 16)), "ctrl commands: at least n slots of 16 bytes"),
            (lambda: ct.step(st, pl, None, 0.1, cmds), "ctrl params: a float32 tensor [n, nparams] on the GPU"),
            (lambda: ct.step(st, pl, pr.int(), 0.1, cmds), "ctrl params: a float32 tensor [n, nparams] on the GPU"),
            (lambda: ct.step(st, pl, f32(n, 3), 0.1, cmds), "ctrl params: records of 8 bytes, 3 of them"),
            (lambda: ct.step(st, pl, f32(n, 4)[:, :2], 0.1, cmds), "ctrl params: contiguous and 4-byte aligned (it is used in place)"),
            (lambda: ct.step(st, pl, pr, 0.1, cmds, counts=f32(2)), "ctrl counts: an int32 tensor [ntrans] on the GPU"),
            (lambda: ct.step(st, pl, pr, 0.1, cmds, counts=i32(1)), "ctrl counts: one word per transition"),
            (lambda: ct.step(st, pl, pr, 0.1, cmds, counts=i32(4)[::2]), "ctrl counts: contiguous and 4-byte aligned (it is used in place)"),
            # the first check that fails speaks: the commands before the parameters, the parameters before the counts
            (lambda: ct.step(st, pl, None, 0.1, u8((n - 1) * 16), counts=f32(2)), "ctrl commands: at least n slots of 16 bytes"),
            (lambda: ct.step(st, pl, pr.int(), 0.1, cmds, counts=f32(2)), "ctrl params: a float32 tensor [n, nparams] on the GPU"),
            (lambda: api.AnimCtrl(gpu_device, [30, 2], [1], nodes, trans), create_msg),
            (lambda: api.AnimCtrl(gpu_device, [30, 2], [1, 0], nodes.view(np.uint8), trans), create_msg),
        ])
        torch.cuda.synchronize()
        assert not st.any().item() and not cmds.any().item(), "nothing ran"
    finally:
        ct.close()
