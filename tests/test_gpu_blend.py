"""GPU: blend spaces (SPEC.md section 23).  k_blend equals the binary32 numpy model (tests/blend_model.py) bit for bit on every
case of the generator -- one advance through the host hook and three consecutive device advances, in the stored states, the
layers, the steps and the shares, on the current stream and a side stream, each output pointer NULL in turn, 3 to 8 layers per
instance (layers 3.. untouched), the parameters read only, 1 to 257 instances; three frames of blend -> animate_layers ->
root_motion -> collect chained on a side stream with nothing uploaded in between, palettes, instance matrices and event lists
equal to the chained models; the set destroyed right after its last call; invalid calls change nothing."""
import ctypes as C

import numpy as np
import pytest

from mt_renderer_amd import anim_blend, anim_events, api, scene
from tests import anim_layers_model as lm
from tests import anim_model as anm
from tests import blend_model as bm
from tests import events_model as em
from tests import player_model as pm
from tests import root_model as rm
from tests.test_gpu_anim import _bits_equal
from tests.test_gpu_anim_layers import _setup
from tests.test_gpu_player import _dev, _host, _same

pytestmark = pytest.mark.gpu

CASES = bm.cases()
F = np.float32


def _blend(dev, bs, max_instances):
    tab = bs["tab"]
    return api.AnimBlend(dev, tab[0], tab[2], tab[1], bs["samples"], bs["tris"] if bs["tris"].size else None, nparams=bs["nparams"], param_x=bs["param_x"],
                         param_y=bs["param_y"], damp=float(bs["damp"]), max_instances=max_instances)


def _f32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F).copy()).to("cuda:0")


# ---- 1. bit for bit against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", bm.COUNTS)
def test_states_and_outputs_are_bit_exact(gpu_device, n):
    import torch
    assert (api.BLEND_SAMPLE, api.BLEND_TRI, api.BLEND_STATE, api.ANIM_LAYER, api.ROOT_STEP) == (bm.SAMPLE, bm.TRI, bm.STATE, bm.LAYER, bm.STEP)
    side = torch.cuda.Stream()
    nan_seen = False
    for k, c in enumerate(c for c in CASES if c["n"] == n):
        want = bm.run_case(c)
        nl, skip = c["nlayers"], (None, "layers", "steps", "shares")[k % 4]  # each output pointer NULL in turn
        bl = _blend(gpu_device, c["set"], n if k % 2 else n + 3)
        try:
            # one advance through the host hook
            dt, pr = c["calls"][0]
            st, ol, os_, sh = bl.advance_host(c["states"], pr, dt, nlayers=0 if skip == "layers" else nl, layers=c["layers"], want_steps=skip != "steps",
                                              want_shares=skip != "shares")
            _same(st, want[0][0], f"{c['name']} host hook: states")
            for got, ref, name in ((ol, want[0][1], "layers"), (os_, want[0][2], "steps"), (sh, want[0][3], "shares")):
                assert (got is None) == (skip == name)
                if got is not None:
                    _same(got, ref, f"{c['name']} host hook: {name}")
            # three consecutive device advances, on the current stream or on a side stream
            t_st, t_ol, t_os, t_sh = _dev(c["states"]), _dev(c["layers"]), _dev(np.zeros((n, 3), dtype=bm.STEP)), _f32(np.zeros((n, 3)))
            t_pr = [_f32(p) for _, p in c["calls"]]
            torch.cuda.synchronize()
            s = side if k % 2 else torch.cuda.current_stream()
            for i, (dt, pr) in enumerate(c["calls"]):
                bl.advance(t_st, t_pr[i], dt, out_layers=None if skip == "layers" else t_ol.view(n, nl, 16), out_steps=None if skip == "steps" else t_os.view(n, 3, 16),
                           out_shares=None if skip == "shares" else t_sh, stream=s)
                s.synchronize()
                _same(_host(t_st, bm.STATE), want[i][0], f"{c['name']} call {i}: states")
                if skip != "layers":
                    _same(_host(t_ol, bm.LAYER, (n, nl)), want[i][1], f"{c['name']} call {i}: layers")
                if skip != "steps":
                    _same(_host(t_os, bm.STEP, (n, 3)), want[i][2], f"{c['name']} call {i}: steps")
                if skip != "shares":
                    _same(t_sh.cpu().numpy(), want[i][3], f"{c['name']} call {i}: shares")
                assert t_pr[i].cpu().numpy().tobytes() == np.ascontiguousarray(pr, dtype=F).tobytes(), f"{c['name']} call {i}: the parameters are read only"
            if skip == "layers":
                _same(_host(t_ol, bm.LAYER, (n, nl)), c["layers"], f"{c['name']}: layers not asked for")
            elif nl > 3:
                _same(_host(t_ol, bm.LAYER, (n, nl))[:, 3:], c["layers"][:, 3:], f"{c['name']}: layers 3.. untouched")
            nan_seen |= bool(np.isnan(c["calls"][0][1]).any() and np.isnan(c["states"]["phase"]).any())
        finally:
            bl.close()
    assert nan_seen or n < 63, "the special values reach the comparison"


# ---- 2. three frames chained on the device -----------------------------------------------------------------------------------
def test_three_frames_of_a_crowd_that_steers(gpu_device):
    import torch
    n, J, nl = 65, 64, 4
    md, mf, m, rng, _, _ = _setup(gpu_device, "uniform", rows=2, cols=3)
    IDLE, WALK, RUN = 0, 1, 2
    tab = pm.table([30, 32, 16], [pm.LOOP] * 3, [30.0, 32.0, 24.0])
    clips = anm.gentle_clips(rng, J, shape=[(30, anm.CLIP_LOOP), (32, anm.CLIP_LOOP), (16, anm.CLIP_LOOP)])
    traj = rm.walk_clip(31, 1) + rm.walk_clip(33, 1) + rm.walk_clip(17, 1)
    rflags = np.array([rm.CYCLIC] * 3, dtype=np.uint32)
    pts = [(0.0, 0.0, IDLE), (0.0, 1.4, WALK), (0.0, 4.0, RUN), (-1.0, 1.0, WALK), (1.0, 1.0, WALK), (-1.5, 3.0, RUN), (1.5, 3.0, RUN), (0.0, -1.0, WALK)]
    samples, tris = anim_blend.build_2d(pts)
    bs = bm.blend_set(tab, [(c, x, y) for x, y, c in pts], [tuple(int(i) for i in v) for v in tris["v"]], nparams=3, param_x=2, param_y=0, damp=6.0)
    assert bm.check_set(bs) is None and bs["samples"].tobytes() == samples.tobytes() and bs["tris"].tobytes() == tris.tobytes()
    marks = {IDLE: [(15.0, 9)], WALK: [(8.0, 1), (24.0, 2)], RUN: [(4.0, 1), (12.0, 2)]}
    counts, markers = anim_events.build(marks, 3)
    es = em.event_set(tab, marks)
    anim, tset, root = api.Anim(gpu_device, J, clips), api.Anim(gpu_device, 1, traj), api.AnimRoot(gpu_device, 1, 3, 0, rflags)
    bl = _blend(gpu_device, bs, n)
    ev = api.AnimEvents(gpu_device, tab[0], tab[1], counts, markers, max_instances=n)
    mats, _ = scene.instance_lattice(9, 8, seed=300)
    mats = np.ascontiguousarray(mats[:n])
    b = api.Batch(gpu_device, m, mats)
    try:
        r2 = np.random.default_rng(2323)
        st = np.zeros(n, dtype=bm.STATE)
        st["phase"], st["speed"] = r2.uniform(0, 1, n), r2.uniform(0.75, 1.25, n)
        st["px"], st["py"] = r2.uniform(-1.5, 1.5, n), r2.uniform(-1, 4, n)
        st["speed"][::6] *= -1  # some run backward
        params = np.zeros((n, 3), dtype=F)
        params[:, 2], params[:, 0] = r2.uniform(-2.5, 2.5, n), r2.uniform(-2, 5, n)  # in the hull and outside it
        params[:8, 2], params[:8, 0] = [p[0] for p in pts], [p[1] for p in pts]     # at the samples
        st["px"][:8], st["py"][:8] = params[:8, 2], params[:8, 0]
        cap = 3 * n
        sentinel = np.frombuffer(bytes([0x5A]) * (cap * 16), dtype=em.EVENT)
        ly0 = np.zeros((n, nl), dtype=bm.LAYER)  # layer 3 stays at weight 0
        t_st, t_pr = _dev(st), _f32(params)
        t_ly = _dev(ly0).view(n, nl, 16)
        t_sp = _dev(np.zeros((n, 3), dtype=bm.STEP)).view(n, 3, 16)
        t_out = [_dev(sentinel) for _ in range(3)]
        t_ct = [torch.zeros(2, dtype=torch.int32, device="cuda:0") for _ in range(3)]
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        M, ly, want, pals = mats, ly0, [], []
        for f in range(3):
            bl.advance(t_st, t_pr, pm.DT, out_layers=t_ly, out_steps=t_sp, stream=side)
            with torch.cuda.stream(side):
                b.animate_layers(anim, t_ly)
                b.root_motion_device(tset, root, t_sp, stream=side)
            ev.collect(t_sp, 0.0, t_out[f], t_ct[f], stream=side)
            st, ly, sp, _ = bm.advance(bs, st, params, pm.DT, nl, ly)
            want.append(em.collect(es, sp, 0.0, cap, out_prev=sentinel))
            M = rm.root_motion(M, traj, (0, rflags), sp.astype(rm.STEP))
            if f == 2:
                side.synchronize()
                assert _bits_equal(b.read_palettes(), anm.palettes(mf, lm.sample(clips, ly.astype(lm.LAYER), J, None))), "palettes"
        side.synchronize()
        for f in range(3):
            assert (t_ct[f].cpu().numpy().view(np.uint32) == want[f][1]).all(), f"frame {f}: count"
            _same(_host(t_out[f], em.EVENT), want[f][0], f"frame {f}: list")
        assert sum(int(w[1][0]) for w in want) > 0, "markers fired"
        _same(_host(t_st, bm.STATE), st, "blend states")
        _same(_host(t_ly, bm.LAYER, (n, nl)), ly, "layers")
        assert pm.same_bits(b.read_model_mats(), M).all() and np.isfinite(M).all(), "instance matrices"
    finally:
        for h in (b, ev, bl, root, tset, anim, m):
            h.close()


# ---- 3. lifetime ---------------------------------------------------------------------------------------------------------------
def test_set_destroyed_right_after_the_last_call(gpu_device):
    import torch
    c = next(c for c in CASES if c["n"] == 257 and c["set"]["tris"].size > 1)
    want = bm.run_case(c, ncalls=1)[0]
    n, nl = c["n"], c["nlayers"]
    dt, pr = c["calls"][0]
    side = torch.cuda.Stream()
    for rnd in range(3):
        bl = _blend(gpu_device, c["set"], n)
        t_st, t_pr, t_ol, t_os = _dev(c["states"]), _f32(pr), _dev(c["layers"]), _dev(np.zeros((n, 3), dtype=bm.STEP))
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)
        bl.advance(t_st, t_pr, dt, out_layers=t_ol.view(n, nl, 16), out_steps=t_os.view(n, 3, 16), stream=side)
        bl.close()  # no host wait: the tables are parked behind the kernel
        side.synchronize()
        _same(_host(t_st, bm.STATE), want[0], f"round {rnd} states")
        _same(_host(t_ol, bm.LAYER, (n, nl)), want[1], f"round {rnd} layers")
        _same(_host(t_os, bm.STEP, (n, 3)), want[2], f"round {rnd} steps")


# ---- 4. invalid calls ------------------------------------------------------------------------------------------------------------
def test_invalid_calls_change_nothing(gpu_device):
    import torch
    c = next(c for c in CASES if c["n"] == 65 and c["set"]["tris"].size > 1)
    n, bs = 65, c["set"]
    NP, nl = bs["nparams"], 4
    bl = _blend(gpu_device, bs, n)
    L, inv, h = api.lib, api.MTR_E_INVALID, C.c_void_p()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    d = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    err = lambda: L.mtr_last_error(gpu_device._h)
    try:
        nk, fl, rt = np.asarray(bs["tab"][0], dtype=np.uint32), np.asarray(bs["tab"][1], dtype=np.uint32), np.asarray(bs["tab"][2], dtype=F)
        sm, tr = bs["samples"], bs["tris"]
        Cn = nk.size
        create = lambda nclips=Cn, nk_=nk, fl_=fl, rt_=rt, sm_=sm, K=sm.size, tr_=tr, T=tr.size, np_=NP, x=bs["param_x"], y=bs["param_y"], damp=4.0, mi=n: \
            L.mtr_anim_blend_create(gpu_device._h, nclips, p(nk_), p(fl_), p(rt_), p(sm_), K, p(tr_), T, np_, x, y, damp, mi, C.byref(h))
        assert create(nclips=0) == inv and create(K=0) == inv and create(K=33) == inv and create(T=65) == inv and create(np_=0) == inv and create(np_=17) == inv
        assert create(x=NP) == inv and create(y=NP) == inv and create(mi=0) == inv and create(mi=(1 << 27) + 1) == inv and not h
        assert create(damp=0.0) == inv and create(damp=-1.0) == inv and create(damp=float("nan")) == inv and not h
        bad = nk.copy(); bad[Cn - 1] = 0
        assert create(nk_=bad) == inv and f"clip {Cn - 1} ".encode() in err()
        bad = rt.copy(); bad[0] = np.inf
        assert create(rt_=bad) == inv and b"clip 0 " in err()
        bad = fl.copy(); bad[int(sm["clip"][2])] = 0
        assert create(fl_=bad) == inv and b"sample " in err(), "a sample on a clip that is not LOOP"
        bad = sm.copy(); bad["clip"][3] = Cn
        assert create(sm_=bad) == inv and b"sample 3 " in err()
        bad = sm.copy(); bad["py"][1] = np.nan
        assert create(sm_=bad) == inv and b"sample 1 " in err()
        bad = tr.copy(); bad["v"][1] = bad["v"][1][[0, 2, 1]]
        assert create(tr_=bad) == inv and b"triangle 1 " in err(), "a clockwise triangle"
        bad = tr.copy(); bad["v"][0][2] = sm.size
        assert create(tr_=bad) == inv and b"triangle 0 " in err()
        bad = tr.copy(); bad["v"][0][2] = bad["v"][0][0]
        assert create(tr_=bad) == inv and b"triangle 0 " in err()
        assert create(T=0) == inv and b"sample " in err(), "as a 1-D space the samples are not increasing"
        assert L.mtr_anim_blend_create(None, Cn, p(nk), p(fl), p(rt), p(sm), sm.size, p(tr), tr.size, NP, 0, 0, 4.0, n, C.byref(h)) == inv and not h
        t_st = torch.zeros(n * 16 + 16, dtype=torch.uint8, device="cuda:0")
        t_pr = torch.zeros(n * NP + 1, dtype=torch.float32, device="cuda:0")
        t_ly = torch.zeros(n * nl * 16 + 16, dtype=torch.uint8, device="cuda:0")
        t_sp = torch.zeros(n * 48 + 16, dtype=torch.uint8, device="cuda:0")
        t_sh = torch.zeros(n * 3 + 1, dtype=torch.float32, device="cuda:0")
        call = lambda bl_=bl._h, st=d(t_st), pr=d(t_pr), n_=n, ly=d(t_ly), nl_=nl, sp=d(t_sp), sh=d(t_sh): L.mtr_anim_blend_advance_device(
            bl_, st, pr, n_, 0.5, ly, nl_, sp, sh, None)
        assert call(bl_=None) == inv and call(st=None) == inv and call(pr=None) == inv and call(n_=0) == inv and call(n_=n + 1) == inv
        assert call(nl_=2) == inv and call(nl_=9) == inv
        assert call(st=d(t_st, 8)) == inv and call(ly=d(t_ly, 4)) == inv and call(sp=d(t_sp, 8)) == inv and call(pr=d(t_pr, 2)) == inv and call(sh=d(t_sh, 1)) == inv
        hs, hp = np.zeros(n, dtype=bm.STATE), np.zeros((n, NP), dtype=F)
        hl, hq, hh = np.zeros((n, nl), dtype=bm.LAYER), np.zeros((n, 3), dtype=bm.STEP), np.zeros((n, 3), dtype=F)
        host = lambda bl_=bl._h, st=p(hs), pr=p(hp), n_=n, ly=p(hl), nl_=nl, sp=p(hq), sh=p(hh): L.mtr_anim_blend_advance_host(bl_, st, pr, n_, 0.5, ly, nl_, sp, sh)
        assert host(bl_=None) == inv and host(st=None) == inv and host(pr=None) == inv and host(n_=0) == inv and host(n_=n + 1) == inv and host(nl_=2) == inv
        ok_st, ok_pr, ok_ly, ok_sp, ok_sh = t_st[:n * 16], t_pr[:n * NP], t_ly[:n * nl * 16], t_sp[:n * 48], t_sh[:n * 3]
        for fn in (lambda: bl.advance(ok_st.cpu(), ok_pr, 0.5), lambda: bl.advance(ok_st, ok_pr.double(), 0.5), lambda: bl.advance(ok_st, t_pr, 0.5),
                   lambda: bl.advance(ok_st, ok_pr, 0.5, out_layers=t_ly[:n * nl * 16 - 16]), lambda: bl.advance(ok_st, ok_pr, 0.5, out_steps=t_sp[:n * 32]),
                   lambda: bl.advance(ok_st, ok_pr, 0.5, out_shares=t_sh), lambda: bl.advance(ok_st, ok_pr, 0.5, out_shares=ok_sh.int()),
                   lambda: api.AnimBlend(gpu_device, nk, rt, fl, sm.view(np.uint8)), lambda: api.AnimBlend(gpu_device, nk, rt[:-1], fl, sm, tr),
                   lambda: bl.advance_host(hs, hp[:, :-1], 0.5)):
            with pytest.raises(api.MtrError) as e:
                fn()
            assert e.value.code == inv
        torch.cuda.synchronize()
        assert not any(t.any().item() for t in (t_st, t_pr, t_ly, t_sp, t_sh)), "nothing was written on the device"
        assert not any(a.view(np.uint8).any() for a in (hs, hp, hl, hq, hh)), "nothing was written on the host"
        # the valid call, for contrast
        ok_pr.copy_(_f32(c["calls"][0][1]).reshape(-1))
        ok_st.copy_(_dev(c["states"]).reshape(-1))
        bl.advance(ok_st, ok_pr, 0.5, out_layers=ok_ly.view(n, nl, 16), out_steps=ok_sp.view(n, 3, 16), out_shares=ok_sh)
        torch.cuda.synchronize()
        want = bm.advance(bs, c["states"], c["calls"][0][1], 0.5, nl, np.zeros((n, nl), dtype=bm.LAYER))
        _same(_host(ok_st, bm.STATE), want[0], "after invalid calls: states")
        _same(_host(ok_ly, bm.LAYER, (n, nl)), want[1], "after invalid calls: layers")
        _same(_host(ok_sp, bm.STEP, (n, 3)), want[2], "after invalid calls: steps")
        _same(ok_sh.cpu().numpy().reshape(n, 3), want[3], "after invalid calls: shares")
        assert not t_st[n * 16:].any().item() and not t_ly[n * nl * 16:].any().item() and not t_sp[n * 48:].any().item() and t_sh[n * 3].item() == 0
    finally:
        bl.close()


def test_argument_errors_of_advance_read_as_before(gpu_device):
    import torch
    from tests.test_gpu_player import _raises_saying
    n = 3
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device="cuda:0")
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda:0")
    samples = np.array([(0, 0.0, 0.0, 0), (1, 1.0, 0.0, 0)], dtype=api.BLEND_SAMPLE)
    create_msg = "anim blend: one key count, rate and flag word per clip, samples of dtype BLEND_SAMPLE [K], triangles of dtype BLEND_TRI [T]"
    bl = api.AnimBlend(gpu_device, [30, 20], [30.0, 30.0], [1, 1], samples, nparams=2, param_x=1, max_instances=n)
    st, pr = u8(n * 16), f32(n, 2)
    try:
        _raises_saying([
            (lambda: bl.advance(st.double(), pr, 0.1), "blend states: a uint8 / int32 / float32 tensor on the GPU"),
            (lambda: bl.advance(u8(n * 16 + 16)[8:8 + n * 16], pr, 0.1), "blend states: contiguous and 16-byte aligned (it is used in place)"),
            (lambda: bl.advance(st, pr.int(), 0.1), "blend params: a float32 tensor [n, nparams] on the GPU"),
            (lambda: bl.advance(st, None, 0.1), "blend params: a float32 tensor [n, nparams] on the GPU"),
            (lambda: bl.advance(st, f32(n, 3), 0.1), "blend params: records of 4 bytes, 6 of them"),
            (lambda: bl.advance(st, pr, 0.1, out_layers=u8((3 * n + 1) * 16)), "blend out_layers: n x L layers of 16 bytes"),
            (lambda: bl.advance(st, pr, 0.1, out_layers=u8(n * 3 * 32).view(n * 3, 32)[:, :16]), "blend out_layers: contiguous and 16-byte aligned (it is used in place)"),
            (lambda: bl.advance(st, pr, 0.1, out_steps=u8(n * 2 * 16)), "blend out_steps: records of 16 bytes, 9 of them"),
            (lambda: bl.advance(st, pr, 0.1, out_shares=f32(n, 3).int()), "blend out_shares: a float32 tensor [n, 3] on the GPU"),
            (lambda: bl.advance(st, pr, 0.1, out_shares=f32(n, 2)), "blend out_shares: records of 4 bytes, 9 of them"),
            # the first check that fails speaks: the parameters before the layers, the layers before the steps and the shares
            (lambda: bl.advance(st, pr.int(), 0.1, out_layers=u8((3 * n + 1) * 16)), "blend params: a float32 tensor [n, nparams] on the GPU"),
            (lambda: bl.advance(st, pr, 0.1, out_layers=u8((3 * n + 1) * 16), out_steps=u8(16), out_shares=f32(1)), "blend out_layers: n x L layers of 16 bytes"),
            (lambda: api.AnimBlend(gpu_device, [30, 20], [30.0], [1, 1], samples), create_msg),
            (lambda: api.AnimBlend(gpu_device, [30, 20], [30.0, 30.0], [1], samples), create_msg),
            (lambda: api.AnimBlend(gpu_device, [30, 20], [30.0, 30.0], [1, 1], samples.view(np.uint8)), create_msg),
            (lambda: api.AnimBlend(gpu_device, [30, 20], [30.0, 30.0], [1, 1], samples, param_x=-1), "anim blend: param_x and param_y are parameter indices"),
        ])
        torch.cuda.synchronize()
        assert not st.any().item(), "nothing ran"
    finally:
        bl.close()
