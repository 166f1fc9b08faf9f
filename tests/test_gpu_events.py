"""GPU: animation events (SPEC.md section 22).  The list, the two counts and the masks of k_events equal the binary32 numpy
model (tests/events_model.py) bit for bit on every case of the generator -- through the host hook and through the device call,
on the current stream and a side stream, bits given and NULL, the list behind count[1] untouched, 1 to 257 instances; one case
of 256 * 1024 + 1 instances, the smallest at which the scan of the block sums takes a second turn; three frames of step ->
advance -> collect -> root_motion chained on a side stream with nothing uploaded in between, the lists equal to the chained
models and the instance matrices still bit-equal; the set destroyed right after its last call; invalid calls change nothing."""
import ctypes as C

import numpy as np
import pytest

from mt_renderer_amd import anim_events, api, scene
from tests import ctrl_model as cm
from tests import events_model as em
from tests import player_model as pm
from tests import root_model as rm
from tests.test_gpu_anim_layers import _setup
from tests.test_gpu_player import _dev, _host, _player, _same

pytestmark = pytest.mark.gpu

CASES = em.cases()
F = np.float32
SCAN_WIDTH = 1024  # the width of k_events_scan's one workgroup; a block sum stands for 256 instances


def _events(dev, es, max_instances):
    return api.AnimEvents(dev, es["tab"][0], es["tab"][1], es["counts"], es["markers"], max_instances=max_instances)


def _steps(steps):
    n, S = steps.shape
    return _dev(steps.reshape(-1)).view(n, S, 16)


def _i32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to("cuda:0")


# ---- 1. bit for bit against the model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", em.COUNTS)
def test_list_count_and_bits_are_bit_exact(gpu_device, n):
    import torch
    assert (api.EVENT_MARKER, api.EVENT, api.ROOT_STEP) == (em.MARKER, em.EVENT, em.STEP)
    side = torch.cuda.Stream()
    fired = nan_seen = 0
    for k, c in enumerate(c for c in CASES if c["n"] == n):
        want = em.run_case(c)
        cap = c["capacity"]
        ev = _events(gpu_device, c["set"], n + (k % 3))
        try:
            # the host hook: the list and the bits go in as they were
            out, count, bits = ev.collect_host(c["steps"], c["min_weight"], cap, out=c["out_prev"], bits=c["bits_prev"])
            _same(out, want[0], f"{c['name']} host hook: list")
            assert (count == want[1]).all() and (bits == want[2]).all(), f"{c['name']} host hook: count {count} {want[1]}, bits"
            # the device call, on the current stream or on a side stream, bits given or NULL
            t_sp, t_ct = _steps(c["steps"]), _i32(np.array([0x5A5A5A5A] * 2))
            t_out = _dev(c["out_prev"]) if cap else None
            t_bits = _i32(c["bits_prev"]) if (k // 2) % 2 == 0 else None
            torch.cuda.synchronize()
            s = side if k % 2 else torch.cuda.current_stream()
            ev.collect(t_sp, c["min_weight"], t_out, t_ct, bits=t_bits, stream=s)
            s.synchronize()
            assert (t_ct.cpu().numpy().view(np.uint32) == want[1]).all(), f"{c['name']} device: count"
            if cap:
                _same(_host(t_out, em.EVENT), want[0], f"{c['name']} device: list")
            if t_bits is not None:
                assert (t_bits.cpu().numpy().view(np.uint32) == want[2]).all(), f"{c['name']} device: bits"
            _same(_host(t_sp, em.STEP, c["steps"].shape), c["steps"], f"{c['name']}: the steps are read only")
            fired += int(want[1][0])
            nan_seen += int(np.isnan(c["steps"]["x"]).any() and np.isnan(c["steps"]["dx"]).any())
        finally:
            ev.close()
    assert fired, "no marker fires at this size"
    assert nan_seen or n < 63, "the special values reach the comparison"


# ---- 2. the scan's second turn -----------------------------------------------------------------------------------------------
def test_the_scan_takes_a_second_turn(gpu_device):
    import torch
    n = 256 * SCAN_WIDTH + 1
    tab = pm.table([30], [pm.LOOP], [30.0])
    es = em.event_set(tab, {0: [(7.0, 5)]})
    steps = np.zeros((n, 1), dtype=em.STEP)
    steps["x"] = 6.5
    steps["dx"] = np.where(np.arange(n) % 3 == 0, F(1.0), F(0.25))[:, None]  # every third instance passes the marker
    cap = n // 3 + 8
    prev = np.frombuffer(bytes([0x5A]) * (cap * 16), dtype=em.EVENT)
    want = em.collect(es, steps, 0.0, cap, out_prev=prev)
    total = (n + 2) // 3
    assert want[1][0] == total == want[1][1] and want[0]["instance"][total - 1] == n - 2, "the last block of one instance adds nothing: its sum is 0"
    steps["dx"][n - 1] = 1.0  # ... so it passes the marker too: the block behind the second turn's carry writes a record
    want = em.collect(es, steps, 0.0, cap, out_prev=prev)
    assert want[1][0] == total + 1 and want[0]["instance"][total] == n - 1
    ev = _events(gpu_device, es, n)
    try:
        t_sp, t_out, t_ct, t_bits = _steps(steps), _dev(prev), _i32(np.zeros(2)), _i32(np.full(n, 0xFFFFFFFF))
        ev.collect(t_sp, 0.0, t_out, t_ct, bits=t_bits)
        torch.cuda.synchronize()
        assert (t_ct.cpu().numpy().view(np.uint32) == want[1]).all()
        _same(_host(t_out, em.EVENT), want[0], "the list")
        assert (t_bits.cpu().numpy().view(np.uint32) == want[2]).all()
    finally:
        ev.close()


# ---- 3. three frames chained on the device -----------------------------------------------------------------------------------
def test_three_frames_of_a_crowd_that_reports(gpu_device):
    import torch
    n = 64
    md, mf, m, rng, _, _ = _setup(gpu_device, "uniform", rows=2, cols=3)
    tab, g = cm.LOCO_TAB, cm.locomotion()
    traj = rm.walk_clip(31, 1) + rm.walk_clip(33, 1) + rm.walk_clip(17, 1) + rm.walk_clip(12, 1)
    rflags = np.array([rm.CYCLIC, rm.CYCLIC, rm.CYCLIC, 0], dtype=np.uint32)
    marks = {cm.IDLE: [(k + 0.5, 100 + k) for k in range(30)], cm.WALK: [(8.0, 1), (24.0, 2)], cm.RUN: [(4.0, 1), (12.0, 2)], cm.JUMP: [(0.5, 40), (11.0, 99)]}
    counts, markers = anim_events.build(marks, 4)
    es = em.event_set(tab, marks)
    assert (counts == es["counts"]).all() and markers.tobytes() == es["markers"].tobytes()
    tset, root = api.Anim(gpu_device, 1, traj), api.AnimRoot(gpu_device, 1, 4, 0, rflags)
    pl = _player(gpu_device, tab, n)
    ct = api.AnimCtrl(gpu_device, tab[0], tab[1], g["nodes"], g["trans"], g["nany"], g["nparams"])
    ev = api.AnimEvents(gpu_device, tab[0], tab[1], counts, markers, max_instances=n)
    mats, _ = scene.instance_lattice(9, 8, seed=300)
    mats = np.ascontiguousarray(mats[:n])
    b = api.Batch(gpu_device, m, mats)
    try:
        r2 = np.random.default_rng(2222)
        play = np.zeros(n, dtype=pm.PLAY)
        play["x_a"], play["speed"] = r2.uniform(0, 30, n), r2.uniform(0.75, 1.25, n)
        play["speed"][::5] *= -1  # some run backward
        st = np.zeros(n, dtype=cm.STATE)
        params = np.zeros((n, 2), dtype=F)
        params[:, cm.SPEED] = r2.uniform(0, 3, n)
        params[::7, cm.TRIGGER] = 1.0
        cap = 2 * n
        t_st, t_pl, t_cm = _dev(st), _dev(play), _dev(np.zeros(n, dtype=pm.CMD))
        t_pr = torch.from_numpy(params.copy()).to("cuda:0")
        t_sp = _dev(np.zeros((n, 2), dtype=pm.STEP).reshape(-1)).view(n, 2, 16)
        t_out = [_dev(np.frombuffer(bytes([0x5A]) * (cap * 16), dtype=em.EVENT)) for _ in range(3)]
        t_ct = [_i32(np.zeros(2)) for _ in range(3)]
        t_bits = [_i32(np.zeros(n)) for _ in range(3)]
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        M, want = mats, []
        for f in range(3):
            ct.step(t_st, t_pl, t_pr, pm.DT, t_cm, stream=side)
            pl.advance(t_pl, pm.DT, t_cm, out_steps=t_sp, stream=side)
            ev.collect(t_sp, 0.0, t_out[f], t_ct[f], bits=t_bits[f], stream=side)
            b.root_motion_device(tset, root, t_sp, stream=side)
            st, params, cmds, _ = cm.step(g, tab, st, play, params, pm.DT)
            play, _, _, sp = pm.advance(play, pm.DT, tab, cmds)
            want.append(em.collect(es, sp, 0.0, cap, out_prev=np.frombuffer(bytes([0x5A]) * (cap * 16), dtype=em.EVENT)))
            M = rm.root_motion(M, traj, (0, rflags), sp.astype(rm.STEP))
        side.synchronize()
        for f in range(3):
            assert (t_ct[f].cpu().numpy().view(np.uint32) == want[f][1]).all(), f"frame {f}: count"
            _same(_host(t_out[f], em.EVENT), want[f][0], f"frame {f}: list")
            assert (t_bits[f].cpu().numpy().view(np.uint32) == want[f][2]).all(), f"frame {f}: bits"
        assert all(int(w[1][0]) > n // 4 for w in want) and any((w[0]["where"] & em.BACKWARD).any() for w in want)
        assert any((w[0]["id"][:int(w[1][1])] == 40).any() for w in want), "a jump started and passed its first marker"
        _same(_host(t_pl, pm.PLAY), play, "play states")
        assert pm.same_bits(b.read_model_mats(), M).all(), "instance matrices: collecting disturbs nothing"
    finally:
        for h in (b, ev, ct, pl, root, tset, m):
            h.close()


# ---- 4. lifetime ---------------------------------------------------------------------------------------------------------------
def test_set_destroyed_right_after_the_last_call(gpu_device):
    import torch
    c = next(c for c in CASES if c["n"] == 257 and c["capacity"] > 0 and int(em.run_case(c)[1][0]) > 100)
    want = em.run_case(c)
    side = torch.cuda.Stream()
    for rnd in range(3):
        ev = _events(gpu_device, c["set"], 257)
        t_sp, t_out, t_ct, t_bits = _steps(c["steps"]), _dev(c["out_prev"]), _i32(np.zeros(2)), _i32(c["bits_prev"])
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)
        ev.collect(t_sp, c["min_weight"], t_out, t_ct, bits=t_bits, stream=side)
        ev.close()  # no host wait: the tables and the block sums are parked behind the kernels
        side.synchronize()
        _same(_host(t_out, em.EVENT), want[0], f"round {rnd} list")
        assert (t_ct.cpu().numpy().view(np.uint32) == want[1]).all() and (t_bits.cpu().numpy().view(np.uint32) == want[2]).all(), f"round {rnd}"


# ---- 5. invalid calls ------------------------------------------------------------------------------------------------------------
def test_invalid_calls_change_nothing(gpu_device):
    import torch
    c = next(c for c in CASES if c["n"] == 65 and c["S"] == 2 and len(c["set"]["markers"]) > 2)
    n, S, es = 65, 2, c["set"]
    Cn = len(es["counts"])
    ev = _events(gpu_device, es, n)
    L, inv, h = api.lib, api.MTR_E_INVALID, C.c_void_p()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    d = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    err = lambda: L.mtr_last_error(gpu_device._h)
    try:
        nk, fl = np.asarray(es["tab"][0], dtype=np.uint32), np.asarray(es["tab"][1], dtype=np.uint32)
        cn, mk = es["counts"].astype(np.uint32), es["markers"]
        create = lambda nclips=Cn, nk_=nk, fl_=fl, cn_=cn, mk_=mk, mi=n: L.mtr_anim_events_create(gpu_device._h, nclips, p(nk_), p(fl_), p(cn_), p(mk_), mi, C.byref(h))
        assert create(nclips=0) == inv and create(mi=0) == inv and create(mi=(1 << 27) + 1) == inv and not h
        bad = nk.copy(); bad[Cn - 1] = 0
        assert create(nk_=bad) == inv and f"clip {Cn - 1} ".encode() in err()
        bad = fl.copy(); bad[0] |= 4
        assert create(fl_=bad) == inv and b"clip 0 " in err()
        bad = cn.copy(); bad[0] = (1 << 24) + 1
        assert create(cn_=bad) == inv and not h
        cl = int(np.flatnonzero(es["counts"] >= 2)[0])
        first = int(es["first"][cl])
        for value in (np.nan, np.inf, -1.0, 1e9):
            bad = mk.copy(); bad["x"][first + 1] = value
            assert create(mk_=bad) == inv and f"clip {cl} marker 1 ".encode() in err(), value
        bad = mk.copy(); bad["x"][first] = np.nextafter(bad["x"][first + 1], F(np.inf))
        if bad["x"][first] <= es["tab"][0][cl] - 1:
            assert create(mk_=bad) == inv and f"clip {cl} marker 1 ".encode() in err(), "a marker before the one ahead of it"
        assert L.mtr_anim_events_create(gpu_device._h, Cn, p(nk), p(fl), p(cn), p(mk), n, None) == inv
        assert L.mtr_anim_events_create(None, Cn, p(nk), p(fl), p(cn), p(mk), n, C.byref(h)) == inv and not h
        cap = 16
        t_sp = _steps(c["steps"])
        t_out = torch.zeros(cap * 16 + 16, dtype=torch.uint8, device="cuda:0")
        t_ct = torch.zeros(4, dtype=torch.int32, device="cuda:0")
        t_bits = torch.zeros(n + 1, dtype=torch.int32, device="cuda:0")
        pad = torch.zeros(n * S * 16 + 32, dtype=torch.uint8, device="cuda:0")
        call = lambda ev_=ev._h, sp=d(t_sp), S_=S, n_=n, out=d(t_out), cap_=cap, cnt=d(t_ct), bits=d(t_bits): L.mtr_anim_events_collect_device(
            ev_, sp, S_, n_, 0.0, out, cap_, cnt, bits, None)
        assert call(ev_=None) == inv and call(sp=None) == inv and call(cnt=None) == inv and call(out=None) == inv
        assert call(S_=0) == inv and call(S_=9) == inv and call(n_=0) == inv and call(n_=n + 1) == inv
        assert call(sp=d(pad, 8)) == inv and call(out=d(t_out, 8)) == inv and call(cnt=d(t_ct, 2)) == inv and call(bits=d(t_bits, 2)) == inv
        hs, ho, hc, hb = c["steps"].copy(), np.zeros(cap, dtype=em.EVENT), np.zeros(2, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        host = lambda ev_=ev._h, sp=p(hs), S_=S, n_=n, out=p(ho), cap_=cap, cnt=p(hc), bits=p(hb): L.mtr_anim_events_collect_host(ev_, sp, S_, n_, 0.0, out, cap_, cnt, bits)
        assert host(ev_=None) == inv and host(sp=None) == inv and host(cnt=None) == inv and host(out=None) == inv and host(S_=9) == inv and host(n_=0) == inv
        assert host(n_=n + 1) == inv and host(cap_=1 << 32) == inv
        ok_out, ok_ct, ok_bits = t_out[:cap * 16], t_ct[:2], t_bits[:n]
        for fn in (lambda: ev.collect(t_sp[:, :, :15], 0.0, ok_out, ok_ct), lambda: ev.collect(t_sp.cpu(), 0.0, ok_out, ok_ct),
                   lambda: ev.collect(t_sp, 0.0, t_out[:cap * 16 - 1], ok_ct), lambda: ev.collect(t_sp, 0.0, ok_out, t_ct[:3]),
                   lambda: ev.collect(t_sp, 0.0, ok_out, ok_ct.float()), lambda: ev.collect(t_sp, 0.0, ok_out, ok_ct, bits=t_bits),
                   lambda: ev.collect(t_sp, 0.0, ok_out, ok_ct, bits=ok_bits.float()),
                   lambda: api.AnimEvents(gpu_device, nk, fl, cn, mk.view(np.uint8)), lambda: api.AnimEvents(gpu_device, nk, fl, cn[:-1] if Cn > 1 else cn[:0], mk),
                   lambda: ev.collect_host(c["steps"].reshape(-1), 0.0, cap)):
            with pytest.raises(api.MtrError) as e:
                fn()
            assert e.value.code == inv
        torch.cuda.synchronize()
        assert not t_out.any().item() and not t_ct.any().item() and not t_bits.any().item(), "nothing was written on the device"
        assert not ho.view(np.uint8).any() and not hc.any() and not hb.any(), "nothing was written on the host"
        # the valid call, for contrast
        ev.collect(t_sp, 0.0, ok_out, ok_ct, bits=ok_bits)
        torch.cuda.synchronize()
        want = em.collect(es, c["steps"], 0.0, cap)
        _same(_host(ok_out, em.EVENT), want[0], "after invalid calls")
        assert (ok_ct.cpu().numpy().view(np.uint32) == want[1]).all() and (ok_bits.cpu().numpy().view(np.uint32) == want[2]).all()
        assert not t_out[cap * 16:].any().item() and not t_ct[2:].any().item() and t_bits[n].item() == 0 and want[1][0] > 0
    finally:
        ev.close()


def test_argument_errors_of_collect_read_as_before(gpu_device):
    import torch
    from tests.test_gpu_player import _raises_saying
    n, S = 3, 2
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device="cuda:0")
    i32 = lambda k: torch.zeros(k, dtype=torch.int32, device="cuda:0")
    markers = np.array([(0.5, 7)], dtype=api.EVENT_MARKER)
    create_msg = "anim events: one flag word and one marker count per clip, markers of dtype EVENT_MARKER [sum of counts]"
    ev = api.AnimEvents(gpu_device, [30, 2], [1, 0], [1, 0], markers, max_instances=n)
    steps, out, count, bits = u8(n * S * 16).view(n, S, 16), u8(4 * 16), i32(2), i32(n)
    try:
        _raises_saying([
            (lambda: ev.collect(steps.view(n * S, 16), 0.0, out, count), "events steps: a tensor [n, S, 16 bytes] on the GPU"),
            (lambda: ev.collect(torch.zeros((n, S, 2), dtype=torch.float64, device="cuda:0"), 0.0, out, count), "events steps: a uint8 / int32 / float32 tensor on the GPU"),
            (lambda: ev.collect(u8(n * S * 16 + 16)[8:8 + n * S * 16].view(n, S, 16), 0.0, out, count), "events steps: contiguous and 16-byte aligned (it is used in place)"),
            (lambda: ev.collect(u8(n * S * 32).view(n, S, 32)[:, :, :16], 0.0, out, count), "events steps: contiguous and 16-byte aligned (it is used in place)"),
            (lambda: ev.collect(steps, 0.0, u8(24), count), "events list: records of 16 bytes"),
            (lambda: ev.collect(steps, 0.0, out, count.float()), "events count: an int32 tensor [2] on the GPU"),
            (lambda: ev.collect(steps, 0.0, out, None), "events count: an int32 tensor [2] on the GPU"),
            (lambda: ev.collect(steps, 0.0, out, i32(3)), "events count: records of 4 bytes, 2 of them"),
            (lambda: ev.collect(steps, 0.0, out, count, bits=bits.float()), "events bits: an int32 tensor [n] on the GPU"),
            (lambda: ev.collect(steps, 0.0, out, count, bits=i32(n + 1)), "events bits: records of 4 bytes, 3 of them"),
            # the first check that fails speaks: the list before the count, the count before the bits
            (lambda: ev.collect(steps, 0.0, u8(24), count.float(), bits=bits.float()), "events list: records of 16 bytes"),
            (lambda: ev.collect(steps, 0.0, out, i32(3), bits=bits.float()), "events count: records of 4 bytes, 2 of them"),
            (lambda: api.AnimEvents(gpu_device, [30, 2], [1], [1, 0], markers), create_msg),
            (lambda: api.AnimEvents(gpu_device, [30, 2], [1, 0], [1], markers), create_msg),
            (lambda: api.AnimEvents(gpu_device, [30, 2], [1, 0], [2, 0], markers), create_msg),
        ])
        torch.cuda.synchronize()
        assert not out.any().item() and not count.any().item() and not bits.any().item(), "nothing ran"
    finally:
        ev.close()
