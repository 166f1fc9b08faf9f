"""GPU: motion matching (SPEC.md section 25).  k_match equals the binary32 numpy model (tests/match_model.py) bit for bit on every
case of the generator: the full n x R score matrix out of the search kernel itself (the premise of whichever instruction it
uses: a k-ordered fmaf chain from c_r), then commands and results through the host hook and the device call, on the current
stream and a side stream, results and filters given and NULL, instance_base 0 and not, junk behind slot n - 1 left alone; a
host command appended behind slot n - 1 overrules the search; the set destroyed right after its last search, one set for two
crowds on two streams; invalid calls change nothing and the binding's argument errors read in the house wording."""
import ctypes as C

import numpy as np
import pytest

from mt_renderer_amd import api
from tests import match_model as mm
from tests import player_model as pm
from tests.test_gpu_anim import _render
from tests.test_gpu_player import _dev, _host, _player, _raises_saying, _same

pytestmark = pytest.mark.gpu

CASES = mm.cases()
F = np.float32
TAB = pm.table(list(mm.NKEYS), list(mm.CLIP_FLAGS), [30.0, 32.0, 24.0, 24.0])


def _match(dev, c, n=None):
    s = c["set"]
    return api.AnimMatch(dev, s["nkeys"], s["clip_flags"], s["rows"], s["feats"], pose_dims=s["pose_dims"], flags=s["flags"], seconds=float(s["seconds"]),
                         near=float(s["near"]), margin=float(s["margin"]), mean=s["mean"] if s["has_norm"] else None, scale=s["scale"] if s["has_norm"] else None,
                         max_instances=n or c["n"])


def _f32(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=F).copy()).to("cuda:0")


def _junk(n, extra=0):
    return _dev(np.frombuffer(bytes([0x5A]) * ((n + extra) * 16), dtype=pm.CMD))


# ---- 1. the premise: every score out of the search kernel --------------------------------------------------------------------------
@pytest.mark.parametrize("family", mm.FAMILIES)
def test_every_score_of_the_search_kernel_is_the_fmaf_chain(gpu_device, family):
    assert (api.MATCH_ROW, api.MATCH_FILTER, api.MATCH_RESULT) == (mm.ROW, mm.FILTER, mm.RESULT)
    nan_seen = inf_seen = zero_seen = 0
    for c in (c for c in CASES if c["family"] == family):
        want = mm.search(c["set"], c["play"], c["raw"], None)[2]
        m = _match(gpu_device, c)
        try:
            got = m.scores_host(c["play"], c["raw"])
        finally:
            m.close()
        bad = ~mm.same_bits(got, want)
        assert got.shape == want.shape and not bad.any(), f"{c['name']}: {int(bad.sum())} of {bad.size} scores differ, first at {np.argwhere(bad)[0]}"
        nan_seen += int(np.isnan(want).sum())
        inf_seen += int(np.isinf(want).sum())
        zero_seen += int((want == 0).sum())
    assert (nan_seen and inf_seen) or family != "large", "NaN and infinite scores reach the comparison"
    assert zero_seen or family != "subnormal", "scores of zero reach the comparison"


# ---- 2. commands and results ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", mm.FAMILIES)
def test_commands_and_results_are_bit_exact(gpu_device, family):
    import torch
    side = torch.cuda.Stream()
    ties = none = nan = jumps = 0
    for k, c in enumerate(c for c in CASES if c["family"] == family):
        s, n = c["set"], c["n"]
        m = _match(gpu_device, c, n if k % 2 else n + 3)
        try:
            # the host hook: filter given, base 0
            cmds, res, S = mm.search(s, c["play"], c["raw"], c["filt"], 0)
            got_c, got_r = m.search_host(c["play"], c["raw"], c["filt"])
            _same(got_c, cmds, f"{c['name']} host hook: commands")
            _same(got_r, res, f"{c['name']} host hook: results")
            key = np.where(mm.candidates(s, c["filt"], n), mm.order_key(S), 0)
            ties += int(((res["row"] != mm.NONE) & ((key == key.max(1)[:, None]).sum(1) > 1)).sum())
            none += int((res["row"] == mm.NONE).sum())
            nan += int(np.isnan(S).any())
            jumps += int((cmds["instance"] != 0xFFFFFFFF).sum())
            # the device call: current stream or side stream, results and filter given or NULL, the case's instance_base
            t_pl, t_q = _dev(c["play"]), _f32(c["raw"])
            for v in range(2):
                use_filter, use_results, st = (k + v) % 2 == 0, (k // 2 + v) % 2 == 0, (side if (k + v) % 2 else torch.cuda.current_stream())
                filt = c["filt"] if use_filter else None
                cmds, res, _ = mm.search(s, c["play"], c["raw"], filt, c["base"])
                t_cm, t_rs = _junk(n, 2), _junk(n)
                t_fl = _dev(filt) if use_filter else None
                torch.cuda.synchronize()
                m.search(t_pl, t_q, t_cm, filters=t_fl, results=t_rs if use_results else None, instance_base=c["base"], stream=st)
                st.synchronize()
                out = _host(t_cm, pm.CMD)
                _same(out[:n], cmds, f"{c['name']} device call {v}: commands")
                assert (out[n:].view(np.uint8) == 0x5A).all(), f"{c['name']} device call {v}: the slots behind n - 1 are the caller's"
                if use_results:
                    _same(_host(t_rs, mm.RESULT), res, f"{c['name']} device call {v}: results")
                else:
                    assert (t_rs == 0x5A).all().item()
                _same(_host(t_pl, pm.PLAY), c["play"], f"{c['name']}: the play states are read only")
        finally:
            m.close()
    assert ties and none and jumps, (ties, none, jumps)
    assert nan or family != "large", "NaN scores reach the comparison"


# ---- 2b. both grid layouts, several tiles per wave -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1024, 1025))
def test_both_grid_layouts_at_their_threshold(gpu_device, n):
    """up to 1024 instances the four waves of a workgroup share 32 instances and are joined through LDS, above that each wave
    owns its own 32; 4100 rows give every wave several tiles, a last one that is partly padding, and waves without any"""
    import torch
    c = mm.make_case(np.random.default_rng(2600 + n), n, 4100, 8, "benign", 5 if n == 1024 else 4)
    s = c["set"]
    m = _match(gpu_device, c)
    try:
        L, p, _ = mm.lead(s, c["play"])
        cur = mm.current_rows(s, L, p)
        S = mm.scores(s, mm.query(s, cur, c["raw"]))  # once: both decisions below are made from it
        got = m.scores_host(c["play"], c["raw"])
        bad = ~mm.same_bits(got, S)
        assert not bad.any(), f"{int(bad.sum())} of {bad.size} scores differ, first at {np.argwhere(bad)[0]}"
        t_pl, t_q, t_fl, t_cm, t_rs = _dev(c["play"]), _f32(c["raw"]), _dev(c["filt"]), _junk(n), _junk(n)
        for what, filt, t_f in (("with filters", c["filt"], t_fl), ("without filters", None, None)):
            cmds, res = mm.decide(s, c["play"], cur, S, mm.candidates(s, filt, n), c["base"])
            m.search(t_pl, t_q, t_cm, filters=t_f, results=t_rs, instance_base=c["base"])
            torch.cuda.synchronize()
            _same(_host(t_cm, pm.CMD), cmds, f"{what}: commands")
            _same(_host(t_rs, mm.RESULT), res, f"{what}: results")
            if filt is not None:
                won = res["row"][res["row"] != mm.NONE]
                assert len(set(won)) > 8 and (won > 4064).any(), "winners in many tiles, the last one too"
    finally:
        m.close()


# ---- 3. the host overrules -----------------------------------------------------------------------------------------------------------
def test_a_host_command_behind_slot_n_minus_1_overrules(gpu_device):
    import torch
    c = next(c for c in CASES if c["n"] == 257 and c["family"] == "benign")
    n, s, dt = c["n"], c["set"], pm.DT
    cmds, _, _ = mm.search(s, c["play"], c["raw"], c["filt"], 0)
    jumping, quiet = np.flatnonzero(cmds["instance"] != 0xFFFFFFFF), np.flatnonzero(cmds["instance"] == 0xFFFFFFFF)
    assert len(jumping) >= 2 and len(quiet) >= 1
    host = np.array([(jumping[0], 0, 3.0, 0.0), (quiet[0], 3, 1.0, 0.25), (jumping[-1], 0, 2.0, 0.5)], dtype=pm.CMD)
    want = pm.advance(c["play"], dt, TAB, np.concatenate([cmds, host]))[0]
    assert not pm.same_bits(want, pm.advance(c["play"], dt, TAB, cmds)[0]).all(), "the host's commands would show"
    m, pl = _match(gpu_device, c), _player(gpu_device, TAB, n)
    try:
        t_pl, t_q, t_fl, t_cm = _dev(c["play"]), _f32(c["raw"]), _dev(c["filt"]), _junk(n, len(host))
        t_cm[n:] = _dev(host)  # written once, behind the search's slots; the search leaves them alone
        torch.cuda.synchronize()
        m.search(t_pl, t_q, t_cm, filters=t_fl)
        pl.advance(t_pl, dt, t_cm)
        torch.cuda.synchronize()
        _same(_host(t_cm, pm.CMD), np.concatenate([cmds, host]), "the list")
        _same(_host(t_pl, pm.PLAY), want, "play states")
    finally:
        m.close()
        pl.close()


# ---- 4. lifetime and ordering --------------------------------------------------------------------------------------------------------
def test_set_destroyed_right_after_the_last_search(gpu_device):
    import torch
    c = next(c for c in CASES if c["n"] == 257 and c["family"] == "benign")
    n, s = c["n"], c["set"]
    cmds, res, _ = mm.search(s, c["play"], c["raw"], c["filt"], 5)
    side = torch.cuda.Stream()
    for rnd in range(3):
        m = _match(gpu_device, c)
        t_pl, t_q, t_fl, t_cm, t_rs = _dev(c["play"]), _f32(c["raw"]), _dev(c["filt"]), _junk(n), _junk(n)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)
        for _ in range(2):
            m.search(t_pl, t_q, t_cm, filters=t_fl, results=t_rs, instance_base=5, stream=side)
        m.close()  # no host wait: the image and the scratch are parked behind the kernels
        side.synchronize()
        _same(_host(t_cm, pm.CMD), cmds, f"round {rnd} commands")
        _same(_host(t_rs, mm.RESULT), res, f"round {rnd} results")


def test_one_set_for_crowds_on_two_streams_destroyed_right_after(gpu_device):
    """one set searches for a crowd on a stalled side stream and then for another on the current stream: the searches share the
    set's scratch, so the second waits for the set's event; destroyed at once, the image is parked behind BOTH"""
    import torch
    c = next(c for c in CASES if c["n"] == 257 and c["family"] == "benign")
    n, s = c["n"], c["set"]
    cmds_a, res_a, _ = mm.search(s, c["play"], c["raw"], c["filt"], 0)
    play_b, raw_b = c["play"][::-1].copy(), None if c["raw"] is None else c["raw"][::-1].copy()
    cmds_b, res_b, _ = mm.search(s, play_b, raw_b, None, 9)
    side = torch.cuda.Stream()
    m = _match(gpu_device, c)
    a_pl, a_q, a_fl, a_cm, a_rs = _dev(c["play"]), _f32(c["raw"]), _dev(c["filt"]), _junk(n), _junk(n)
    b_pl, b_q, b_cm, b_rs = _dev(play_b), _f32(raw_b), _junk(n), _junk(n)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(20_000_000)
    m.search(a_pl, a_q, a_cm, filters=a_fl, results=a_rs, stream=side)
    m.search(b_pl, b_q, b_cm, results=b_rs, instance_base=9)
    m.close()
    _render(gpu_device, 32, 32, lambda fr: None)  # a submit collects what is parked and done
    other = _match(gpu_device, next(x for x in CASES if x["n"] == 65 and x["family"] == "benign"))
    torch.cuda.synchronize()
    other.close()
    _same(_host(a_cm, pm.CMD), cmds_a, "the side stream's crowd: commands")
    _same(_host(a_rs, mm.RESULT), res_a, "the side stream's crowd: results")
    _same(_host(b_cm, pm.CMD), cmds_b, "the current stream's crowd: commands")
    _same(_host(b_rs, mm.RESULT), res_b, "the current stream's crowd: results")


# ---- 5. invalid calls ------------------------------------------------------------------------------------------------------------------
def test_invalid_calls_change_nothing(gpu_device):
    import torch
    c = next(c for c in CASES if c["n"] == 65 and c["family"] == "benign")
    n, s = c["n"], c["set"]
    R, D, Cn = c["R"], c["D"], len(s["nkeys"])
    assert s["pose_dims"] == 0 and c["raw"] is not None
    m = _match(gpu_device, c)
    L, inv, h = api.lib, api.MTR_E_INVALID, C.c_void_p()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    d = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    err = lambda: L.mtr_last_error(gpu_device._h)
    try:
        nk, fl, rw, ft = s["nkeys"], s["clip_flags"], s["rows"], s["feats"]
        create = lambda nclips=Cn, nk_=nk, fl_=fl, D_=D, pose=0, flags=0, near=0.5, margin=0.1, rw_=rw, R_=R, ft_=ft, mean=None, scale=None, ni=n, out=C.byref(h): \
            L.mtr_anim_match_create(gpu_device._h, nclips, p(nk_), p(fl_), D_, pose, flags, 0.2, near, margin, p(rw_), R_, p(ft_), p(mean), p(scale), ni, out)
        assert create(nclips=0) == inv and create(D_=0) == inv and create(D_=6) == inv and create(D_=68) == inv and not h
        assert create(R_=0) == inv and create(R_=(1 << 22) + 1) == inv and create(ni=0) == inv and create(ni=(1 << 20) + 1) == inv and not h
        assert create(flags=2) == inv and create(nk_=None) == inv and create(rw_=None) == inv and create(ft_=None) == inv and create(out=None) == inv and not h
        assert create(pose=1 << D) == inv and f"dimension {D} ".encode() in err()
        for kw in (dict(near=-1.0), dict(near=float("nan")), dict(near=float("inf")), dict(margin=-0.5), dict(margin=float("nan")), dict(margin=float("inf"))):
            assert create(**kw) == inv and not h, kw
        bad = nk.copy(); bad[Cn - 1] = 0
        assert create(nk_=bad) == inv and f"clip {Cn - 1} ".encode() in err()
        bad = fl.copy(); bad[0] |= 4
        assert create(fl_=bad) == inv and b"clip 0 " in err()
        P = s["P"]
        for field, row, value in (("clip", 7, Cn), ("clip", 7, 0xFFFFFFFF), ("x", 7, float("nan")), ("x", 7, -0.5), ("x", 7, float(rw["x"][6])), ("x", 7, float(P[rw["clip"][7]])),
                                  ("bias", 7, float("inf")), ("bias", 7, float("nan")), ("clip", R - 1, 0)):
            bad = rw.copy(); bad[field][row] = value
            assert create(rw_=bad) == inv and f"row {row} ".encode() in err() and not h, (field, row, value)
        bad = ft.copy(); bad[9, 3] = np.inf
        assert create(ft_=bad) == inv and b"row 9 " in err() and b"dimension 3" in err()
        bad = ft.copy(); bad[11] = 1.5e19  # finite features whose squares do not sum to a finite c
        assert create(ft_=bad) == inv and b"row 11 " in err()
        bad = np.zeros(D, dtype=F); bad[2] = np.nan
        assert create(mean=bad) == inv and b"dimension 2 " in err() and create(scale=bad) == inv and b"dimension 2 " in err() and not h
        assert L.mtr_anim_match_create(None, Cn, p(nk), p(fl), D, 0, 0, 0.2, 0.5, 0.1, p(rw), R, p(ft), None, None, n, C.byref(h)) == inv and not h
        # at a call
        t_pl, t_q, t_fl = _dev(c["play"]), _f32(c["raw"]), _dev(c["filt"])
        t_cm, t_rs = torch.zeros(n * 16 + 16, dtype=torch.uint8, device="cuda:0"), torch.zeros(n * 16 + 16, dtype=torch.uint8, device="cuda:0")
        pad = torch.zeros(n * 32 + 32, dtype=torch.uint8, device="cuda:0")
        call = lambda m_=m._h, pl=d(t_pl), q=d(t_q), f=d(t_fl), n_=n, base=0, cm=d(t_cm), rs=d(t_rs): L.mtr_anim_match_search_device(m_, pl, q, f, n_, base, cm, rs, None)
        assert call(m_=None) == inv and call(pl=None) == inv and call(cm=None) == inv
        assert call(q=None) == inv and b"dimension 0 " in err()
        assert call(n_=0) == inv and call(n_=n + 1) == inv and call(base=0xFFFFFFFF - n + 1) == inv
        assert call(pl=d(pad, 8)) == inv and call(q=d(t_q, 8)) == inv and call(cm=d(t_cm, 8)) == inv and call(rs=d(t_rs, 8)) == inv and call(f=d(t_fl, 4)) == inv
        hc, hr = np.zeros(n, dtype=pm.CMD), np.zeros(n, dtype=mm.RESULT)
        host = lambda m_=m._h, pl=p(c["play"]), q=p(c["raw"]), n_=n, cm=p(hc): L.mtr_anim_match_search_host(m_, pl, q, None, n_, 0, cm, p(hr))
        assert host(m_=None) == inv and host(pl=None) == inv and host(q=None) == inv and host(n_=0) == inv and host(n_=n + 1) == inv and host(cm=None) == inv
        sc = np.zeros((n, R), dtype=F)
        assert L.mtr_anim_match_scores_host(m._h, p(c["play"]), p(c["raw"]), n, None) == inv and L.mtr_anim_match_scores_host(None, p(c["play"]), p(c["raw"]), n, p(sc)) == inv
        assert L.mtr_anim_match_scores_host(m._h, p(c["play"]), None, n, p(sc)) == inv and L.mtr_anim_match_scores_host(m._h, p(c["play"]), p(c["raw"]), n + 1, p(sc)) == inv
        cm_ok = t_cm[:n * 16]
        for fn in (lambda: m.search(t_pl[:, :31], t_q, cm_ok), lambda: m.search(t_pl, t_q[:n - 1], cm_ok), lambda: m.search(t_pl, None, cm_ok),
                   lambda: m.search(t_pl, t_q, t_cm[:(n - 1) * 16]), lambda: m.search(t_pl.cpu(), t_q, cm_ok), lambda: m.search(t_pl, t_q, cm_ok, filters=t_fl[:n - 1]),
                   lambda: m.search(t_pl, t_q, cm_ok, results=t_rs[:(n - 1) * 16]), lambda: m.search(t_pl, t_q, cm_ok, instance_base=1 << 32),
                   lambda: api.AnimMatch(gpu_device, nk, fl, rw.view(np.uint8), ft), lambda: m.search_host(c["play"], c["raw"][:3]),
                   lambda: m.scores_host(c["play"][:3], c["raw"])):
            with pytest.raises(api.MtrError) as e:
                fn()
            assert e.value.code == inv
        torch.cuda.synchronize()
        _same(_host(t_pl, pm.PLAY), c["play"], "the play states are untouched")
        assert not hc.view(np.uint8).any() and not hr.view(np.uint8).any() and not sc.any() and not t_cm.any().item() and not t_rs.any().item(), "nothing was written"
        # the valid call, for contrast
        m.search(t_pl, t_q, cm_ok, filters=t_fl, results=t_rs[:n * 16])
        torch.cuda.synchronize()
        cmds, res, _ = mm.search(s, c["play"], c["raw"], c["filt"], 0)
        _same(_host(cm_ok, pm.CMD), cmds, "after invalid calls: commands")
        _same(_host(t_rs[:n * 16], mm.RESULT), res, "after invalid calls: results")
        assert not t_cm[n * 16:].any().item() and not t_rs[n * 16:].any().item()
    finally:
        m.close()


def test_argument_errors_of_search_read_in_the_house_wording(gpu_device):
    import torch
    n, D = 3, 8
    u8 = lambda k: torch.zeros(k, dtype=torch.uint8, device="cuda:0")
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda:0")
    rows = np.zeros(2, dtype=api.MATCH_ROW)
    rows["x"] = [0.0, 1.0]
    feats = np.ones((2, D), dtype=F)
    create_msg = "anim match: one flag word per clip, rows of dtype MATCH_ROW [R], features float32 [R, D], mean and scale float32 [D]"
    m = api.AnimMatch(gpu_device, [30, 2], [1, 0], rows, feats, pose_dims=0x0F, max_instances=n)
    pl, q, cmds = u8(n * 32), f32(n, D), u8(n * 16)
    try:
        _raises_saying([
            (lambda: m.search(pl.double(), q, cmds), "match play states: a uint8 / int32 / float32 tensor on the GPU"),
            (lambda: m.search(u8(n * 32 + 16)[8:8 + n * 32], q, cmds), "match play states: contiguous and 16-byte aligned (it is used in place)"),
            (lambda: m.search(pl, q, u8((n - 1) * 16)), "match commands: at least n slots of 16 bytes"),
            (lambda: m.search(pl, None, cmds), "match query: the set has dimensions that are not pose dimensions and no query is given"),
            (lambda: m.search(pl, q.int(), cmds), "match query: a float32 tensor [n, D] on the GPU"),
            (lambda: m.search(pl, f32(n, D + 4), cmds), "match query: records of 32 bytes, 3 of them"),
            (lambda: m.search(pl, f32(n, 2 * D)[:, :D], cmds), "match query: contiguous and 16-byte aligned (it is used in place)"),
            (lambda: m.search(pl, q, cmds, filters=u8((n - 1) * 8)), "match filters: records of 8 bytes, 3 of them"),
            (lambda: m.search(pl, q, cmds, filters=u8(n * 8 + 8)[4:4 + n * 8]), "match filters: contiguous and 8-byte aligned (it is used in place)"),
            (lambda: m.search(pl, q, cmds, results=u8((n + 1) * 16)), "match results: records of 16 bytes, 3 of them"),
            (lambda: m.search(pl, q, cmds, instance_base=-1), "match search: instance_base is a 32-bit index"),
            # the first check that fails speaks: the commands before the query, the query before the filters
            (lambda: m.search(pl, q.int(), u8((n - 1) * 16), filters=u8(8)), "match commands: at least n slots of 16 bytes"),
            (lambda: m.search(pl, q.int(), cmds, filters=u8(8)), "match query: a float32 tensor [n, D] on the GPU"),
            (lambda: api.AnimMatch(gpu_device, [30, 2], [1], rows, feats), create_msg),
            (lambda: api.AnimMatch(gpu_device, [30, 2], [1, 0], rows.view(np.uint8), feats), create_msg),
            (lambda: api.AnimMatch(gpu_device, [30, 2], [1, 0], rows, feats, mean=np.zeros(3)), create_msg),
            (lambda: m.search_host(np.zeros(n, dtype=api.PLAY_STATE), np.zeros((n, D + 1))), "match query: float32 [n, D]"),
            (lambda: m.search_host(np.zeros(n, dtype=api.PLAY_STATE), np.zeros((n, D)), filters=np.zeros(n - 1, dtype=api.MATCH_FILTER)),
             "match filters: an array [n] of dtype MATCH_FILTER"),
        ])
        torch.cuda.synchronize()
        assert not cmds.any().item(), "nothing ran"
    finally:
        m.close()


# ---- 6. end to end: forty frames with nothing uploaded in between --------------------------------------------------------------------
def crowd_database(rng, J):
    """four gentle clips, their walk trajectories and the database anim_match.py builds from them: per row four pose features
    (where two joints stand) and eight trajectory features (where the root will be 4 and 8 keys on)"""
    from mt_renderer_amd import anim_match
    from tests import anim_model as anm
    from tests import root_model as rm
    shape = [(30, anm.CLIP_LOOP), (32, anm.CLIP_LOOP), (16, anm.CLIP_LOOP), (12, 0)]
    clips = anm.gentle_clips(rng, J, shape=shape)
    traj = rm.walk_clip(31, 1) + rm.walk_clip(33, 1) + rm.walk_clip(17, 1) + rm.walk_clip(12, 1)
    nkeys, flags = [s[0] for s in shape], [s[1] for s in shape]
    rows = anim_match.rows_of(nkeys, flags, stride=2, tail=4)
    raw = np.zeros((len(rows), 12))
    for c in range(4):
        tf = anim_match.trajectory_features(traj[c][0], (4, 8), cyclic=bool(flags[c]))
        for r in np.flatnonzero(rows["clip"] == c):
            k = int(rows["x"][r])
            raw[r, 0:2], raw[r, 2:4], raw[r, 4:] = clips[c][0][k, 1, 0:2], clips[c][0][k, 2, 0:2], tf[k]
    feats, mean, scale = anim_match.normalise(raw, [0.5] * 4 + [1.0] * 8)
    return clips, traj, nkeys, flags, rows, raw.astype(F), feats, mean, scale


def test_forty_frames_of_a_crowd_that_searches(gpu_device):
    import torch
    from mt_renderer_amd import scene
    from tests import anim_layers_model as lm
    from tests import anim_model as anm
    from tests import root_model as rm
    from tests.helpers import assert_same, render_oracle
    from tests.test_gpu_anim import _bits_equal
    from tests.test_gpu_anim_layers import _setup
    W, H, n, J, Q = 160, 96, 64, 64, 16
    md, mf, m, rng, _, _ = _setup(gpu_device, "uniform", rows=2, cols=3)
    clips, traj, nkeys, flags, rows, raw, feats, mean, scale = crowd_database(rng, J)
    tab = pm.table(nkeys, flags, [30.0, 32.0, 24.0, 24.0])
    rflags = np.array([rm.CYCLIC, rm.CYCLIC, rm.CYCLIC, 0], dtype=np.uint32)
    s = mm.make_set(nkeys, flags, rows, feats, pose_dims=0xF, flags=0, seconds=0.2, near=3.0, margin=0.05, mean=mean, scale=scale)
    anim, tset, root = api.Anim(gpu_device, J, clips), api.Anim(gpu_device, 1, traj), api.AnimRoot(gpu_device, 1, 4, 0, rflags)
    pl = _player(gpu_device, tab, n)
    mt = api.AnimMatch(gpu_device, nkeys, flags, rows, feats, pose_dims=0xF, flags=0, seconds=0.2, near=3.0, margin=0.05, mean=mean, scale=scale, max_instances=Q)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
    mats, _ = scene.instance_lattice(9, 8, seed=300)
    mats = np.ascontiguousarray(mats[:n])
    b = api.Batch(gpu_device, m, mats)
    try:
        play = np.zeros(n, dtype=pm.PLAY)
        play["clip_a"], play["x_a"], play["speed"] = rng.integers(0, 4, n), rng.uniform(0, 10, n), rng.uniform(0.75, 1.25, n)
        # the game's wish: the trajectory of some row, drifting a little every frame (a device-side add: nothing is uploaded)
        q = raw[rng.integers(0, len(rows), n)].copy()
        slope = (rng.standard_normal((n, 12)) * 0.004).astype(F)
        slope[:, :4] = 0
        t_pl, t_q, t_slope, t_cm = _dev(play), _f32(q), _f32(slope), _junk(n)
        t_rs = _junk(n)
        t_ly, t_sp = _dev(np.zeros((n, 2), dtype=pm.LAYER)).view(n, 2, 16), _dev(np.zeros((n, 2), dtype=pm.STEP)).view(n, 2, 16)
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        M, jumps, ignored, fading_seen = mats, 0, 0, False
        for frame in range(1, 41):
            k = (frame % 4) * Q  # a quarter of the crowd searches per frame
            with torch.cuda.stream(side):
                t_q += t_slope
            mt.search(t_pl[k:k + Q], t_q[k:k + Q], t_cm[k:k + Q], results=t_rs[k:k + Q], instance_base=k, stream=side)
            pl.advance(t_pl, pm.DT, t_cm[k:k + Q], out_layers=t_ly, out_steps=t_sp, stream=side)
            with torch.cuda.stream(side):
                b.animate_layers(anim, t_ly)
                b.root_motion_device(tset, root, t_sp, stream=side)
            q = (q + slope).astype(F)
            cmds, res, _ = mm.search(s, play[k:k + Q], q[k:k + Q], None, k)
            play, _, ly, sp = pm.advance(play, pm.DT, tab, cmds, 2)
            M = rm.root_motion(M, traj, (0, rflags), sp.astype(rm.STEP))
            jumps += int((cmds["instance"] != 0xFFFFFFFF).sum())
            ignored += int((cmds["instance"] == 0xFFFFFFFF).sum())
            fading_seen |= bool(((ly["w"][:, 1] > 0) & (ly["w"][:, 1] < 1)).any())
            side.synchronize()
            _same(_host(t_cm[k:k + Q], pm.CMD), cmds, f"frame {frame}: commands")  # 16 bytes each: the frame that goes wrong is named
            _same(_host(t_rs[k:k + Q], mm.RESULT), res, f"frame {frame}: results")
            if frame in (1, 2, 9, 17, 28, 40):
                pals = anm.palettes(mf, lm.sample(clips, ly.astype(lm.LAYER), J, None))
                _same(_host(t_pl, pm.PLAY), play, f"frame {frame}: play states")
                assert _bits_equal(b.read_palettes(), pals), f"frame {frame}: palettes"
                assert pm.same_bits(b.read_model_mats(), M).all(), f"frame {frame}: instance matrices"
        assert jumps >= 8 and ignored >= 8 and fading_seen and np.isfinite(M).all(), (jumps, ignored, fading_seen)
        # the last frame renders like the oracle from those palettes and matrices
        ref = render_oracle(W, H, [dict(md=md, vp=vp, model_mats=M, palettes=pals)])
        assert_same(_render(gpu_device, W, H, lambda fr: fr.draw_batch(b, vp)), ref, "the last frame")
    finally:
        for h in (b, mt, pl, root, tset, anim, m):
            h.close()
