"""CPU: the numpy model of SPEC.md section 20 (tests/player_model.py) against the text's own stated consequences, the generator's
coverage of every edge value and branch of the rule (conditions checked from the model alone), the table of wrong readings,
and the chain player -> section 14's model / section 19's model against the same models driven by the host recipe the player
replaces.  The figures printed here are the ones SPEC.md section 20 records."""
import numpy as np

from tests import anim_model as am
from tests import player_model as pm
from tests import root_model as rm

F = np.float32
CASES = pm.cases()


def _traces(c):
    tr = []
    res = pm.run_case(c, trace=tr)
    return res, tr


ALL = [(c,) + _traces(c) for c in CASES]


def test_layouts():
    assert pm.PLAY.itemsize == 32 and pm.CMD.itemsize == 16 and pm.STATE.itemsize == 24 and pm.LAYER.itemsize == 16 and pm.STEP.itemsize == 16
    assert pm.PLAY.names == ("clip_a", "clip_b", "x_a", "x_b", "w", "fade", "speed", "flags")
    assert [pm.PLAY.fields[k][1] for k in pm.PLAY.names] == [0, 4, 8, 12, 16, 20, 24, 28]
    assert pm.CMD.names == ("instance", "clip", "x", "seconds") and [pm.CMD.fields[k][1] for k in pm.CMD.names] == [0, 4, 8, 12]


def _has(values, v):
    values = np.asarray(values, dtype=F).reshape(-1)
    if v != v:
        return bool(np.isnan(values).any())
    return bool(((values == F(v)) & (np.signbit(values) == np.signbit(F(v)))).any())


def test_generator_holds_every_edge_value():
    assert sorted({c["n"] for c in CASES}) == [1, 5, 63, 64, 65, 257]
    assert {len(c["tab"][0]) for c in CASES} == {1, 3}
    nk = np.concatenate([c["tab"][0] for c in CASES])
    assert {1, 2, 30, 1 << 24} <= set(nk.tolist())
    for n_keys in (1, 2, 30, 1 << 24):  # LOOP and not, at every key count
        kinds = {int(f) for c in CASES for k, f in zip(c["tab"][0], c["tab"][1]) if k == n_keys}
        assert kinds == {0, 1}, (n_keys, kinds)
    assert {int(f) for c in CASES for f in c["tab"][1]} == {0, 1}
    dts = [dt for c in CASES for dt, _ in c["calls"]]
    first = [c["calls"][0][0] for c in CASES]
    for v in (0.0, -pm.DT, pm.NAN, pm.INF):
        assert _has(dts, v) and _has(first, v), v
    st = np.concatenate([c["states"] for c in CASES])
    for v in (-1.0, -0.0, pm.NAN):
        assert _has(st["speed"], v), v
    for v in (-0.0, -1e-7, 1e30, pm.NAN):
        assert _has(st["x_a"], v) and _has(st["x_b"], v), v
    for field in ("w", "fade"):
        assert _has(st[field], pm.NAN) and _has(st[field], pm.INF) and (st[field] < 0).any(), field
    cm = np.concatenate([cmd for c in CASES for _, cmd in c["calls"]])
    for v in (0.0, -1.0, pm.NAN, pm.INF, pm.DENORMAL):
        assert _has(cm["seconds"], v), v
    assert 0 < float(F(pm.DENORMAL)) < float(np.finfo(np.float32).tiny)
    for v in (-0.0, -1e-7, 1e30, pm.NAN):
        assert _has(cm["x"], v), v
    past = lambda c, field, arr: (arr[field] >= len(c["tab"][0])).any()
    assert any(past(c, "clip_a", c["states"]) for c in CASES) and any(past(c, "clip_b", c["states"]) for c in CASES)
    assert any(past(c, "clip", cmd) for c in CASES for _, cmd in c["calls"])
    lists = [(c["n"], cmd) for c in CASES for _, cmd in c["calls"]]
    assert any(len(cmd) == 0 for _, cmd in lists) and any(len(cmd) == 1 for _, cmd in lists)
    assert any((cmd["instance"] >= n).any() for n, cmd in lists)
    assert any(len(np.unique(cmd["instance"][cmd["instance"] < n])) < (cmd["instance"] < n).sum() for n, cmd in lists)
    # a call without commands directly after a call with commands
    assert any(len(c["calls"][0][1]) > 0 and len(c["calls"][1][1]) == 0 for c in CASES)
    assert {c["nlayers"] for c in CASES} == {2, 8}


def test_every_branch_occurs():
    seen = {k: 0 for k in ("fwd_wrap", "back_wrap", "complete", "below", "above", "cut", "dup_lost", "ended_then_cut", "exact_one", "end_clamp")}
    for c, res, tr in ALL:
        for k in ("fwd_wrap", "back_wrap", "complete", "below", "above", "cut", "exact_one", "end_clamp"):
            seen[k] += int(sum(np.count_nonzero(t[k]) for t in tr) > 0)
        seen["dup_lost"] += int(any(t["dup_lost"] for t in tr))
        # MTR_PLAY_ENDED set by a clamp at the end, and cleared by a later call's cut
        for i in range(len(tr)):
            for j in range(i + 1, len(tr)):
                was = tr[i]["ended"] & tr[i]["end_clamp"] & ((res[i][0]["flags"] & 1) == 1)
                now = tr[j]["cut"] & ((res[j][0]["flags"] & 1) == 0)
                still = np.logical_and.reduce([(res[k][0]["flags"] & 1) == 1 for k in range(i, j)])
                seen["ended_then_cut"] += int((was & now & still).any())
    print("cases in which each branch occurs:", seen)
    assert all(v > 0 for v in seen.values()), seen


def test_outputs_are_defined_for_every_pattern():
    """clip indices clamped, positions -0 or inside [0, P] (a LOOP clip: [0, P)), the user's flag bits kept, speed untouched"""
    for c, res, tr in ALL:
        P, loop = pm.periods(c["tab"])
        C = len(P)
        prev = c["states"]
        for st, os_, ly, sp in res:
            assert (st["clip_a"] < C).all() and (st["clip_b"] < C).all() and (os_["clip_a"] < C).all() and (os_["clip_b"] < C).all()
            for x, clip in ((st["x_a"], st["clip_a"]), (os_["x_a"], os_["clip_a"])):
                assert ((x >= 0) & np.where(loop[clip], x < P[clip], x <= P[clip])).all(), c["name"]
            assert ((st["flags"] ^ prev["flags"]) & 0xFFFFFFFE == 0).all()
            assert pm.same_bits(st["speed"], prev["speed"]).all()
            assert (os_["pad"] == 0).all() and (ly["mask"][:, :2] == 0).all() and (ly["mode"][:, :2] == 0).all()
            assert pm.same_bits(ly[:, 2:], c["layers"][:, 2:]).all()
            assert (sp["w"][:, 0] == 0).all() and pm.same_bits(sp["w"][:, 1], os_["w"]).all()
            prev = st


def test_wrong_readings_are_told_apart():
    shares = {}
    for v in pm.WRONG_VARIANTS:
        can = changed = inst_changed = inst_total = 0
        for c, res, tr in ALL:
            wrong = pm.run_case(c, variant=v)
            differs = np.zeros(c["n"], dtype=bool)
            for a, b in zip(res, wrong):
                for x, y in zip(a, b):
                    ok = pm.same_bits(x, y)
                    differs |= ~(ok.reshape(c["n"], -1).all(axis=1))
            if pm.can_show(v, tr, c["calls"]):
                can += 1
                changed += int(differs.any())
                if differs.any():
                    inst_changed += int(differs.sum())
                    inst_total += c["n"]
            else:
                assert not differs.any(), (v, c["name"], "a case that cannot show the reading is changed by it")
        shares[v] = (changed, can, inst_changed / max(inst_total, 1))
        assert can > 0 and changed > 0, (v, can, changed)
    print("wrong readings: cases changed of those that can show it, share of their instances:")
    for v, (ch, can, sh) in shares.items():
        print(f"  {v}: {ch} of {can}, {100 * sh:.0f} %")


def test_equals_the_host_recipe_without_commands_and_fades():
    """the (x_a', w) of the mtr_anim_state output on a LOOP clip are the host recipe's binary32 numbers, forwards and backwards"""
    tab = pm.table([30, 20], [pm.LOOP, pm.LOOP], [30.0, 24.0])
    n = 64
    rng = np.random.default_rng(5)
    st = np.zeros(n, dtype=pm.PLAY)
    st["clip_a"] = rng.integers(0, 2, n)
    st["x_a"] = rng.uniform(0, 20, n)
    st["speed"] = rng.uniform(0.5, 1.5, n) * np.where(rng.random(n) < 0.25, -1, 1)
    x = st["x_a"].copy()
    N, rate = tab[0][st["clip_a"]], tab[2][st["clip_a"]]
    for _ in range(400):
        st, os_, _, sp = pm.advance(st, pm.DT, tab)
        want = [pm.host_recipe(x[i], pm.DT, st["speed"][i], rate[i], N[i]) for i in range(n)]
        mod = np.mod(x + np.array([w[1] for w in want], dtype=F), N.astype(F))  # what `x = (x + dx) % N` computes in float32
        x = np.array([w[0] for w in want], dtype=F)
        assert mod.dtype == F and pm.same_bits(mod, x).all()
        assert pm.same_bits(os_["x_a"], x).all() and (os_["w"] == 0).all()
        assert pm.same_bits(sp["dx"][:, 0], np.array([w[1] for w in want], dtype=F)).all()
        assert pm.same_bits(st["x_a"], x).all()


def test_a_fade_completes_when_the_accumulated_weight_reaches_one():
    tab = pm.table([30, 20, 40], [pm.LOOP, pm.LOOP, 0], [30.0, 24.0, 30.0])
    for T in (0.05, 0.25, 1.0 / 3.0, 0.5, 1.0):
        st = np.zeros(3, dtype=pm.PLAY)
        st["speed"] = 1.0
        st["x_a"] = (1.0, 2.0, 3.0)
        cm = np.array([(i, 1, 0.5, T) for i in range(3)], dtype=pm.CMD)
        r = F(1) / F(T)
        w, calls = F(0), 0
        while True:  # the accumulated binary32 weight, by the text
            w = F(w + F(F(pm.DT) * r))
            calls += 1
            if w >= 1:
                break
        for k in range(calls + 3):
            st, os_, _, sp = pm.advance(st, pm.DT, tab, cm if k == 0 else None)
            if k < calls - 1:
                assert (st["fade"] > 0).all() and (st["clip_a"] == 0).all() and (os_["w"] > 0).all() and (os_["w"] < 1).all()
            elif k == calls - 1:
                assert (os_["w"] == 1).all() and (os_["clip_a"] == 0).all() and (os_["clip_b"] == 1).all()  # the frame before the swap
                assert (st["clip_a"] == 1).all() and (st["fade"] == 0).all() and (st["w"] == 0).all()
                assert pm.same_bits(st["x_a"], os_["x_b"]).all()
            else:  # afterwards clip B is not read: whatever stands there changes nothing
                other = st.copy()
                other["clip_b"], other["x_b"] = 2, np.nan
                a, b = pm.advance(st, pm.DT, tab), pm.advance(other, pm.DT, tab)
                assert (os_["w"] == 0).all() and (sp["dx"][:, 1] == 0).all()
                assert pm.same_bits(a[0]["x_a"], b[0]["x_a"]).all() and pm.same_bits(a[1]["x_a"], b[1]["x_a"]).all() and (b[1]["w"] == 0).all()


def test_dt_zero_moves_nothing_but_still_clamps_and_flags():
    """on states a player itself produced (positions in range, w in [0, 1], a finite fade): no stored x_a, x_b or w changes;
    the clip indices are still clamped and MTR_PLAY_ENDED is recomputed"""
    for c, res, tr in ALL:
        st = res[-1][0].copy()
        good = np.isfinite(st["fade"]) & np.isfinite(st["speed"])
        idle = ~(st["fade"] > 0)  # a clip index past C where clip B is not playing (its position belongs to the clip it names)
        st["clip_b"][idle] = 0xFFFFFFF0
        st["flags"] ^= 1
        out = pm.advance(st, 0.0, c["tab"])[0]
        C = len(c["tab"][0])
        for k in ("x_a", "x_b", "w"):
            assert pm.same_bits(out[k], st[k])[good].all(), (c["name"], k)
        assert (out["clip_b"] == np.minimum(st["clip_b"], C - 1)).all()
        P, loop = pm.periods(c["tab"])
        ended = ~loop[out["clip_a"]] & (out["x_a"] >= P[out["clip_a"]])
        assert ((out["flags"] & 1) == ended).all()


def test_command_lists():
    c = next(c for c in CASES if c["n"] == 65 and len(c["tab"][0]) == 3)
    st, tab = c["states"], c["tab"]
    none = pm.advance(st, pm.DT, tab)
    empty = pm.advance(st, pm.DT, tab, np.zeros(0, dtype=pm.CMD))
    outside = pm.advance(st, pm.DT, tab, np.array([(65, 1, 2.0, 0.5), (0xFFFFFFFF, 0, 1.0, 0.0)], dtype=pm.CMD))
    for a in (empty, outside):
        assert all(pm.same_bits(x, y).all() for x, y in zip(none[:2] + none[3:], a[:2] + a[3:]))
    # the last of several commands to one instance wins whatever stands between them, and the losers leave no trace
    rng = np.random.default_rng(9)
    last = np.array([(7, 2, 3.0, 0.25)], dtype=pm.CMD)
    alone = pm.advance(st, pm.DT, tab, last)
    for _ in range(5):
        others = pm.make_cmds(rng, 65, 3, 20, [(7, 0, 9.0, 0.0), (7, 1, 1.0, 0.5)])
        others = others[rng.permutation(len(others))]
        full = np.concatenate([others, last])
        got = pm.advance(st, pm.DT, tab, full)
        assert all(pm.same_bits(x[7], y[7]).all() for x, y in zip(got[:2] + got[3:], alone[:2] + alone[3:]))
    # a call without commands right after a call with commands: nothing of the commands is left over
    after = pm.advance(alone[0], pm.DT, tab, None)
    again = pm.advance(alone[0], pm.DT, tab, np.zeros(0, dtype=pm.CMD))
    assert pm.same_bits(after[0], again[0]).all()


def _walk_scene():
    rng = np.random.default_rng(11)
    J = 3
    inplace = am.gentle_clips(rng, J, shape=[(30, am.CLIP_LOOP), (20, am.CLIP_LOOP)])
    traj = rm.walk_clip(31, 1) + rm.walk_clip(21, 1)
    root = (0, np.array([rm.CYCLIC, rm.CYCLIC], dtype=np.uint32))
    tab = pm.table([30, 20], [pm.LOOP, pm.LOOP], [30.0, 24.0])
    return J, inplace, traj, root, tab


def test_chain_poses_and_moves_the_same_positions_as_the_host_recipe():
    """40 calls at dt = 1/30: the player's states through section 14's model and its steps through section 19's model equal
    those models driven by the host recipe wherever no fade runs; while one runs, pose and motion still read one frame"""
    J, inplace, traj, root, tab = _walk_scene()
    n = 9
    rng = np.random.default_rng(12)
    st = np.zeros(n, dtype=pm.PLAY)
    st["clip_a"] = rng.integers(0, 2, n)
    st["x_a"] = rng.uniform(0, 20, n)
    st["speed"] = rng.uniform(0.5, 1.5, n)
    st["speed"][:2] *= -1
    x, clip = st["x_a"].copy(), st["clip_a"].copy()
    M = rm.trs(rng, n)
    M_host = M.copy()
    plain = np.ones(n, dtype=bool)
    for frame in range(40):
        cm = np.array([(i, 1 - clip[i], 0.0, 0.2) for i in (3, 4)], dtype=pm.CMD) if frame == 10 else None
        if frame == 10:
            plain[[3, 4]] = False
        st, os_, _, sp = pm.advance(st, pm.DT, tab, cm)
        # the pose and the motion of the frame read the same clips, and the pose stands where the motion ends
        assert (os_["clip_a"] == sp["clip"][:, 0]).all() and (os_["clip_b"] == sp["clip"][:, 1]).all()
        P = tab[0][os_["clip_a"]].astype(F)
        end = F(sp["x"][:, 0] + sp["dx"][:, 0])
        end = F(end - F(np.floor(F(end / P)) * P))
        assert pm.same_bits(np.where((end >= 0) & (end < P), end, F(0)), os_["x_a"]).all()
        want = [pm.host_recipe(x[i], pm.DT, st["speed"][i], tab[2][clip[i]], tab[0][clip[i]]) for i in range(n)]
        hs = np.zeros(n, dtype=pm.STATE)
        hs["clip_a"], hs["x_a"] = clip, [w[0] for w in want]
        hp = np.zeros((n, 1), dtype=pm.STEP)
        hp["clip"][:, 0], hp["x"][:, 0], hp["dx"][:, 0] = clip, x, [w[1] for w in want]
        pose, pose_host = am.sample(inplace, os_, J), am.sample(inplace, hs, J)
        M = rm.root_motion(M, traj, root, sp.astype(rm.STEP))
        M_host = rm.root_motion(M_host, traj, root, hp.astype(rm.STEP))
        assert pm.same_bits(pose[plain], pose_host[plain]).all() and pm.same_bits(M[plain], M_host[plain]).all(), frame
        x = np.array([w[0] for w in want], dtype=F)
    assert plain.sum() == n - 2 and (st["fade"] == 0).all() and (st["clip_a"][[3, 4]] != clip[[3, 4]]).all()


def test_drift_is_recorded():
    worst, end, wraps = pm.drift()
    print(f"drift of 20 000 binary32 advances against float64: largest {worst:.2e}, at the end {end:.2e} positions, {wraps} wraps")
    assert wraps == 246 and worst < 0.05
