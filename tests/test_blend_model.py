"""CPU: the numpy model of SPEC.md section 23 (tests/blend_model.py) holds what the section states -- every branch is reached
and every wrong reading changes a case (the counts stand in the section), a parameter at a sample gives that sample share 1, all
three positions are at one phase and below their periods over a 400-frame chain, the shares lie in [0, 1] with their sum
within the section's bound and follow the float64 twin across interior edges, rounding cracks and the hull, dt = 0 stores a
self-produced state unchanged, a NaN parameter plays the first sample and heals -- and chains with the models it feeds: the
layers through tests/anim_layers_model.py and the steps through tests/root_model.py equal one clip played alone at a sample
point, 400 frames through tests/events_model.py count the passages that the abutment of section 23 costs (printed, a record),
and what anim_blend.build_2d returns passes the creation check."""
import os
from math import ceil, floor

import numpy as np
import pytest

from mt_renderer_amd import anim_blend, api
from tests import anim_layers_model as lm
from tests import anim_model as anm
from tests import blend_model as bm
from tests import events_model as em
from tests import player_model as pm
from tests import root_model as rm

F = np.float32
U = bm.U
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALK_RUN = pm.table([32, 16], [pm.LOOP, pm.LOOP], [30.0, 30.0])


def _spec23():
    text = open(os.path.join(ROOT, "SPEC.md")).read()
    return text[text.index("## 23."):]


def _states(n, phase=0.25, speed=1.0, px=0.0, py=0.0):
    st = np.zeros(n, dtype=bm.STATE)
    st["phase"], st["speed"], st["px"], st["py"] = phase, speed, px, py
    return st


# ---- the generator --------------------------------------------------------------------------------------------------------
def test_every_branch_is_reached_and_every_wrong_reading_changes_a_case():
    reach, told, ncases = bm.census()
    print("cases", ncases, "branches", reach, "wrong readings", told)
    assert ncases == 36 and len(bm.WRONG_VARIANTS) >= 8
    assert all(reach[b] > 0 for b in bm.BRANCHES), reach
    assert all(told[v] > 0 for v in bm.WRONG_VARIANTS), told
    spec = _spec23()
    for name, count in list(reach.items()) + list(told.items()):
        assert f"`{name}` {count}" in spec, f"SPEC.md section 23 records {name} {count}"
    # one wave of the 64- and 65-instance cases holds lanes inside different triangles and lanes in the fallback
    for c in (c for c in bm.cases() if c["n"] in (64, 65) and c["set"]["tris"].size > 1):
        tr = {}
        bm.run_case(c, trace=tr, ncalls=1)
        assert tr["tri_first"] and tr["tri_later"] and tr["fb_outside"], (c["name"], tr)


def test_the_generator_covers_what_the_section_lists():
    cs = bm.cases()
    assert {c["n"] for c in cs} == {1, 5, 63, 64, 65, 257} and all(len(c["calls"]) == 3 for c in cs)
    assert {c["set"]["samples"].size for c in cs if not c["set"]["tris"].size} == {1, 2, 5}
    assert {c["set"]["tris"].size for c in cs if c["set"]["tris"].size} == {1, 8}
    assert {int(k) for c in cs for k in c["set"]["tab"][0]} >= {1, 2, 30, 32, 16, 1 << 24}
    assert {float(c["set"]["damp"]) for c in cs} >= {np.inf, 4.0, float(F(pm.DENORMAL))}
    pr = np.concatenate([p.reshape(-1) for c in cs for _, p in c["calls"]])
    ph = np.concatenate([c["states"]["phase"] for c in cs])
    px = np.concatenate([c["states"]["px"] for c in cs])
    assert np.isnan(pr).any() and np.isposinf(pr).any() and np.isneginf(pr).any() and ((pr == 0) & np.signbit(pr)).any() and (pr == F(pm.DENORMAL)).any()
    assert np.isnan(ph).any() and (ph == 1).any() and (ph == F(1e30)).any() and ((ph == 0) & np.signbit(ph)).any() and np.isnan(px).any() and np.isinf(px).any()
    assert all(bm.check_set(c["set"]) is None for c in cs)
    assert {c["nlayers"] for c in cs} == {3, 5, 8}


# ---- consequences -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(bm.SPACES)))
def test_a_parameter_at_a_sample_gives_it_share_one(si):
    bs = bm.make_space(si, bm.CLIPSETS[3], 2, np.inf)
    s = bs["samples"]
    K = s.size
    params = np.zeros((K, 2), dtype=F)
    params[:, bs["param_x"]], params[:, bs["param_y"]] = s["px"], s["py"]
    st, ly, sp, sh = bm.advance(bs, _states(K), params, pm.DT, 3)
    dense = bm.dense_shares(bs, s["px"], s["py"])
    assert (dense == np.eye(K)).all(), "the sample's share is exactly 1, every other exactly 0"
    e = ly["w"][:, 1:]
    assert ((e == 0) | (e == 1)).all(), "the other layers are not read (e == 0) or replace everything (e == 1)"
    # the clip that ends up on top is the sample's
    top = np.where(e[:, 1] == 1, ly["clip"][:, 2], np.where(e[:, 0] == 1, ly["clip"][:, 1], ly["clip"][:, 0]))
    assert (top == s["clip"]).all()


def test_one_phase_for_all_three_positions_over_400_frames():
    n = 64
    for tab, exact in ((WALK_RUN, True), (pm.table([30, 2, 1 << 24], [pm.LOOP] * 3, [30.0, 3.0, 1.0e6]), False)):
        C = len(tab[0])
        bs = bm.blend_set(tab, [(k % C, float(k)) for k in range(4)], None, nparams=1, damp=4.0)
        rng = np.random.default_rng(5)
        st = _states(n, phase=rng.uniform(0, 1, n), speed=rng.uniform(-2, 2, n), px=rng.uniform(0, 3, n))
        P, _ = pm.periods(tab)
        for f in range(400):
            params = (1.5 + 2.0 * np.sin(0.05 * f + np.arange(n))).astype(F)[:, None]
            st, ly, sp, sh = bm.advance(bs, st, params, pm.DT, 3)
            Pi = P[ly["clip"].astype(np.int64)]
            assert (ly["x"] < Pi).all() and (ly["x"] >= 0).all(), "phi' * P < P always"
            assert ((st["phase"] >= 0) & (st["phase"] < 1)).all()
            want = st["phase"].astype(np.float64)[:, None] * Pi.astype(np.float64)
            assert (np.abs(ly["x"].astype(np.float64) - want) <= U * want).all(), "one rounding of phi' * P"
            if exact:
                assert (ly["x"] / Pi == st["phase"][:, None]).all(), "periods that are powers of two: exactly one phase"
    # the largest phase and every period up to 2^24: the product stays below the period
    top = np.nextafter(F(1), F(0))
    Ps = np.concatenate([np.arange(1, 4097), 2 ** np.arange(12, 25), (1 << 24) - np.arange(1, 200)]).astype(F)
    assert (top * Ps < Ps).all()


def _points_near_edges(bs, rng, m=400):
    """points on every edge of every triangle, and their neighbours one unit in the last place to every side"""
    sx, sy = bs["samples"]["px"].astype(np.float64), bs["samples"]["py"].astype(np.float64)
    out = []
    for v in bs["tris"]["v"]:
        for a, b in ((v[0], v[1]), (v[1], v[2]), (v[2], v[0])):
            t = rng.uniform(0, 1, m)
            q = np.stack([sx[a] + t * (sx[b] - sx[a]), sy[a] + t * (sy[b] - sy[a])], axis=1).astype(F)
            up, dn = np.nextafter(q, F(np.inf)), np.nextafter(q, F(-np.inf))
            out += [q, up, dn, np.stack([up[:, 0], dn[:, 1]], axis=1), np.stack([dn[:, 0], up[:, 1]], axis=1)]
    return np.concatenate(out)


@pytest.mark.parametrize("si", (3, 4, 5))
def test_shares_follow_the_float64_twin_across_edges_cracks_and_the_hull(si):
    bs = bm.make_space(si, bm.CLIPSETS[3], 2, np.inf)
    rng = np.random.default_rng(40 + si)
    s = bs["samples"]
    lo, hi = np.array([s["px"].min(), s["py"].min()]), np.array([s["px"].max(), s["py"].max()])
    pts = np.concatenate([_points_near_edges(bs, rng), bm.crack_points(bs), (lo + rng.uniform(-0.5, 1.5, (4000, 2)) * (hi - lo)).astype(F)])
    sl, e1, e2 = bm.find_slots(bs, pts[:, 0], pts[:, 1])
    sh = bm.shares_of(e1, e2)
    assert ((sh >= 0) & (sh <= 1)).all() and ((e1 >= 0) & (e1 <= 1) & (e2 >= 0) & (e2 <= 1)).all(), "the shares lie in [0, 1]"
    total = sh.astype(np.float64).sum(axis=1)
    sl64, f1, f2 = bm.find_slots(bs, pts[:, 0], pts[:, 1], np.float64)
    total64 = bm.shares_of(f1, f2).sum(axis=1)
    print(bm.SPACES[si][0], "share sum: worst |sum - twin's|", float(np.abs(total - total64).max()), "bound", bm.SUM_BOUND)
    assert (np.abs(total - total64) <= bm.SUM_BOUND + 4 * 2.0 ** -53).all()
    # continuity: whichever triangle, crack or edge a point lands in, each sample's share is the twin's within the bound of the
    # section: 2 k u kappa, k = 15 operations on the longest path, kappa = 8 R^2 / A_min the conditioning of the space
    R = float(max(np.abs(pts).max(), np.abs(s["px"]).max(), np.abs(s["py"]).max()))
    A_min = min(float(bm.area2(*(s[f][int(i)].astype(np.float64) for i in v for f in ("px", "py")))) for v in bs["tris"]["v"])
    bound = 2 * 15 * U * 8 * R * R / A_min
    d32, d64 = bm.dense_shares(bs, pts[:, 0], pts[:, 1]), bm.dense_shares(bs, pts[:, 0], pts[:, 1], np.float64)
    worst = float(np.abs(d32 - d64).max())
    print(bm.SPACES[si][0], "dense shares: worst |binary32 - twin|", worst, "bound", bound, "fallback points", int((sl[:, 0] == sl[:, 2]).sum()))
    assert worst <= bound
    if si == 5:
        hit32 = bm._hit32(bs, pts[:, 0], pts[:, 1])
        assert (~hit32 & bm._hit64(bs, pts[:, 0], pts[:, 1])).sum() > 100, "rounding cracks are among the points"


def test_dt_zero_stores_a_self_produced_state_unchanged():
    for c in bm.cases():
        bs = c["set"]
        st = bm.run_case(c)[-1][0]
        params = np.nan_to_num(c["calls"][2][1], nan=0.5, posinf=2.0, neginf=-2.0)
        params = np.clip(params, -1e6, 1e6).astype(F)
        st1 = bm.advance(bs, st, params, pm.DT)[0]           # a state made by the rule from finite targets
        st2 = bm.advance(bs, st1, params, 0.0)[0]
        # bit for bit, but for a smoothed parameter of -0, which -0 + 0 * d turns into +0 (the section says so)
        for k in ("px", "py"):
            zero = (st1[k] == 0) & (st2[k] == 0)
            st2[k][zero] = st1[k][zero]
        assert bm.same_bits(st2, st1).all(), c["name"]


@pytest.mark.parametrize("si", (2, 4, 5))
def test_a_nan_parameter_plays_the_first_sample_and_heals(si):
    for damp in (np.inf, 4.0):
        bs = bm.make_space(si, bm.CLIPSETS[3], 2, damp)
        two_d = bs["tris"].size > 0
        n = 4
        params = np.full((n, 2), 0.3, dtype=F)
        params[0, bs["param_x"]] = np.nan
        if two_d:
            params[1, bs["param_y"]] = np.nan
        st, ly, sp, sh = bm.advance(bs, _states(n, px=0.2, py=0.1), params, pm.DT, 3)
        first = int(bs["tris"]["v"][0][0]) if two_d else 0
        for i in ((0, 1) if two_d else (0,)):
            assert (ly["clip"][i] == bs["samples"]["clip"][first]).all() and (ly["w"][i] == 0).all() and (sh[i] == (1, 0, 0)).all()
        assert np.isnan(st["px"][0])
        good = np.full((n, 2), 0.3, dtype=F)
        st2, ly2, _, sh2 = bm.advance(bs, st, good, pm.DT, 3)
        assert (st2["px"][0] == F(0.3)) and np.isfinite(st2["py"]).all(), "the stored NaN is replaced by the next finite target"
        fresh = bm.advance(bs, _states(n, px=0.3, py=st["py"], phase=st["phase"]), good, pm.DT, 3)  # as if px had been at the target
        assert bm.same_bits(ly2[0], fresh[1][0]).all()


# ---- chains -----------------------------------------------------------------------------------------------------------------
def test_at_a_sample_the_layers_and_steps_equal_the_one_clip_played_alone():
    J = 5
    rng = np.random.default_rng(9)
    tab = pm.table([30, 32, 16, 2], [pm.LOOP] * 4, [30.0, 32.0, 24.0, 3.0])
    clips = anm.gentle_clips(rng, J, shape=[(30, anm.CLIP_LOOP), (32, anm.CLIP_LOOP), (16, anm.CLIP_LOOP), (2, anm.CLIP_LOOP)])
    traj = rm.walk_clip(31, 1) + rm.walk_clip(33, 1) + rm.walk_clip(17, 1) + rm.walk_clip(3, 1)
    rflags = np.array([rm.CYCLIC] * 4, dtype=np.uint32)
    P, _ = pm.periods(tab)
    for si in range(len(bm.SPACES)):
        bs = bm.make_space(si, tab, 2, np.inf)
        s = bs["samples"]
        K = s.size
        params = np.zeros((K, 2), dtype=F)
        params[:, bs["param_x"]], params[:, bs["param_y"]] = s["px"], s["py"]
        st = _states(K, phase=rng.uniform(0, 1, K), speed=rng.uniform(0.5, 1.5, K))
        for f in range(3):  # a chain: the state of one frame is the next one's
            phi0 = st["phase"].copy()
            st, ly, sp, sh = bm.advance(bs, st, params, pm.DT, 3)
            alone = np.zeros((K, 1), dtype=lm.LAYER)
            alone["clip"][:, 0], alone["x"][:, 0] = s["clip"], st["phase"] * P[s["clip"]]
            # bit for bit where the other layers are at e == 0 and not read: every sample of a 1-D space, v0 of a triangle.  At
            # v1 or v2 the sample's layer is at e == 1 and goes through section 14's lerp, v0 + 1 * (v1 - v0), and a second
            # renormalisation: equal within the operations of one layer step and the local matrix, (21 + 24) u on terms <= 2
            exact = (ly["w"][:, 1] == 0) & (ly["w"][:, 2] == 0)
            assert exact.any() and (exact.all() or bs["tris"].size)
            near = (lm.K_STEP[("uniform", lm.OVERRIDE)] + anm.K_LOCALS) * U * 2
            got, want = lm.sample(clips, ly.astype(lm.LAYER), J, None), lm.sample(clips, alone, J, None)
            assert pm.same_bits(got[exact], want[exact]).all(), f"{bm.SPACES[si][0]} frame {f}: the pose of the sample's clip at phi' * P"
            assert (np.abs(got.astype(np.float64) - want) <= near).all(), f"{bm.SPACES[si][0]} frame {f}: the pose at e == 1"
            one = np.zeros((K, 1), dtype=rm.STEP)
            one["clip"][:, 0], one["x"][:, 0] = s["clip"], phi0 * P[s["clip"]]
            one["dx"][:, 0] = sp["dx"][np.arange(K), np.argmax(sp["clip"] == s["clip"][:, None], axis=1)]
            got, want = rm.deltas(traj, (0, rflags), sp.astype(rm.STEP)), rm.deltas(traj, (0, rflags), one)
            assert pm.same_bits(got[exact], want[exact]).all(), f"{bm.SPACES[si][0]} frame {f}: the motion of the sample's clip"
            assert (np.abs(got.astype(np.float64) - want) <= near * (1 + np.abs(want))).all(), f"{bm.SPACES[si][0]} frame {f}: the motion at e == 1"


def test_400_frames_through_the_events_model_count_what_the_abutment_costs():
    """markers at every integer key of the walk and the run; the parameter swept through a 1-D space.  A marker within a unit
    in the last place of a frame boundary can fire in both frames or in neither: counted, printed, and recorded in section 23."""
    n, frames = 64, 400
    tab = WALK_RUN
    bs = bm.blend_set(tab, [(0, 0.0), (1, 2.0), (0, 4.0)], None, nparams=1, damp=4.0)
    es = em.event_set(tab, {0: [(float(k), k) for k in range(32)], 1: [(float(k), 100 + k) for k in range(16)]})
    P, _ = pm.periods(tab)
    rng = np.random.default_rng(23)
    st = _states(n, phase=rng.uniform(0, 1, n), speed=rng.uniform(0.3, 1.6, n), px=rng.uniform(0, 4, n))
    st["speed"][1::4] *= F(-1)
    prev_end = None
    fired = double = missed = pairs = 0
    where = []
    for f in range(frames):
        params = (2.0 + 2.6 * np.sin(0.03 * f + 0.4 * np.arange(n))).astype(F)[:, None]
        st, _, sp, sh = bm.advance(bs, st, params, pm.DT)
        assert (np.abs(sp["dx"]) < P[sp["clip"].astype(np.int64)]).all()
        out, count, _ = em.collect(es, sp, 0.0, 16 * n)
        assert count[0] == count[1]
        fired += int(count[0])
        end, r0, _ = em.end_position(es, sp)
        assert em.same_bits(r0, sp["x"]).all(), "phi0 * P lies in [0, P): the event rule takes it as it is"
        live = np.ones((n, 3), dtype=bool)
        live[:, 1:] = sp["w"][:, 1:] > 0  # section 22: a step i >= 1 with e_i == 0 fires nothing
        cur = {}
        for i in range(n):
            for k in range(3):
                c = int(sp["clip"][i, k])
                if live[i, k] and (i, c) not in cur:
                    cur[(i, c)] = (float(sp["x"][i, k]), float(end[i, k]), float(sp["dx"][i, k]))
        if prev_end is not None:
            for key, (x0, _, dx) in cur.items():
                if key not in prev_end or dx == 0:
                    continue
                a, b, Pc = prev_end[key][1], x0, float(P[key[1]])  # where the last frame ended, where this one starts
                pairs += 1
                if a == b:
                    continue
                d = b - a
                d = d - Pc if d > Pc / 2 else d + Pc if d < -Pc / 2 else d
                lo, hi = min(a, a + d), max(a, a + d)
                k_ = (floor(hi) - floor(lo)) if dx > 0 else (ceil(hi) - ceil(lo))  # integers in (lo, hi] forward, [lo, hi) backward
                if k_:
                    gap = (d > 0) == (dx > 0)  # the start lies ahead of the end: the markers between are never covered
                    missed, double = missed + (k_ if gap else 0), double + (0 if gap else k_)
                    where.append((f, key[0], key[1], "missed" if gap else "twice"))
        prev_end = cur
    print(f"abutment: {fired} events over {frames} frames of {n} instances, {pairs} (instance, clip) frame boundaries, fired twice {double}, not at all {missed}: {where}")
    assert fired > 20000 and pairs > 30000
    assert f"fired twice {double}, not at all {missed}" in _spec23(), "SPEC.md section 23 records the measured count"


# ---- the Python helpers ------------------------------------------------------------------------------------------------------
def test_build_2d_output_passes_the_creation_check():
    rng = np.random.default_rng(31)
    tab = pm.table([30, 32, 16], [pm.LOOP] * 3, [30.0, 32.0, 24.0])
    for trial in range(60):
        K = int(rng.integers(3, 33))
        scale = float(rng.choice([1.0, 1e-3, 1e4]))
        if trial % 4 == 0:    # a lattice: points on common lines and circles
            g = [(x, y) for x in range(6) for y in range(6)]
            pts = np.array([g[i] for i in rng.permutation(36)[:K]], dtype=np.float64) * scale
        else:
            pts = rng.uniform(-1, 1, (K, 2)) * scale
        if trial % 5 == 1:    # three points on a line among the others
            pts[2] = (pts[0] + pts[1]) / 2
        rows = [(float(x), float(y), int(i % 3)) for i, (x, y) in enumerate(pts)]
        samples, tris = anim_blend.build_2d(rows)
        assert samples.dtype == api.BLEND_SAMPLE and tris.dtype == api.BLEND_TRI and samples.size == K and 1 <= tris.size <= 64
        bs = bm.blend_set(tab, [(c, x, y) for x, y, c in rows], [tuple(int(i) for i in v) for v in tris["v"]], nparams=2, param_x=0, param_y=1, damp=4.0)
        assert bm.check_set(bs) is None, (trial, bm.check_set(bs))
        # the triangles cover the hull: a point inside the box of the points that no triangle holds lies outside the hull or on a sliver
        if trial % 4:
            inner = pts.mean(axis=0)
            d = anim_blend.shares(samples, tris, inner)
            assert abs(d.sum() - 1) < 1e-9 and (d >= 0).all()
    for bad in ([(0, 0, 0), (1, 1, 0), (2, 2, 0), (3, 3, 0)],                 # all on one line: no triangle
                [(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 0, 1)],                 # a duplicate point
                [(0, 0, 0), (1, 0, 0)], [(0, 0, 0), (1, 0, 0), (0, np.nan, 0)], [(0, 0), (1, 0), (0, 1)]):
        with pytest.raises(api.MtrError):
            anim_blend.build_2d(bad)
    s1 = anim_blend.build_1d([(4.0, 2), (0.0, 0), (1.4, 1)])
    assert list(s1["px"]) == [0.0, F(1.4), 4.0] and list(s1["clip"]) == [0, 1, 2]
    assert bm.check_set(bm.blend_set(tab, [(int(c), float(x)) for c, x in zip(s1["clip"], s1["px"])])) is None
    for bad in ([(0.0, 0), (0.0, 1)], [(np.inf, 0)], [], [(-3e38, 0), (3e38, 1)]):
        with pytest.raises(api.MtrError):
            anim_blend.build_1d(bad)
    assert np.allclose(anim_blend.shares(s1, None, 0.7), [0.5, 0.5, 0]) and list(anim_blend.shares(s1, None, float("nan"))) == [1, 0, 0]
