"""CPU: the numpy model of SPEC.md section 24 (tests/spring_model.py) against the section's own statements.

The generator reaches every branch of the rule (counted here): fresh by live == 0, fresh by a state that is not finite,
paused calls, the carry by a motion, kk clamped at 1, ul == 0, the aim's guard failing; L == 0 cannot be reached through a
valid set; the plain path (not fresh, not paused, guard held) is at least half of the (instance, spring) pairs.  Every wrong
reading of the section (sm.WRONG_VARIANTS) changes some case.

Against the float64 twin, ONE spring step from the same binary32 (T, Q, S) and states (longer runs diverge legitimately, and
the chains in front have no bound of their own, section 17), over the plain path of the generator's cases, measured here:
the local matrices differ by at most 1.24e-5 (the springs at depth 60 and 66 of the 70-joint chain; 1.8e-6 on the short
skeletons); | |cur - p_a| - L | <= 3.5e-6 L; a fresh state with zero gravity leaves the local matrices within 5.6e-6 of
what the chains left.  The tests hold four times these figures, as room for other numpy and libm builds.

300 frames on a static clip from a displaced particle at rest, drag 0.2, gravity 0, stiffness 0.6 / s (kk = 0.01: with 0.8
of the velocity kept the step is overdamped for kk <= 0.011): in the float64 twin the distance to rest never grows after
the first frame and ends at 3.6e-10 of its start.  In binary32 the same run ends at 5.8e-6 of its start.  From 2e-5 of the
start downwards the stored positions move by units in the last place, and the distance with them (measured: 2.4e-7 at most).
A coordinate of cur goes through five rounded operations a step (c + v, + kk (r - c), + h g, c - p_a, p_a + (L / ul) u), each
within half an ulp of a coordinate no larger than |p_a| + L, so a frame can move the distance by sqrt(3) * 2.5 such ulps
without the particle moving at all: there the test holds growth to that, and to none above the floor."""
from collections import Counter

import numpy as np
import pytest

from tests import anim_ik_model as ik
from tests import anim_layers_model as lm
from tests import anim_model as am
from tests import spring_model as sm

F = np.float32
MEASURED = dict(locals=1.24e-5, length=3.5e-6, fresh=5.6e-6)  # the largest deviations over the generator's cases (SPEC.md section 24)
ROOM = 4.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _after_chains(c):
    """the binary32 (T, Q, S) the springs of the case start from"""
    T, Q, S = ik.stack_tqs(c["clips"], c["layers"], c["J"], c["masks"])
    if c["chains"] is not None:
        Q = ik.solve(T, Q, S, c["parents"], c["chains"], c["targets"])
    return T, Q, S


def test_the_generator_reaches_every_branch():
    cnt, pairs = Counter(), 0
    for c in sm.cases():
        probe = []
        out, st = sm.run(c, probe=probe)
        assert np.isfinite(out).all() and (st["live"] == 1).all() and (st["pad"] == 0).all()
        assert [p["round"] for p in probe] == sorted(p["round"] for p in probe), "by rounds"
        for p in probe:
            n = c["n"]
            pairs += n
            cnt["dead"] += int(p["dead"].sum())
            cnt["nonfinite"] += int(p["nonfinite"].sum())
            cnt["paused"] += n * int(p["paused"])
            cnt["carried"] += int((~p["fresh"]).sum()) * int(p["carried"])
            cnt["clamped"] += int((~p["fresh"]).sum()) * int(p["clamped"])
            cnt["ul_zero"] += int(p["ul_zero"].sum())
            cnt["L_zero"] += int(p["L_zero"].sum())
            cnt["guard_failed"] += int((~p["guard"]).sum())
            cnt["plain"] += int(p["plain"].sum())
    print(dict(cnt), "of", pairs)
    for branch in ("dead", "nonfinite", "paused", "carried", "clamped", "ul_zero", "guard_failed"):
        assert cnt[branch] > 0, branch
    assert cnt["L_zero"] == 0, "a valid tail has a length"
    assert 2 * cnt["plain"] >= pairs, f"the plain path: {cnt['plain']} of {pairs}"


def test_rounds_follow_ancestry_not_the_list():
    J, parents, joints, _ = sm.SKELETONS["strands9"]
    sp = sm.make_springs(joints, np.ones((4, 3)))
    assert joints == [3, 2, 6, 5] and sm.rounds_of(parents, sp) == [1, 0, 1, 0]
    assert sm.rounds_of(ik.skeleton(70), sm.make_springs([66, 30, 60], np.ones((3, 3)))) == [2, 0, 1]
    assert sm.rounds_of(ik.skeleton(4), sm.make_springs([2], np.ones((1, 3)))) == [0]


# which cases can tell a wrong reading apart at all
NEEDS = {"carry_R": lambda c: c["motion"] is not None, "prev_not_carried": lambda c: c["motion"] is not None,
         "before_ik": lambda c: c["chains"] is not None, "paused_integrates": lambda c: not (c["h"] > 0 and np.isfinite(c["h"])),
         "list_order": lambda c: c["name"] == "strands9"}


@pytest.mark.parametrize("variant", sm.WRONG_VARIANTS)
def test_every_wrong_reading_shows(variant):
    told = 0
    for c in sm.cases():
        if not NEEDS.get(variant, lambda c: True)(c):
            continue
        out, st = sm.run(c)
        wrong, wrong_st = sm.run(c, variant=variant)
        differs = (_bits(wrong) != _bits(out)).any() or (_bits(wrong_st["cur"]) != _bits(st["cur"])).any() or (_bits(wrong_st["prev"]) != _bits(st["prev"])).any()
        told += bool(differs)
    assert told >= 1, variant


def test_one_step_against_the_float64_twin():
    worst = dict(locals=0.0, length=0.0)
    checked = 0
    for c in sm.cases():
        T, Q, S = _after_chains(c)
        sp, st = c["springs"].astype(sm.SPRING), c["states"].astype(sm.STATE)
        probe = []
        Q32, s32 = sm.step(T, Q, S, c["parents"], sp, st, c["h"], c["motion"], probe=probe)
        T64, Q64, S64 = (v.astype(np.float64) for v in (T, Q, S))
        Qt, _ = sm.step(T64, Q64, S64, c["parents"], sp, st, c["h"], c["motion"], dt=np.float64)
        if np.abs(sp["tail"]).max(axis=1).min() < 1e-3:
            continue  # a tail below the resolution of the joint's position: the direction is rounding, in either precision
        plain = np.ones(c["n"], dtype=bool)
        for p in probe:  # ul == 0 in binary32 is a tiny u of any direction in float64
            plain &= ~p["fresh"] & p["guard"] & ~p["ul_zero"]
        assert plain.sum() >= c["n"] // 2
        d = np.abs(ik.local_matrix(T, Q32, S).astype(np.float64) - ik.local_matrix(T64, Qt, S64))[plain].max()
        worst["locals"] = max(worst["locals"], float(d))
        for p in probe:
            k, L = p["k"], p["L"].astype(np.float64)
            dist = np.linalg.norm(s32["cur"][:, k].astype(np.float64) - p["pa"].astype(np.float64), axis=-1)
            worst["length"] = max(worst["length"], float((np.abs(dist - L) / L).max()))  # every instance, whatever its branch
        checked += 1
    print(f"binary32 against float64 over {checked} cases: local matrices {worst['locals']:.3e}, | |cur - pa| - L | / L {worst['length']:.3e}")
    assert checked >= 15
    assert worst["locals"] <= ROOM * MEASURED["locals"], worst
    assert worst["length"] <= ROOM * MEASURED["length"], worst


def test_a_fresh_state_without_gravity_leaves_the_pose():
    worst = 0.0
    for c in sm.cases():
        sp = c["springs"].astype(sm.SPRING).copy()
        if np.abs(sp["tail"]).max(axis=1).min() < 1e-3:
            continue
        sp["gravity"] = 0
        T, Q, S = _after_chains(c)
        nan = np.zeros(c["states"].shape, dtype=sm.STATE)
        nan["cur"], nan["prev"], nan["live"] = np.nan, np.inf, 7
        for states in (np.zeros(c["states"].shape, dtype=sm.STATE), nan):
            Qn, st = sm.step(T, Q, S, c["parents"], sp, states, c["h"], c["motion"])
            js = [int(j) for j in sp["joint"]]
            d = np.abs(ik.local_matrix(T, Qn, S)[:, js].astype(np.float64) - ik.local_matrix(T, Q, S)[:, js])
            worst = max(worst, float(d.max()))
            rest = [j for j in range(c["J"]) if j not in js]
            assert (_bits(Qn[:, rest]) == _bits(Q[:, rest])).all(), "only spring joints change"
            # at rest: prev is the rest position, cur the same put onto the sphere of radius L, a few roundings away
            assert (np.abs(st["cur"] - st["prev"]) <= 4 * np.spacing(np.abs(st["prev"]).max(axis=-1, keepdims=True))).all(), "at rest"
    print(f"a fresh state, zero gravity: the local matrices move by at most {worst:.3e}")
    assert worst <= ROOM * MEASURED["fresh"], worst


def _static_run(dt):
    rng = np.random.default_rng(5)
    J, parents = 4, ik.skeleton(4)
    clips = ik.uniform_scale(am.random_clips(rng, J, trans=2.0))
    ly = np.zeros((1, 1), dtype=lm.LAYER)
    ly["clip"], ly["w"] = 3, 1  # the one-key clip: static
    sp = sm.make_springs([3], [(0.2, 1.0, -0.3)], stiffness=0.6, drag=0.2, gravity=(0.0, 0.0, 0.0))
    probe = []
    sm.sample(clips, ly, J, None, parents, sp, np.zeros((1, 1), dtype=sm.STATE), 1.0 / 60.0, probe=probe, dt=dt)
    r, pa, L = probe[0]["r"][0], probe[0]["pa"][0], probe[0]["L"][0]
    start = (pa + L * np.array([1.0, 0.0, 0.0], dtype=dt)).astype(dt)  # on the sphere, about a radius from rest
    rec = np.zeros((1, 1), dtype=sm.STATE)
    rec["live"] = 1
    rec["cur"], rec["prev"] = start, start
    s64 = (start[None, None, :].copy(), start[None, None, :].copy())
    dist = [np.linalg.norm(start.astype(np.float64) - r)]
    for _ in range(300):
        if dt == F:
            _, rec = sm.sample(clips, ly, J, None, parents, sp, rec, 1.0 / 60.0)
            cur = rec["cur"][0, 0]
        else:
            _, s64 = sm.sample(clips, ly, J, None, parents, sp, rec, 1.0 / 60.0, dt=dt, states64=s64)
            cur = s64[0][0, 0]
        dist.append(np.linalg.norm(cur.astype(np.float64) - r))
    return np.array(dist), float(np.abs(pa).max() + L)


def test_three_hundred_frames_come_to_rest():
    # the rule itself: the float64 twin
    d, _ = _static_run(np.float64)
    assert d[0] > 0.5
    grow = np.diff(d[1:])
    assert (grow <= 0).all(), f"the distance to rest grows at frames {np.argwhere(grow > 0).ravel()[:5] + 2}"
    assert d[-1] < 0.01 * d[0], d[-1] / d[0]
    # binary32: the same, down to where the stored coordinates move by units in the last place
    d32, big = _static_run(F)
    ulp = float(np.spacing(F(big)))
    grow = np.diff(d32[1:])
    above = d32[1:-1] > 2e-5 * d32[0]
    assert above.sum() > 100 and (grow[above] <= 0).all(), "binary32: the distance grows above the rounding floor"
    floor = np.sqrt(3.0) * 2.5 * ulp
    assert (grow <= floor).all(), f"binary32: grows by {grow.max():.3e}, the rounding floor is {floor:.3e}"
    assert d32[-1] < 0.01 * d32[0], d32[-1] / d32[0]
    print(f"float64: ends at {d[-1] / d[0]:.3e} of the start; binary32: {d32[-1] / d32[0]:.3e}, largest growth {grow.max():.3e} (ulp {ulp:.3e})")
