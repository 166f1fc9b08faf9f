"""CPU: SPEC.md section 22 (animation events) on the numpy model (tests/events_model.py): the vectorised model equals its
brute-force twin on the whole generator; chained with the player model (tests/player_model.py) over 400 frames of 64 instances
on a LOOP clip in both directions every frame's end position is the player's stored x_a bit for bit and every marker fires once
per passage, the passages counted in exact rationals; chained with the controller model (tests/ctrl_model.py) over 200 frames of
its locomotion graph the jump's end marker fires once per jump and footsteps fire from both clips of a SYNC fade with weights
that sum to 1.  And the generator's census: every branch is reached and every wrong reading changes a case."""
from fractions import Fraction
from math import ceil, floor

import numpy as np

from tests import ctrl_model as cm
from tests import events_model as em
from tests import player_model as pm

F = np.float32


def test_the_model_equals_its_brute_force_twin_on_every_case():
    fired = 0
    for c in em.cases():
        want, twin = em.run_case(c), em.run_case(c, fn=em.brute)
        for a, b, what in zip(want, twin, ("list", "count", "bits")):
            bad = ~em.same_bits(a, b)
            assert a.shape == b.shape and not bad.any(), f"{c['name']} {what}: {int(bad.sum())} differ, first at {np.argwhere(bad)[0]}"
        # the list behind count[1] is what it was, count[1] = min(count[0], capacity), and the masks are the fired ids'
        assert em.same_bits(want[0][int(want[1][1]):], c["out_prev"][int(want[1][1]):]).all() and want[1][1] == min(int(want[1][0]), c["capacity"])
        fired += int(want[1][0])
    assert fired > 10000


def test_the_generator_reaches_every_branch_and_tells_every_wrong_reading():
    reach, changed = em.census()
    cases = em.cases()
    assert len(cases) == 36 and len(em.WRONG_VARIANTS) >= 6
    assert {c["n"] for c in cases} == {1, 5, 63, 64, 65, 257} and {c["S"] for c in cases} == {1, 2, 8}
    assert {k for c in cases for k in c["kinds"]} == set(em.KINDS)
    assert {c["capacity"] == 0 for c in cases} == {True, False}
    print("section 22 census: reach", reach, "changed", changed)
    for k in em.BRANCHES:
        assert reach[k] >= 3, f"{k} is reached in {reach[k]} cases"
    for v in em.WRONG_VARIANTS:
        assert changed[v] >= 1, f"{v} changes no case"
    # the figures SPEC.md section 22 records
    assert reach == dict(fwd_seam=21, back_seam=18, t_eq_P=15, full_fwd=19, full_back=18, end_clamp=12, drop_e0=22, drop_minw=12, truncated=16)
    assert changed == dict(half_open_fwd=20, seam_ignored=20, period_n1=20, ties_reversed=8, e_without_later=11, bits_ored=36, step_major=9)


def test_the_generator_holds_every_special_value():
    tiny = lambda a: ((np.abs(a) > 0) & (np.abs(a) < np.finfo(F).tiny)).any()
    negz = lambda a: ((a == 0) & np.signbit(a)).any()
    kinds = dict(nan=lambda a: np.isnan(a).any(), pinf=lambda a: (a == np.inf).any(), negzero=negz)
    for fname in ("x", "dx", "w"):
        for kname, has in kinds.items():
            if (fname, kname) in (("x", "pinf"), ("w", "pinf"), ("w", "negzero")):
                continue
            assert any(has(c["steps"][fname]) for c in em.cases()), f"no {kname} in {fname}"
    assert any(tiny(c["steps"]["dx"]) for c in em.cases()) and any((c["steps"]["dx"] == -np.inf).any() for c in em.cases())
    assert any((c["steps"]["w"] > 1).any() for c in em.cases()) and any((c["steps"]["x"] == F(1e30)).any() for c in em.cases())
    assert any((c["steps"]["clip"] >= len(c["set"]["counts"])).any() for c in em.cases()), "clip indices past C"
    # positions exactly on a marker and one ulp on either side of one
    on = below = above = 0
    for c in em.cases():
        mx = c["set"]["markers"]["x"]
        if len(mx):
            on += int(np.isin(c["steps"]["x"], mx).sum())
            below += int(np.isin(c["steps"]["x"], np.nextafter(mx, F(-np.inf))).sum())
            above += int(np.isin(c["steps"]["x"], np.nextafter(mx, F(np.inf))).sum())
    assert on > 50 and below > 50 and above > 50
    assert {np.isnan(c["min_weight"]) or c["min_weight"] for c in em.cases()} == {0.0, 0.5, 1.0, True}


# ---- chained with the player -----------------------------------------------------------------------------------------------
def test_chained_with_the_player_the_intervals_abut_and_a_marker_fires_once_per_passage():
    n, frames, N = 64, 400, 30
    tab = pm.table([N], [pm.LOOP], [30.0])
    P = Fraction(N)
    marks = [(0.0, 10), (7.0, 11), (7.0, 12), (15.5, 13), (float(em.pred(N)), 14)]
    es = em.event_set(tab, {0: marks})
    rng = np.random.default_rng(22)
    play = np.zeros(n, dtype=pm.PLAY)
    play["x_a"] = rng.uniform(0, N, n).astype(F)
    play["x_a"][:4] = (0.0, 7.0, float(em.pred(N)), 15.5)  # starts at a marker
    speed = rng.uniform(0.05, 3.0, n).astype(F)
    speed[::7] = rng.uniform(20.0, 29.0, len(speed[::7])).astype(F)  # most of a cycle per frame
    speed[1::2] *= F(-1)
    play["speed"] = speed
    fires = np.zeros((n, len(marks)), dtype=np.int64)
    passages = np.zeros((n, len(marks)), dtype=np.int64)
    seams = 0
    for _ in range(frames):
        play, _, _, steps = pm.advance(play, pm.DT, tab)
        assert (np.abs(steps["dx"][:, 0]) < N).all() and (steps["w"][:, 1] == 0).all()
        out, count, _ = em.collect(es, steps, 0.0, n * len(marks))
        end, r0, y = em.end_position(es, steps)
        assert em.same_bits(end[:, 0], play["x_a"]).all(), "the rule ends where the player stores"
        assert em.same_bits(r0[:, 0], steps["x"][:, 0]).all()
        ev = out[:int(count[0])]
        assert count[0] == count[1] and (ev["where"] & 0x7F000000 == 0).all() and (ev["w"] == 1).all()
        np.add.at(fires, (ev["instance"], ev["id"] - 10), 1)
        for i in range(n):
            a, b = Fraction(float(r0[i, 0])), Fraction(float(y[i, 0]))
            for k, (m, _) in enumerate(marks):
                m = Fraction(float(F(m)))
                if b > a:    # r0 < m + jP <= y
                    passages[i, k] += floor((b - m) / P) - floor((a - m) / P)
                elif b < a:  # y <= m + jP < r0
                    passages[i, k] += ceil((a - m) / P) - ceil((b - m) / P)
        seams += int(((y[:, 0] < 0) | (y[:, 0] >= N)).sum())
    assert (fires == passages).all(), np.argwhere(fires != passages)[:5]
    assert seams > 1000 and fires.min() >= 1 and (fires[:, 1] == fires[:, 2]).all()


# ---- chained with the controller -------------------------------------------------------------------------------------------
END, FOOT_L, FOOT_R = 99, 1, 2


def test_chained_with_the_controller_the_jump_ends_once_and_footsteps_fire_from_both_clips_of_a_fade():
    n, frames, quiet = 64, 200, 24
    g, tab = cm.locomotion(), cm.LOCO_TAB
    es = em.event_set(tab, {cm.WALK: [(8.0, FOOT_L), (24.0, FOOT_R)], cm.RUN: [(4.0, FOOT_L), (12.0, FOOT_R)], cm.JUMP: [(11.0, END)]})
    rng = np.random.default_rng(7)
    st, play = np.zeros(n, dtype=cm.STATE), np.zeros(n, dtype=pm.PLAY)
    play["speed"] = 1.0
    play["x_a"] = np.linspace(0, 29, n).astype(F)
    params = np.zeros((n, 2), dtype=F)
    speed = rng.uniform(0, 3, n).astype(F)
    jumps, ends = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    both = from_a = from_b = 0
    for f in range(frames):
        speed = np.clip(speed + rng.normal(0, 0.15, n).astype(F), 0, 3).astype(F)
        params[:, cm.SPEED] = speed
        if f < frames - quiet:  # a jump takes 11 keys at 0.8 keys per frame: the last ones must have time to end
            params[rng.random(n) < 0.02, cm.TRIGGER] = 1.0
        st, params, cmds, _ = cm.step(g, tab, st, play, params, pm.DT)
        play, frame, _, steps = pm.advance(play, pm.DT, tab, cmds)
        jumps += st["fired"] == 0
        out, count, bits = em.collect(es, steps, 0.0, 4 * n)
        ev = out[:int(count[0])]
        assert count[0] == count[1]
        end = ev[ev["id"] == END]
        np.add.at(ends, end["instance"], 1)
        assert ((end["where"] & 0xFFFFFF) == cm.JUMP).all()
        assert (((bits >> END % 32) & 1) == np.isin(np.arange(n), end["instance"])).all()
        # footsteps while walk fades into run or run into walk: step 0 carries 1 - w, step 1 carries w
        foot = ev[ev["id"] != END]
        fading = frame["w"][foot["instance"]] > 0
        step = (foot["where"] >> 24) & 0x7F
        w = frame["w"][foot["instance"]]
        assert (foot["w"][step == 1] == w[step == 1]).all() and (foot["w"][step == 0] == (F(1) - w)[step == 0]).all()
        from_a += int((fading & (step == 0)).sum())
        from_b += int((fading & (step == 1)).sum())
        for i in np.unique(foot["instance"][fading]):
            mine = foot[(foot["instance"] == i)]
            s_ = (mine["where"] >> 24) & 0x7F
            if (s_ == 0).any() and (s_ == 1).any():
                total = float(mine["w"][s_ == 0][0]) + float(mine["w"][s_ == 1][0])
                assert abs(total - 1.0) <= 2.0 ** -23, total
                both += 1
    assert (ends == jumps).all() and jumps.sum() > n, (ends, jumps)
    assert from_a > 20 and from_b > 20 and both >= 3, (from_a, from_b, both)
