"""CPU: the numpy model of SPEC.md section 25 (tests/match_model.py) has the properties the section states, every wrong reading
of the rule changes a non-zero share of the generator's instances (the shares are printed and quoted in section 25), and the
generator alone meets the caps the GPU tests rely on: exact ties at every size with R >= 32, instances without a winner, NaN
scores, and binary32 winners that differ from the float64 ones only where the costs lie within the section's bound, on under
2 % of the instances."""
import numpy as np
import pytest

from tests import match_model as mm

CASES = mm.cases()
TOTAL = sum(c["n"] for c in CASES)


@pytest.fixture(scope="module")
def right():
    return [mm.search(c["set"], c["play"], c["raw"], c["filt"], c["base"]) for c in CASES]


def _keys(c, S):
    return np.where(mm.candidates(c["set"], c["filt"], c["n"]), mm.order_key(S), 0)


def test_the_generator_covers_the_sizes_and_families():
    assert {c["n"] for c in CASES} == set(mm.NS) and {c["R"] for c in CASES} == set(mm.RS) and {c["D"] for c in CASES} == set(mm.DS)
    for fam in mm.FAMILIES:
        mine = [c for c in CASES if c["family"] == fam]
        assert {c["n"] for c in mine} == set(mm.NS) and {c["R"] for c in mine} == set(mm.RS) and {c["D"] for c in mine} == set(mm.DS)
    full = lambda c: (1 << c["D"]) - 1
    assert any(c["set"]["pose_dims"] == 0 for c in CASES) and any(c["set"]["pose_dims"] == full(c) for c in CASES)
    assert any(0 < c["set"]["pose_dims"] < full(c) for c in CASES) and any(c["raw"] is None for c in CASES)
    assert any(c["set"]["flags"] & mm.INTERRUPT for c in CASES) and any(not c["set"]["flags"] & mm.INTERRUPT for c in CASES)
    assert all(not (c["set"]["rows"]["clip"] == 2).any() for c in CASES), "clip 2 has no rows"
    for c in CASES:  # what mtr_anim_match_create demands of a database
        rows, P, loop = c["set"]["rows"], c["set"]["P"], c["set"]["loop"]
        assert np.isfinite(c["set"]["feats"]).all() and np.isfinite(c["set"]["c"]).all() and (np.diff(rows["clip"].astype(np.int64)) >= 0).all()
        assert (rows["x"] >= 0).all() and (rows["x"] <= P[rows["clip"]]).all() and (rows["x"][loop[rows["clip"]]] < P[rows["clip"]][loop[rows["clip"]]]).all()
        same = np.diff(rows["clip"].astype(np.int64)) == 0
        assert (np.diff(rows["x"])[same] > 0).all()


def test_winner_is_the_greatest_candidate_and_ties_go_to_the_lowest_row(right):
    for c, (cmds, res, S) in zip(CASES, right):
        key = _keys(c, S)
        have = res["row"] != mm.NONE
        assert (have == (key.max(1) > 0)).all(), c["name"]
        for i in np.flatnonzero(have):
            best = np.flatnonzero(key[i] == key[i].max())
            assert res["row"][i] == best[0], (c["name"], i)
        # an instance whose scores are all NaN, or whose filter admits nothing, has no winner and commands nothing
        none = ~have
        assert (cmds["instance"][none] == 0xFFFFFFFF).all() and (res["score"][none].view(np.uint32) == mm.QNAN).all()
        allnan = np.isnan(S).all(1)
        assert not have[allnan].any()


def test_decisions_follow_the_four_reasons(right):
    seen = dict(fade=0, near=0, margin=0, jump=0, on_near=0, on_margin=0)
    for c, (cmds, res, S) in zip(CASES, right):
        s = c["set"]
        L, p, running = mm.lead(s, c["play"])
        jump = cmds["instance"] != 0xFFFFFFFF
        assert (cmds["instance"][jump] == c["base"] + np.flatnonzero(jump)).all() and (cmds["seconds"][jump] == s["seconds"]).all()
        ign = cmds[~jump]
        assert not (ign["clip"].any() or ign["x"].view(np.uint32).any() or ign["seconds"].view(np.uint32).any())
        if not s["flags"] & mm.INTERRUPT:
            assert not jump[running].any()
            seen["fade"] += int(running.sum())
        have, have_cur = res["row"] != mm.NONE, res["cur"] != mm.NONE
        win = np.where(have, res["row"], 0)
        with np.errstate(all="ignore"):
            dist = np.abs((s["rows"]["x"][win] - p).astype(mm.F))
            gain = (res["score"] - res["cur_score"]).astype(mm.F)
        near = have & have_cur & (s["rows"]["clip"][win] == L) & (dist <= s["near"])
        weak = have & have_cur & ~np.isnan(res["cur_score"]) & ~(gain > s["margin"])
        assert not jump[near].any() and not jump[weak].any()
        seen["near"] += int(near.sum()); seen["margin"] += int(weak.sum()); seen["jump"] += int(jump.sum())
        seen["on_near"] += int((near & (dist == s["near"])).sum()); seen["on_margin"] += int((weak & (gain == s["margin"])).sum())
        assert (cmds["clip"][jump] == s["rows"]["clip"][win][jump]).all() and mm.same_bits(cmds["x"][jump], s["rows"]["x"][win][jump]).all()
    assert all(seen.values()), seen  # near and margin sit exactly on their thresholds somewhere


def test_every_wrong_reading_changes_a_share_of_the_instances(right):
    print()
    for v in mm.WRONG_VARIANTS:
        changed = 0
        for c, (cmds, res, S) in zip(CASES, right):
            w = mm.search(c["set"], c["play"], c["raw"], c["filt"], c["base"], variant=v)
            changed += int((~(mm.same_bits(cmds, w[0]) & mm.same_bits(res, w[1]))).sum())
        print(f"  {v:18s} {changed:5d} of {TOTAL} instances, {100.0 * changed / TOTAL:.2f} %")
        assert changed > 0, v


def test_caps_the_gpu_tests_rely_on(right):
    ties_at = {}
    none = nan = differ = beyond = 0
    worst = 0.0
    for c, (cmds, res, S) in zip(CASES, right):
        key = _keys(c, S)
        have = res["row"] != mm.NONE
        ties = int((have & ((key == key.max(1)[:, None]).sum(1) > 1)).sum())
        ties_at[(c["n"], c["R"])] = ties
        none += int((~have).sum())
        nan += int(np.isnan(S).sum())
        # the float64 winner among the same candidates: compared by cost, not by index
        S64, bound = mm.costs64(c["set"], c["play"], c["raw"])
        ok = mm.candidates(c["set"], c["filt"], c["n"]) & np.isfinite(S64)
        S64m = np.where(ok, S64, -np.inf)
        w64, ar = np.argmax(S64m, axis=1), np.arange(c["n"])
        w32 = np.where(have, res["row"], 0)
        fin = have & np.isfinite(S64m[ar, w32]) & np.isfinite(S64m[ar, w64]) & np.isfinite(res["score"])
        with np.errstate(all="ignore"):
            gap = np.where(fin, S64m[ar, w64] - S64m[ar, np.where(fin, w32, w64)], 0.0)
        differ += int((fin & (gap != 0)).sum())
        room = bound[ar, w64] + bound[ar, w32]
        beyond += int((fin & (gap > room)).sum())
        with np.errstate(all="ignore"):
            err = np.abs(S.astype(np.float64) - S64)
            m = np.isfinite(err) & np.isfinite(S) & (bound > 0) & (np.abs(S64) < 3e38)
            assert (err[m] <= bound[m]).all(), c["name"]
            worst = max(worst, float((err[m] / bound[m]).max()) if m.any() else 0.0)
    print(f"\n  no winner {none}, NaN scores {nan}, binary32 and float64 winners differ in cost on {differ} of {TOTAL} instances "
          f"({100.0 * differ / TOTAL:.2f} %), beyond the bound {beyond}; worst score error {worst:.3f} of the bound")
    assert all(t > 0 for (n, R), t in ties_at.items() if R >= 32), ties_at
    assert none > 0 and nan > 0 and beyond == 0 and differ < 0.02 * TOTAL
