"""CPU: every grid case of tests/match_grid_cases.py has what it is for, from its plan (match_model.grid, which
tests/test_match_launch_plan.py holds to the launcher's rule) and the numpy model alone.  The plan of each forced tuning is
what tests/test_gpu_match_grid.py says it forces; every tie kind that exists under a plan is placed in every case of it and is
a tie the model decides: some instance admits both rows, their order keys are equal and not NaN's, and its winner is the lower
row; without a filter every kind is the winner somewhere among a plan's cases; and the special values of the `large` and
`subnormal` families (NaN and +-inf in the one, zero in the other) occur in tiles that are not the first of their wave, under
the search's plan and under the plan of the call that stores the scores."""
import numpy as np
import pytest

from tests import match_grid_cases as gc
from tests import match_model as mm

# tuning -> (SHARE, slabs, tiles per slab, tiles of the waves of a slab's workgroup, the kinds that exist)
FORCED = {
    "32,1": (True, 1, 10, [[3, 3, 3, 1]], "abcdefh"),
    "0,1": (False, 1, 10, [[10]], "abcdeh"),
    "32,6": (True, 2, 5, [[2, 2, 1, 0], [2, 2, 1, 0]], "abcdefgh"),
    "0,2": (False, 2, 5, [[5], [5]], "abcdegh"),
}


def wave_counts(plan):
    return [[t1 - t0 for t0, t1 in mm.wave_tiles(plan, s)] for s in range(plan["gy"])]


def check_ties(c, S, filt):
    """every placed pair is a tie the model decides for some instance; returns the kinds met"""
    s, n = c["set"], c["n"]
    cand = mm.candidates(s, filt, n)
    key = np.where(cand, mm.order_key(S), 0)
    _, res, _ = mm.search(s, c["play"], c["raw"], filt, c["base"])
    met = ""
    for kind, a, b, k in c["pairs"]:
        assert kind in gc.kind_of(a, b, c["plan"]), (c["name"], kind, a, b)
        assert mm.same_bits(s["feats"][a], s["feats"][b]).all() and s["rows"]["bias"][a] == s["rows"]["bias"][b] and mm.same_bits(S[:, a], S[:, b]).all()
        hit = (res["row"] == a) & cand[:, a] & cand[:, b] & (key[:, a] == key[:, b]) & (key[:, a] > 0) & (key.max(1) == key[:, a])
        if hit.any():
            met += kind
    return met


@pytest.mark.parametrize("tune", gc.TUNES)
def test_forced_plans_and_their_cases(tune):
    share, slabs, tps, waves, kinds = FORCED[tune]
    plan = gc.plan_of(tune, gc.FORCED_N, gc.FORCED_R)
    assert (plan["share"], plan["gy"], plan["tiles_per_slab"], wave_counts(plan)) == (share, slabs, tps, waves), plan
    assert plan["gx"] == (3 if share else 1) and plan["ngroups"] == 3 and gc.FORCED_N % 32 and gc.FORCED_R % 32 == 12 and plan["ntiles"] == 10
    assert max(max(w) for w in waves) >= 2, "some wave pipelines at least two tiles"
    if share:
        assert any(0 < w[k + 1] < w[k] for w in waves for k in range(3)), "a SHARE wave with fewer tiles than its neighbour"
    if tune == "32,6":
        assert all(w[3] == 0 for w in waves), "a SHARE wave with no tile: its key in the LDS join is 0"
    if tune == "0,1":
        assert plan["gx"] * 4 > plan["ngroups"], "the workgroup's fourth wave has no instance group and returns"
    assert "".join(k for k, _, _ in gc.place_pairs(plan)) == kinds
    assert not gc.plan_of(tune, gc.FORCED_N, gc.FORCED_R, scores=True)["share"], "a scores call is wave-owned under every tuning"

    cases = gc.forced_cases(tune)
    assert [(c["family"], c["D"]) for c in cases] == [(f, gc.forced_width(gc.TUNES.index(tune), g)) for g in range(1, 9) for f in mm.FAMILIES]
    assert sorted({(c["D"] + 7) // 8 for c in cases}) == list(range(1, 9))
    top, special = set(), {"nan": 0, "inf": 0, "zero": 0}
    for c in cases:
        assert (c["n"], c["R"]) == (gc.FORCED_N, gc.FORCED_R) and "".join(sorted(k for k, _, _, _ in c["pairs"])) == kinds
        S = mm.search(c["set"], c["play"], c["raw"], None)[2]
        assert check_ties(c, S, c["filt"]) == "".join(k for k, _, _, _ in c["pairs"]), c["name"]
        top.update(check_ties(c, S, None))
        later = np.array([not gc.first_tile_of_its_wave(r // 32, plan) and not gc.first_tile_of_its_wave(r // 32, gc.plan_of(tune, c["n"], c["R"], True))
                          for r in range(c["R"])])
        if c["family"] == "large":
            assert np.isnan(S[:, later]).any() and np.isinf(S[:, later]).any(), c["name"]
        if c["family"] == "subnormal":
            assert (S[:, later] == 0).any(), c["name"]
        if c["family"] in ("large", "subnormal"):
            special["nan"] += int(np.isnan(S[:, later]).sum())
            special["inf"] += int(np.isinf(S[:, later]).sum())
            special["zero"] += int((S[:, later] == 0).sum())
    assert top == set(kinds), "without a filter every kind is the winner in some case"
    assert all(special.values()), special


def test_width_cases_of_the_default_tuning():
    cases = gc.width_cases()
    share = [c for c in cases if (c["n"], c["R"]) == gc.WIDTHS_SHARE]
    owned = [c for c in cases if (c["n"], c["R"]) == gc.WIDTHS_OWNED]
    assert [c["D"] for c in share] == list(range(4, 68, 4)) and [c["D"] for c in owned] == list(range(8, 72, 8)) and len(cases) == 24
    for group in (share, owned):
        padded = {c["family"] for c in group if c["D"] % 8}
        assert {c["family"] for c in group if c["D"] % 8 == 0} == set(mm.FAMILIES) and padded in (set(), set(mm.FAMILIES))
    p = share[0]["plan"]
    assert p == mm.grid(33, 97) and (p["share"], p["gx"], p["gy"], p["tiles_per_slab"]) == (True, 2, 4, 1) and 33 % 32 == 1 and 97 % 32 == 1
    p = owned[0]["plan"]
    assert p == mm.grid(1025, 65) and (p["share"], p["gx"], p["gy"], p["tiles_per_slab"], p["ngroups"]) == (False, 9, 3, 1, 33) and 4 * p["gx"] - p["ngroups"] == 3
    top = set()
    for c in cases:
        kinds = "".join(k for k, _, _, _ in c["pairs"])
        assert "".join(sorted(kinds)) == "abcdg", c["name"]  # one tile per slab: nothing else exists
        S = mm.search(c["set"], c["play"], c["raw"], None)[2]
        assert check_ties(c, S, c["filt"]) == kinds, c["name"]
        top.update(check_ties(c, S, None))
    assert top == set("abcdg")


def test_owner_is_the_lane_layout_of_the_result():
    """lane l of a wave holds rows 8 (i >> 2) + 4 (l >> 5) + (i & 3) of its tile in register i"""
    plan = gc.plan_of("32,6", gc.FORCED_N, gc.FORCED_R)
    seen = set()
    for row in range(gc.FORCED_R):
        slab, wave, tile, half, reg = mm.owner(row, plan)
        assert row == 32 * tile + 8 * (reg >> 2) + 4 * half + (reg & 3) and tile // 5 == slab
        t0, t1 = mm.wave_tiles(plan, slab)[wave]
        assert t0 <= tile < t1
        seen.add((tile, half, reg))
    assert len(seen) == gc.FORCED_R
