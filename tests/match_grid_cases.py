"""The grid cases of motion matching: a second generator next to match_model.cases(), built on make_case's value families, for
what the 24 cases cannot reach under the default tuning -- every feature width, several tiles per wave (the software pipeline
of k_match_search), SHARE waves with fewer tiles than their neighbours and with none, several slabs of several tiles, and ties
placed by the plan: for a grid plan (match_model.grid) `place_pairs` puts one pair of rows with equal features and bias of each
kind that exists under it

  a  one lane, one register quad          (r, r + 1)
  b  one lane, two register quads         (r, r + 8)
  c  the two half-waves, lower row in 0   (r, r + 4), r % 8 < 4
  d  the two half-waves, lower row in 1   rows 4 and 8 of a tile
  e  two tiles of one wave
  f  two waves of one SHARE workgroup in one slab
  g  two slabs
  h  both rows in a last tile that is partly padding

in a tile that is not the first of its wave where the plan has one, and for e to h with the lower row in half-wave 1 and the
upper in half-wave 0, so that "the lower row wins" and "half-wave 0 wins" differ.  The tag word holds the eight group bits,
six pair bits, ZERO_BIT and seventeen free bits, so pairs seven and eight take the two bits above ZERO_BIT
(match_model.pair_bit) and all kinds of a plan live in one case.  Pair k's bias is -big (1 + k), so the last pair of the list
is the best row of all and every pair the best of what a filter leaves that excludes the pairs behind it; the list is rotated
from case to case, so every kind is the winner of the calls without a filter somewhere.  The filters of five instances in
eight are replaced: in turn for each pair, one that excludes every other pair (the pair wins against all other rows) and one
that requires the pair's bit (the two rows are the only candidates, so they tie whatever the score is, +-inf too, unless it
is NaN).  The other instances keep the filters and the special queries make_case gave them.

tests/test_match_grid_premises.py asserts, without a device, that every case has what it is for."""
import numpy as np

from tests import match_model as mm

KINDS = "abcdefgh"
TUNES = ("32,1", "0,1", "32,6", "0,2")  # share_groups,target as MTR_MATCH_TUNE reads them
FORCED_N, FORCED_R = 65, 300
WIDTHS_SHARE = (33, 97)  # SHARE, two groups, the second with one live lane; four tiles, the last with one row
WIDTHS_OWNED = (1025, 65)  # wave-owned, 33 groups: the last workgroup's last three waves have no group
ALL_PAIR_BITS = sum(mm.pair_bit(k) for k in range(8))


def plan_of(tune, n, R, scores=False):
    """the plan of a call under a tuning string (None: the defaults)"""
    if tune is None:
        return mm.grid(n, R, scores)
    share_groups, target = (int(v) for v in tune.split(","))
    return mm.grid(n, R, scores, share_groups, target)


def first_tile_of_its_wave(tile, plan):
    slab = tile // plan["tiles_per_slab"]
    return any(t0 == tile for t0, t1 in mm.wave_tiles(plan, slab) if t0 < t1)


def kind_of(a, b, plan):
    """the kinds (a string of letters) that the pair of rows a < b is under a plan"""
    (sa, wa, ta, ha, ia), (sb, wb, tb, hb, ib) = mm.owner(a, plan), mm.owner(b, plan)
    out = ""
    if ta == tb:
        if ha == hb and ia >> 2 == ib >> 2:
            out += "a"
        if ha == hb and ia >> 2 != ib >> 2:
            out += "b"
        if (ha, hb) == (0, 1):
            out += "c"
        if (ha, hb) == (1, 0):
            out += "d"
        if ta == plan["ntiles"] - 1 and plan["R"] % 32:
            out += "h"
    elif sa != sb:
        out += "g"
    elif wa != wb:
        out += "f"
    else:
        out += "e"
    return out


def place_pairs(plan):
    """[(kind, a, b)] in the order of KINDS, one pair for every kind that exists under the plan, no row used twice.  Rows whose
    index is 0 or 1 modulo 7 are left alone where the kind can be had without them: the subnormal family keeps its rows of
    zeroes there (grid_case takes ZERO_BIT off a pair's rows, which stop being rows of zeroes)."""
    R, ntiles = plan["R"], plan["ntiles"]
    used, tiles_used, out = set(), {}, []
    free = lambda r, spare: 0 <= r < R and r not in used and (r % 7 > 1 or not spare)

    def candidates(kind):
        tiles = sorted(range(ntiles), key=lambda t: (tiles_used.get(t, 0), first_tile_of_its_wave(t, plan), t))
        if kind in "abcd":
            for t in tiles:
                for r in range(32):
                    a = 32 * t + r
                    yield {"a": (a, a + 1), "b": (a, a + 8), "c": (a, a + 4), "d": (32 * t + 4, 32 * t + 8)}[kind]
        elif kind == "h":
            t = ntiles - 1
            for ra in (4, 5, 6, 7, 0, 1, 2, 3):
                for rb in range(R - 32 * t - 1, ra, -1):
                    yield 32 * t + ra, 32 * t + rb
        else:
            for ta in tiles:
                for tb in range(ta + 1, ntiles):
                    for ra in (5, 6, 7, 4, 13, 14, 21, 30):  # half-wave 1
                        for rb in (2, 3, 10, 11, 17, 24):  # half-wave 0
                            yield 32 * ta + ra, 32 * tb + rb

    for kind in KINDS:
        for a, b, spare in [(a, b, True) for a, b in candidates(kind)] + [(a, b, False) for a, b in candidates(kind)]:
            if free(a, spare) and free(b, spare) and a < b and kind in kind_of(a, b, plan):
                out.append((kind, a, b))
                used.update((a, b))
                for t in {a // 32, b // 32}:
                    tiles_used[t] = tiles_used.get(t, 0) + 1
                break
    return out


def tie_instances(n):
    """the instances whose filters are replaced: those make_case gives no special query (NaN, inf, the rows of zeroes)"""
    return [i for i in range(n) if i % 8 not in (1, 2, 5)]


def grid_case(seed, n, R, D, family, idx, plan, tune):
    placed = place_pairs(plan)
    rot = (idx + idx // 4) % len(placed)  # every kind comes last, and so wins the calls without a filter, in more than one family
    placed = placed[rot:] + placed[:rot]
    if family == "large" and idx % 3 == 0:
        idx += 1  # its NaN and infinite scores come from the raw queries: never every dimension from the pose
    c = mm.make_case(np.random.default_rng(seed), n, R, D, family, idx, pairs=[(a, b) for _, a, b in placed])
    filt = c["filt"].copy()
    every = (filt["exclude"] & (mm.PAIR_BIT * 0x3F)) == mm.PAIR_BIT * 0x3F
    filt["exclude"][every] |= ALL_PAIR_BITS  # "all pairs excluded" means all eight
    base = mm.ZERO_BIT if family == "subnormal" else 0
    for j, i in enumerate(tie_instances(n)):
        bit = mm.pair_bit(j % len(placed))
        if (j // len(placed)) % 2 == 0:
            filt["require"][i], filt["exclude"][i] = 0, (ALL_PAIR_BITS & ~bit) | base
        else:
            filt["require"][i], filt["exclude"][i] = bit, base
    c["filt"] = filt
    for _, a, b in placed:
        c["set"]["rows"]["tags"][[a, b]] &= ~np.uint32(mm.ZERO_BIT)
    c.update(name=f"{tune or 'default'}:{c['name']}", pairs=[(kind, a, b, k) for k, (kind, a, b) in enumerate(placed)], tune=tune, plan=plan)
    return c


_FORCED, _WIDTHS = {}, None


def forced_width(ti, g):
    """tuning ti, G = g: 8 g and 8 g - 4 alternate, so that every G runs padded under two tunings and unpadded under the other two"""
    return 8 * g if (g + ti) % 2 == 0 else 8 * g - 4


def forced_cases(tune):
    """the 32 cases of one forced tuning: the four value families at eight widths, one per G, at n = 65 and R = 300"""
    if tune not in _FORCED:
        ti = TUNES.index(tune)
        plan = plan_of(tune, FORCED_N, FORCED_R)
        out = []
        for g in range(1, 9):
            for fi, family in enumerate(mm.FAMILIES):
                idx = len(out)
                out.append(grid_case(2700 + 100 * ti + idx, FORCED_N, FORCED_R, forced_width(ti, g), family, idx + ti, plan, tune))
        _FORCED[tune] = out
    return _FORCED[tune]


def width_cases():
    """the default tuning at every width: D = 4 .. 64 at n = 33 and R = 97, and D = 8 g also at n = 1025 and R = 65; the
    families alternate so that each meets padded and unpadded widths"""
    global _WIDTHS
    if _WIDTHS is None:
        _WIDTHS = []
        for j in range(1, 17):
            shapes = (WIDTHS_SHARE,) if j % 2 else (WIDTHS_SHARE, WIDTHS_OWNED)
            for k, (n, R) in enumerate(shapes):
                idx = len(_WIDTHS)
                _WIDTHS.append(grid_case(2600 + idx, n, R, 4 * j, mm.FAMILIES[(j // 2 + 2 * k) % 4], idx, plan_of(None, n, R), None))
    return _WIDTHS
