"""CPU: the premises of tests/test_gpu_tile_paths.py -- that each scene of tests/tile_path_scenes.py puts its bin on the
path its docstring names -- computed from the scenes' integers, and the integer model itself against the oracle: the
pixels it says are covered are exactly those whose depth the oracle wrote."""
import numpy as np
import pytest

from tests import tile_path_scenes as tp
from tests.helpers import render_oracle

SCENES = {
    "list_overflow": tp.list_overflow,
    "pair_cap": tp.pair_cap,
    "large_among_small": tp.large_among_small,
    "lists_across_passes": tp.lists_across_passes,
    "partial_last_bin": lambda: tp.list_overflow(24, 24, 20, 19),
}


def strictly_nearer_in_turn(tris):
    return all(b.z < a.z for a, b in zip(tris, tris[1:]))


def premise_list_overflow(sc, bx, by):
    """one pass without a 64-bit triangle and within the pair cap, so k_tile builds the lists; one pixel is listed more than
    FRAG_K times, so it falls back to the sub-tile loop.  The fragments of that pixel come nearer and nearer, so none is
    dominated by an earlier one and k_tile_vis lists them all: more than STAIR_K, it hands the bin over"""
    e = sc.entries(bx, by)
    assert len(e) < tp.TRI_PASS and not any(t.large for t in e)
    assert 0 < sum(sc.box_pixels(t, bx, by) for t in e) <= tp.PAIR_CAP
    assert all(3 <= len(t.pixels(sc.w, sc.h)) <= 5 for t in e if not t.opaque)  # about 3 px each
    worst = max(sc.hits(e, bx, by).values(), key=len)
    assert len(worst) == 12 > max(tp.FRAG_K, tp.STAIR_K) and strictly_nearer_in_turn(worst)
    assert any(t.opaque for t in e)


def premise_pair_cap(sc):
    a, b = sc.entries(0, 0), sc.entries(2, 0)
    assert len(a) == 8 and len(b) == 10 and not any(t.large for t in a + b)
    assert sum(sc.box_pixels(t, 0, 0) for t in a) == tp.PAIR_CAP                # the list path, at its cap
    assert {len(v) for v in sc.hits(a, 0, 0).values()} == {4} and len(sc.hits(a, 0, 0)) == 256  # every pixel 4 times <= FRAG_K
    assert sum(sc.box_pixels(t, 2, 0) for t in b) == 2560 > tp.PAIR_CAP         # the sub-tile loop
    assert all(len(v) == 5 and v[4].z > max(t.z for t in v[:4]) for v in sc.hits(b, 2, 0).values())  # the fifth is hidden
    assert sc.entries(1, 0) == [] and any(t.opaque for t in a)


def premise_large_among_small(sc):
    e = sc.entries(2, 0)
    assert len(e) == 31 < tp.TRI_PASS                                            # one pass, so the whole bin takes the loop
    assert [t.large for t in e] == [False] * 15 + [True] + [False] * 15          # submitted in the middle
    big = e[15]
    assert max(big.X) - min(big.X) > 64 * 256 and len([p for p in big.pixels(sc.w, sc.h) if p[0] // 16 == 2]) > 100
    assert all(2 <= len(t.pixels(sc.w, sc.h)) <= 6 and all(p[0] // 16 == 2 and p[1] // 16 == 0 for p in t.pixels(sc.w, sc.h)) for t in e if not t.large)
    assert sum(t.opaque for t in e) == 1


def premise_lists_across_passes(sc):
    ps = sc.passes(1, 0)
    assert [len(p) for p in ps] == [64, 64, 2] and ps[0] + ps[1] + ps[2] == sc.tris  # three passes, submission order
    for p in ps[:2]:
        assert not any(t.large for t in p) and sum(sc.box_pixels(t, 1, 0) for t in p) <= tp.PAIR_CAP
        h = sc.hits(p, 1, 0)
        assert len(h) == 8 and {len(v) for v in h.values()} == {tp.FRAG_K}       # exactly the cap: lists, no overflow
    total = sc.hits(sc.tris, 1, 0)
    assert len(total) == 8 and all(16 <= len(v) <= 17 for v in total.values())
    zs = [t.z for t in sc.tris]
    assert len(set(zs)) < len(zs) and zs != sorted(zs) and zs != sorted(zs, reverse=True)  # ties, and no order
    assert any(a.z == b.z for v in total.values() for a, b in zip(v, v[1:]) ) or any(len({t.z for t in v}) < len(v) for v in total.values())


def check_premise(name, sc):
    if name == "list_overflow":
        premise_list_overflow(sc, 1, 0)
    elif name == "partial_last_bin":
        assert sc.w % tp.BIN != 0 and sc.h % tp.BIN != 0  # the bin is cut by the right and the bottom edge
        assert (sc.w - 1) // tp.BIN == 1 and (sc.h - 1) // tp.BIN == 1
        premise_list_overflow(sc, 1, 1)
    elif name == "pair_cap":
        premise_pair_cap(sc)
    elif name == "large_among_small":
        premise_large_among_small(sc)
    else:
        premise_lists_across_passes(sc)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_premise_and_model(name):
    sc = SCENES[name]()
    assert sc.w <= 128 and sc.h <= 32
    if name != "partial_last_bin":
        assert sc.w & (sc.w - 1) == 0 and sc.h & (sc.h - 1) == 0
    check_premise(name, sc)
    color, depth, stats = render_oracle(sc.w, sc.h, sc.draws())
    assert stats["tris_setup"] == len(sc.tris)
    assert ((depth < 1.0) == sc.covered()).all()
    assert len(np.unique(color.reshape(-1, 4), axis=0)) > 3  # clear, the opaque colour and several blends
