"""CPU: the premises of tests/test_gpu_vertex_edges.py.

1. The oracle's vertex stage equals the exact model of tests/vertex_edge_cases.py (integer arithmetic, one rounding per
   multiply-add) on every case model and every palette size: bits equal, or both NaN.  The GPU tests compare with the oracle,
   so this pins their reference independently of libm's fmaf and of the CPU's FMA unit.
2. The inputs can tell the mistakes apart.  Counted from the exact model and its three wrong variants alone, at the full
   palette of 256 matrices (vertices that differ from the exact result / vertices the variant was run on):

       unfused   benign family (benign, s16n)     303 / 384      cancel family (cancel, blocks)   502 / 716
       unfused   unskinned_cancel, no palette     128 / 128
       daz       subnormal family                 249 / 256      ... with no palette (clip chain)  160 / 256
       ftz       subnormal family                 123 / 256      ... with no palette (clip chain)   96 / 256

   Of the 8 752 clip words of all case models, 64 are -0, 36 are +-inf, 29 are NaN and 302 are subnormal; 32 words of
   `cancel` are an exact zero left by a cancelling chain, 172 of the 192 `large` vertices stay finite.
   The assertions below hold the generator to the bounds of the issue, not to these figures.
3. The frame models: the oracle renders each with covered pixels in every draw, and no clip coordinate is non-finite.
"""
import collections

import numpy as np
import pytest

from oracle import oracle as orc
from tests import vertex_edge_cases as vx
from tests.helpers import render_oracle

CASES = {c.name: c for c in vx.cases()}


def _words(case, npal, variant="exact"):
    return np.concatenate([vx.model_clip(case, p, npal, variant) for p in range(len(case.prims))])


def _oracle_words(case, npal):
    om = orc.OracleModel(case.md)
    return np.concatenate([om.vertex_stage(p, case.M, vx.palette_of(case, npal))[0].view(np.uint32) for p in range(len(case.prims))])


def _differing(names, variant, npal=256):
    """(vertices on which the variant differs from the exact model, vertices) over the named cases; as a mutant of the
    model it fails against the oracle on exactly those vertices"""
    bad = total = 0
    for n in names:
        ok = vx.same_words(_words(CASES[n], npal, variant), _words(CASES[n], npal)).all(axis=1)
        assert (vx.same_words(_words(CASES[n], npal, variant), _oracle_words(CASES[n], npal)).all(axis=1) == ok).all()
        bad, total = bad + int((~ok).sum()), total + len(ok)
    return bad, total


def _of_family(family):
    names = [c.name for c in vx.cases() if family in c.family and c.name != "unskinned_cancel"]
    assert all(set(CASES[n].family) == {family} for n in names)
    return names


@pytest.mark.parametrize("name", list(CASES))
def test_oracle_vertex_stage_equals_the_exact_model(name):
    c = CASES[name]
    om = orc.OracleModel(c.md)
    for npal in vx.NPALS:
        for prim, (v0, n) in enumerate(c.prims):
            oc, ou = om.vertex_stage(prim, c.M, vx.palette_of(c, npal))
            exact = vx.model_clip(c, prim, npal)
            ok = vx.same_words(oc, exact)
            assert ok.all(), (npal, vx.describe_first_difference(c, prim, ok, oc, exact))
            assert (ou.view(np.uint32) == c.uv[v0:v0 + n].view(np.uint32)).all(), (name, npal, prim)


def test_the_exact_fma_on_known_values():
    f = lambda x: int(np.float32(x).view(np.uint32))
    assert vx.fma32(f(3.0), f(0.5), f(0.25)) == f(1.75)
    assert vx.fma32(1, f(0.5), 0) == 0 and vx.fma32(1 | vx.NEG_ZERO, f(0.5), 0) == vx.NEG_ZERO  # half a quantum: ties to even
    assert vx.fma32(3, f(0.5), 0) == 2 and vx.fma32(1, f(0.75), 0) == 1                           # subnormal results
    assert vx.fma32(f(2.0 ** 100), f(2.0 ** 100), f(-1.0)) == vx.INF
    assert vx.fma32(f(2.0 ** 100), f(2.0 ** 100), vx.INF | vx.NEG_ZERO) == vx.INF | vx.NEG_ZERO
    assert vx.is_nan(vx.fma32(vx.INF, 0, f(1.0))) and vx.is_nan(vx.fma32(vx.INF, f(1.0), vx.INF | vx.NEG_ZERO))
    assert vx.fma32(0, f(-1.0), 0) == 0 and vx.fma32(0, f(-1.0), vx.NEG_ZERO) == vx.NEG_ZERO and vx.fma32(f(1.0), f(-1.0), f(1.0)) == 0
    # one rounding: (1 + 2^-12)^2 - (1 + 2^-11) = 2^-24, which the rounded product has lost
    a = f(1.0 + 2.0 ** -12)
    assert vx.fma32(a, a, f(-(1.0 + 2.0 ** -11))) == f(2.0 ** -24) and vx.VARIANTS["unfused"](a, a, f(-(1.0 + 2.0 ** -11))) == 0
    assert vx.UNORM8[255] == vx.ONE and vx.UNORM8[0] == 0 and vx.UNORM8[1] == f(np.float32(1) / np.float32(255))
    assert vx.snorm16_bits(-32768) == f(-1.0) and vx.snorm16_bits(-32767) == f(-1.0) and vx.snorm16_bits(1) == f(np.float32(1) / np.float32(32767))


def test_unfused_arithmetic_would_show():
    for family in ("benign", "cancel"):
        bad, total = _differing(_of_family(family), "unfused")
        print(f"unfused, {family}: {bad} / {total}")
        assert 2 * bad >= total
    bad, total = _differing(["unskinned_cancel"], "unfused", None)
    print(f"unfused, unskinned_cancel without palette: {bad} / {total}")
    assert 2 * bad >= total


@pytest.mark.parametrize("variant", ["daz", "ftz"])
def test_a_flush_of_subnormals_would_show(variant):
    names = _of_family("subnormal")
    bad, total = _differing(names, variant)
    print(f"{variant}, subnormal: {bad} / {total}")
    assert bad >= 64
    bad, total = _differing(names, variant, None)  # the four-step clip chain alone
    print(f"{variant}, subnormal without palette: {bad} / {total}")
    assert bad >= 64


def test_special_results_occur():
    w = np.concatenate([_words(c, 256).reshape(-1) for c in vx.cases()])
    mag = w & 0x7FFFFFFF
    counts = dict(neg_zero=int((w == vx.NEG_ZERO).sum()), inf=int((mag == vx.INF).sum()), nan=int((mag > vx.INF).sum()),
                  subnormal=int(((mag > 0) & (mag < 0x00800000)).sum()))
    print(counts)
    assert counts["neg_zero"] >= 16 and counts["inf"] >= 16 and counts["nan"] >= 4 and counts["subnormal"] >= 64
    cw = _words(CASES["cancel"], 256)
    assert int(((cw & 0x7FFFFFFF) == 0).sum()) >= 16           # exact zeros out of a cancelling chain
    lw = _words(CASES["large"], 256)
    assert int(((lw & 0x7FFFFFFF) < vx.INF).all(axis=1).sum()) >= 16  # and large vertices that stay finite


def test_every_block_pattern_and_tail_occurs():
    seen = collections.Counter()
    for c in vx.cases():
        for p in range(len(c.prims)):
            seen.update(c.patterns(p))
    need = ["coherent", "zero_weight_slot", "mixed", "tail1", "tail2", "tail3"] + [f"one_differs_lane{l}" for l in range(4)]
    assert all(seen[t] > 0 for t in need), seen
    b = CASES["blocks"]
    assert tuple(n for _, n in b.prims) == vx.TAIL_VERTEX_NUMS == (1, 2, 3, 5, 63, 64, 65, 257)
    big = collections.Counter(b.patterns(len(b.prims) - 1))
    assert all(big[t] >= 4 for t in need if not t.startswith("tail")) and big["tail1"] == 1, big  # all of them in one primitive too
    # every numeric family meets both chains: coherent blocks (MFMA) and blocks with a lane of its own (VALU)
    for c in vx.cases():
        pats = set(c.patterns(len(c.prims) - 1))
        assert "coherent" in pats and any(t.startswith("one_differs") or t == "mixed" for t in pats), c.name
    # the words of the `weights` and `joints` families
    wts = {tuple(r) for r in CASES["weights"].weights.tolist()}
    assert set(vx.WEIGHT_WORDS) <= wts and any(sum(r) != 255 for r in wts - set(vx.WEIGHT_WORDS))
    j = CASES["joints"].joints
    assert (j == 255).any() and (j.max(axis=1) == j.min(axis=1)).any()
    assert all((j >= n).any() and (j < n).any() for n in (1, 5, 64))  # and 255 above: the last entry of npal = 256
    perm = [b0 for b0 in range(0, len(j), 4) if len({bytes(r) for r in j[b0:b0 + 4]}) > 1 and len({tuple(sorted(r)) for r in j[b0:b0 + 4].tolist()}) == 1]
    assert len(perm) >= 4  # one set of joints in permuted slot order
    assert sum(case.pos_bits.shape[0] for case in vx.cases()) <= 2600  # the exact model stays affordable


@pytest.mark.parametrize("name", list(vx.frame_scenes()))
def test_frame_models_are_finite_and_visible(name):
    draws = vx.frame_scenes()[name]
    for d in draws:
        om = orc.OracleModel(d["md"])
        if "model_mats" in d:
            singles = [dict(md=d["md"], M=orc.mat4_mul(d["vp"], m), palette=p) for m, p in zip(d["model_mats"], d["palettes"])]
        else:
            singles = [d]
        for s in singles:
            clip, _ = om.vertex_stage(0, s["M"], s["palette"])
            assert np.isfinite(clip).all(), name
            _, depth, stats = render_oracle(vx.FRAME_W, vx.FRAME_H, [s])
            assert int((depth < 1.0).sum()) >= 16 and stats["tris_setup"] > 0, name
    assert vx.FRAME_W <= 192 and vx.FRAME_H <= 112
    _, depth, _ = render_oracle(vx.FRAME_W, vx.FRAME_H, draws)
    bits = depth.view(np.uint32)
    if name == "tiny_z":  # the depth buffer holds subnormals
        assert int(((bits > 0) & (bits < 0x00800000)).sum()) >= 1000
    if name == "near_plane_random":  # clipped triangles next to unclipped ones
        clip, _ = orc.OracleModel(draws[0]["md"]).vertex_stage(0, draws[0]["M"], draws[0]["palette"])
        assert (clip[:, 2] < 0).sum() > 50 and (clip[:, 2] > 0).sum() > 50


def test_frame_models_hit_the_restart_phases():
    md = vx.frame_model("rail", vx.scene.TOPO_STRIP)
    idx = md.index_buf
    cuts = np.nonzero(idx == 0xFFFF)[0]
    runs = np.diff(np.concatenate([[-1], cuts, [len(idx)]])) - 1
    assert set(runs.tolist()) == set(vx.STRIP_LENGTHS)
    # every phase of the 62-position chunk (restart at every lane of the wave but the two halo lanes of the first chunk),
    # hence every phase of the block of four and both parities of the rails
    assert {int(c) % 62 for c in cuts} == set(range(62)) and {int(c) % 8 for c in cuts} == set(range(8))
    assert (runs % 2 == 1).any() and (runs % 2 == 0).any()  # odd runs: the rails change places
    f = vx.scene.unpack_primitive(md.prims[0])
    assert f["index_base"] == vx.INDEX_BASE > 0
    ordinary = idx[idx != 0xFFFF].astype(np.int64) + f["index_base"]
    assert 0 < (ordinary >= f["vertex_num"]).sum() <= 4
    lst = vx.frame_model("rail", vx.scene.TOPO_LIST)
    assert (lst.vertex_buf == md.vertex_buf).all() and len(lst.index_buf) == 3 * int(np.clip(runs - 2, 0, None).sum())
