"""No GPU: the premises of tests/test_gpu_cull_model.py.

* no decision of the culling model (tests/cull_model.py) is ambiguous on any scene of tests/cull_scenes.py, for any rank
  and map the GPU tests use: the predicted count is one number;
* every family keeps and culls, and every edge the scenes are there for is reached;
* the model's brute-force ownership agrees with a transcription of the documented super-tile rule;
* the scenes tell a kernel with a 2^-12 margin or a 0.25 px slack from the specified one (the model with those
  constants predicts other counts);
* the bound itself: every clip x, y, w of the exact fma-chain model of the vertex stage
  (tests/vertex_edge_cases.shade) lies inside the interval of its chunk's boxes.

Tightness, measured here: the largest |value - v| - rad over all bounded vertices is 0.0046 m on the cases of
tests/vertex_edge_cases.py and 0.0030 m on the skinned scenes of family c (asserted below 1/2): the "about 40 operations
at 2^-24" of geom_cull.h, 40 * 2^-24 / 2^-16 = 0.16 m at the very worst, is a safe figure.  The matrices with subnormal
rows of the case `subnormal_b` used to step out of the interval by up to 3444 m (subnormal results are rounded to
multiples of 2^-149, which a relative margin does not cover); since then a clip row whose magnitudes lie below 2^-100
has an infinite margin (MTR_CULL_MIN_MAG) and the geometry is kept.
"""
import numpy as np
import pytest

from mt_renderer_amd import sharding
from tests import cull_model as cm
from tests import cull_scenes as cs
from tests import vertex_edge_cases as vx

W, H = cs.W, cs.H
SCENES = cs.scenes()


def _predictions(name):
    s = SCENES[name]
    for di, d in enumerate(s.draws):
        for cfg in cs.configs(s.all_ranks):
            yield di, cfg, cm.predict(d, W, H, cs.shard_of(*cfg))


@pytest.mark.parametrize("name", list(SCENES))
def test_no_decision_is_ambiguous(name):
    n = namb = 0
    for di, cfg, p in _predictions(name):
        n += 1
        namb += p.n_ambiguous
        assert p.n_ambiguous == 0 and p.culled_lo == p.culled_hi, f"{name} draw {di} as {cfg}:\n{p.describe()}"
    print(f"{name}: {n} predictions, {namb} ambiguous decisions")


@pytest.mark.parametrize("family", cs.FAMILIES)
def test_every_family_keeps_and_culls(family):
    kept = culled = 0
    for name, s in SCENES.items():
        if s.family == family:
            for _, _, p in _predictions(name):
                culled += p.culled_lo
                kept += p.chunks - p.culled_lo
    assert kept > 0 and culled > 0, (family, kept, culled)


# ---------------------------------------------------------------------------------------------
# the edges
# ---------------------------------------------------------------------------------------------
def _states(p):
    return [st[0] for st in p.instances]


def _mixed(p):
    return sum(1 for row in p.chunk_kept if row[0] is not None and len({c[0] for c in row}) == 2)


D_CFG = ("bands", cs.D_WORLD, cs.D_RANK)


def test_family_d_reaches_the_instance_edges():
    draws = {k: d for k, d in zip(("straddle", "inside", "outside"), SCENES["d_batch"].draws)}
    rows_launched = -(-2 * cs.D_NINST // cs.D_WORLD)  # ceil(2 * 24 / 4): the rows of k_cull_chunks without a hint
    p = cm.predict(draws["straddle"], W, H, cs.shard_of(*D_CFG))
    st = _states(p)
    assert st.count(cm.STRADDLE) >= 13 > rows_launched and cm.INSIDE in st and cm.CULLED in st
    assert _mixed(p) >= 13  # straddlers with kept and culled chunks
    p = cm.predict(draws["inside"], W, H, cs.shard_of(*D_CFG))
    assert _states(p).count(cm.INSIDE) >= 18 and cs.D_NCHUNKS % 16 == 1  # the mask tail of an inside instance: one bit
    p = cm.predict(draws["outside"], W, H, cs.shard_of(*D_CFG))
    assert _states(p).count(cm.CULLED) >= 18
    few, many = SCENES["d_sequence"].draws
    assert _states(cm.predict(few, W, H, cs.shard_of(*D_CFG))).count(cm.STRADDLE) == 2
    assert _states(cm.predict(many, W, H, cs.shard_of(*D_CFG))).count(cm.STRADDLE) == 20 > 2 + 2 // 8 + 2  # the rows the hint gives


def test_family_b_reaches_the_rows_and_tails():
    counts = [cm.predict(d, W, H, None).chunks for d in SCENES["b_single"].draws]
    assert counts == list(cs.B_COUNTS) and {n % 16 for n in counts} == {0, 1, 15}
    assert any(0 < n % 16 <= 12 for n in counts)  # a workgroup with a wave that has no chunk
    # consecutive chunks disagree for the rank that owns one of the two regions
    for d in SCENES["b_single"].draws[1:]:
        p = cm.predict(d, W, H, cs.shard_of("bands", 2, 0))
        row = [c[0] for c in p.chunk_kept[0]]
        assert row == [k % 2 == 0 for k in range(len(row))], row
    for d in SCENES["b_batch"].draws:
        p = cm.predict(d, W, H, cs.shard_of("bands", 2, 0))
        assert cm.CULLED in _states(p) and _mixed(p) >= 2
    # the mask tail of an inside instance: 1 bit (17 chunks) and 15 bits (63 chunks), on a target that one rank owns
    for d, tail in zip(SCENES["b_batch"].draws, (1, 15)):
        p = cm.predict(d, W, H, None)
        assert cm.INSIDE in _states(p) and (p.chunks // len(p.instances)) % 16 == tail


def test_family_c_reaches_the_skinned_edges():
    main, m254, mixed, m72 = (d["md"] for d in SCENES["c_batch"].draws)
    b = cm.bounds(main)
    njoints = sorted({len(c.joints) for c in b.chunks})
    assert {1, 2, 15} <= set(njoints) and b.weights_ok
    over = [c for c in b.chunks if c.unbounded]
    assert len(over) == 2 and all(c.joints == [] and c.whole is not None for c in over)  # 16 joints: over the table
    assert any(j.joint >= cs.NPAL_C for c in b.chunks for j in c.joints)  # joints past the palette
    b254 = cm.bounds(m254)
    assert not b254.weights_ok and [c.unbounded for c in b254.chunks].count(True) == 3 and b254.chunks[cs.SUM254_CHUNK].unbounded
    p = cm.predict(SCENES["c_batch"].draws[1], W, H, cs.shard_of("bands", 4, 1))
    assert _states(p) == [None, None]  # not instance-boundable: chunk tests for every instance
    bm = cm.bounds(mixed)
    assert bm.inst_rigid is not None and {c.skinnable for c in bm.chunks} == {True, False}
    b72 = cm.bounds(m72)
    assert len(b72.inst_joints) >= 70
    # the boxes past the 64th decide: without them instance 0 would lie inside the upper band
    d = SCENES["c_batch"].draws[3]
    own = cm.ownership(W, H, cs.shard_of("bands", 2, 0))
    _, Ms, pals = cm.draw_matrices(d)
    r_all = cm.screen_rect(cm.union_interval(b72.inst_joints, Ms[0], pals[0]), W, H)
    r_64 = cm.screen_rect(cm.union_interval(b72.inst_joints[:64], Ms[0], pals[0]), W, H)
    assert cm.all_inside(r_64, own) and cm.may_touch(r_all, own) and not cm.all_inside(r_all, own)
    assert _states(cm.predict(d, W, H, cs.shard_of("bands", 2, 0)))[0] == cm.STRADDLE
    # the palette that cancels the model matrix's translation: the margin is a sizeable part of a pixel there
    _, Ms, pals = cm.draw_matrices(SCENES["c_batch"].draws[0])
    ch = next(c for c in b.chunks if len(c.joints) == 1)
    m_px = [float((cm.interval_parts(ch.joints[0], *cm.composite(Ms[i], cm.pal4(pals[i][ch.joints[0].joint])))[2][:2] * (W / 2, H / 2)).max()) / cs.DIST
            for i in (0, 2, 3)]  # the margin in x or y, in pixels at the scene's distance
    assert m_px[0] < 0.02 and m_px[1] > 0.5 and m_px[2] > 1.0, m_px


def test_family_e_is_kept():
    draws = SCENES["e_unboundable"].draws
    for cfg in cs.configs(False):
        shard = cs.shard_of(*cfg)
        p = cm.predict(draws[0], W, H, shard)  # 2: behind the camera, 3: through w = 0
        assert _states(p)[2] == _states(p)[3] == cm.STRADDLE and all(c == (True, True) for i in (2, 3) for c in p.chunk_kept[i])
        p = cm.predict(draws[1], W, H, shard)  # NaN and inf in a model matrix
        assert all(c == (True, True) for i in (0, 1) for c in p.chunk_kept[i])
        p = cm.predict(draws[2], W, H, shard)  # NaN / inf in joint 5 / 12 of instances 1 / 2
        assert _states(p)[1] == _states(p)[2] == cm.STRADDLE
        for di in (3, 5):  # chunk 1 holds the position of 3e38 / has no vertex in range
            assert cm.predict(draws[di], W, H, shard).chunk_kept[0][1] == (True, True)
        assert cm.predict(draws[7], W, H, shard).culled_hi == 0  # a clip row among the subnormals
    assert cm.bounds(draws[5]["md"]).chunks[1].whole is None
    assert not np.isfinite(cm.bounds(draws[3]["md"]).chunks[1].whole.e).any()


def test_family_f_uses_the_boxes_of_the_third_primitive():
    hidden, _, whole = SCENES["f_hidden_part"].draws
    b = cm.bounds(hidden["md"])
    vis = cm.visible_chunks(hidden["md"], hidden["parts_disp"])
    assert vis == [0, 1, 2, 8, 9, 10, 11] and [b.chunks[i].prim for i in vis] == [0, 0, 0, 2, 2, 2, 2]
    # with the boxes of the hidden primitive in their place the count would differ
    differs = 0
    for cfg in cs.configs(False):
        p, pw = cm.predict(hidden, W, H, cs.shard_of(*cfg)), cm.predict(whole, W, H, cs.shard_of(*cfg))
        shifted = [pw.chunk_kept[0][i][0] for i in (0, 1, 2, 3, 4, 5, 6)]  # chunks 3.. of the whole model are the second primitive's
        differs += shifted != [c[0] for c in p.chunk_kept[0]]
    assert differs > 5


def test_family_a_keeps_at_half_a_pixel_and_culls_at_one_and_a_half():
    """every quad is kept exactly by the ranks that own a bin it reaches through the 1 px slack; then the pairs"""
    s = SCENES["a_batch"]
    quads = s.tags["quads"]
    seen = set()
    for cfg in cs.configs(True):
        own = cm.ownership(W, H, cs.shard_of(*cfg))
        p = cm.predict(s.draws[0], W, H, cs.shard_of(*cfg))
        for q, st in zip(quads, _states(p)):
            want = any(own.grid[by, bx] == own.rank for bx, by in q["bins"])
            assert (st != cm.CULLED) == want, (cfg, q, st)
        kept = {q["border"]: st != cm.CULLED for q, st in zip(quads, _states(p))}
        for border in {q["border"][:-1] for q in quads if q["border"][-1] == 0.5}:
            if kept[border + (0.5,)] and not kept[border + (1.5,)]:
                seen.add((cfg[0], cfg[1]) + border)
    for world, bands in ((w, sharding.equal_bands(H, w)) for w in cs.WORLDS):
        for r in range(world):  # the top and the bottom of every band
            if r > 0:
                assert ("bands", world, "h", bands[r], "above") in seen
            if r + 1 < world:
                assert ("bands", world, "h", bands[r + 1], "below") in seen
    for world in cs.WORLDS:
        if cs.UNEVEN[world][-2] > 0:
            assert ("bands-uneven", world, "h", cs.UNEVEN[world][-2], "above") in seen  # the uneven bands' last border
        for m, lines in (("supertiles1", (1, 7, 19)), ("supertiles4", (4, 8, 12, 16))):
            for k in lines:  # the left and the right of a super-tile
                assert (m, world, "v", k, "left") in seen and (m, world, "v", k, "right") in seen, (m, world, k)
        if 5 % world:  # five super-tiles per row: with world 5 a column of them has one owner
            assert ("supertiles4", world, "h", 12, "above") in seen  # the last super-tile row: 8 px of bins
    for edge in ("target-left", "target-right", "target-top", "target-bottom"):
        assert (cs.WORLD1, 1, edge) in seen
    # an empty band keeps nothing; on the target's corner and in the last bin row the owner keeps
    for world in cs.WORLDS:
        empty = next(r for r in range(world) if cs.UNEVEN[world][r] == cs.UNEVEN[world][r + 1])
        for d in s.draws:
            p = cm.predict(d, W, H, cs.shard_of("bands-uneven", world, empty))
            assert p.culled_lo == p.chunks
    p = cm.predict(s.draws[0], W, H, None)
    assert _states(p)[-2] == cm.STRADDLE and _states(p)[-1] == cm.INSIDE  # ends on fx == W, fy == H: hangs over with the slack
    # the two-quad instances: 1.5 px either side of a line one rank keeps one chunk each, 0.5 px both keep both
    p = cm.predict(s.draws[1], W, H, cs.shard_of("bands", 4, 1))
    rows = {(t["line"], t["d"]): row for t, row in zip(s.tags["two"], p.chunk_kept)}
    assert [c[0] for c in rows[(3, 1.5)]] == [False, True] and [c[0] for c in rows[(6, 1.5)]] == [True, False]
    assert [c[0] for c in rows[(3, 0.5)]] == [True, True] and [c[0] for c in rows[(6, 0.5)]] == [True, True]
    # the same quads as single models
    singles = SCENES["a_single"]
    for cfg in cs.configs(True):
        own = cm.ownership(W, H, cs.shard_of(*cfg))
        for d, q in zip(singles.draws, singles.tags["quads"]):
            want = any(own.grid[by, bx] == own.rank for bx, by in q["bins"])
            assert cm.predict(d, W, H, cs.shard_of(*cfg)).culled_lo == (0 if want else 1), (cfg, q)


# ---------------------------------------------------------------------------------------------
# ownership
# ---------------------------------------------------------------------------------------------
def _documented_rule(bx0, by0, bx1, by1, rank, world, shift, nsx):
    """DESIGN.md section 4 / mtr_internal.h: super-tile ids run row-major, `world` consecutive ones hit every rank, a
    rectangle more than 8 rows tall is kept, else row by row the distance from the row's first id to the rank's residue"""
    x0, x1, y0, y1 = bx0 >> shift, bx1 >> shift, by0 >> shift, by1 >> shift
    w = x1 - x0
    if w + 1 >= world or y1 - y0 >= 8:
        return True
    return any((rank - (y * nsx + x0)) % world <= w for y in range(y0, y1 + 1))


@pytest.mark.parametrize("shift", [0, 1, 2])
@pytest.mark.parametrize("world", [2, 3, 5, 8])
def test_brute_force_ownership_agrees_with_the_documented_super_tile_rule(world, shift):
    w, h = 1000, 1100  # 63 x 69 bins: ragged super-tiles at both edges, room for rectangles more than 8 super-tiles tall
    nbx, nby, _ = sharding.grid(w, h)
    nsx = (nbx + (1 << shift) - 1) >> shift
    rng = np.random.default_rng(world * 10 + shift)
    n_true = 0
    for _ in range(10000):
        rank = int(rng.integers(0, world))
        own = cm.ownership(w, h, (rank, world, sharding.SUPERTILES, shift, None))
        bx0, by0 = int(rng.integers(0, nbx)), int(rng.integers(0, nby))
        bx1 = min(nbx - 1, bx0 + int(rng.integers(0, 4 << shift)))
        by1 = min(nby - 1, by0 + int(rng.integers(0, 3 << shift) if rng.random() < 0.8 else rng.integers(0, nby)))
        rect = (16.0 * bx0 + 3, 16.0 * bx1 + 9, 16.0 * by0 + 5, 16.0 * by1 + 11)
        got = cm.may_touch(rect, own)
        n_true += got
        assert got == _documented_rule(bx0, by0, bx1, by1, rank, world, shift, nsx), (rank, bx0, by0, bx1, by1)
    assert 1000 < n_true < 9900  # both answers occur


# ---------------------------------------------------------------------------------------------
# the scenes tell other constants apart
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,m_scale,slack_px,families", [("a margin of 2^-12", 16.0, cm.SLACK_PX, "c"), ("a slack of 0.25 px", 1.0, 0.25, "acd")])
def test_the_scenes_tell_a_kernel_with_other_constants_from_the_specified_one(what, m_scale, slack_px, families):
    """the margin only shows where it is a sizeable part of a pixel: the perspective scenes with skinning (family c);
    the slack shows in every family that has geometry near a bin line"""
    differing = []
    for name, s in SCENES.items():
        for di, d in enumerate(s.draws):
            other = cm.draw_rects(d, W, H, (m_scale, m_scale), (0.0, 0.0), slack_px)
            for cfg in cs.configs(s.all_ranks):
                shard = cs.shard_of(*cfg)
                if cm.predict_from(other, cm.ownership(W, H, shard)).culled_lo != cm.predict(d, W, H, shard).culled_lo:
                    differing.append((name, di, cfg))
                    break
    print(f"{what}: other counts in {len(differing)} draws, e.g. {differing[:3]}")
    assert len(differing) >= 3 and {SCENES[n].family for n, _, _ in differing} >= set(families), (what, differing)


# ---------------------------------------------------------------------------------------------
# the bound itself, against the exact model of the vertex stage
# ---------------------------------------------------------------------------------------------
def _check(what, clip, boxes, M16, pal):
    s = cm.margin_fraction(clip, boxes, cm.mat4(M16), pal)
    if s is None:
        return None  # an interval that is not finite: kept
    assert np.isfinite(np.asarray(clip)[:, [0, 1, 3]]).all(), f"{what}: bounded, but a clip coordinate is not finite"
    assert (s <= 1.0).all(), f"{what}: vertex {int(s.argmax())} lies {float(s.max()):.3f} margins outside the interval"
    return float(s.max())


def test_the_exact_vertex_stage_stays_inside_the_interval_on_the_edge_cases():
    worst, bounded, kept = 0.0, 0, 0
    for c in vx.cases():
        for npal in vx.NPALS:
            pal = vx.palette_of(c, npal)
            for prim in range(len(c.prims)):
                clip = vx.model_clip(c, prim, npal).view(np.float32)
                for vids, boxes in cm.case_blocks(c, prim, npal is not None):
                    s = _check(f"{c.name} npal {npal} prim {prim} vertices {vids[0]}..", clip[vids], boxes, c.M, pal)
                    if s is None:
                        kept += len(vids)
                    else:
                        bounded += len(vids)
                        worst = max(worst, s)
    print(f"edge cases: {bounded} vertices bounded, {kept} in blocks that are kept; largest |value - v| - rad = {worst:.4f} m")
    assert bounded > 5000 and worst < 0.5


def _exact_clip(md, prim, pal, M16):
    pos = cm.decode_positions(md, prim).view(np.uint32)
    skin = cm._skin_bytes(md, prim)
    palw = None if (pal is None or skin is None) else np.ascontiguousarray(pal, dtype=np.float32).view(np.uint32).reshape(-1, 16).tolist()
    Mw = np.ascontiguousarray(M16, dtype=np.float32).view(np.uint32).tolist()
    zero = [0, 0, 0, 0]
    out = [vx.shade(pos[v].tolist(), zero if skin is None else skin[0][v].tolist(), zero if skin is None else skin[1][v].tolist(), palw, Mw)
           for v in range(len(pos))]
    return np.array(out, dtype=np.uint32).view(np.float32).reshape(-1, 4)


def test_the_exact_vertex_stage_stays_inside_the_interval_on_the_skinned_scenes():
    worst, bounded = 0.0, 0
    for di, d in enumerate(SCENES["c_single"].draws):
        b = cm.bounds(d["md"])
        base = 0
        for prim in range(d["md"].nprims):
            clip = _exact_clip(d["md"], prim, d["palette"], d["M"])
            ids = cm.chunk_vertex_ids(d["md"], prim)
            for k, vids in enumerate(ids):
                ch = b.chunks[base + k]
                if ch.whole is None or (ch.skinnable and ch.unbounded):
                    continue
                s = _check(f"c_single draw {di} prim {prim} chunk {k}", clip[vids], ch.joints if ch.skinnable else [ch.whole], d["M"],
                           d["palette"] if ch.skinnable else None)
                assert s is not None
                bounded += len(vids)
                worst = max(worst, s)
            base += len(ids)
    print(f"skinned scenes: {bounded} vertices bounded; largest |value - v| - rad = {worst:.4f} m")
    assert bounded > 1500 and worst < 0.5
