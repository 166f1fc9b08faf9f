"""-m gpu: the records k_tile_vis.hip stages for its flat walks (stage_flat), whose edge constants the set-up now takes at
the bbox origin (csrc/tri_setup.h: tri_setup_box) instead of rebasing them for every staged triangle.  One 64 x 48 frame of
12 bins against the oracle, bit for bit in colour and depth, at 2, 4 and 8 waves per bin:
  * bin (1, 1): one pass (fewer than 64 entries) of triangles whose boxes are 1, 2, 3 and 16 rows high, with horizontal and
    vertical edges, boxes that start inside the bin and boxes the bin's left / top edge cuts (origin column / row 0);
  * a triangle over 64 px across (the 64-bit class, whose constants stay at the bin's first pixel) through bin rows 1 and 2:
    it shares the span pass of bin (1, 1) and of every bin it crosses;
  * boxes cut by the right / bottom edge of a bin and of the viewport (bins (3, y) and (x, 2));
  * bin (2, 1): more than 64 x 8 entries of 3 x 3 px boxes, so that at every wave count a wave meets a second pass and
    stages over its own earlier records.
The premises (box heights, entry counts, the span walk's majority rule) are computed here from the scene's integers before
anything is rendered."""
import os

import numpy as np
import pytest

from mt_renderer_amd import scene
from tests.helpers import assert_same, render_gpu, render_oracle
from tests.pixel_scenes import pixel_model, pixel_to_ndc_matrix

W, H, BIN = 64, 48, 16


def front(a, b, c):
    """the winding the reference keeps (tests/test_gpu_overflow.py's quads): (x, y), (x, y + s), (x + s, y)"""
    cross = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    assert cross != 0
    return (a, b, c) if cross < 0 else (a, c, b)


def box_of(tri):
    """pixel-centre bbox (x0, y0, x1, y1) of a triangle given in pixels (multiples of 1/256), clipped to the viewport"""
    xs, ys = [int(round(v[0] * 256)) for v in tri], [int(round(v[1] * 256)) for v in tri]
    return (max((min(xs) + 127) >> 8, 0), max((min(ys) + 127) >> 8, 0), min((max(xs) - 128) >> 8, W - 1), min((max(ys) - 128) >> 8, H - 1))


def in_bin(box, bx, by):
    """the part of a bbox inside bin (bx, by): (columns, rows), 0 if none"""
    x0, y0, x1, y1 = max(box[0], bx * BIN), max(box[1], by * BIN), min(box[2], bx * BIN + BIN - 1), min(box[3], by * BIN + BIN - 1)
    return (x1 - x0 + 1, y1 - y0 + 1) if x1 >= x0 and y1 >= y0 else (0, 0)


def build_scene():
    tris = []  # ((x, y, z) x 3)

    def add(a, b, c, z):
        zs = z if isinstance(z, tuple) else (z, z, z)
        t = front(a, b, c)
        tris.append(tuple((p[0], p[1], zs[i]) for i, p in enumerate(t)))

    # ---- bin (1, 1) = pixels [16, 32) x [16, 32): the pass of mixed box heights
    mixed = len(tris)
    add((17.25, 17.25), (22.75, 17.25), (17.25, 17.75), 0.30)            # 1 row high, a horizontal edge on top, starts inside the bin
    add((24.25, 17.25), (24.25, 19.25), (30.75, 19.25), 0.31)            # 2 rows, a vertical and a horizontal edge
    add((17.5, 20.25), (23.5, 21.0), (19.0, 23.25), (0.2, 0.5, 0.8))     # 3 rows, no axis-aligned edge, a z plane
    add((25.0, 16.0), (31.0, 16.0), (28.0, 32.0), (0.6, 0.6, 0.1))       # 16 rows: top to bottom of the bin
    add((12.5, 24.5), (20.5, 24.5), (12.5, 30.5), 0.33)                  # cut by the bin's left edge: origin column 0
    add((21.5, 12.5), (27.5, 12.5), (21.5, 18.5), 0.34)                  # cut by the bin's top edge: origin row 0
    add((20.5, 26.5), (26.5, 26.5), (26.5, 31.5), 0.35)                  # vertical edge on the right
    add((18.5, 25.5), (24.5, 29.5), (18.5, 29.5), 0.25)                  # overlaps its neighbours: nearer, wins where covered
    n_mixed = len(tris) - mixed
    # ---- the 64-bit class: over 64 px across, through bin rows 1 and 2, behind some and in front of others
    large = len(tris)
    add((-6.0, 18.0), (66.0, 22.0), (30.0, 44.0), (0.32, 0.32, 0.45))
    # ---- boxes cut by the right / bottom edge of the last bins = of the viewport
    add((58.5, 4.5), (70.5, 4.5), (58.5, 12.5), 0.4)    # leaves the viewport to the right
    add((52.5, 40.5), (60.5, 40.5), (52.5, 52.5), 0.4)  # ... and below
    add((44.5, 2.5), (51.5, 2.5), (44.5, 9.5), 0.4)     # cut by the edge between bins (2, 0) and (3, 0)
    add((2.5, 12.5), (9.5, 12.5), (2.5, 19.5), 0.4)     # ... between bins (0, 0) and (0, 1)
    # ---- bin (2, 1) = pixels [32, 48) x [16, 32): 64 x 8 + 28 boxes of 3 x 3 px on a 13 x 13 lattice of origins, at
    #      descending z so that later ones win where they overlap
    dense = len(tris)
    for k in range(540):
        x, y = 32.25 + (k % 13), 16.25 + (k // 13) % 13
        add((x, y), (x, y + 3.0), (x + 3.0, y), 0.9 - k * 1e-3)
    return tris, dict(mixed=(mixed, n_mixed), large=large, dense=(dense, 540))


def premises(tris, where):
    m0, nm = where["mixed"]
    heights = sorted(in_bin(box_of(t), 1, 1)[1] for t in tris[m0:m0 + nm])
    assert {1, 2, 3, 16} <= set(heights), heights
    # the large triangle: over 64 px across, and bin (1, 1) holds part of its bbox
    lg = tris[where["large"]]
    assert max(v[0] for v in lg) - min(v[0] for v in lg) > 64 and in_bin(box_of(lg), 1, 1) != (0, 0)
    # bin (1, 1): one pass, and a span pass -- at least half of its i32-class boxes hold more than four pixels
    ent = [in_bin(box_of(t), 1, 1) for t in tris]
    here = [e for i, e in enumerate(ent) if e != (0, 0) and i != where["large"]]
    assert len(here) + 1 < 64 and sum(1 for c, r in here if c * r > 4) * 2 >= len(here)
    assert any(in_bin(box_of(t), 1, 1)[0] and box_of(t)[0] < BIN for t in tris[m0:m0 + nm])   # origin column 0 by the cut
    assert any(in_bin(box_of(t), 1, 1)[0] and box_of(t)[1] < BIN for t in tris[m0:m0 + nm])   # origin row 0
    # bin (2, 1): more entries than 8 waves take in one pass each, every box over four pixels
    d0, nd = where["dense"]
    dense = [in_bin(box_of(t), 2, 1) for t in tris[d0:d0 + nd]]
    assert sum(1 for e in dense if e != (0, 0)) > 64 * 8 and all(c * r > 4 for c, r in dense if (c, r) != (0, 0))
    # the viewport cuts: a bbox that would pass the right / bottom edge
    assert any(max(v[0] for v in t) > W for t in tris) and any(max(v[1] for v in t) > H for t in tris)


@pytest.fixture(scope="module")
def staged_scene():
    tris, where = build_scene()
    premises(tris, where)
    verts = [v for t in tris for v in t]
    md = pixel_model([dict(verts=verts, indices=list(range(len(verts))), topology=scene.TOPO_LIST, debug_id=5)])
    draws = [dict(md=md, M=pixel_to_ndc_matrix(W, H))]
    ref = render_oracle(W, H, draws)
    assert ref[2]["tris_setup"] == len(tris)  # every triangle faces front and holds a pixel centre
    return draws, ref


def test_scene_premises(staged_scene):
    """no device: the fixture has checked the premises and the oracle has set up every triangle; the frame is not empty"""
    draws, ref = staged_scene
    assert (ref[1] != 1.0).sum() > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("waves", ["2", "4", "8"])
def test_staged_records_at_every_wave_count(staged_scene, waves):
    from mt_renderer_amd import api
    draws, ref = staged_scene
    old = os.environ.get("MTR_VIS_WAVES")
    os.environ["MTR_VIS_WAVES"] = waves  # read when the device is created (tests/test_gpu_vis_waves.py)
    try:
        dev = api.Device(0)
    finally:
        if old is None:
            del os.environ["MTR_VIS_WAVES"]
        else:
            os.environ["MTR_VIS_WAVES"] = old
    try:
        g = render_gpu(dev, W, H, draws)  # ordered two-pass, ordered single-pass and auto agree; auto is returned
        assert g[2]["tile_kernel"] == api.TILE_VISIBILITY and g[2]["binning"] == 1, g[2]
        assert_same(g, ref, "waves=" + waves)
        dev.set_binning(False)  # the visibility kernel once more, behind the exact two-pass queues
        g2 = render_gpu(dev, W, H, draws, tile_mode=api.TILE_AUTO)
        assert g2[2]["tile_kernel"] == api.TILE_VISIBILITY and g2[2]["binning"] == 2, g2[2]
        assert_same(g2, ref, "waves=%s, two-pass queues" % waves)
    finally:
        dev.close()
