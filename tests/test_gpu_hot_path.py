"""-m gpu: the corners the tile kernels' cheaper prologue and pass set-up must not cut (csrc/tile_common.h: udiv_apply,
row_magic).

Mixed classes in one pass: k_tile_vis.hip computes the pair walk's row multiplier only in the branches that read it -- the
pair walk and the whole-wave walk of a 64-bit-class triangle -- so the scenes put such a triangle into a 64-entry pass that
takes the span walk, into one that takes the pair walk, and both passes into one bin.  The premises (entries of the bin,
boxes over four pixels per pass, the edge class) are computed from the scene's integers and asserted before it is rendered.

Odd grids: the bin -> (column, row) step and the block -> bin map divide by multiply-high; 13 x 3 bins (a prime number of
bins per row) and a single bin are rendered with the contiguous block order, with interleaved runs, and as the ranks of a
band-sharded frame (an own_list).

Every frame is compared with the oracle bit for bit, in colour and depth, through both tile kernels."""
import os

import numpy as np
import pytest

from mt_renderer_amd import scene, sharding
from tests.helpers import assert_same, render_gpu, render_oracle
from tests.pixel_scenes import pixel_model, pixel_to_ndc_matrix
from tests.tile_path_scenes import BIN
from tests.vis_wave_scenes import BX, PAIR_PASS, SPAN_PASS, TH, TW, _pass  # the triangles and passes of this file's scenes live there

pytestmark = pytest.mark.gpu

W, H = TW, TH  # 8 x 1 bins; BX: the bin under test


def _check_premise(tris, walks):
    def in_bin(t):
        x0, x1, y0, y1 = t.box(W, H)
        return x0 <= x1 and y0 <= y1 and x0 <= BX * BIN + BIN - 1 and x1 >= BX * BIN
    def box_px(t):
        x0, x1, y0, y1 = t.box(W, H)
        return (min(x1, BX * BIN + BIN - 1) - max(x0, BX * BIN) + 1) * (y1 - y0 + 1)
    ent = [t for t in tris if in_bin(t)]
    assert len(ent) == len(tris) == 64 * len(walks)
    for p, walk in enumerate(walks):
        e = ent[64 * p:64 * p + 64]
        assert sum(t.large for t in e) == 1
        cand = [t for t in e if not t.large]
        assert all(box_px(t) in (1,) or box_px(t) >= 9 for t in cand)
        over4 = sum(box_px(t) > 4 for t in cand)
        assert (over4 * 2 >= len(cand)) == (walk == "span"), (p, over4, len(cand))
        assert any(len(t.pixels(W, H)) for t in cand)


def _draws(tris):
    prims = []
    for i in range(0, len(tris), 8):  # submission order kept; a debug colour per run of eight
        verts = [(float(x), float(y), float(t.z)) for t in tris[i:i + 8] for x, y in t.pts]
        prims.append(dict(verts=verts, indices=list(range(len(verts))), debug_id=(i // 8) % 20))
    return [dict(md=pixel_model(prims), M=pixel_to_ndc_matrix(W, H))]


@pytest.mark.parametrize("name,passes", [("span", [SPAN_PASS]), ("pair", [PAIR_PASS]), ("span_then_pair", [SPAN_PASS, PAIR_PASS])])
def test_large_triangle_in_a_pass_of_either_walk(gpu_device, name, passes):
    from mt_renderer_amd import api
    tris = [t for k, nbig in enumerate(passes) for t in _pass(nbig, k)]
    _check_premise(tris, ["span" if n == SPAN_PASS else "pair" for n in passes])
    draws = _draws(tris)
    ref = render_oracle(W, H, draws)
    g = render_gpu(gpu_device, W, H, draws)  # ordered (both queue builders) and auto agree
    assert g[2]["tile_kernel"] == api.TILE_VISIBILITY
    assert_same(g, ref, name)
    # the exact two-pass queues keep the submission order, so here the passes are the ones the premise describes
    gpu_device.set_binning(False)
    try:
        g2 = render_gpu(gpu_device, W, H, draws, tile_mode=api.TILE_AUTO)
    finally:
        gpu_device.set_binning(True)
    assert g2[2]["tile_kernel"] == api.TILE_VISIBILITY and g2[2]["binning"] == 2
    assert_same(g2, ref, name + " (two-pass queues)")
    assert g2[2]["bin_entries"] == g[2]["bin_entries"]
    assert int((g[1][:, BX * BIN:BX * BIN + BIN] < 1.0).sum()) > 128  # the large triangle covers most of the bin


# ---- odd grids ----
GRIDS = [("13x3", 208, 40), ("1x1", 16, 16), ("1x1_ragged", 13, 9)]
_REF = {}


def _grid_scene(w, h):
    if (w, h) not in _REF:
        md = scene.skinned_capsule_model([((0.0, 0.0, 0.0), 0.35, 1.6)], rows=16, cols=24)
        draws = [dict(md=md, M=scene.to_f32_colmajor(scene.headline_transform(w, h)), palette=scene.bone_palette())]
        _REF[(w, h)] = (draws, render_oracle(w, h, draws))
    return _REF[(w, h)]


@pytest.fixture(scope="module", params=["0", "3"], ids=["contiguous", "runs_of_3"])
def run_device(request):
    """a device whose tile kernels take their bins in the forced order (MTR_TILE_RUN is read when the device is created)"""
    from mt_renderer_amd import api
    old = os.environ.get("MTR_TILE_RUN")
    os.environ["MTR_TILE_RUN"] = request.param
    try:
        dev = api.Device(0)
    finally:
        if old is None:
            del os.environ["MTR_TILE_RUN"]
        else:
            os.environ["MTR_TILE_RUN"] = old
    yield dev
    dev.close()


@pytest.mark.parametrize("name,w,h", GRIDS, ids=[g[0] for g in GRIDS])
def test_odd_grid_in_forced_block_order(run_device, name, w, h):
    draws, ref = _grid_scene(w, h)
    g = render_gpu(run_device, w, h, draws)
    assert_same(g, ref, name)
    assert int((g[1] < 1.0).sum()) > 0
    # the ranks of a band-sharded frame take their bins from an own_list
    nby = (h + BIN - 1) // BIN
    bands = [0, 1, nby] if nby > 1 else [0, 1, 1]
    owner = sharding.owner_map(w, h, 2, sharding.BANDS, 0, bands)
    for rank in range(2):
        own = owner == rank
        part = render_gpu(run_device, w, h, draws, shard=(rank, 2, sharding.BANDS, 0, bands))
        assert (part[0][own] == ref[0][own]).all() and (part[1].view(np.uint32)[own] == ref[1].view(np.uint32)[own]).all(), (name, rank)
