"""-m gpu: the skinned vertex stage at its numeric edges, HIP against the oracle, bit for bit.

"A k-step v_mfma_f32_4x4x1 chain is bitwise an fmaf chain" (geom_vertex.h) carries the parity of all
skinned geometry: coherent blocks are skinned on the matrix cores, the others by the VALU chain, and clipped triangles
re-shade through the VALU chain vertices that their unclipped neighbours took from the MFMA.  tests/vertex_edge_cases.py
holds the inputs (cancellation, subnormal operands / products / sums, signed zeros, overflow, every weight and joint
edge, every block pattern and tail length); tests/test_vertex_edge_premises.py pins the oracle on those inputs to an
exact integer model and shows that unfused arithmetic or a flush of subnormals would change them.  Here:

* Model.vertex_stage (k_vertex_stage) equals the oracle on every case model at every palette size: words equal, or both NaN;
* the same inputs' kind through k_geom and the tile kernels: frames equal the oracle's (tests.helpers), finite numbers only.

No tolerance anywhere.
"""
import functools

import numpy as np
import pytest

from mt_renderer_amd import scene, sharding
from oracle import oracle as orc
from tests import vertex_edge_cases as vx
from tests.helpers import assert_same, render_gpu, render_oracle

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in vx.cases()}


@functools.lru_cache(maxsize=None)
def _oracle_vertices(name, prim, npal):
    c = CASES[name]
    return orc.OracleModel(c.md).vertex_stage(prim, c.M, vx.palette_of(c, npal))


def _vertex_stage_differences(dev, c, npals, exact_npals=()):
    from mt_renderer_amd import api
    msgs = []
    m = api.Model.new(dev, c.md)
    try:
        for npal in npals:
            m.set_palette(vx.palette_of(c, npal))
            for prim, (v0, n) in enumerate(c.prims):
                gc, gu = m.vertex_stage(prim, c.M)
                oc, ou = _oracle_vertices(c.name, prim, npal)
                refs = [("oracle", oc)] + ([("exact model", vx.model_clip(c, prim, npal))] if npal in exact_npals else [])
                for what, ref in refs:
                    ok = vx.same_words(gc, ref)
                    if not ok.all():
                        msgs.append(f"npal {npal}, against the {what}: " + vx.describe_first_difference(c, prim, ok, gc, ref))
                if not (gu.view(np.uint32) == ou.view(np.uint32)).all():
                    msgs.append(f"npal {npal}, prim {prim}: uv differs")
    finally:
        m.close()
    return msgs


@pytest.mark.parametrize("name", list(CASES))
def test_vertex_stage_equals_the_oracle_at_the_numeric_edges(gpu_device, name):
    """every palette size of the issue: none (the four-MFMA chain clip = M (p, 1) alone), 1, 5, 64, 256 (joint indices
    clamped to npal - 1).  The cases made for the unskinned path -- a matrix that cancels from thousands to order one,
    matrices with tiny and subnormal rows -- are held to the exact model directly as well."""
    c = CASES[name]
    msgs = _vertex_stage_differences(gpu_device, c, vx.NPALS, exact_npals=(None,) if name in vx.UNSKINNED_CASES else ())
    assert not msgs, "\n".join(msgs)


# ---------------------------------------------------------------------------------------------
# through k_geom and the tile kernels
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_frame(name):
    return render_oracle(vx.FRAME_W, vx.FRAME_H, vx.frame_scenes()[name])


def _frame(dev, name):
    # tile_mode None: two-pass, single-pass and auto binning x both tile kernels must agree among themselves first
    gpu = render_gpu(dev, vx.FRAME_W, vx.FRAME_H, vx.frame_scenes()[name])
    assert_same(gpu, _oracle_frame(name), name)
    return gpu


@pytest.mark.parametrize("pattern", vx.JOINT_PATTERNS)
@pytest.mark.parametrize("topology", ["strips", "list"])
def test_frame_restart_phases(gpu_device, topology, pattern):
    """strips whose restarts fall at every phase of the chunk and of the block (rail order), and the same
    vertices as a triangle list (identity order); joints coherent along a rail, random per vertex, or differing only in
    a slot of weight 0; a non-zero index_base and a few indices past vertex_num"""
    _frame(gpu_device, f"{topology}_{pattern}")


def test_frame_cancel_palette(gpu_device):
    """translations of +-2^k (k up to 16) that cancel to positions of order one: depth bits hang on the single rounding"""
    _frame(gpu_device, "cancel_palette")


def test_frame_near_plane_with_random_joints(gpu_device):
    """clipped triangles re-shade their vertices through the VALU shade_vertex; their unclipped neighbours hold the same
    vertices from shade_vertex_mfma.  First draw, random joints: incoherent blocks, its VALU fallback, the clip chain on
    the MFMA.  Second draw, joints per rail on the cancel palette: skinned on the MFMA too, where one bit shows"""
    g = _frame(gpu_device, "near_plane_random")
    assert g[2]["tris_setup"] > 0


def test_frame_tiny_z(gpu_device):
    """clip z and the depth buffer hold subnormals.  The vertex-stage test of `subnormal_b` covers the same kind of
    matrix: if only this one fails, look at the depth interpolation of the tile stage"""
    g = _frame(gpu_device, "tiny_z")
    bits = g[1].view(np.uint32)
    assert int(((bits > 0) & (bits < 0x00800000)).sum()) >= 1000


def test_frame_batch_with_256_matrices(gpu_device):
    """five instances, npal = 256 (the largest palette in LDS), palettes rolled per instance, cancellation in
    view_proj * model (stage_palette's chain)"""
    _frame(gpu_device, "batch_npal256")


def test_frame_batch_with_256_matrices_as_rank_1_of_3(gpu_device):
    """the same batch as rank 1 of 3 on the BANDS map with culling on (k_geom's culled variant): the rank's owned pixels
    are the oracle's"""
    draws = vx.frame_scenes()["batch_npal256"]
    ref = _oracle_frame("batch_npal256")
    gpu_device.set_culling(True)  # the default, whatever an earlier test left
    part = render_gpu(gpu_device, vx.FRAME_W, vx.FRAME_H, draws, shard=(1, 3, sharding.BANDS))
    own = sharding.owner_map(vx.FRAME_W, vx.FRAME_H, 3, sharding.BANDS) == 1
    assert part[2]["chunks_culled"] > 0  # the culled variant ran and had something to skip
    assert int((ref[1][own] < 1.0).sum()) > 100  # the rank has something to draw
    assert (part[0][own] == ref[0][own]).all() and (part[1].view(np.uint32)[own] == ref[1].view(np.uint32)[own]).all()
