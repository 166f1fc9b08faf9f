"""-m gpu: every code of every vertex format through both decode paths of the geometry stage, and through the host mirror.

tests/vertex_decode_cases.py holds the reference tables (integer arithmetic) and the models; tests/test_vertex_decode_premises.py
pins the tables to the IEEE division, the oracle to the tables, and the models to what they claim.  Here:

* k_vertex_stage (load_elem + decode_regs) against the reference: every (format, count) pair as Position and as TexCoord, at
  four placements in memory, every code in every component, words equal; a NaN input of a decode that computes must give
  a NaN (SPEC section 2), F32 texcoords are bits and compared as bits;
* every weight byte in every slot, on the MFMA blocks and on the VALU redo, at palette sizes 1 and 64;
* the clipper's re-shade (geom_vertex.h: shade_vertex + decode_elem, reached by nothing else): frames whose triangles straddle the near
  plane or leave the guard band, every pair aligned and unaligned, both tile kernels, bit-exact against the oracle;
* the host mirror (decode_pos_host) behind the culling boxes: the same models, unsharded with culling of all frames and as
  rank 1 of 3, must come out the same with and without culling.

No tolerance anywhere.
"""
import functools

import numpy as np
import pytest

from mt_renderer_amd import sharding
from tests import vertex_decode_cases as vd
from tests import vertex_edge_cases as vx
from tests.helpers import assert_same, render_gpu, render_oracle

pytestmark = pytest.mark.gpu

EXHAUSTIVE = [(p, pl, r) for p in vd.PAIRS for pl in vd.PLACEMENTS for r in vd.ROLES]


@pytest.mark.parametrize("pair,placement,role", EXHAUSTIVE, ids=lambda v: v)
def test_vertex_stage_decodes_every_code(gpu_device, pair, placement, role):
    """identity matrix: clip is the decoded position (-0 as +0, w = 1), uv the decoded texcoord untouched.  As Position
    also under a matrix with no zero in it, on the sample that holds every edge code: exactly shade()."""
    from mt_renderer_amd import api
    c = vd.exhaustive_case(pair, role, placement)
    msgs = []
    m = api.Model.new(gpu_device, c.md)
    try:
        got = [m.vertex_stage(prim, vd.IDENTITY_M) for prim in range(len(c.prims))]
        head = np.concatenate([m.vertex_stage(prim, vx.HEADLINE_M)[0] for prim in range(len(c.prims))]) if role == "position" else None
    finally:
        m.close()
    for prim, (v0, n) in enumerate(c.prims):
        for what, g, ref in (("clip", got[prim][0], c.exp.clip[v0:v0 + n]), ("uv", got[prim][1], c.exp.uv[v0:v0 + n])):
            ok = vd.same_words(g, ref, nan_by_class=not (what == "uv" and c.uv_is_bits))
            if not ok.all():
                msgs.append(vd.describe_difference(c, f"{what}, prim {prim}", v0, ok, g, ref))
    if head is not None:
        ref = vd.headline_clip(pair)
        ok = vd.same_words(head[c.exp.sample], ref)
        if not ok.all():
            v = int(c.exp.sample[np.nonzero(~ok.all(axis=1))[0][0]])
            msgs.append(f"{c.name}, headline matrix: {int((~ok.all(axis=1)).sum())} of {len(ref)} sampled vertices differ; first: vertex {v}, "
                        f"fields {[hex(int(x)) for x in c.exp.codes[v]]}, got {[hex(int(x)) for x in head[v].view(np.uint32)]}, "
                        f"expected {[hex(int(x)) for x in ref[list(c.exp.sample).index(v)]]}")
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("npal", vd.WEIGHT_NPALS)
def test_vertex_stage_decodes_every_weight_byte(gpu_device, npal):
    """unorm8f as the weight decode: with one identity matrix clip.x is the decoded weight; with 64 matrices the
    expectation is shade()'s.  Every (byte, slot) sits in a coherent block (MFMA) and in one that is not (VALU redo)."""
    from mt_renderer_amd import api
    c = vd.weight_case()
    ref = vd.weight_clip(npal)
    m = api.Model.new(gpu_device, c.md)
    try:
        m.set_palette(c.pal[:npal])
        got = [m.vertex_stage(prim, vd.IDENTITY_M) for prim in range(len(c.prims))]
    finally:
        m.close()
    clip, uv = np.concatenate([g[0] for g in got]), np.concatenate([g[1] for g in got])
    ok = vd.same_words(clip, ref).all(axis=1)
    if not ok.all():
        v = int(np.nonzero(~ok)[0][0])
        prim = max(p for p, (v0, _) in enumerate(c.prims) if v0 <= v)
        pytest.fail(f"npal {npal}: {int((~ok).sum())} vertices differ; first: vertex {v}, block {c.patterns(prim)[v - c.prims[prim][0]]}, "
                    f"joints {c.joints[v].tolist()}, weights {c.weights[v].tolist()}, got {[hex(int(x)) for x in clip[v].view(np.uint32)]}, "
                    f"expected {[hex(int(x)) for x in ref[v]]}")
    assert (uv.view(np.uint32) == 0).all()


# ---------------------------------------------------------------------------------------------
# frames: the clipper's decode_elem, and the host mirror behind the culling boxes
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_frame(name, view):
    return render_oracle(vd.CLIP_W, vd.CLIP_H, vd.clip_scene(name).draws(view))


@pytest.mark.parametrize("name", vd.CLIP_SCENE_NAMES)
def test_clip_path_decodes_every_format(gpu_device, name):
    """the pair as Position and TexCoord of a textured triangle list: the plain view (nothing clips: the scene is well
    formed), the near-plane view (most triangles re-shade through decode_elem) and the guard-band view (vertices beyond
    +-2^20 px): two-pass, single-pass and auto binning x both tile kernels agree, and equal the oracle bit for bit"""
    s = vd.clip_scene(name)
    for view in ("plain", "near", "guard"):
        g = render_gpu(gpu_device, vd.CLIP_W, vd.CLIP_H, s.draws(view))
        assert_same(g, _oracle_frame(name, view), f"{name}, {view} view")
        assert g[2]["tris_setup"] > 0, (name, view)


@pytest.mark.parametrize("name", vd.CLIP_SCENE_NAMES)
def test_culling_keeps_every_edge_code_vertex(gpu_device, name):
    """decode_pos_host builds the boxes that culling trusts; a box that misses a vertex drops a triangle.  The plain view
    of every clip scene, unsharded with culling applied to all frames and as rank 1 of 3 on the band map with culling on and
    off: owned pixels, depth words, tris_setup and bin_entries are identical, and the unsharded frame is the oracle's."""
    from mt_renderer_amd import api
    s = vd.clip_scene(name)
    draws, w, h = s.draws("plain"), vd.CLIP_W, vd.CLIP_H
    shard = (1, 3, sharding.BANDS)
    own = sharding.owner_map(w, h, 3, sharding.BANDS) == 1
    res = {}
    try:
        for mode in (api.GEOM_CULL_OFF, api.GEOM_CULL_ALL_FRAMES):
            gpu_device.set_culling(mode)
            res[mode] = (render_gpu(gpu_device, w, h, draws, tile_mode=api.TILE_AUTO),
                         render_gpu(gpu_device, w, h, draws, shard=shard, tile_mode=api.TILE_AUTO))
    finally:
        gpu_device.set_culling(api.GEOM_CULL_SHARDED)
    assert_same(res[api.GEOM_CULL_OFF][0], _oracle_frame(name, "plain"), f"{name}, no culling")
    off, on = res[api.GEOM_CULL_OFF], res[api.GEOM_CULL_ALL_FRAMES]
    assert off[1][2]["chunks_culled"] == 0 and on[1][2]["chunks_culled"] > 0  # the boxes did decide something for the rank
    for k, (what, mask) in enumerate((("unsharded", np.ones((h, w), dtype=bool)), ("rank 1 of 3", own))):
        a, b = off[k], on[k]
        assert int(mask.sum()) > 0 and int((a[1][mask] < 1.0).sum()) > 100, (name, what)  # there is something to lose
        ncol = int((a[0][mask] != b[0][mask]).any(axis=-1).sum())
        nd = int((a[1].view(np.uint32)[mask] != b[1].view(np.uint32)[mask]).sum())
        assert ncol == 0 and nd == 0, f"{name}, {what}: culling changes {ncol} colour and {nd} depth pixels"
        for key in ("tris_setup", "bin_entries"):
            assert a[2][key] == b[2][key], (name, what, key, a[2][key], b[2][key])
