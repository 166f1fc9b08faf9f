"""What the scenes of tests/clip_defer_scenes.py claim about themselves, checked with their float64 model on the CPU: which
chunks hold a triangle to clip (those the geometry kernel defers), how many vertices the clipped triangles keep, and that
the strip built to overflow a chunk's record slots does."""
import numpy as np

from tests import clip_defer_scenes as cs


def _prim(md):
    (p,) = md.scene_prims
    return p


def test_one_vertex_behind_clips_one_chunk_of_three():
    for ordered, lanes in ((False, 1), (True, 3)):  # a corner vertex is in one triangle, one inside the last row in three
        p = _prim(cs.one_vertex_behind(ordered))
        assert cs.chunks_that_clip(p, cs.W, cs.H) == (3, {1})
        verts = np.asarray(p["verts"], dtype=np.float64)[:, :3]
        tris = [(pos, t) for pos, t in cs._strip_triangles(p["indices"]) if cs.needs_clip([verts[i] for i in t], cs.W, cs.H)]
        assert len(tris) == lanes and all(pos // cs.CHUNK_NEW == 1 for pos, _ in tris)
        # under M_W the near plane is w = 0: the cut lands where nothing projects, so the guard band clips the quad again
        # (the near-clipped quad whose corners all project is skinned_batch_two_of_four_clip's, under a real camera)
        for _, t in tris:
            assert 4 <= len(cs.clipped_polygon([verts[i] for i in t])) <= 8


def test_the_fan_triangle_keeps_seven_vertices_in_the_last_chunk():
    for tri in (cs.FAN_TRIANGLE, cs.FAN_TRIANGLE_OUT_OF_BAND):
        assert len(cs.clipped_polygon(tri)) == 7
        p = _prim(cs.fan_after_a_grid(tri))
        assert cs.chunks_that_clip(p, cs.W, cs.H) == (3, {2})
        slots = cs.fan_slots(p, cs.W, cs.H)
        assert slots[2] <= cs.CHUNK_SLOTS and slots[2] - 5 > 30  # five fan slots behind more than thirty ordinary triangles
    # the second one without the near plane: every w positive, one vertex beyond +-2^20 px
    assert all(v[2] > 0.0 for v in cs.FAN_TRIANGLE_OUT_OF_BAND)
    assert [cs._projectable(v, cs.W, cs.H) for v in cs.FAN_TRIANGLE_OUT_OF_BAND] == [True, True, False]


def test_the_overflow_strip_needs_more_slots_than_a_chunk_has():
    p = _prim(cs.fans_that_overflow())
    verts = np.asarray(p["verts"], dtype=np.float32).astype(np.float64)[:, :3]  # as the vertex buffer holds them
    for pos, t in cs._strip_triangles(p["indices"]):
        assert len(cs.clipped_polygon([verts[i] for i in t])) == 6, pos
    assert cs.fan_slots(p, cs.W, cs.H)[0] == 240 > cs.CHUNK_SLOTS


def test_every_chunk_or_none():
    assert cs.chunks_that_clip(_prim(cs.every_chunk_clips()), cs.W, cs.H) == (3, {0, 1, 2})
    assert cs.chunks_that_clip(_prim(cs.nothing_clips()), cs.W, cs.H) == (3, set())


def test_the_lattice_keeps_every_w_one_vertex_inside_the_frustum():
    """so an instance clips exactly the chunks the model clips: 18 x 20 instances x 3 chunks = 1080 deferred chunks, more
    than the 1024 the clip kernel's grid takes in one pass (256 workgroups of four waves)"""
    mats = cs.lattice_mats(18, 20).reshape(-1, 4, 4).transpose(0, 2, 1).astype(np.float64)
    corners = np.array([[x, y, 1.0, 1.0] for x in (-0.8, 0.8) for y in (-0.6, 0.6)])
    out = np.einsum("kij,cj->kci", mats, corners)
    assert (np.abs(out[..., 0]) < 1.0).all() and (np.abs(out[..., 1]) < 1.0).all() and (out[..., 2] == 1.0).all()
    assert 18 * 20 * 3 > 256 * 4
