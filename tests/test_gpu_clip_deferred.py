"""-m gpu: the deferred-clip path of the geometry stage.  k_geom holds no clipper: a wave that meets a triangle to clip (a
vertex behind the near plane, or one that cannot be projected) appends its chunk to the frame's deferred list and emits
nothing; k_geom_clip, behind the draw's geometry launches, runs the listed chunks whole.  Records live at fixed places and
queue entries carry the chunk id, so which kernel emits a chunk must change no pixel and no statistic: every scene is
compared with the CPU oracle bit for bit -- colour, depth, tris_in, tris_setup (helpers.assert_same) -- through the exact
two-pass queues (geometry MODE 0), the ordered single-pass queues (MODE 1) and the unordered ones of the visibility kernel
(MODE 2): helpers.render_gpu runs the three and requires them to agree.  tests/test_clip_defer_premises.py checks on the
CPU which chunks of each scene clip."""
import numpy as np
import pytest

from mt_renderer_amd import api, scene, sharding
from tests import clip_defer_scenes as cs
from tests.helpers import assert_same, render_gpu, render_oracle

pytestmark = pytest.mark.gpu

W, H = cs.W, cs.H


def _check(dev, draws, what, w=W, h=H, min_setup=1):
    ref = render_oracle(w, h, draws)
    assert ref[2]["tris_setup"] >= min_setup and (ref[0][..., :3] != 255).any(), what
    got = render_gpu(dev, w, h, draws)
    assert_same(got, ref, what)
    return got, ref


@pytest.mark.parametrize("ordered", [False, True], ids=["opaque", "translucent_ordered"])
def test_one_lane_clips_among_ordinary_lanes(gpu_device, ordered):
    """chunk 1 of 3 is deferred.  translucent_ordered: the triangles of the chunk overlap and blend without depth write, so
    the records of the chunk's run -- the clipped triangle's among them -- must come out in submission order"""
    draws = [dict(md=cs.one_vertex_behind(ordered), M=cs.M_W)]
    got, _ = _check(gpu_device, draws, f"one lane clips, ordered={ordered}", min_setup=100)
    assert got[2]["chunks"] == 3
    assert got[2]["tile_kernel"] == (api.TILE_ORDERED if ordered else api.TILE_VISIBILITY)


@pytest.mark.parametrize("which", ["behind_the_eye", "out_of_band"])
def test_a_seven_vertex_fan_behind_ordinary_lanes(gpu_device, which):
    """five fan slots reserved behind the ordinary records of the last chunk; the fan triangles that cover no pixel of the
    target leave holes in the run.  behind_the_eye: a vertex at w < 0, near plane and guard band; out_of_band: every w
    positive, one vertex beyond +-2^20 px, the guard band alone"""
    tri = cs.FAN_TRIANGLE if which == "behind_the_eye" else cs.FAN_TRIANGLE_OUT_OF_BAND
    draws = [dict(md=cs.fan_after_a_grid(tri), M=cs.M_W)]
    _check(gpu_device, draws, f"seven-vertex fan, {which}", min_setup=100)


def test_a_chunk_that_needs_more_slots_than_it_has_fails_the_frame(gpu_device):
    draws = [dict(md=cs.fans_that_overflow(), M=cs.M_W)]
    for binning, mode in ((False, api.TILE_ORDERED), (True, api.TILE_ORDERED), (True, api.TILE_AUTO)):
        gpu_device.set_binning(binning)
        try:
            with pytest.raises(api.MtrError) as e:
                render_gpu(gpu_device, W, H, draws, tile_mode=mode)
        finally:
            gpu_device.set_binning(True)
        assert e.value.code == api.MTR_E_OVERFLOW and "124 records" in str(e.value), e.value
    ok = [dict(md=cs.nothing_clips(), M=cs.M_W)]  # the device is fine afterwards
    _check(gpu_device, ok, "after the overflow", min_setup=160)


def test_every_chunk_deferred_then_none_on_the_same_slots(gpu_device):
    """render_gpu submits three frames, one per slot of the device: after the first scene every slot's list holds three
    entries and every counter block has counted three.  The second scene defers nothing and the third again everything:
    stale entries or a count that was not zeroed would run chunks twice (tris_setup) or under the wrong draw"""
    clip = [dict(md=cs.every_chunk_clips(), M=cs.M_W)]
    plain = [dict(md=cs.nothing_clips(), M=cs.M_W)]
    a, _ = _check(gpu_device, clip, "every chunk deferred", min_setup=100)
    b, ref = _check(gpu_device, plain, "none deferred, after a frame that deferred", min_setup=160)
    assert b[2]["tris_setup"] == ref[2]["tris_setup"] == 160
    c, _ = _check(gpu_device, clip, "every chunk deferred again", min_setup=100)
    assert (a[0] == c[0]).all() and a[2]["tris_setup"] == c[2]["tris_setup"]
    fresh = api.Device(0)
    try:
        f = render_gpu(fresh, W, H, plain)
    finally:
        fresh.close()
    assert (f[0] == b[0]).all() and (f[1].view(np.uint32) == b[1].view(np.uint32)).all()


def test_four_draws_share_the_frames_list(gpu_device):
    """clip, plain, clip, clip: each draw's clip launch must take its own entries of the frame's list and no other's"""
    a, b = cs.every_chunk_clips(), cs.nothing_clips()
    shift = lambda dx, dy: scene.to_f32_colmajor(np.array([[0.4, 0, dx, 0], [0, 0.4, dy, 0], [0, 0, 0.25, 0], [0, 0, 1, 0]], dtype=np.float64))
    draws = [dict(md=a, M=shift(-0.5, -0.5)), dict(md=b, M=shift(0.5, -0.5)), dict(md=cs.one_vertex_behind(), M=shift(-0.5, 0.5)),
             dict(md=a, M=shift(0.5, 0.5))]
    _check(gpu_device, draws, "four draws, three that clip", min_setup=400)


def test_a_batch_where_two_of_four_instances_clip(gpu_device):
    """a palette per instance: a clip workgroup that staged another instance's palette or matrix moves the clipped chunks"""
    w, h = 320, 200
    draws = [cs.skinned_batch_two_of_four_clip(w, h)]
    got, ref = _check(gpu_device, draws, "two of four instances clip", w, h, min_setup=300)
    owned = dict(draws[0], owned=True)  # a batch the frame owns goes the same way
    assert_same(render_gpu(gpu_device, w, h, [owned]), ref, "owned batch")


def test_a_sharded_frame_with_a_clipped_triangle_in_each_band(gpu_device):
    """world 2 on one GPU, bands: the culled geometry launch (work masks) defers, the clip kernel emits for the rank"""
    draws = [dict(md=cs.every_chunk_clips(strips=6, cols=40), M=cs.M_W), cs.skinned_batch_two_of_four_clip(W, H)]
    full, _ = _check(gpu_device, draws, "unsharded", min_setup=400)
    owner = sharding.owner_map(W, H, 2, sharding.BANDS)
    for rank in range(2):
        for mode in (api.TILE_AUTO, api.TILE_ORDERED):
            part = render_gpu(gpu_device, W, H, draws, shard=(rank, 2, sharding.BANDS), tile_mode=mode)
            own = owner == rank
            assert (part[0][own] == full[0][own]).all() and (part[1].view(np.uint32)[own] == full[1].view(np.uint32)[own]).all(), (rank, mode)
            assert 0 < part[2]["tris_setup"] <= full[2]["tris_setup"]


def test_more_deferred_chunks_than_the_clip_grid_takes_at_once(gpu_device):
    """360 instances x 3 chunks, all deferred: 1080 entries against 256 workgroups of four waves, so the stride loop runs;
    neighbouring entries belong to different instances, so the workgroups stage more than once"""
    md = cs.every_chunk_clips()
    draws = [dict(md=md, vp=cs.M_W, model_mats=cs.lattice_mats(18, 20))]
    got, _ = _check(gpu_device, draws, "1080 deferred chunks", 256, 192, min_setup=2000)
    assert got[2]["chunks"] == 1080
