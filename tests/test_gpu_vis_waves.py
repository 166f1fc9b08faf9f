"""-m gpu: k_tile_vis.hip at 2, 4 and 8 waves per bin, on the edges of its per-wave pipeline.  The launcher picks the wave
count from the number of bins a rank owns (mtr_vis_waves_for, mtr_internal.h): every other directed scene of the suite is small
and runs 8 waves, where a wave never meets a second pass of its own.  Here a device is created with MTR_VIS_WAVES forced and
the scenes of tests/vis_wave_scenes.py are built for that count: a wave's second and third iteration (a_cur = a_nxt, ord_nxt =
ord_nn, the e0 + 2 * stride load), a partial last pass on any wave, waves without a pass, the three walks in successive
iterations of one wave, a pass at the span walk's bound of 64 x 16 rows and pair walks of two and of three rounds (the most a
pass can need) as a second iteration, the
speculative entry loads against a queue capacity that is no multiple of the stride, order lists filled by several waves at
once, and the resolve with two pixels per thread.

Before a scene is rendered its premise is computed from its integers (tests/test_vis_wave_premises.py holds the same premises
without a device, and the oracle frames).  Every scene goes through tests.helpers.render_gpu -- ordered two-pass, ordered
single-pass and auto must agree -- and once more through the exact two-pass queues; each frame equals the oracle's bit for
bit in colour and depth.  What a premise says about the entry count (iterations per wave, the wave of the partial pass, idle
waves) holds for every queue builder.  What it says about WHICH triangles share a pass -- the walk kinds in successive
iterations, ties between two iterations of one wave, fragment k in pass k, the rounds of a pair walk -- holds in the
single-pass queues: a scene is one draw per 32 triangles, and a frame's draws are geometry launches that follow one another on
one stream.  The two-pass fill places a frame's chunks as their waves arrive, in any order.  Nothing reads a queue back, so the
order is not asserted here; a build that skips a partial last pass fails exactly the sizes that have one, at every wave count.

All builds give the same pixels by design, so pixels cannot show that the forced build ran: tests/cpp/frame_launch_log.cpp
pins the hook's way to the launcher and the launcher's rule on the CPU."""
import os

import numpy as np
import pytest

from mt_renderer_amd import sharding
from tests import vis_wave_scenes as vs
from tests.helpers import assert_same, render_gpu
from tests.test_vis_wave_premises import RESOLVE_CASES, case_id, cases, check_premise, frame

pytestmark = pytest.mark.gpu

OPAQUE = ("pipeline_edges", "walks_per_iteration", "big_boxes_second_iteration")


@pytest.fixture(scope="module", params=["2", "4", "8"], ids=["w2", "w4", "w8"])
def wave_device(request):
    """(device, W): a device whose visibility kernel runs W waves per bin (MTR_VIS_WAVES is read when the device is created)"""
    from mt_renderer_amd import api
    old = os.environ.get("MTR_VIS_WAVES")
    os.environ["MTR_VIS_WAVES"] = request.param
    try:
        dev = api.Device(0)
    finally:
        if old is None:
            del os.environ["MTR_VIS_WAVES"]
        else:
            os.environ["MTR_VIS_WAVES"] = old
    yield dev, int(request.param)
    dev.close()


def both_queue_builders(dev, sc, draws, ref, what, kernel, clear_depth=1.0):
    """render_gpu (ordered two-pass, ordered single-pass, auto: all agree), then auto through the exact two-pass queues"""
    from mt_renderer_amd import api
    try:
        g = render_gpu(dev, sc.w, sc.h, draws, clear_depth=clear_depth)
        assert g[2]["tile_kernel"] == kernel, (what, g[2])
        assert_same(g, ref, what)
        dev.set_binning(False)
        g2 = render_gpu(dev, sc.w, sc.h, draws, clear_depth=clear_depth, tile_mode=api.TILE_AUTO)
    finally:
        dev.set_binning(True, 1024)  # a single-pass frame over 1024 entries per bin doubles the device's bound
    assert g2[2]["tile_kernel"] == kernel and g2[2]["binning"] == 2, (what, g2[2])
    assert_same(g2, ref, what + " (two-pass queues)")
    return g


def kernel_of(name):
    from mt_renderer_amd import api
    return api.TILE_VISIBILITY if name in OPAQUE else api.TILE_MIXED


# the scenes are built per W, so the cases are named by their place in cases(W): the same list of names at every W
CASE_IDS = [case_id((n, ("N%d" % i,) if n == "pipeline_edges" else a)) for i, (n, a) in enumerate(cases(2))]


@pytest.mark.parametrize("ci", range(len(CASE_IDS)), ids=CASE_IDS)
def test_scene_matches_the_oracle(wave_device, ci):
    dev, W = wave_device
    name, args = cases(W)[ci]
    sc, draws, ref = frame(name, W, *args)
    check_premise(name, sc, W, *args)
    both_queue_builders(dev, sc, draws, ref, "W=%d %s%s" % (W, name, args), kernel_of(name))


@pytest.mark.parametrize("ni", range(8), ids=["N1", "N65", "S-1", "S", "S+1", "2S", "2S+1", "3S+1"])
def test_direct_queue_exactly_full_and_ragged(wave_device, ni):
    """single-pass queues of exactly N entries, and of a capacity that is neither a multiple of the stride nor of 64: the
    guards of the two speculative entry loads fall inside a wave's 64 lanes"""
    from mt_renderer_amd import api
    dev, W = wave_device
    S = 64 * W
    N = vs.pipeline_edge_sizes(W)[ni]
    sc, draws, ref = frame("pipeline_edges", W, N)
    check_premise("pipeline_edges", sc, W, N)
    caps = [max(N, 64)]  # 64 is the smallest capacity the library takes
    if N >= S:
        caps.append(N + 37)
        assert (N + 37) % 64 != 0 and (N + 37) % S != 0
    try:
        for q in caps:
            dev.set_binning(True, q)
            g = render_gpu(dev, sc.w, sc.h, draws, tile_mode=api.TILE_AUTO)
            assert g[2]["tile_kernel"] == api.TILE_VISIBILITY and g[2]["binning"] == 1, (W, N, q, g[2])
            assert_same(g, ref, "W=%d N=%d qcap=%d" % (W, N, q))
    finally:
        dev.set_binning(True, 1024)


@pytest.mark.parametrize("clear_depth", [0.5, -1.0])
def test_clear_depth_below_one_and_below_zero(wave_device, clear_depth):
    """zlim below 1: the far fragments fail; a negative clear depth (zlim_ok false): nothing passes and the frame is the clear
    colour and the clear depth, as the oracle says (test_vis_wave_premises.py: test_clear_depths_of_the_gpu_file)"""
    from mt_renderer_amd import api
    dev, W = wave_device
    N = 2 * 64 * W + 1
    sc, draws, ref = frame("pipeline_edges", W, N, clear_depth=clear_depth)
    both_queue_builders(dev, sc, draws, ref, "W=%d clear_depth=%g" % (W, clear_depth), api.TILE_VISIBILITY, clear_depth)


@pytest.mark.parametrize("name", ["pipeline_edges", "lists_from_every_wave"])
def test_band_shard_ranks_at_forced_waves(wave_device, name):
    """rank 0 and rank 1 of a 2-way band shard of a target of two bin rows take their bins from an own_list"""
    dev, W = wave_device
    args = (3 * 64 * W + 1,) if name == "pipeline_edges" else ()
    sc, draws, ref = frame(name, W, *args, h=32)
    check_premise(name, sc, W, *args)
    bands = [0, 1, 2]
    owner = sharding.owner_map(sc.w, sc.h, 2, sharding.BANDS, 0, bands)
    try:
        whole = render_gpu(dev, sc.w, sc.h, draws)
        assert_same(whole, ref, name)
        for rank in range(2):
            own = owner == rank
            assert own.any()
            part = render_gpu(dev, sc.w, sc.h, draws, shard=(rank, 2, sharding.BANDS, 0, bands))
            assert (part[0][own] == whole[0][own]).all() and (part[1].view(np.uint32)[own] == whole[1].view(np.uint32)[own]).all(), (name, W, rank)
    finally:
        dev.set_binning(True, 1024)


def test_dominated_fragments_whatever_the_timing(wave_device):
    """how many of the 12 fragments get listed depends on which wave is first; the pixels must not.  Five renders in a row,
    each equal to the oracle: an invariant over timing, not a retry -- the first difference fails"""
    from mt_renderer_amd import api
    dev, W = wave_device
    sc, draws, ref = frame("dominated_across_waves", W)
    check_premise("dominated_across_waves", sc, W)
    for i in range(5):
        g = render_gpu(dev, sc.w, sc.h, draws, tile_mode=api.TILE_AUTO)
        assert g[2]["tile_kernel"] == api.TILE_MIXED
        assert_same(g, ref, "W=%d render %d" % (W, i))


@pytest.mark.parametrize("w,h,mixed", RESOLVE_CASES, ids=["%dx%d-%s" % (w, h, "mixed" if m else "opaque") for w, h, m in RESOLVE_CASES])
def test_resolve_pairs(wave_device, w, h, mixed):
    """two pixels per thread at two waves (t and t + 128); built for W = 2 and rendered at every W"""
    from mt_renderer_amd import api
    dev, W = wave_device
    sc, draws, ref = frame("resolve_pairs", 2, w, h, mixed)
    check_premise("resolve_pairs", sc, 2, w, h, mixed)
    both_queue_builders(dev, sc, draws, ref, "W=%d resolve_pairs %dx%d" % (W, w, h), api.TILE_MIXED if mixed else api.TILE_VISIBILITY)
