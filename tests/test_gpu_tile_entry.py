"""-m gpu: the entry path both tile kernels share (csrc/tile_common.h: tile_head, tile_enter, zero_next_counters).

A tile launch does three things for the NEXT frame on its framebuffer set before it looks at its own bin: it clears the
other counter block (4 128 words), clears the slot's culling counters (32 words per draw) after publishing the ones the
host asked for, and publishes the overflow flags.  The workgroups share that work by a grid-stride loop over
blockIdx.x * (threads per workgroup) -- a block size the kernels take from their template and a grid they take from the head
of their parameters -- and a workgroup that owns no word skips the loop.  So the launches that matter are the small ones:
fewer threads than words (one bin: 8 workgroups), and more workgroups than own a word.

Every frame here is one of several in a row on recycled colour / depth / counter sets and is held to the CPU oracle bit for
bit in colour and depth, with tris_in and tris_setup.  The oracle has no bin queues; for them the scenes are built so that the
numbers are known: every triangle lies inside one bin, so bin_entries == tris_setup, and `segments` must be what the first
frame of a device that has rendered nothing reports (its counters come from the allocation's memset, not from a tile kernel).
A counter word left dirty shows as a statistic of the second use of a set that is the sum of two frames'.  Two scenes with
different counts alternate, so that no stale value can pass for the right one.

Then the bin order (MTR_TILE_RUN 0, 1, 16, 65 536 on 153 bins, an own_list, a rank without a bin), and the culling counters
of a frame of more draws than the launch has threads per word.  Whether a launch hint reached the host has no public
observable; what is held is that the frames sized by them stay exact and cull the same chunks, frame after frame."""
import os

import numpy as np
import pytest

from mt_renderer_amd import scene, sharding
from tests.helpers import render_oracle
from tests.pixel_scenes import pixel_model, pixel_to_ndc_matrix

pytestmark = pytest.mark.gpu

TARGETS = [(16, 16), (48, 32), (272, 144)]  # 1 bin (8 workgroups: the loops stride), 6 bins, 153 bins (more workgroups than words / 128)
NFRAMES = 6


def _quad(x0, y0, size, z, did):
    v = [(x0, y0, z), (x0, y0 + size, z), (x0 + size, y0 + size, z), (x0 + size, y0, z)]
    return dict(verts=v, indices=[0, 1, 2, 0, 2, 3], debug_id=did)


def _scene(w, h, variant):
    """quads of 5 to 9 px, each inside one 16 x 16 bin (2 px clear of its edges), one to three per used bin, nearer ones
    later or earlier in submission order; variant 1 uses other bins and other counts than variant 0.  Some bins stay empty."""
    nbx, nby = (w + 15) // 16, (h + 15) // 16
    quads = []
    for b in range(nbx * nby):
        if nbx * nby > 1 and (b * 7 + variant * 3) % 5 in (1, 3):
            continue  # an empty bin
        bx, by = b % nbx, b // nbx
        n = 1 + (b + variant) % 3
        for k in range(n):
            size = 5.0 + (b + 2 * k + variant) % 5
            x0 = 16.0 * bx + 2.0 + (k * 2 + variant) % (12.0 - size + 1.0)
            y0 = 16.0 * by + 2.0 + (k + b) % (12.0 - size + 1.0)
            if x0 + size > w - 1 or y0 + size > h - 1:
                continue
            z = 0.2 + 0.1 * ((k * 2 + b + variant) % 7)
            quads.append(_quad(x0, y0, size, z, (b + 5 * k + variant) % 20))
    return [dict(md=pixel_model(quads), M=pixel_to_ndc_matrix(w, h))]


_refs = {}


def _ref(w, h, variant):
    """(draws, oracle frame) of a scene, computed once"""
    if (w, h, variant) not in _refs:
        draws = _scene(w, h, variant)
        _refs[(w, h, variant)] = (draws, render_oracle(w, h, draws))
    return _refs[(w, h, variant)]


def _device(**env):
    """a device of its own: MTR_VIS_WAVES, MTR_TILE_RUN and MTR_NSLOTS are read when a device is created"""
    from mt_renderer_amd import api
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return api.Device(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _frame(dev, w, h, model, M, shard=None):
    from mt_renderer_amd import api
    fr = api.Frame(dev, w, h)
    try:
        if shard:
            fr.set_shard(*shard)
        model.render(fr, M)
        fr.end()
        return fr.color(), fr.depth().view(np.uint32), fr.stats()
    finally:
        fr.close()


def _same(got, ref, own, what):
    gc, gd, gs = got
    rc, rd, rs = ref
    assert (gc[own] == rc[own]).all() and (gd[own] == rd.view(np.uint32)[own]).all(), what


_first = {}


def _first_use(w, h, variant, single_pass, tile_mode):
    """bin statistics of the scene's frame as the first frame of a device that has rendered nothing"""
    from mt_renderer_amd import api
    key = (w, h, variant, single_pass, tile_mode)
    if key not in _first:
        draws, _ = _ref(w, h, variant)
        with api.Device(0) as dev:
            dev.set_binning(single_pass)
            dev.set_tile_mode(tile_mode)
            model = api.Model.new(dev, draws[0]["md"])
            try:
                _first[key] = _frame(dev, w, h, model, draws[0]["M"])[2]
            finally:
                model.close()
    return _first[key]


KERNELS = [("vis-w2", "2"), ("vis-w4", "4"), ("vis-w8", "8"), ("ordered", None)]


@pytest.fixture(scope="module", params=KERNELS, ids=[k[0] for k in KERNELS])
def kernel_device(request):
    """(device, tile mode): the visibility kernel at 2, 4 and 8 waves per bin, and the ordered kernel"""
    from mt_renderer_amd import api
    name, waves = request.param
    dev = _device(MTR_VIS_WAVES=waves) if waves else api.Device(0)
    yield dev, (api.TILE_AUTO if waves else api.TILE_ORDERED)
    dev.close()


@pytest.mark.parametrize("single_pass", [False, True], ids=["two-pass", "single-pass"])
@pytest.mark.parametrize("w,h", TARGETS, ids=["%dx%d" % t for t in TARGETS])
def test_counters_are_clean_on_every_reuse_of_a_set(kernel_device, w, h, single_pass):
    """six frames in a row, scenes 0, 1, 0, 1, ...: each is the oracle's, with the statistics of a first use"""
    from mt_renderer_amd import api
    dev, tile_mode = kernel_device
    models = []
    try:
        dev.set_binning(single_pass)
        dev.set_tile_mode(tile_mode)
        scenes = [_ref(w, h, v) for v in (0, 1)]
        models = [api.Model.new(dev, draws[0]["md"]) for draws, _ in scenes]
        everything = np.ones((h, w), dtype=bool)
        counts = set()
        for k in range(NFRAMES):
            v = k & 1
            draws, ref = scenes[v]
            got = _frame(dev, w, h, models[v], draws[0]["M"])
            st, first = got[2], _first_use(w, h, v, single_pass, tile_mode)
            what = (w, h, "frame %d" % k, st, first)
            print(what)
            _same(got, ref, everything, what)
            assert st["tile_kernel"] == (api.TILE_VISIBILITY if tile_mode == api.TILE_AUTO else api.TILE_ORDERED), what
            assert st["binning"] == (1 if single_pass else 2), what
            assert st["tris_in"] == ref[2]["tris_in"] and st["tris_setup"] == ref[2]["tris_setup"] > 0, what
            assert st["bin_entries"] == ref[2]["tris_setup"], what  # every triangle lies inside one bin
            assert st["segments"] == first["segments"] > 0, what
            counts.add((st["bin_entries"], st["segments"]))
        assert len(counts) == 2, counts  # the two scenes really differ: a stale count cannot pass for the right one
    finally:
        for m in models:
            m.close()
        dev.set_binning(True)
        dev.set_tile_mode(api.TILE_AUTO)


RUNS = ["0", "1", "16", "65536"]


@pytest.mark.parametrize("run", RUNS)
def test_bin_order_at_forced_run_lengths(run):
    """153 bins -- no multiple of 16, nor of 65 536 -- dealt to the XCDs in runs of 1, 16 and 65 536 bins and in contiguous
    eighths; then through an own_list (rank 1 of 3, super-tiles of 2 x 2 bins) and as a rank that owns no bin.  Both kernels."""
    from mt_renderer_amd import api
    w, h = 272, 144
    dev = _device(MTR_TILE_RUN=run)
    model = None
    try:
        draws, ref = _ref(w, h, 0)
        model = api.Model.new(dev, draws[0]["md"])
        M = draws[0]["M"]
        everything = np.ones((h, w), dtype=bool)
        for tile_mode in (api.TILE_AUTO, api.TILE_ORDERED):
            dev.set_tile_mode(tile_mode)
            for k in range(2):
                got = _frame(dev, w, h, model, M)
                _same(got, ref, everything, (run, tile_mode, k))
                assert got[2]["tris_setup"] == ref[2]["tris_setup"] == got[2]["bin_entries"], (run, tile_mode, k, got[2])
            owner = sharding.owner_map(w, h, 3, sharding.SUPERTILES, 1)
            own = owner == 1
            assert own.any() and not own.all()
            part = _frame(dev, w, h, model, M, shard=(1, 3, sharding.SUPERTILES, 1))
            _same(part, ref, own, (run, tile_mode, "super-tiles rank 1 of 3"))
            assert 0 < part[2]["bin_entries"] < ref[2]["tris_setup"]
            bands = [0, 5, 5, 9]  # rank 1 owns no bin row: no tile workgroup is launched, the host publishes the status itself
            assert not (sharding.owner_map(w, h, 3, sharding.BANDS, 0, bands) == 1).any()
            none = _frame(dev, w, h, model, M, shard=(1, 3, sharding.BANDS, 0, bands))
            assert none[2]["shard_bins"] == 0, none[2]
            # ... and the next frame of the set is whole again
            _same(_frame(dev, w, h, model, M), ref, everything, (run, tile_mode, "after the empty rank"))
    finally:
        if model:
            model.close()
        dev.close()


def test_culling_counters_of_more_draws_than_the_launch_has_threads_per_word():
    """A sharded frame of 136 batch draws on a rank that owns ONE bin (a 16 x 48 target in three bands): its tile launch is
    8 workgroups of 512 threads and has 136 x 32 = 4 352 culling-counter words to clear for the next frame of the slot, so the
    loop strides; the first four draws report their counters before they are cleared.  Six frames on one slot: the owned
    pixels are the oracle's, and every frame culls what the first frame of a fresh device culled."""
    from mt_renderer_amd import api
    w, h, world, rank, nb = 16, 48, 3, 1, 136
    bands = [0, 1, 2, 3]
    own = sharding.owner_map(w, h, world, sharding.BANDS, 0, bands) == rank
    assert own.sum() == 16 * 16
    md = pixel_model([_quad(0.0, 0.0, 6.0, 0.0, d) for d in (3, 11)])
    vp = pixel_to_ndc_matrix(w, h)
    draws = []
    for b in range(nb):
        mats = []
        for k, (x, y) in enumerate(((2.0 + b % 7, 2.0 + 16.0 * ((b + 1) % 3) + b % 5), (3.0 + b % 5, 18.0 + (b * 3) % 8))):
            m = np.eye(4)
            m[0, 3], m[1, 3], m[2, 3] = x, y, 0.1 + 0.005 * ((b * 13 + k * 7) % 150)
            mats.append(scene.to_f32_colmajor(m))
        draws.append(dict(md=md, vp=vp, model_mats=np.stack(mats)))
    ref = render_oracle(w, h, draws)
    assert nb * 32 > 8 * 512  # MTR_CULL_CTR_WORDS per draw against the threads of the launch

    def frames(dev, n):
        model = api.Model.new(dev, md)
        batches = [api.Batch(dev, model, d["model_mats"]) for d in draws]
        out = []
        try:
            for _ in range(n):
                fr = api.Frame(dev, w, h)
                try:
                    fr.set_shard(rank, world, sharding.BANDS, 0, bands)
                    for b in batches:
                        fr.draw_batch(b, vp)
                    fr.end()
                    out.append((fr.color(), fr.depth().view(np.uint32), fr.stats()))
                finally:
                    fr.close()
        finally:
            for b in batches:
                b.close()
            model.close()
        return out

    with api.Device(0) as fresh_dev:
        fresh = frames(fresh_dev, 1)[0]
    assert fresh[2]["shard_bins"] == 1 and fresh[2]["ndraws"] == nb and fresh[2]["chunks_culled"] > 0, fresh[2]
    dev = _device(MTR_NSLOTS="1", MTR_VIS_WAVES="8")
    try:
        for k, got in enumerate(frames(dev, NFRAMES)):
            print("frame", k, got[2])
            _same(got, ref, own, ("frame", k))
            for key in ("tris_setup", "bin_entries", "segments", "chunks", "chunks_culled"):
                assert got[2][key] == fresh[2][key], (k, key, got[2], fresh[2])
    finally:
        dev.close()
