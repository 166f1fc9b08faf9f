"""-m gpu: frames of many draws through the sharded, culled submit path (host_submit.cpp: prepare_stream, pick_launch_hints,
record_draw, record_tiles).  Every stage of a single draw is pinned elsewhere; here a frame has 5 to 260 draws of every kind
(tests/many_draw_scenes.py, its premises in tests/test_many_draw_premises.py) and what is held is the per-draw bookkeeping:
each draw's share of the four culling buffers, the culling counters that the previous frame of a slot cleared only up to
ITS draw count, the launch-size hints of more than four batches and of more batches than the device has hint slots, the
mixed frame's second tile kernel, the overflow re-run, chunk_base / mat_base over many draws.

Every sharded comparison has one form: the pixels the rank owns, colour and depth bits, are the unsharded frame's;
tris_setup and bin_entries do not depend on culling; with culling off nothing is culled."""
import numpy as np
import pytest

from mt_renderer_amd import scene, sharding
from tests import many_draw_scenes as mds
from tests.helpers import assert_same, render_gpu, render_oracle

pytestmark = pytest.mark.gpu

W, H = mds.W, mds.H
COUNTS = ("tris_setup", "bin_entries", "chunks_culled")


@pytest.fixture(scope="module")
def crowd40():
    return mds.crowd(40)


@pytest.fixture(scope="module")
def unsharded(gpu_device, crowd40):
    """the unsharded frame of every prefix the tests render, once: n -> (colour, depth bits, stats)"""
    cache = {}

    def get(n):
        if n not in cache:
            res = mds.Resident(gpu_device, crowd40.draws[:n])
            try:
                cache[n] = res.render(n)
            finally:
                res.close()
        return cache[n]
    return get


def _owned_equal(part, full, own, what):
    assert (part[0][own] == full[0][own]).all() and (part[1].view(np.uint32)[own] == full[1].view(np.uint32)[own]).all(), what


def _shard(bands, rank):
    return (rank, mds.WORLD, sharding.BANDS, 0, bands)


# ---- parity ----
@pytest.mark.parametrize("n", [5, 12, 40])
def test_many_draw_frames_equal_the_oracle(gpu_device, crowd40, unsharded, n):
    from mt_renderer_amd import api
    draws = crowd40.draws[:n]
    g = render_gpu(gpu_device, W, H, draws)  # both tile kernels x both queue builders inside
    assert_same(g, render_oracle(W, H, draws), f"crowd({n})")
    assert g[2]["tile_kernel"] == api.TILE_MIXED and g[2]["ndraws"] == n
    # the frame loop of the other tests (persistent batches, Frame.draw_instances) renders the same frame
    u = unsharded(n)
    assert (u[0] == g[0]).all() and (u[1] == g[1].view(np.uint32)).all() and u[2]["tris_setup"] == g[2]["tris_setup"]


def test_the_big_single_model_has_two_mask_groups_with_a_ragged_second(gpu_device, crowd40):
    from mt_renderer_amd import api
    big = [d for d in crowd40.of_kind("single") if mds.chunks_of(d["md"]) > 16][0]
    g = render_gpu(gpu_device, W, H, [big], tile_mode=api.TILE_AUTO)
    assert 17 <= g[2]["chunks"] <= 31 and g[2]["chunks"] == mds.chunks_of(big["md"])


# ---- every rank, every map ----
MAPS = [("bands", sharding.BANDS, 0, None), ("bands-uneven", sharding.BANDS, 0, mds.UNEVEN_BANDS), ("supertiles", sharding.SUPERTILES, 0, None)]


@pytest.mark.parametrize("name,own_map,param,bands", MAPS, ids=[m[0] for m in MAPS])
@pytest.mark.parametrize("n", [12, 40])
def test_every_rank_of_every_map_owns_the_unsharded_pixels(gpu_device, crowd40, unsharded, n, name, own_map, param, bands):
    draws = crowd40.draws[:n]
    full = unsharded(n)
    owner = sharding.owner_map(W, H, mds.WORLD, own_map, param, bands)
    for rank in range(mds.WORLD):
        own = owner == rank
        res = {}
        for cull in (True, False):
            gpu_device.set_culling(cull)
            try:
                res[cull] = render_gpu(gpu_device, W, H, draws, shard=(rank, mds.WORLD, own_map, param, bands))
            finally:
                gpu_device.set_culling(True)
            _owned_equal(res[cull], full, own, (name, n, rank, cull))
        assert res[False][2]["chunks_culled"] == 0 and res[True][2]["chunks_culled"] > 0, (name, n, rank)
        for key in ("tris_setup", "bin_entries"):
            assert res[True][2][key] == res[False][2][key], (name, n, rank, key)


# ---- one slot, changing draw counts ----
SEQUENCE = (12, 3, 12, 40, 1, 40, 5)
RANKS = [(mds.EVEN_BANDS, 1), (mds.EVEN_BANDS, 2), (mds.UNEVEN_BANDS, 1)]  # the last: an empty band, no tile kernel ever runs
_fresh_cache = {}


def _fresh(crowd, n, bands, rank):
    """the sharded frame of the first n draws on a device that has rendered nothing: clean counters, no hints"""
    from mt_renderer_amd import api
    key = (n, tuple(bands), rank)
    if key not in _fresh_cache:
        with api.Device(0) as dev:
            res = mds.Resident(dev, crowd.draws[:n])
            try:
                _fresh_cache[key] = res.render(n, _shard(bands, rank))
            finally:
                res.close()
    return _fresh_cache[key]


@pytest.mark.parametrize("wait_each", [True, False], ids=["wait-each", "submit-all-first"])
@pytest.mark.parametrize("nslots", ["1", None], ids=["one-slot", "default-slots"])
def test_frames_of_changing_draw_counts_on_recycled_slots(crowd40, unsharded, monkeypatch, nslots, wait_each):
    """12, 3, 12, 40, 1, 40, 5 draws, frame after frame, as one rank of three bands.  The tile kernel of a frame clears the
    culling counters of the slot for the next one, but only those of its own draws: the frame of 40 after the frame of 3 finds
    the rest as the frame of 12 before left them, unless the host clears them; a rank with an empty band runs no tile kernel
    at all.  A counter that does not start from zero puts an instance list past its end."""
    from mt_renderer_amd import api
    if nslots:
        monkeypatch.setenv("MTR_NSLOTS", nslots)
    dev = api.Device(0)  # a device of its own: the variable is read when a device is created
    if nslots:
        monkeypatch.delenv("MTR_NSLOTS")
    res = None
    try:
        res = mds.Resident(dev, crowd40.draws)
        for bands, rank in RANKS:
            own = sharding.owner_map(W, H, mds.WORLD, sharding.BANDS, 0, bands) == rank
            assert bool(own.any()) == (bands[rank + 1] > bands[rank])
            frames, got = [], []
            try:
                for n in SEQUENCE:
                    frames.append(res.frame(n, _shard(bands, rank)))
                    if wait_each:  # ... and the next frame recycles its colour / depth / counter set
                        got.append(mds.read(frames[-1]))
                        frames.pop().close()
                if not wait_each:
                    got = [mds.read(fr) for fr in frames]
            finally:
                for fr in frames:
                    fr.close()
            for k, (n, part) in enumerate(zip(SEQUENCE, got)):
                _owned_equal(part, unsharded(n), own, (bands, rank, k, n))
                fresh = _fresh(crowd40, n, bands, rank)
                _owned_equal(part, fresh, own, (bands, rank, k, n, "fresh device"))
                for key in COUNTS:
                    assert part[2][key] == fresh[2][key], (bands, rank, k, n, key)
                assert part[2]["ndraws"] == n
    finally:
        if res:
            res.close()
        dev.close()


# ---- more than four batch draws, stale hints ----
def _lattice_batches():
    """six batches of 2640 instances of the 17-chunk capsule (two mask groups): with a launch hint of fewer than ~120 instances
    the slots left to the second geometry launch are worth it ((2640 - slots) * 2 * 4 workgroups > 20 000, k_geom.hip); without
    a hint the full-rate launch takes them all"""
    md = scene.skinned_capsule_model([((0.0, 0.0, 0.0), 0.35, 1.6)], rows=24, cols=20, nbones=8)
    nx, ny = 44, 60
    pals8 = np.stack([scene.bone_palette(8, t=0.25 + 0.37 * k) for k in range(7)])
    base = np.zeros((nx * ny, 16), dtype=np.float32)
    for k in range(nx * ny):
        i, j = k % nx, k // nx
        x, y = -1.65 + 3.3 / nx * (i + 0.5), -0.93 + 1.86 / ny * (j + 0.5)
        base[k] = scene.to_f32_colmajor(scene.mat_translate(-5.0 + x, y, 1.0 - 2.3) @ scene.mat_rot_y(0.7 * k) @ scene.mat_scale(0.02, 0.02, 0.02))
    draws = []
    for b in range(6):
        mats = base.copy()
        mats[:, 12:15] += np.array([0.01 * b, 0.004 * b, -0.01 * b], dtype=np.float32)  # the translation column
        draws.append(dict(md=md, model_mats=mats, palettes=pals8[(np.arange(nx * ny) + b) % 7], kind="batch"))
    return draws


def test_more_than_four_batches_with_stale_launch_hints():
    """A frame reports the instance counts of its first four batch draws; a batch keeps its hint slot across frames.  After
    four frames under camera A (few instances of every batch in the band) the draw order is reversed: the batches that
    reported as draws 0-3 are now draws 4-5, do not report, and size their launches by A's low counts under camera B (most
    instances in the band).  k_geom_rest takes what the hint misses.  No hint's value is asserted: two draws of one batch in
    a frame race for one slot by design."""
    from mt_renderer_amd import api
    rank, bands = 1, mds.EVEN_BANDS
    own = sharding.owner_map(W, H, mds.WORLD, sharding.BANDS, 0, bands) == rank
    draws = _lattice_batches()
    # the camera positions of test_launch_sizes_from_reported_counts... in this scene: A slid down until only the top rows of the
    # lattice reach band 1, B far away with every instance in the middle rows
    cams = {"A": scene.to_f32_colmajor(scene.reference_view_proj(W, H, position=(-5.0, 1.21, 1.0))),
            "B": scene.to_f32_colmajor(scene.reference_view_proj(W, H, position=(-5.0, 0.0, 6.0)))}
    fwd, rev = list(range(6)), list(range(5, -1, -1))
    twice = [0, 1, 0, 2, 3, 4, 0, 5]  # the same batch three times in one frame

    def references(order, cam):
        with api.Device(0) as dev:
            res = mds.Resident(dev, draws)
            try:
                return res.render(order, vp=cams[cam]), res.render(order, _shard(bands, rank), vp=cams[cam])
            finally:
                res.close()

    steps = [(fwd, "A")] * 4 + [(rev, "B"), (rev, "A"), (rev, "B"), (twice, "A"), (twice, "B"), (fwd, "B")]
    refs = {}
    for order, cam in steps:
        if (tuple(order), cam) not in refs:
            refs[(tuple(order), cam)] = references(order, cam)
    kept = {cam: refs[(tuple(rev), cam)][1][2] for cam in cams}
    kept = {cam: st["chunks"] - st["chunks_culled"] for cam, st in kept.items()}
    assert kept["A"] > 0 and kept["B"] > 8 * kept["A"], kept  # the views really differ in what the rank keeps
    with api.Device(0) as dev:
        res = mds.Resident(dev, draws)
        try:
            for k, (order, cam) in enumerate(steps):
                part = res.render(order, _shard(bands, rank), vp=cams[cam])
                full, fresh = refs[(tuple(order), cam)]
                _owned_equal(part, full, own, (k, cam))
                for key in COUNTS:
                    assert part[2][key] == fresh[2][key], (k, cam, key)
        finally:
            res.close()


# ---- more batches than hint slots ----
def test_more_batches_than_the_device_has_hint_slots():
    """260 batches of two cubes in one frame: 256 get a hint slot, four stay without (260 is the smallest count past the 256
    slots that leaves a few without one) and size their launches by the defaults; half of the batches are then destroyed and
    new ones take over their slots with whatever those last held."""
    from mt_renderer_amd import api
    w, h, world, nb = 64, 48, 2, 260
    md = scene.cube_model(4)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(w, h))
    owner = sharding.owner_map(w, h, world, sharding.BANDS)

    def mats_of(b, gen):
        out = []
        for k in range(2):
            x = -1.5 + 3.0 * ((b * 37 + k * 101 + gen * 13) % 260) / 259.0
            y = -0.9 + 1.8 * ((b * 11 + k * 7 + gen * 5) % 13) / 12.0
            out.append(scene.to_f32_colmajor(scene.mat_translate(-5.0 + x, y, 1.0 - 2.3 - 0.002 * b) @ scene.mat_rot_y(0.1 * b + k) @ scene.mat_scale(0.06, 0.06, 0.06)))
        return np.stack(out)

    with api.Device(0) as dev:
        dev.set_tile_mode(api.TILE_AUTO)
        model = api.Model.new(dev, md)
        batches = [api.Batch(dev, model, mats_of(b, 0)) for b in range(nb)]

        def frame(shard):
            fr = api.Frame(dev, w, h)
            try:
                if shard is not None:
                    fr.set_shard(shard, world, sharding.BANDS)
                for b in batches:
                    fr.draw_batch(b, vp)
                fr.submit()
                return mds.read(fr)
            finally:
                fr.close()
        try:
            full = frame(None)
            assert full[2]["ndraws"] == nb and full[2]["tris_setup"] > nb
            for rank in range(world):  # a rank's three frames in a row: the hints of one rank are no use to the other
                for k in range(3):
                    part = frame(rank)
                    _owned_equal(part, full, owner == rank, (k, rank))
                    assert part[2]["tris_setup"] <= full[2]["tris_setup"]
            for b in range(0, nb, 2):  # slots change hands
                batches[b].close()
                batches[b] = api.Batch(dev, model, mats_of(b, 1))
            full = frame(None)
            for rank in (world - 1, 0):  # the rank of the last frames first: the slots still hold its counts
                _owned_equal(frame(rank), full, owner == rank, ("new batches", rank))
        finally:
            for b in batches:
                b.close()
            model.close()


# ---- overflow re-run of a culled many-draw frame ----
def test_the_overflow_rerun_of_a_culled_many_draw_frame(gpu_device, crowd40, unsharded, monkeypatch):
    """A bounded per-bin queue of 64 entries fills up under 400 quads stacked in one bin: the frame runs again through the
    exact queues, on culling counters that the overflowed run's tile kernel has already cleared and reported; the next frames
    of the slot, of 12 draws and of 3, find their counters clean."""
    from mt_renderer_amd import api
    from tests.pixel_scenes import pixel_model, pixel_to_ndc_matrix
    rank, bands = 1, mds.EVEN_BANDS
    own = sharding.owner_map(W, H, mds.WORLD, sharding.BANDS, 0, bands) == rank
    quads = []
    for q in range(400):  # inside bin (5, 5), pixel rows 80 .. 96: band 1
        x0, y0 = 81.0 + (q % 5), 81.0 + (q // 5) % 5
        v = [(x0, y0, 0.7), (x0, y0 + 8.0, 0.7), (x0 + 8.0, y0 + 8.0, 0.7), (x0 + 8.0, y0, 0.7)]
        quads.append(dict(verts=v, indices=[0, 1, 2, 0, 2, 3], debug_id=q % 20))
    stack = dict(md=pixel_model(quads), M=pixel_to_ndc_matrix(W, H), kind="stack")
    draws = crowd40.draws[:12] + [stack]
    ref = render_gpu(gpu_device, W, H, draws, tile_mode=api.TILE_AUTO)
    monkeypatch.setenv("MTR_NSLOTS", "1")
    dev = api.Device(0)
    monkeypatch.delenv("MTR_NSLOTS")
    res = None
    try:
        dev.set_binning(True, 64)
        res = mds.Resident(dev, draws)
        part = res.render(13, _shard(bands, rank))
        assert part[2]["binning"] == 2, "the frame fell back to the exact two-pass queues"
        _owned_equal(part, (ref[0], ref[1].view(np.uint32)), own, "overflowed frame")
        assert part[2]["chunks_culled"] > 0
        for n in (12, 3):
            _owned_equal(res.render(n, _shard(bands, rank)), unsharded(n), own, ("after the re-run", n))
    finally:
        if res:
            res.close()
        dev.close()


# ---- frustum culling of an unsharded many-draw frame ----
def test_frustum_culling_of_an_unsharded_many_draw_frame(gpu_device, crowd40):
    from mt_renderer_amd import api
    try:
        gpu_device.set_culling(api.GEOM_CULL_SHARDED)
        ref = render_gpu(gpu_device, W, H, crowd40.draws)
        gpu_device.set_culling(api.GEOM_CULL_ALL_FRAMES)
        got = render_gpu(gpu_device, W, H, crowd40.draws)  # every queue builder x both tile kernels inside
    finally:
        gpu_device.set_culling(api.GEOM_CULL_SHARDED)
    assert (got[0] == ref[0]).all() and (got[1].view(np.uint32) == ref[1].view(np.uint32)).all()
    for key in ("tris_setup", "bin_entries", "chunks"):
        assert got[2][key] == ref[2][key], key
    assert ref[2]["chunks_culled"] == 0 and got[2]["chunks_culled"] > 0
