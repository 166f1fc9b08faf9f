"""-m gpu: frames at the limits of the frame size (1 x 1 .. 16384 on a side) through the HIP path.  Everything that depends
on the frame's shape and nothing else runs here at the shapes of tests/frame_shape_scenes.py: the launch size in whole XCD
runs and the two multiply-high divisions of the tile kernels' entry path, k_scan's rounds of 1024 bins, the pixel-centre box
clamps at W - 1 and H - 1, quad partners outside a frame one pixel thick, clear and resolve at ragged bins, ownership maps
in which a rank owns nothing, the colour-shard copies on their uint4 and scalar paths, and the host's queue sizing.

Tiny frames are pinned by the crop property (a lattice scene's w x h frame is the crop of a 64 x 64 one, bit for bit), long
ones by the float64 reference (tests/ideal_renderer.py); every frame equals the oracle's bit for bit.  The premises --
that the scenes are fit, that the oracle agrees with the reference on them, that mutants fail, what each shape is for --
are tests/test_frame_shape_premises.py's, on the CPU; its docstring carries the measured figures."""
import numpy as np
import pytest

from mt_renderer_amd import sharding
from tests import frame_shape_scenes as fs
from tests import ideal_compare as cmp
from tests.helpers import assert_same, render_gpu, render_oracle
from tests.test_gpu_sharding import MAPS, _bands

pytestmark = pytest.mark.gpu

EVERY_SHAPE = fs.TINY + fs.LONG + fs.GRID
CLEAR, CLEAR_DEPTH = (0.1, 0.2, 0.3, 0.4), 0.5


def shape_id(case):
    return f"{case[0]}x{case[1]}" + "".join(f"-{c}" for c in case[2:])


def _same_bits(a, b, what):
    nc = int((a[0] != b[0]).any(axis=-1).sum())
    nd = int((a[1].view(np.uint32) != b[1].view(np.uint32)).sum())
    assert nc == 0 and nd == 0, f"{what}: {nc} colour pixels and {nd} depth pixels differ"


# -------------------------------------------------------------------------------------------------------------------
# 1. bit for bit against the oracle
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [s + (v,) for s in EVERY_SHAPE for v in fs.VARIANTS], ids=shape_id)
def test_ribbon_equals_the_oracle(gpu_device, case):
    """both tile kernels behind both queue builders (render_gpu requires them equal); opaque variants take the visibility
    kernel, the translucent strip of ``alpha`` keeps the frame off it"""
    from mt_renderer_amd import api
    w, h, variant = case
    draws = fs.ribbon(w, h, variant)
    gpu = render_gpu(gpu_device, w, h, draws)
    assert_same(gpu, render_oracle(w, h, draws), shape_id(case))
    if variant == "alpha":
        assert gpu[2]["tile_kernel"] != api.TILE_VISIBILITY, gpu[2]
    else:
        assert gpu[2]["tile_kernel"] == api.TILE_VISIBILITY, gpu[2]
    assert gpu[2]["nbins"] == ((w + 15) // 16) * ((h + 15) // 16)


@pytest.mark.parametrize("shape", [(16381, 3), (1, 16384), (15, 17)], ids=shape_id)
def test_block_compressed_ribbon_equals_the_oracle_under_both_residencies(gpu_device, shape):
    """``tex`` with BC7 chains, decoded at upload and block-resident (csrc/bc_sample.h: decoded per fetch)"""
    from mt_renderer_amd import api
    w, h = shape
    draws = fs.ribbon(w, h, "bc7")
    ref = render_oracle(w, h, draws)
    try:
        gpu_device.set_texture_residency(api.TEXRES_BLOCKS)
        blocks = render_gpu(gpu_device, w, h, draws)
    finally:
        gpu_device.set_texture_residency(api.TEXRES_DECODED)
    decoded = render_gpu(gpu_device, w, h, draws)
    assert_same(blocks, ref, shape_id(shape) + " (blocks resident)")
    assert_same(decoded, ref, shape_id(shape) + " (decoded at upload)")


# -------------------------------------------------------------------------------------------------------------------
# 2. against the float64 reference directly
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [s + (v,) for s in fs.LONG for v in fs.VARIANTS], ids=shape_id)
def test_gpu_ribbon_against_exact_arithmetic(gpu_device, case):
    w, h, variant = case
    ideal = fs.ribbon_ideal(w, h, variant)
    cmp.assert_scene_caps(ideal, shape_id(case))
    rep = cmp.compare(render_gpu(gpu_device, w, h, fs.ribbon(w, h, variant)), ideal)
    print(f"{shape_id(case)}: {rep.line()}")
    if variant != "ids":
        print(f"{shape_id(case)}: {rep.fragment_line()}")
    assert rep.ok, (case, rep.failures)
    assert rep.compared > 0.02 * w * h


@pytest.mark.parametrize("shape,far", fs.LATTICE_FRAMES, ids=lambda a: shape_id(a) if isinstance(a, tuple) else str(a))
def test_gpu_lattice_against_exact_arithmetic(gpu_device, shape, far):
    w, h = shape
    ideal = fs.lattice_ideal(w, h, far)
    cmp.assert_scene_caps(ideal, f"lattice {shape_id(shape)}")
    rep = cmp.compare(render_gpu(gpu_device, w, h, fs.lattice(w, h, far)), ideal)
    print(f"lattice {shape_id(shape)}: {rep.line()}")
    assert rep.ok, (shape, rep.failures)
    assert rep.compared > 0.02 * w * h


# -------------------------------------------------------------------------------------------------------------------
# 3. the crop property
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small,large,far", fs.CROPS, ids=[f"{shape_id(s)}-of-{shape_id(l)}" for s, l, _ in fs.CROPS])
def test_small_frame_is_the_crop_of_a_larger_one(gpu_device, small, large, far):
    """every vertex on the 1/256 px lattice: the frame's size changes which pixels exist and nothing else"""
    (w, h), (W, H) = small, large
    got = render_gpu(gpu_device, w, h, fs.lattice(w, h, far))
    big = render_gpu(gpu_device, W, H, fs.lattice(W, H, far))
    _same_bits(got, (big[0][:h, :w], np.ascontiguousarray(big[1][:h, :w])), f"{shape_id(small)} of {shape_id(large)}")
    assert got[2]["tris_in"] == big[2]["tris_in"] == fs.LATTICE_TRIS * (fs.LATTICE_COPIES if far else 1)
    assert (got[1] < 1.0).any(), "the crop holds no geometry"


# -------------------------------------------------------------------------------------------------------------------
# 4. empty frames
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(set(EVERY_SHAPE + fs.SHARD)), ids=shape_id)
def test_frame_without_a_draw_is_the_clear_colour_and_depth(gpu_device, shape):
    from mt_renderer_amd import api
    w, h = shape
    want = np.rint(np.array(CLEAR) * 255.0).astype(np.uint8)      # 25.5 and 76.5 round to even: 26, 51, 76, 102
    ref = render_oracle(1, 1, [], CLEAR, CLEAR_DEPTH)
    assert (ref[0][0, 0] == want).all() and ref[1][0, 0] == np.float32(CLEAR_DEPTH)
    for mode in (api.TILE_ORDERED, api.TILE_AUTO):
        c, d, st = render_gpu(gpu_device, w, h, [], CLEAR, CLEAR_DEPTH, tile_mode=mode)
        assert c.shape == (h, w, 4) and d.shape == (h, w)
        assert (c == want).all(), (shape, mode, int((c != want).any(axis=-1).sum()))
        assert (d.view(np.uint32) == np.float32(CLEAR_DEPTH).view(np.uint32)).all(), (shape, mode)
        assert st["tris_in"] == 0 and st["bin_entries"] == 0


# -------------------------------------------------------------------------------------------------------------------
# 5. the limits themselves
# -------------------------------------------------------------------------------------------------------------------
def test_frame_sizes_outside_the_limits_are_refused(gpu_device):
    from mt_renderer_amd import api
    for w, h in ((0, 5), (5, 0), (16385, 1), (1, 16385)):
        with pytest.raises(api.MtrError) as e:
            api.Frame(gpu_device, w, h)
        assert e.value.code == api.MTR_E_INVALID, (w, h, e.value)
    for w, h in ((16384, 1), (1, 16384)):
        fr = api.Frame(gpu_device, w, h)
        fr.close()
    w, h = 64, 64      # the device is as good as before
    draws = fs.lattice(w, h)
    assert_same(render_gpu(gpu_device, w, h, draws), render_oracle(w, h, draws), "after the refused frames")


# -------------------------------------------------------------------------------------------------------------------
# 6. sharded
# -------------------------------------------------------------------------------------------------------------------
SHARD_CASES = [s + ("ids",) for s in fs.SHARD] + [(20, 7, "alpha")]
OFFSET_SHAPES = [(20, 7), (16384, 16)]     # W % 4 == 0: the uint4 copies would take them; a 4-byte offset forces the scalar ones


@pytest.mark.parametrize("name,own_map,param,bands_kind", MAPS, ids=[m[0] for m in MAPS])
@pytest.mark.parametrize("world", [2, 3, 8])
@pytest.mark.parametrize("case", SHARD_CASES, ids=shape_id)
def test_every_ownership_map_rebuilds_the_unsharded_frame_at_the_limits(gpu_device, case, world, name, own_map, param, bands_kind):
    """the pattern of tests/test_gpu_sharding.py at frames with fewer bins than ranks, one bin thick, 1024 bins wide, and
    at widths that take the uint4 copies with whole bins (16384), with a ragged right edge (20) and the scalar ones (17,
    16381)"""
    import torch
    from mt_renderer_amd import api
    w, h, variant = case
    draws = fs.ribbon(w, h, variant)
    full = render_gpu(gpu_device, w, h, draws, tile_mode=api.TILE_AUTO)
    bands = _bands(bands_kind, h, world)
    args = (w, h, world, own_map, param, bands)
    owner = sharding.owner_map(*args)
    lists = sharding.own_lists(*args)
    nbytes = api.shard_bytes_map(*args)
    assert nbytes == sharding.shard_bytes(*args)
    shards = []
    for rank in range(world):
        own = owner == rank
        assert bool(own.any()) == bool(lists[rank])      # 1 x 1 and 17 x 1: most ranks own nothing
        setups = {}
        for cull in (True, False):
            gpu_device.set_culling(cull)
            try:
                part = render_gpu(gpu_device, w, h, draws, shard=(rank, world, own_map, param, bands))  # every kernel variant
            finally:
                gpu_device.set_culling(True)
            assert (part[0][own] == full[0][own]).all(), (case, name, world, rank, cull)
            assert (part[1].view(np.uint32)[own] == full[1].view(np.uint32)[own]).all(), (case, name, world, rank, cull)
            assert part[2]["shard_bins"] == len(lists[rank])
            setups[cull] = (part[2]["tris_setup"], part[2]["bin_entries"])
        assert setups[True] == setups[False], "culling must not drop a triangle that reaches one of the rank's bins"
        # pack this rank's bins (a fresh frame: render_gpu closed its own)
        fr = api.Frame(gpu_device, w, h)
        m = api.Model.new(gpu_device, draws[0]["md"])
        try:
            fr.set_shard(rank, world, own_map, param, bands)
            m.render(fr, draws[0]["M"])
            fr.end()
            assert fr.shard_bytes() == nbytes
            assert fr.stats()["shard_bins"] == len(lists[rank])
            buf = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            fr.pack_color_shard(buf.data_ptr(), nbytes)
            torch.cuda.synchronize()
            mine = np.where(own[..., None], full[0], 0).astype(np.uint8)
            want = sharding.pack_shard(mine, rank, world, own_map, param, bands)
            assert (buf.cpu().numpy().reshape(-1, 16, 16, 4) == want).all(), (case, name, world, rank)
            if not lists[rank]:
                assert not want.any()
            if (w, h) in OFFSET_SHAPES:
                off = torch.full((nbytes + 4,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                fr.pack_color_shard(off[4:].data_ptr(), nbytes)
                torch.cuda.synchronize()
                assert torch.equal(off[4:], buf) and (off[:4] == 0xA5).all(), (case, name, world, rank, "scalar pack")
            shards.append(buf)
            if rank == world - 1:
                gathered = torch.cat(shards)
                out = torch.zeros(w * h * 4, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()  # torch's stream made them; the unpack runs on the device's own (non-blocking) stream
                fr.unpack_color_shards(gathered.data_ptr(), out.data_ptr())
                torch.cuda.synchronize()
                assert (out.cpu().numpy().reshape(h, w, 4) == full[0]).all(), (case, name, world)
                if (w, h) in OFFSET_SHAPES:
                    g4 = torch.cat([torch.zeros(4, dtype=torch.uint8, device="cuda"), gathered])
                    o4 = torch.full((w * h * 4 + 8,), 0xA5, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    fr.unpack_color_shards(g4[4:].data_ptr(), o4[4:].data_ptr())
                    torch.cuda.synchronize()
                    assert torch.equal(o4[4:-4], out) and (o4[:4] == 0xA5).all() and (o4[-4:] == 0xA5).all(), (case, name, world, "scalar unpack")
        finally:
            fr.close()
            m.close()
