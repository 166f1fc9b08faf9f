"""-m gpu: the lane-parallel path of single-pass unordered binning (csrc/geom_bins.h: emit_bins_unordered), where the lane that
reserves a bin's queue space also works out the entry index the stores add their rank to, and the strip assembly of
k_geom.hip in front of it, on the lanes where a chunk's neighbours lane - 1 and lane - 2 are special.  One 256 x 256 frame of
strips and lists against the oracle, bit for bit, and its per-bin entry counts against a count of bbox bins made here:
  * records over 1 bin, 2 bins (side by side, one above the other), 3 bins (a row, a column) and 4 bins (1 x 4, 4 x 1, 2 x 2);
  * chunks whose first triangle lies in bin column / row 0, 1 and 2 (the window's clamp at the frame's corner), a chunk whose
    later triangles lie more than three bins left of and above the first (the true min / max window), a chunk whose bins
    span more than eight columns, a chunk with one record over 6 bins and a record over 36 bins (the group loop and the
    cooperative path: they must still take everything the lane-parallel path leaves);
  * strips of three chunks: a restart at lane 1 of a chunk and at lane 2 of another, chunks whose lanes 0 and 1 hold the two
    halo positions and whose lane 2 completes a triangle from them, and a first chunk whose lanes 0 and 1 lie before the
    primitive's first index;
  * the frame as rank 1 of 3 under bands and under interleaved ownership;
  * the same frame with the per-bin bound forced to 64 (a bin holds 100): it ends as tests/test_gpu_overflow.py expects.
The CPU side (strip assembly, culling, bbox bins) is held to the oracle's tris_setup without a device."""
import numpy as np
import pytest

from mt_renderer_amd import scene, sharding
from tests.helpers import assert_same, render_gpu, render_oracle
from tests.pixel_scenes import pixel_model, pixel_to_ndc_matrix

W = H = 256
BIN = 16
NBX = W // BIN
RESTART = 0xFFFF


def strip_ribbon(x0, y_top, y_bot, npos, restarts, step=2.5):
    """npos index positions of a strip along +x: even vertices of a run on the top rail, odd ones on the bottom rail (the
    winding the reference keeps); `restarts`: positions that hold the restart index; a run starts on the top rail again"""
    verts, idx, k, x = [], [], 0, x0
    for p in range(npos):
        if p in restarts:
            idx.append(RESTART)
            k = 0
            continue
        verts.append((x, y_top if k % 2 == 0 else y_bot))
        idx.append(len(verts) - 1)
        if k % 2 == 1:
            x += step
        k += 1
    return dict(verts=verts, indices=idx, topology=scene.TOPO_STRIP)


def tri_list(tris):
    verts = [v for t in tris for v in t]
    return dict(verts=verts, indices=list(range(len(verts))), topology=scene.TOPO_LIST)


def right(x, y, dx, dy):
    """a right triangle with its corner at (x, y), in the winding the reference keeps"""
    return ((x, y), (x, y + dy), (x + dx, y))


def build_prims():
    prims = []
    # strips, 140 positions = chunks at 0, 62, 124: inside bin row 1 from bin column 0 on (records over 1 bin, and 2 side by side
    # at every bin edge), restart at position 61 = lane 1 of the second chunk; lanes 0 / 1 of the third chunk are the halo
    prims.append(strip_ribbon(3.0, 20.0, 24.0, 140, {61}))
    # across the edge between bin rows 2 and 3 (2 bins one above the other, 2 x 2 at the corners), restart at position 62 = lane 2
    prims.append(strip_ribbon(5.0, 46.0, 50.0, 140, {62}))
    # lists: every record shape the lane-parallel path takes, in one chunk whose first triangle lies in bin (6, 6)
    prims.append(tri_list([right(100.5, 100.5, 5, 5), right(109, 101, 6, 5), right(101, 109, 5, 6), right(98, 120, 32, 3), right(120, 98, 3, 32),
                           right(98, 125, 48, 3), right(125, 98, 3, 48), right(108, 108, 8, 8)]))
    # the window's clamp: first triangles in bin column / row 2, 0 and 1
    prims.append(tri_list([right(35, 5, 5, 5), right(5, 37, 5, 5), right(20, 20, 5, 5)]))
    prims.append(tri_list([right(5, 70, 5, 5), right(40, 75, 5, 5)]))
    # the min / max window: later triangles three and more bins left of / above the first
    prims.append(tri_list([right(165, 165, 5, 5), right(85, 150, 5, 5), right(180, 195, 5, 5)]))
    # a record over 3 x 2 bins among small ones: the round goes to the group loop
    prims.append(tri_list([right(200, 36, 5, 5), right(200, 40, 40, 20), right(210, 66, 5, 5)]))
    # bins 13 columns apart in one chunk: no 8 x 8 window
    prims.append(tri_list([right(5, 230, 5, 5), right(200, 228, 5, 5)]))
    # a record over 6 x 6 bins: cooperative, lane = bin
    prims.append(tri_list([right(130, 130, 85.5, 85.5)]))
    # 100 triangles in bin (14, 14): five chunks, each of which reserves 20 places of that bin at once
    prims.append(tri_list([right(226 + (k % 10), 226 + (k // 10), 3, 3) for k in range(100)]))
    z = 0.2
    for i, p in enumerate(prims):
        vs = []
        for (x, y) in p["verts"]:
            z += 1e-4
            vs.append((x, y, z))
        p["verts"] = vs
        p["debug_id"] = i
    return prims


def assemble(prims):
    """the triangles the geometry stage records, as pixel triples: strip assembly with restarts and parity, back faces and
    degenerate triangles culled, a bbox without a pixel centre dropped"""
    out = []
    for p in prims:
        v, idx = p["verts"], p["indices"]
        if p["topology"] == scene.TOPO_LIST:
            cand = [(v[idx[i]], v[idx[i + 1]], v[idx[i + 2]]) for i in range(0, len(idx) - 2, 3)]
        else:
            cand, q = [], 0
            for i, ix in enumerate(idx):
                q = 0 if ix == RESTART else q + 1
                if q >= 3:
                    a, b, c = v[idx[i - 2]], v[idx[i - 1]], v[idx[i]]
                    cand.append((a, c, b) if (q - 3) & 1 else (a, b, c))
        for a, b, c in cand:
            if (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0]) < 0 and bins_of((a, b, c)) is not None:
                out.append((a, b, c))
    return out


def bins_of(tri):
    """(bx0, by0, bx1, by1) of the pixel-centre bbox, None if it holds no centre of the viewport"""
    xs, ys = [int(round(p[0] * 256)) for p in tri], [int(round(p[1] * 256)) for p in tri]
    x0, y0 = max((min(xs) + 127) >> 8, 0), max((min(ys) + 127) >> 8, 0)
    x1, y1 = min((max(xs) - 128) >> 8, W - 1), min((max(ys) - 128) >> 8, H - 1)
    if x0 > x1 or y0 > y1:
        return None
    assert (max(xs) - min(xs)) >= 512 or (max(ys) - min(ys)) >= 512  # never a candidate for the coverage test of tiny triangles
    return x0 // BIN, y0 // BIN, x1 // BIN, y1 // BIN


def expected_bin_counts(tris):
    cnt = np.zeros((H // BIN, NBX), dtype=np.uint32)
    for t in tris:
        bx0, by0, bx1, by1 = bins_of(t)
        cnt[by0:by1 + 1, bx0:bx1 + 1] += 1
    return cnt


@pytest.fixture(scope="module")
def bin_scene():
    prims = build_prims()
    md = pixel_model(prims)
    draws = [dict(md=md, M=pixel_to_ndc_matrix(W, H))]
    ref = render_oracle(W, H, draws)
    tris = assemble(prims)
    return prims, draws, ref, tris


def test_scene_premises(bin_scene):
    """no device: the CPU assembly agrees with the oracle, and the scene holds the shapes and chunk edges it claims"""
    prims, draws, ref, tris = bin_scene
    assert len(tris) == ref[2]["tris_setup"]
    shapes = {(b[2] - b[0] + 1, b[3] - b[1] + 1) for b in map(bins_of, tris)}
    assert {(1, 1), (2, 1), (1, 2), (3, 1), (1, 3), (4, 1), (1, 4), (2, 2), (3, 2), (6, 6)} <= shapes, shapes
    assert prims[0]["indices"][61] == RESTART and prims[1]["indices"][62] == RESTART  # lane = position - chunk start + 2
    assert all(len(p["indices"]) == 140 and RESTART not in p["indices"][120:128] for p in prims[:2])  # the third chunk's halo completes a triangle
    first = [bins_of(right_) for right_ in (tuple(p["verts"][i][:2] for i in p["indices"][:3]) for p in prims[:6])]
    assert {0, 1, 2} <= {b[0] for b in first} | {b[1] for b in first}
    mm = [bins_of(t) for t in assemble([prims[5]])]
    assert mm[0][0] - min(b[0] for b in mm) > 3 and max(b[2] for b in mm) - min(b[0] for b in mm) < 8  # misses the guessed window, fits the true one
    far = [bins_of(t) for t in assemble([prims[7]])]
    assert max(b[2] for b in far) - min(b[0] for b in far) >= 8
    assert expected_bin_counts(tris)[14, 14] >= 100


def _frame(dev, draws, shard=None):
    from mt_renderer_amd import api
    dev.set_tile_mode(api.TILE_AUTO)
    model = api.Model.new(dev, draws[0]["md"])
    fr = api.Frame(dev, W, H)
    try:
        if shard:
            fr.set_shard(*shard)
        model.set_palette(None)
        model.render(fr, draws[0]["M"])
        fr.end()
        return fr.color(), fr.depth(), fr.stats(), fr.bin_counts()[0]
    finally:
        fr.close()
        model.close()


@pytest.mark.gpu
def test_frame_and_bin_counts(bin_scene, gpu_device):
    from mt_renderer_amd import api
    prims, draws, ref, tris = bin_scene
    g = render_gpu(gpu_device, W, H, draws)  # both tile kernels behind both queue builders agree; auto is returned
    assert g[2]["tile_kernel"] == api.TILE_VISIBILITY and g[2]["binning"] == 1, g[2]
    assert_same(g, ref, "unordered single-pass queues")
    want = expected_bin_counts(tris)
    for rep in range(2):  # the second frame finds the fill words its predecessor's tile kernel parked
        c, d, st, ent = _frame(gpu_device, draws)
        assert st["tile_kernel"] == api.TILE_VISIBILITY and st["binning"] == 1, st
        assert_same((c, d, st), ref, "frame %d" % rep)
        got = ent.reshape(H // BIN, NBX)
        assert (got == want).all(), (rep, np.argwhere(got != want)[:8], got[got != want][:8], want[got != want][:8])
        assert int(want.sum()) == st["bin_entries"]


@pytest.mark.gpu
@pytest.mark.parametrize("own", ["bands", "interleaved"])
def test_rank_1_of_3(bin_scene, gpu_device, own):
    prims, draws, ref, tris = bin_scene
    bands = [0, 3, 9, H // BIN]
    shard = (1, 3, sharding.BANDS, 0, bands) if own == "bands" else (1, 3, sharding.INTERLEAVED, 0, None)
    mine = sharding.owner_map(W, H, 3, shard[2], 0, shard[4]) == 1
    assert mine.any() and not mine.all()
    c, d, st, ent = _frame(gpu_device, draws, shard)
    assert (c[mine] == ref[0][mine]).all() and (d.view(np.uint32)[mine] == ref[1].view(np.uint32)[mine]).all(), own
    bin_mine = mine[::BIN, ::BIN]
    assert (ent.reshape(H // BIN, NBX)[bin_mine] == expected_bin_counts(tris)[bin_mine]).all(), own


@pytest.mark.gpu
def test_forced_overflow_ends_as_the_overflow_test_expects(bin_scene):
    """the bound at 64 entries per bin: bin (14, 14) overflows inside the lane-parallel path (the fourth chunk's reservation of
    20 places).  Submitted, packed, never waited for: every bin at the clear colour, the error latched and reported once
    (tests/test_gpu_overflow.py: test_unwaited_overflow_is_latched_never_a_wrong_frame)"""
    import torch
    from mt_renderer_amd import api
    prims, draws, ref, tris = bin_scene
    with api.Device(0) as dev:
        dev.set_tile_mode(api.TILE_AUTO)
        dev.set_binning(True, 64)
        model = api.Model.new(dev, draws[0]["md"])
        fr = api.Frame(dev, W, H)
        model.render(fr, draws[0]["M"])
        fr.submit()
        nbytes = int(api.lib.mtr_shard_bytes(W, H, 1))
        packed = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        fr.pack_color_shard(packed.data_ptr(), nbytes)
        torch.cuda.synchronize()
        assert (packed.cpu().numpy() == 255).all(), "an overflowed frame must be left at the clear colour"
        fr.close()
        with pytest.raises(api.MtrError, match="overflowed its bin queues"):
            dev.synchronize()
        dev.synchronize()  # reported once
        # the bound was doubled: the scene fits now and is the oracle's frame
        fr = api.Frame(dev, W, H)
        model.render(fr, draws[0]["M"])
        fr.end()
        st = fr.stats()
        assert st["binning"] == 1, st
        assert_same((fr.color(), fr.depth(), st), ref, "after the bound was raised")
        fr.close()
        dev.synchronize()
        model.close()
