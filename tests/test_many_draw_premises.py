"""CPU: the many-draw frames of tests/many_draw_scenes.py are what tests/test_gpu_many_draws.py takes them for.  Oracle only:
its vertex stage projects every instance of every batch, its frames say which draws set triangles up and that the order of
the translucent / opaque pair shows."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import many_draw_scenes as mds
from tests.helpers import render_oracle


@pytest.fixture(scope="module")
def crowd40():
    return mds.crowd(40)


def _pixel_boxes(d):
    """(x0, y0, x1, y1) in pixels of every instance of a batch draw, from the oracle's vertex stage (every w > 0)"""
    om = orc.OracleModel(d["md"])
    out = []
    for i in range(len(d["model_mats"])):
        pal = None if d.get("palettes") is None else d["palettes"][i]
        lo, hi = np.full(2, np.inf), np.full(2, -np.inf)
        for p in range(d["md"].nprims):
            clip, _ = om.vertex_stage(p, orc.mat4_mul(d["vp"], d["model_mats"][i]), pal)
            clip = clip.astype(np.float64)
            assert (clip[:, 3] > 0).all()
            xy = np.stack([(clip[:, 0] / clip[:, 3] * 0.5 + 0.5) * mds.W, (0.5 - clip[:, 1] / clip[:, 3] * 0.5) * mds.H], axis=1)
            lo, hi = np.minimum(lo, xy.min(axis=0)), np.maximum(hi, xy.max(axis=0))
        out.append((lo[0], lo[1], hi[0], hi[1]))
    return out


def test_a_prefix_of_the_crowd_is_the_smaller_crowd(crowd40):
    small = mds.crowd(12)
    assert small.kinds == crowd40.kinds[:12]
    for a, b in zip(small.draws, crowd40.draws):
        for key in ("M", "model_mats", "palettes", "palette", "overlay"):
            if a.get(key) is not None:
                assert (np.asarray(a[key]) == np.asarray(b[key])).all(), key
    for n in range(7, 41):
        assert set(crowd40.kinds[:n]) == set(mds.KINDS)
    assert crowd40.kinds[:5] == ["single", "batch", "unboundable", "owned", "overlay"]


def test_every_rank_sees_instances_culled_straddling_and_inside(crowd40):
    boxes = [b for d in crowd40.of_kind("batch") for b in _pixel_boxes(d)]
    assert len(boxes) == 3 + 5 + 7 + 9 + 3 + 5
    on_target = [b for b in boxes if b[2] > 0 and b[0] < mds.W and b[3] > 0 and b[1] < mds.H]
    assert len(on_target) < len(boxes), "some instances are wholly off the target"
    for rank in range(mds.WORLD):
        y0, y1 = 16 * mds.EVEN_BANDS[rank], min(mds.H, 16 * mds.EVEN_BANDS[rank + 1])
        inside = [b for b in on_target if b[1] > y0 + 2 and b[3] < y1 - 2 and b[0] > 2 and b[2] < mds.W - 2]
        outside = [b for b in boxes if b[3] < y0 - 2 or b[1] > y1 + 2 or b[2] < -2 or b[0] > mds.W + 2]
        crossing = [b for b in on_target if (b[1] < y0 - 2 and b[3] > y0 + 2 and y0 > 0) or (b[1] < y1 - 2 and b[3] > y1 + 2 and y1 < mds.H)]
        assert inside and outside and crossing, (rank, len(inside), len(outside), len(crossing))


def test_the_masks_of_the_batches_end_on_an_odd_count_and_the_big_model_has_two_ragged_groups(crowd40):
    for d in crowd40.of_kind("batch"):
        nx = (mds.chunks_of(d["md"]) + 15) // 16
        assert mds.chunks_of(d["md"]) <= 16 and (nx * len(d["model_mats"])) % 2 == 1
    assert any("tex_override" in d for d in crowd40.of_kind("batch")) and any("tex_override" not in d for d in crowd40.of_kind("batch"))
    for d in crowd40.of_kind("batch"):
        if "tex_override" in d:  # one texture with alpha < 255, one opaque, both in use
            alphas = [orc.decode_texture(t.fmt, t.width, t.height, t.data)[..., 3] for t in d["md"].textures]
            assert alphas[0].min() < 255 and alphas[1].min() == 255 and set(d["tex_override"]) == {0, 1}
    singles = {mds.chunks_of(d["md"]) for d in crowd40.of_kind("single")}
    assert len(singles) == 2 and min(singles) <= 16 and 17 <= max(singles) <= 31 and max(singles) % 16 != 0
    assert 17 <= mds.chunks_of(crowd40.of_kind("unboundable")[0]["md"]) <= 31
    # the unboundable model: weights that do not sum to 255
    vb = crowd40.of_kind("unboundable")[0]["md"].vertex_buf.reshape(-1, 24)
    assert (vb[:, 20:24].astype(np.int64).sum(axis=1) != 255).any()
    assert all(d.get("owned") and d.get("palettes") is None for d in crowd40.of_kind("owned"))


def test_every_kind_sets_triangles_up_in_every_band_and_the_pair_shows_its_order(crowd40):
    full = render_oracle(mds.W, mds.H, crowd40.draws)
    for rank in range(mds.WORLD):
        y0, y1 = 16 * mds.EVEN_BANDS[rank], min(mds.H, 16 * mds.EVEN_BANDS[rank + 1])
        for kind in mds.KINDS:
            hit = False
            for d in crowd40.of_kind(kind):
                c, _, st = render_oracle(mds.W, mds.H, [d])
                hit = hit or (st["tris_setup"] > 0 and bool((c[y0:y1] != 255).any()))  # set up, and visible in this rank's band
            assert hit, (rank, kind)
    i = crowd40.kinds.index("translucent")
    assert crowd40.kinds[i + 1] == "opaque"
    swapped = crowd40.draws[:i] + [crowd40.draws[i + 1], crowd40.draws[i]] + crowd40.draws[i + 2:]
    other = render_oracle(mds.W, mds.H, swapped)
    assert other[2]["tris_setup"] == full[2]["tris_setup"]
    assert (other[0] != full[0]).any(), "submission order across draws must be observable"
    # ... and the frame has both translucent and opaque materials in its first five draws too (a mixed frame)
    assert "tex_override" in crowd40.draws[1]
