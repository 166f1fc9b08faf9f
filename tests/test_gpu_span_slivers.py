"""-m gpu: fans of long, thin slivers at many slopes across bin borders -- the triangles whose bboxes are mostly empty, where
k_tile_vis.hip walks only each bbox row's covered run (span_row.h) instead of every pixel of the box.  The fans' centres sit
on pixel centres, on bin corners and off every grid; spokes reach up to 60 px (the i32 edge class) or beyond 64 px (the
64-bit class), and overlapping fans at different depths make the depth test pick winners along the slivers.  Everything is
compared with the oracle bit for bit through both tile kernels (tests/helpers.render_gpu)."""
import math

import numpy as np
import pytest

from tests.helpers import assert_same, render_gpu, render_oracle
from tests.pixel_scenes import pixel_model, pixel_to_ndc_matrix

pytestmark = pytest.mark.gpu

W = H = 128  # 8 x 8 bins


def _fan(cx, cy, radius, n, z0, z1, phase=0.0, gap=0.0):
    """n slivers around (cx, cy): spoke k runs from the centre to angle 2 pi (k + phase) / n; `gap` > 0 leaves a wedge of that
    fraction of the step between neighbouring slivers uncovered"""
    verts = [(cx, cy, z0)]
    idx = []
    for k in range(n):
        a0 = 2.0 * math.pi * (k + phase) / n
        a1 = 2.0 * math.pi * (k + phase + 1.0 - gap) / n
        z = z0 + (z1 - z0) * k / n
        verts.append((cx + radius * math.cos(a0), cy + radius * math.sin(a0), z))
        verts.append((cx + radius * math.cos(a1), cy + radius * math.sin(a1), z1))
        idx += [0, len(verts) - 2, len(verts) - 1] if k % 2 == 0 else [0, len(verts) - 1, len(verts) - 2]  # both windings
    return dict(verts=np.asarray(verts, dtype=np.float32), indices=idx)


def _render(dev, prims):
    md = pixel_model(prims)
    draws = [dict(md=md, M=pixel_to_ndc_matrix(W, H))]
    g = render_gpu(dev, W, H, draws)
    assert_same(g, render_oracle(W, H, draws), "slivers")
    return g


@pytest.mark.parametrize("n", [90, 257, 720])
@pytest.mark.parametrize("centre", [(64.5, 64.5), (64.0, 64.0), (47.37109375, 80.62890625), (16.0, 111.5)])
def test_sliver_fans(gpu_device, n, centre):
    """one fan per case: every slope from the nearly horizontal to the nearly vertical, both windings of the
    top-left rule's cases, runs from one to sixteen columns long inside each bin row"""
    g = _render(gpu_device, [_fan(centre[0], centre[1], 60.0, n, 0.25, 0.75, phase=0.125)])
    assert int((g[1] < 1.0).sum()) > 0


@pytest.mark.parametrize("radius", [20.0, 63.0, 90.0])
def test_overlapping_sliver_fans(gpu_device, radius):
    """three fans with gaps between their slivers, offset and rotated against each other, at crossing depths; radius 90:
    the longest slivers need 64-bit edge functions"""
    prims = [
        _fan(64.5, 64.5, radius, 360, 0.2, 0.8, phase=0.0, gap=0.5),
        _fan(60.25, 67.75, radius, 301, 0.8, 0.2, phase=0.3, gap=0.3),
        _fan(70.0, 58.0, radius, 173, 0.5, 0.5, phase=0.7, gap=0.0),
    ]
    _render(gpu_device, prims)
