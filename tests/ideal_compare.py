"""The rule by which a rendered frame (oracle or HIP) is compared with tests/ideal_renderer.py (SPEC.md "Accuracy against
exact arithmetic").  Every tolerance is derived from the rules, none from what the renderers give:

* a pixel is *ambiguous* (left out) when an edge of a triangle that can reach the depth range passes within
  ``delta = 1/128 px + rounding of the clip coordinates carried to the pixel`` of its centre, or when a fragment's depth is
  within ``2 tol`` of 0 or 1.  SPEC 5 snaps a vertex by at most sqrt(2)/512 = 0.0028 px; 1/128 leaves 2.8x for the
  binary32 steps of the projection.  At most 2 % of a scene's pixels may be ambiguous;
* elsewhere coverage agrees exactly: ``depth < clear``  <=>  the ideal has a fragment;
* depth: ``|depth - z_ideal| <= tol = |grad z| sqrt(2)/512 + 2^-21 + sum |lambda_i| (e_z,i + |z| e_w,i)`` where the
  winner leads its nearest competitor by more than ``2 tol``; a near tie (at most 1 % of the pixels) is compared on depth
  against either competitor;
* identity: debug-id pixels carry exactly ``PALETTE[id mod 20]``, alpha 255, of the ideal's winner;
* uv (256 x 256 ramp texture R = x, G = y): ``|R - clamp(256 u - 0.5, 0, 255)| <= 0.5 + 0.5 + 256 (|grad u| sqrt(2)/512 +
  rounding terms) + 2^-10``: half a texel between the nearest and the linear filter, half a step for the store;
* ``tris_in`` is the ideal's count of assembled triangles.
"""
from __future__ import annotations

import numpy as np

from tests.ideal_renderer import PALETTE, SNAP

AMBIGUOUS_CAP = 0.02
NEAR_TIE_CAP = 0.01


def ramp_texture():
    from mt_renderer_amd import scene
    y, x = np.mgrid[0:256, 0:256]
    img = np.zeros((256, 256, 4), dtype=np.uint8)
    img[..., 0], img[..., 1], img[..., 3] = x, y, 255
    return scene.TextureData(256, 256, scene.TEX_RGBA8, img.tobytes())


def scene_shares(ideal):
    """(ambiguous share, near-tie share) of a scene -- from the ideal alone"""
    n = ideal.w * ideal.h
    tie = ideal.covered & ~ideal.ambiguous & (ideal.gap <= 2.0 * ideal.tol)
    return float(ideal.ambiguous.sum()) / n, float(tie.sum()) / n


def assert_scene_caps(ideal, what=""):
    amb, tie = scene_shares(ideal)
    assert amb <= AMBIGUOUS_CAP, f"{what}: {100 * amb:.2f} % of the pixels are ambiguous (cap 2 %): the scene is unfit"
    assert tie <= NEAR_TIE_CAP, f"{what}: {100 * tie:.2f} % of the pixels are near ties (cap 1 %): the scene is unfit"
    assert ideal.covered.mean() > 0.02, f"{what}: the scene covers next to nothing"


class Report:
    def __init__(self):
        self.failures = []
        self.coverage_wrong = self.identity_wrong = 0
        self.depth_ratio = self.uv_ratio = 0.0
        self.compared = 0

    @property
    def ok(self):
        return not self.failures

    def line(self):
        return (f"compared {self.compared} px, coverage wrong {self.coverage_wrong}, identity wrong {self.identity_wrong}, "
                f"depth err/tol {self.depth_ratio:.3f}, uv err/bound {self.uv_ratio:.3f}")


def compare(frame, ideal) -> Report:
    color, depth, stats = frame
    depth = depth.astype(np.float64)
    r = Report()
    ok = ~ideal.ambiguous
    got = depth < ideal.clear_depth
    r.coverage_wrong = int((ok & (got != ideal.covered)).sum())
    if r.coverage_wrong:
        r.failures.append(f"coverage: {r.coverage_wrong} unambiguous pixels disagree")
    both = ok & got & ideal.covered
    r.compared = int(both.sum())
    tie = both & (ideal.gap <= 2.0 * ideal.tol)
    clear = both & ~tie
    err = np.abs(depth - ideal.depth)
    err_tie = np.minimum(err, np.abs(depth - ideal.depth2))
    ratio = np.where(clear, err, np.where(tie, err_tie, 0.0)) / np.where(both, ideal.tol, 1.0)
    r.depth_ratio = float(ratio.max()) if ratio.size else 0.0
    if r.depth_ratio > 1.0:
        r.failures.append(f"depth: {int((ratio > 1.0).sum())} pixels over tol, worst {r.depth_ratio:.2f} x tol")
    # identity / uv of the winner
    tri = np.where(clear, ideal.tri, 0)
    table = np.array([(t[3], t[4]) for t in ideal.tris] or [(0, 0)], dtype=np.int64)
    did, textured = table[tri, 0], table[tri, 1].astype(bool)
    flat = clear & ~textured
    want = PALETTE[did % 20]
    wrong = flat & ((color[..., :3] != want).any(axis=-1) | (color[..., 3] != 255))
    r.identity_wrong = int(wrong.sum())
    if r.identity_wrong:
        r.failures.append(f"identity: {r.identity_wrong} pixels do not carry the colour of the ideal's winner")
    tex = clear & textured
    if tex.any():
        worst = 0.0
        for byte, u, g, e in ((color[..., 0], ideal.u, ideal.grad_u, ideal.err_u), (color[..., 1], ideal.v, ideal.grad_v, ideal.err_v)):
            bound = 0.5 + 0.5 + 256.0 * (g * SNAP + e) + 2.0 ** -10
            d = np.abs(byte.astype(np.float64) - np.clip(256.0 * u - 0.5, 0.0, 255.0))
            worst = max(worst, float((d / bound)[tex].max()))
        wrong_a = int((tex & (color[..., 3] != 255)).sum())
        r.uv_ratio = worst
        if worst > 1.0 or wrong_a:
            r.failures.append(f"uv: worst {worst:.2f} x bound, {wrong_a} alpha bytes not 255")
    if stats["tris_in"] != ideal.tris_in:
        r.failures.append(f"tris_in {stats['tris_in']} != {ideal.tris_in}")
    return r


def vertex_stage_ratio(got_clip, got_uv, clip, uv, e_clip, e_uv):
    """max |got - ideal| / e over a primitive's vertices; an exact component (e = 0) must be equal (ratio inf otherwise)"""
    worst = 0.0
    for g, x, e in ((got_clip, clip, e_clip), (got_uv, uv, e_uv)):
        d = np.abs(g.astype(np.float64) - x)
        with np.errstate(all="ignore"):
            q = np.where(d == 0.0, 0.0, d / e)
        worst = max(worst, float(q.max()) if q.size else 0.0)
    return worst


def palette_ratio(got, pal, pal_abs, depth):
    """read-back palettes [n, J, 16] column-major against the float64 ones [n, J, 4, 4]: |diff| / (4 (depth + 1) 2^-24
    sum|products|), worst element"""
    g = np.asarray(got, dtype=np.float64).reshape(pal.shape[0], pal.shape[1], 4, 4).transpose(0, 1, 3, 2)
    bound = 4.0 * (np.asarray(depth)[None, :, None, None] + 1) * 2.0 ** -24 * pal_abs
    d = np.abs(g - pal)
    with np.errstate(all="ignore"):
        q = np.where(d == 0.0, 0.0, d / bound)
    return float(q.max())
