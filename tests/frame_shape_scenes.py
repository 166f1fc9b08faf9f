"""Frames at the limits of the frame size (include/mtr.h: 1 x 1 .. 16384 x 16384): the shapes, and two scenes that can be
built for any of them.  Plain numpy; no device and no oracle.  tests/test_frame_shape_premises.py proves on the CPU that
the scenes are fit and have teeth, tests/test_gpu_frame_shapes.py renders them through the HIP path.

*Ribbon* (``ribbon(w, h, variant)``): two triangle strips along the frame's long axis, from -0.03 L to 1.03 L, between rails
at -3 S - 0.27 and 4 S + 0.31 px across the short one (L, S the long and the short side), so that the only edges inside a
thin frame are cross edges and diagonals, none near-parallel to a row of pixel centres.  Depth and clip w are functions of
the long-axis coordinate alone: a one-pixel-thick frame turns any depth slope across it into an enormous gradient per
pixel, which the near-tie rule of tests/ideal_compare.py (it weighs the gap against the winner's tolerance only) does not
see on the loser.  ``z = 0.5 + a sin(..)`` with one period per strip; the matrix adds 0.4 x the long-axis NDC coordinate to
clip w, and the vertices are the pre-images of the screen positions above, so w runs from 0.70 to 1.74 along the frame.
Each strip has 48 quads, not about 24: two depths that are linear between 25 cross edges each change winner about once per
quad, and 40 changes are asked for; these periods give 50, with the depths at least 0.016 apart at every cross edge.

Texture coordinates (variants ``tex`` and ``alpha``): u is 0 at every even cross edge and ``U_j`` at every odd one, with ``U_j``
chosen so that the product ``|du/dpx| Wt`` of SPEC 7 sits at a target from P_FIRST / P_SECOND, a sixth or more away from every
threshold (1 for the filter, 2^(l - 1/2) for the levels) -- the perspective (w^2 grows 2.5 % per quad) and the slant of
the cross edges (at most a fortieth of a quad) move it by a few per cent inside a quad.  u that simply grew along 16384 px would reach hundreds, its rounding (gamma_11 (max|u_i| + |u|))
a tenth of a product, and a smooth product would cross each threshold over hundreds of pixels: 7.9 % decision-ambiguous in
a first attempt.  v runs from 0 across the ribbon to ``vspan``: 1 on the first strip (100 x 60, 7 levels) unless the
product 60 / (7 S + 0.58) that follows lies within 15 % of a threshold (S = 3: 2.78 against 2.83), in which case it is
lowered to the next target; on the second strip (64 x 64, 4 levels) the product is 0.75 or what v = 0 .. 1 gives, whichever
is less, so that the linear filter is reachable on a frame one pixel thick -- where the partner ``y ^ 1`` of every quad
lies outside the frame.  On such a frame the first strip's level comes from that outside partner alone (product 7.9, level 3).

*Lattice* (``lattice(w, h, far)``): 180 triangles in three primitives (centres from -8 to 72 px, a third of them from -4 to
20 px, where the tiny crops are; extents up to 47 px; z = k/256), every vertex on the 1/256-pixel lattice, w = 1, the
matrix exactly ``pixel_to_ndc_matrix(w, h)``.  Snapping (SPEC 5) returns every vertex to its lattice point whatever the frame's
size is, so a w x h frame equals, bit for bit, the ``[0:h, 0:w]`` crop of a larger frame of the same scene.  ``far`` adds
eleven copies of the triangles along the long axis, the last one 16384 - 64 px away at the far end: two copies alone
cover 1 % of a 16384 x 16 frame, and the comparison wants 2 % of the pixels compared."""
from __future__ import annotations

import functools
import math

import numpy as np

from mt_renderer_amd import scene
from tests import ideal_renderer
from tests.ideal_scenes import _tagged_chain, _tex
from tests.pixel_scenes import pixel_model

TINY = [(1, 1), (2, 1), (1, 2), (3, 5), (7, 7), (15, 17), (16, 16), (17, 1), (1, 33), (31, 3)]
LONG = [(16384, 1), (1, 16384), (16384, 16), (16, 16384), (16381, 3), (5, 16383), (8200, 40)]
GRID = [(16384, 272)]      # 1024 x 17 bins: k_scan takes 17 rounds
SHARD = [(1, 1), (17, 1), (20, 7), (16384, 16), (16381, 3), (16, 16384)]
VARIANTS = ("ids", "tex", "alpha")

# crop property: (small shape, the frame it is a crop of, far instance present)
CROPS = [(s, (64, 64), False) for s in TINY] + \
        [((16384, 1), (16384, 16), True), ((16381, 3), (16384, 16), True),
         ((1, 16384), (16, 16384), True), ((5, 16383), (16, 16384), True)]
LATTICE_FRAMES = [((64, 64), False), ((16384, 16), True), ((16, 16384), True)]

QUADS = 48
W_SLOPE = 0.4               # clip w = 1 + 0.4 x (long-axis NDC coordinate)
IDS = (3, 11)
Z_FIRST = (0.30, 17.4, 0.4)      # amplitude, periods over the frame, phase
Z_SECOND = (0.22, 17.1, 1.9)
SHIFT = 0.37                # the second strip's cross edges, in quads, against the first's
TEX_FIRST, TEX_SECOND = (100, 60, 7), (64, 64, 4)
P_FIRST = (0.75, 2.0, 8.0, 1.19, 4.0, 16.0, 32.0)     # targets of |du/dpx| Wt, one per pair of quads, in turn
P_SECOND = (0.75, 0.75, 2.0, 0.75, 4.0)
P_SAFE = (0.75, 1.19, 2.0, 4.0, 8.0, 16.0, 32.0)
ST_CULL_NONE = (0, 1, 1, 1)      # blend ALPHA, depth write, depth test, cull NONE


def _thresholds():
    return [1.0] + [2.0 ** (l - 0.5) for l in range(1, 8)]


def v_product_first(S):
    """the product |dv/dpx| Ht of the first strip: what v = 0 .. 1 gives, or the next target below it where that lies
    within 15 % of a threshold"""
    width = 7.0 * S + 0.58
    p = TEX_FIRST[1] / width
    if any(abs(p / t - 1.0) < 0.15 for t in _thresholds()):
        p = max(t for t in P_SAFE if t < p)
    return p


@functools.lru_cache(maxsize=None)
def _textures(translucent):
    first = _tagged_chain(*TEX_FIRST, 2100)
    second = _tagged_chain(*TEX_SECOND, 2200)
    if translucent:
        for a in second:
            a[..., 3] = 40 + (a[..., 0] % 200)
    return _tex(first), _tex(second)


@functools.lru_cache(maxsize=None)
def _bc7_textures():
    """the two chains as random BC7 blocks (tests/test_gpu_texture_blocks.py): for the block-resident sampling path"""
    out = []
    for (wt, ht, nl), seed in ((TEX_FIRST, 2300), (TEX_SECOND, 2400)):
        data = b"".join(scene.random_bc7_texture(max(1, wt >> l), max(1, ht >> l), seed=seed + l).data for l in range(nl))
        out.append(scene.TextureData(wt, ht, scene.TEX_BC7, data, levels=nl))
    return tuple(out)


def _strip(w, h, which, textured):
    """one strip as a pixel_model primitive: vertices are pre-images, under clip w = 1 + 0.4 l, of the screen positions"""
    tall = h > w
    L, S = (h, w) if tall else (w, h)
    q = 1.06 * L / QUADS
    amp, periods, phase = Z_SECOND if which else Z_FIRST
    n = QUADS + (1 if which else 0)
    start = -0.03 * L - ((1.0 - SHIFT) * q if which else 0.0)
    rng = np.random.default_rng(50 + which)
    cap = min(float(S), q / 40.0)
    r0, r1 = -3.0 * S - 0.27, 4.0 * S + 0.31
    wt, ht, _ = TEX_SECOND if which else TEX_FIRST
    targets = P_SECOND if which else P_FIRST
    pv = min(0.75, ht / (r1 - r0)) if which else v_product_first(S)
    vspan = pv * (r1 - r0) / ht
    verts = []
    for k in range(n + 1):
        slant = rng.uniform(0.3, 0.7) * cap * (1.0 if rng.integers(0, 2) else -1.0)
        u = 0.0 if k % 2 == 0 else targets[(k // 2) % len(targets)] * q / wt
        for across, along, v in ((r0, start + k * q + 0.5 * slant, 0.0), (r1, start + k * q - 0.5 * slant, vspan)):
            z = 0.5 + amp * math.sin(2.0 * math.pi * periods * along / L + phase)
            sx, sy = (across, along) if tall else (along, across)
            xs, ys = 2.0 * sx / w - 1.0, 1.0 - 2.0 * sy / h
            cw = 1.0 / (1.0 - W_SLOPE * (ys if tall else xs))
            p = ((xs * cw + 1.0) * w / 2.0, (1.0 - ys * cw) * h / 2.0, z * cw)
            verts.append(p + (u, v) if textured else p)
    prim = dict(verts=verts, indices=list(range(len(verts))), topology=scene.TOPO_STRIP, debug_id=IDS[which])
    if textured:
        prim["texture"] = which
    return prim


def ribbon_matrix(w, h):
    N = np.eye(4)
    N[0, 0], N[0, 3] = 2.0 / w, -1.0
    N[1, 1], N[1, 3] = -2.0 / h, 1.0
    P = np.eye(4)
    P[3, 1 if h > w else 0] = W_SLOPE
    return scene.to_f32_colmajor(P @ N)


@functools.lru_cache(maxsize=None)
def ribbon(w, h, variant):
    """-> draws of the ribbon scene for a w x h frame, in the form tests/helpers.render_oracle / render_gpu take"""
    assert variant in VARIANTS + ("bc7",)      # bc7: ``tex`` with block-compressed chains, for the oracle alone to check
    textured = variant != "ids"
    textures = None
    if textured:
        textures = list(_bc7_textures() if variant == "bc7" else _textures(variant == "alpha"))
    md = pixel_model([_strip(w, h, 0, textured), _strip(w, h, 1, textured)], textures=textures)
    md.prim_states = np.array([ST_CULL_NONE, ST_CULL_NONE], dtype=np.uint8)
    return [dict(md=md, M=ribbon_matrix(w, h))]


@functools.lru_cache(maxsize=None)
def ribbon_ideal(w, h, variant, mutate=None):
    return ideal_renderer.render(w, h, ribbon(w, h, variant), mutate=mutate, fragments=variant != "ids")


# -------------------------------------------------------------------------------------------------------------------
# the lattice scene
# -------------------------------------------------------------------------------------------------------------------
LATTICE_TRIS = 180
LATTICE_EXTENTS = (300, 900, 4000, 12000)     # 1/256 px
FAR_SHIFT = 16384 - 64
LATTICE_COPIES = 12           # of a ``far`` scene: whole-pixel shifts from 0 to FAR_SHIFT


@functools.lru_cache(maxsize=None)
def _lattice_tris():
    """[180, 3, 3] integers: x, y in 1/256 px, z in 1/256"""
    rng = np.random.default_rng(4242)
    c = rng.integers(-8 * 256, 72 * 256 + 1, size=(LATTICE_TRIS, 1, 2))
    near = LATTICE_TRIS // 3      # a third of them about the origin, where the tiny crops are
    c[:near] = rng.integers(-4 * 256, 20 * 256 + 1, size=(near, 1, 2))
    e = np.array(LATTICE_EXTENTS)[rng.integers(0, 4, size=(LATTICE_TRIS, 1, 1))]
    off = rng.integers(-500, 501, size=(LATTICE_TRIS, 3, 2)) * e // 1000
    z = rng.integers(1, 256, size=(LATTICE_TRIS, 3, 1))
    return np.concatenate([c + off, z], axis=2)


@functools.lru_cache(maxsize=None)
def _lattice_model(far_axis):
    """far_axis: None, or the axis (0 = x, 1 = y) along which the further copies stand, the last one FAR_SHIFT px away"""
    T = _lattice_tris()
    if far_axis is not None:
        copies = []
        for k in range(LATTICE_COPIES):
            Tk = T.copy()
            Tk[:, :, far_axis] += (k * FAR_SHIFT // (LATTICE_COPIES - 1)) * 256
            copies.append(Tk)
        T = np.concatenate(copies)
    prims = []
    for k, did in enumerate((2, 7, 13)):
        t = T[k::3].astype(np.float64) / 256.0
        prims.append(dict(verts=t.reshape(-1, 3), indices=list(range(3 * t.shape[0])), debug_id=did))
    md = pixel_model(prims)
    md.prim_states = np.array([ST_CULL_NONE] * 3, dtype=np.uint8)
    return md


def lattice(w, h, far=False):
    """-> draws; ``far``: with the further copies along the frame's long axis"""
    from tests.pixel_scenes import pixel_to_ndc_matrix
    md = _lattice_model((1 if h > w else 0) if far else None)
    return [dict(md=md, M=pixel_to_ndc_matrix(w, h))]


@functools.lru_cache(maxsize=None)
def lattice_ideal(w, h, far=False):
    return ideal_renderer.render(w, h, lattice(w, h, far))


# -------------------------------------------------------------------------------------------------------------------
# conditions, from the ideal alone
# -------------------------------------------------------------------------------------------------------------------
def level_wins(ideal):
    """-> (compared pixels won by each level of the first strip's chain [7], compared pixels won by the linear filter)"""
    from tests import ideal_compare
    F = ideal.frags
    ok = ideal_compare.expected(ideal).compare.reshape(-1)[F.pix] & F.passes
    wins = np.bincount(F.level[ok & (F.kind == 2) & (F.tex == 0)], minlength=TEX_FIRST[2])
    return wins, int((ok & (F.kind == 1)).sum())


def winner_changes(ideal):
    """changes of the winning primitive along the middle line of the long axis"""
    did = np.array([t[3] for t in ideal.tris])[ideal.tri]
    did = np.where(ideal.tri >= 0, did, -1)
    line = did[:, ideal.w // 2] if ideal.h > ideal.w else did[ideal.h // 2, :]
    return int((line[1:] != line[:-1]).sum()), set(int(x) for x in np.unique(did))
