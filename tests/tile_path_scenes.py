"""Scenes that put a bin on one particular path of the tile kernels (tests/test_gpu_tile_paths.py), and the integer model
that proves it: SPEC.md sections 5 and 6 in exact Python integers -- snapped vertices, pixel-centre boxes, coverage -- so
that every premise (box pixels per bin and pass, hits per pixel, the edge class) is computed, not claimed.  No device is
needed here: tests/test_tile_path_premises.py checks the premises and the model itself (against the oracle's coverage).

Vertex positions are multiples of 1/256 px, so the snapped X, Y are known exactly.  Materials: a translucent texture
(alpha 30..230, alpha-blended by the default pipeline state) and one opaque debug-colour triangle per scene, so that
both tile kernels see bins that mix order-free and order-dependent triangles."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from mt_renderer_amd import scene
from tests.pixel_scenes import pixel_model, pixel_to_ndc_matrix

BIN = 16
TRI_PASS = 64         # triangles per pass of k_tile
FRAG_K = 8            # k_tile: triangle numbers kept per pixel and pass
STAIR_K = 8           # k_tile_vis: submission orders kept per pixel
PAIR_CAP = 2048       # k_tile: (triangle, box pixel) pairs a pass may flatten
CLASS_LIMIT = 16384   # extent (1/256 px) above which a triangle needs 64-bit edge functions


def translucent_texture():
    t = scene.checker_rgba8_texture(8, 8, cell=1, alpha=(230, 30))
    a = np.frombuffer(t.data, dtype=np.uint8).reshape(8, 8, 4)[..., 3]
    assert a.min() == 30 and a.max() == 230
    return t


class Tri:
    """one triangle of a scene: three (x, y) in pixels, a constant depth, textured (translucent) or opaque"""

    def __init__(self, pts, z, opaque=False, uv_span=BIN):
        self.pts, self.z, self.opaque = [tuple(p) for p in pts], z, opaque
        # texcoords: the position relative to the first vertex's bin, so that a translated copy samples the same texels
        ox, oy = int(pts[0][0]) // BIN * BIN, int(pts[0][1]) // BIN * BIN
        self.uv = [(float(x - ox) / uv_span, float(y - oy) / uv_span) for x, y in self.pts]
        self.X, self.Y = [], []
        for x, y in self.pts:
            fx, fy = Fraction(x) * 256, Fraction(y) * 256
            assert fx.denominator == 1 and fy.denominator == 1, "vertices are multiples of 1/256 px"
            self.X.append(int(fx))
            self.Y.append(int(fy))
        X, Y = self.X, self.Y
        self.area2 = (X[2] - X[0]) * (Y[1] - Y[0]) - (X[1] - X[0]) * (Y[2] - Y[0])
        assert self.area2 > 0, "front-facing (SPEC.md 5.4)"
        self.large = max(X) - min(X) > CLASS_LIMIT or max(Y) - min(Y) > CLASS_LIMIT

    def box(self, w, h):
        """pixel-centre candidate range clamped to the target (SPEC.md 5.5): x0, x1, y0, y1, inclusive"""
        return (max((min(self.X) + 127) >> 8, 0), min((max(self.X) - 128) >> 8, w - 1),
                max((min(self.Y) + 127) >> 8, 0), min((max(self.Y) - 128) >> 8, h - 1))

    def covers(self, px, py):
        X, Y = self.X, self.Y
        Px, Py = 256 * px + 128, 256 * py + 128
        for a, b in ((1, 2), (2, 0), (0, 1)):
            dx, dy = X[b] - X[a], Y[b] - Y[a]
            e = dy * (Px - X[a]) - dx * (Py - Y[a])
            if not (e > 0 or (e == 0 and (dy > 0 or (dy == 0 and dx < 0)))):
                return False
        return True

    def pixels(self, w, h):
        x0, x1, y0, y1 = self.box(w, h)
        return [(px, py) for py in range(y0, y1 + 1) for px in range(x0, x1 + 1) if self.covers(px, py)]


class PathScene:
    def __init__(self, w, h, tris):
        self.w, self.h, self.tris = w, h, tris
        assert sum(t.opaque for t in tris) == 1, "one opaque triangle per scene"

    def draws(self):
        """one primitive per run of triangles of the same material, in submission order"""
        prims, i = [], 0
        while i < len(self.tris):
            j = i
            while j < len(self.tris) and self.tris[j].opaque == self.tris[i].opaque:
                j += 1
            verts = []
            for t in self.tris[i:j]:
                for (x, y), uv in zip(t.pts, t.uv):
                    v = (float(x), float(y), float(t.z))
                    verts.append(v if t.opaque else v + uv)
            prims.append(dict(verts=verts, indices=list(range(len(verts))), texture=-1 if self.tris[i].opaque else 0, debug_id=3))
            i = j
        md = pixel_model(prims, [translucent_texture()])
        return [dict(md=md, M=pixel_to_ndc_matrix(self.w, self.h))]

    def covered(self):
        """boolean [h, w]: pixels some triangle covers (every depth is inside 0..1, so the depth buffer shows them)"""
        m = np.zeros((self.h, self.w), dtype=bool)
        for t in self.tris:
            for px, py in t.pixels(self.w, self.h):
                m[py, px] = True
        return m

    def entries(self, bx, by):
        """the bin's triangles in submission order: those whose candidate range reaches into the bin"""
        out = []
        for t in self.tris:
            x0, x1, y0, y1 = t.box(self.w, self.h)
            if x0 <= x1 and y0 <= y1 and x0 <= bx * BIN + BIN - 1 and x1 >= bx * BIN and y0 <= by * BIN + BIN - 1 and y1 >= by * BIN:
                out.append(t)
        return out

    def box_pixels(self, t, bx, by):
        """pixels of the triangle's box inside the bin: the pairs the fragment-list path flattens"""
        x0, x1, y0, y1 = t.box(self.w, self.h)
        x0, x1, y0, y1 = max(x0, bx * BIN), min(x1, bx * BIN + BIN - 1), max(y0, by * BIN), min(y1, by * BIN + BIN - 1)
        return max(x1 - x0 + 1, 0) * max(y1 - y0 + 1, 0)

    def hits(self, tris, bx, by):
        """{pixel: [triangles covering it, in submission order]} inside the bin"""
        out = {}
        for t in tris:
            for p in t.pixels(self.w, self.h):
                if p[0] // BIN == bx and p[1] // BIN == by:
                    out.setdefault(p, []).append(t)
        return out

    def passes(self, bx, by):
        e = self.entries(bx, by)
        return [e[i:i + TRI_PASS] for i in range(0, len(e), TRI_PASS)]


def F(a, b=1):
    return Fraction(a, b)


def _stack(cx, cy, n=12):
    """n triangles of about 3 px that all cover the centre of pixel (cx, cy), nearer and nearer in submission order"""
    tris = []
    for k in range(n):
        j = F(k % 4, 16)
        a = (cx + F(1, 4) - j, cy + F(1, 4))
        b = (cx + F(3, 4), cy + F(11, 4) - j)
        c = (cx + F(11, 4) - j, cy + F(1, 2) + j)
        tris.append(Tri([a, b, c], F(48 - 2 * k, 64)))
    return tris


def list_overflow(w=32, h=32, cx=20, cy=4):
    """1 (and 5 with a 24 x 24 target): twelve small triangles on one pixel, then an opaque one beside them"""
    tris = _stack(cx, cy)
    tris.insert(6, Tri([(cx - 3, cy + F(1, 4)), (cx - 3, cy + 3), (cx, cy + 1)], F(1, 2), opaque=True))
    return PathScene(w, h, tris)


def _quad_layer(x0, y0, z, first_opaque=False):
    a, b, c, d = (x0, y0), (x0, y0 + BIN), (x0 + BIN, y0 + BIN), (x0 + BIN, y0)
    return [Tri([a, b, c], z, opaque=first_opaque), Tri([a, c, d], z)]


def pair_cap():
    """2: bin (0, 0) holds four layers of a bin-filling quad (2048 pairs: the cap), bin (2, 0) the same four and a fifth,
    farther one behind them (2560 pairs).  The fifth fails the depth test everywhere, so where both bins hold the same
    triangles -- the half of the quad the opaque triangle of bin (0, 0) does not cover -- they show the same pixels"""
    tris = []
    for layer in range(4):
        z = F(40 - 4 * layer, 64)
        tris += _quad_layer(0, 0, z, first_opaque=(layer == 0))
        tris += _quad_layer(2 * BIN, 0, z)
    tris += _quad_layer(2 * BIN, 0, F(50, 64))
    return PathScene(64, 16, tris)


def large_among_small():
    """3: bin (2, 0) of a 128 x 32 target: 14 small translucent triangles, a small opaque one, a translucent triangle over
    64 px across, 15 more small ones"""
    def small(i):
        x, y = 2 * BIN + 1 + (i * 5) % 13, 1 + (i * 3) % 12
        s = F(3 + i % 3, 2)
        return [(x + F(1, 4), y + F(1, 4)), (x + F(1, 2), y + F(1, 4) + s), (x + F(1, 4) + s, y + F(1, 2))]
    tris = [Tri(small(i), F(20 + (i * 7) % 23, 64)) for i in range(14)]
    tris.append(Tri(small(14), F(30, 64), opaque=True))
    tris.append(Tri([(F(5, 2), F(3, 2)), (F(40), F(61, 2)), (F(251, 2), F(5, 2))], F(33, 64), uv_span=128))
    tris += [Tri(small(i), F(20 + (i * 7) % 23, 64)) for i in range(15, 30)]
    return PathScene(128, 32, tris)


def lists_across_passes(n=130):
    """4: n one-pixel triangles in bin (1, 0), on eight pixels in turn; depths shuffled, some tied exactly"""
    rng = np.random.default_rng(4)
    zs = [F(int(v), 128) for v in rng.permutation(n) // 2 + 20]  # pairs of equal depths, in shuffled places
    tris = []
    for i in range(n):
        k = i % 8
        x, y = BIN + 2 + 3 * (k % 4), 3 + 7 * (k // 4)
        j = F((i // 8) % 4, 32)
        tris.append(Tri([(x + F(1, 8) + j, y + F(1, 8)), (x + F(1, 2), y + F(7, 8) + j), (x + F(7, 8), y + F(3, 8) - j)], zs[i], opaque=(i == 70)))
    return PathScene(32, 16, tris)
