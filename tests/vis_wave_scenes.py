"""Scenes for k_tile_vis.hip at a forced number of waves per bin (tests/test_gpu_vis_waves.py), on the integer model of
tests/tile_path_scenes.py.  A bin's 64-entry passes are dealt round-robin to its W waves: the pass at entry 64 * k is pass k,
wave k mod W, that wave's iteration k div W.  Every scene here takes W and places its content by pass of the SUBMISSION
order, so that a particular wave meets it in a particular iteration of its two-deep pipeline.  No device is needed:
tests/test_vis_wave_premises.py computes each scene's claim from its integers.

How far a queue follows the submission order: what depends on N alone -- how many iterations each wave runs, which wave gets
the partial last pass, which waves own no pass -- holds for every queue builder.  Which triangles share a pass depends on the
order in which geometry chunks claim their place in the bin's queue, and a chunk claims it when its wave arrives (only the
ordered kernel sorts chunks back).  So a scene is submitted as one DRAW per run of at most RUN triangles (one chunk, one
wave): the draws of a frame are geometry launches on one stream, one after the other, and the single-pass queues then hold
the runs in submission order -- there the passes are the ones the premises describe.  The two-pass fill is one launch over
every chunk of the frame and takes the runs in any order; the pixels may not depend on it.

Targets are at most 128 x 32, vertices lie on the 1/256 px lattice, one bin is under test (BX, 0), or (1, 0) for
resolve_pairs.  Materials: None = a debug colour (given per run of up to RUN triangles), "texa" / "texb" = opaque textures,
"trans" = the translucent texture of tile_path_scenes (alpha-blended: the frame is then a mixed one)."""
from __future__ import annotations

from fractions import Fraction as F

import numpy as np

from mt_renderer_amd import scene
from tests.pixel_scenes import pixel_model, pixel_to_ndc_matrix
from tests.tile_path_scenes import BIN, STAIR_K, PathScene, Tri, translucent_texture

TW, TH = 128, 16  # 8 x 1 bins (8 x 2 with h = 32)
BX = 2            # the bin under test
RUN = 32          # triangles per draw at the most (one geometry chunk): a colour per half pass
WAVES = (2, 4, 8)


# ---- the triangles of tests/test_gpu_hot_path.py (which imports them from here) ----
def _big(i):
    """a triangle of bin BX whose box holds nine pixels or more"""
    x, y = BX * BIN + 1 + (i * 5) % 10, 1 + (i * 3) % 11
    s = 3 + F(i % 3, 2)
    return Tri([(x + F(1, 4), y + F(1, 4)), (x + F(1, 2), y + F(1, 4) + s), (x + F(1, 4) + s, y + F(1, 2))], F(20 + (i * 7) % 23, 64))


def _one(i):
    """a triangle of bin BX whose box is the one pixel it covers"""
    x, y = BX * BIN + (i * 7) % 16, (i * 5) % 16
    return Tri([(x + F(5, 16), y + F(5, 16)), (x + F(7, 16), y + F(13, 16)), (x + F(13, 16), y + F(7, 16))], F(10 + (i * 11) % 40, 64))


def _large(k):
    """more than 64 px across: 64-bit edge functions; covers most of bin BX"""
    return Tri([(F(5, 2) + k, F(3, 2)), (F(40) - 3 * k, F(31, 2)), (F(251, 2) - k, F(5, 2) + k)], F(33 - 6 * k, 64))


def _pass(nbig, k):
    """64 entries of bin BX: nbig boxes over four pixels, one-pixel boxes, and one large triangle in the middle"""
    small = [_big(i) for i in range(nbig)] + [_one(i) for i in range(63 - nbig)]
    order = np.random.default_rng(nbig).permutation(63)
    tris = [small[j] for j in order]
    tris.insert(31, _large(k))
    return tris


SPAN_PASS, PAIR_PASS = 40, 20  # boxes over four pixels among the 63 small triangles: 80 >= 63 > 40


# ---- the scenes of this file ----
def opaque_textures():
    return {"texa": scene.checker_rgba8_texture(8, 8, cell=1), "texb": scene.checker_rgba8_texture(4, 4, cell=2)}


def mk(pts, z, mat=None, uv_span=BIN):
    t = Tri(pts, z, opaque=(mat != "trans"), uv_span=uv_span)
    t.mat = mat
    return t


def one_px(px, py, z, mat=None):
    """covers the centre of pixel (px, py) and nothing else: the shape of _one"""
    return mk([(px + F(5, 16), py + F(5, 16)), (px + F(7, 16), py + F(13, 16)), (px + F(13, 16), py + F(7, 16))], z, mat)


def two_px(px, py, z, mat=None):
    """covers the centres of (px, py) and (px + 1, py)"""
    return mk([(px + F(1, 4), py + F(1, 4)), (px + F(1, 2), py + F(7, 8)), (px + F(15, 8), py + F(1, 2))], z, mat)


def winner(frags):
    """of the triangles that cover a pixel, in submission order: the smallest z, the latest among equals"""
    zmin = min(t.z for t in frags)
    return [t for t in frags if t.z == zmin][-1]


class WaveScene(PathScene):
    """a PathScene with a material per triangle and no rule about how many are opaque"""

    def __init__(self, w, h, tris, bx=BX, by=0):
        self.w, self.h, self.tris, self.bx, self.by = w, h, tris, bx, by
        self.mixed = any(getattr(t, "mat", None) == "trans" for t in tris)
        self.textured = any(isinstance(getattr(t, "mat", None), str) for t in tris)
        # one primitive per run of at most RUN triangles of one material, in submission order; a debug colour per run
        self.runs, i = [], 0
        while i < len(tris):
            m, j = getattr(tris[i], "mat", None), i
            while j < len(tris) and j - i < RUN and getattr(tris[j], "mat", None) == m:
                j += 1
            cid = (7 * len(self.runs)) % 20
            for t in tris[i:j]:
                t.mat, t.cid = m, (cid if m is None else m)
            self.runs.append((i, j, m, cid))
            i = j

    def draws(self):
        """one draw (a model of one primitive) per run.  The draws of a frame are geometry launches on one stream, one after
        the other, so the single-pass queues take the runs in submission order; the two-pass fill is one launch over every
        chunk of the frame and takes them as their waves arrive"""
        texs = dict(opaque_textures(), trans=translucent_texture())
        M = pixel_to_ndc_matrix(self.w, self.h)
        out = []
        for i, j, m, cid in self.runs:
            verts = []
            for t in self.tris[i:j]:
                for (x, y), uv in zip(t.pts, t.uv):
                    v = (float(x), float(y), float(t.z))
                    verts.append(v if m is None else v + uv)
            prim = dict(verts=verts, indices=list(range(len(verts))), texture=-1 if m is None else 0, debug_id=cid)
            out.append(dict(md=pixel_model([prim], [] if m is None else [texs[m]]), M=M))
        return out

    def bin_entries(self):
        return self.entries(self.bx, self.by)

    def bin_hits(self):
        return self.hits(self.bin_entries(), self.bx, self.by)


def pass_of(W, k):
    """(wave, iteration) of pass k"""
    return k % W, k // W


def pipeline_edge_sizes(W):
    S = 64 * W
    return [1, 65, S - 1, S, S + 1, 2 * S, 2 * S + 1, 3 * S + 1]


def pipeline_edges(W, N, h=TH):
    """opaque: N triangles of one to three pixels in bin (BX, 0), depths shuffled with exact ties.  Placed by hand: a
    champion per pass (the nearest triangle of a pixel of its own), a tie between passes 0 and 1 (two waves) on pixel 255, one
    between passes 0 and W (wave 0, iterations 0 and 1) on pixel 254 and one between passes W and 2W on pixel 253; the rest
    lands on pixels 0..249 at random"""
    S = 64 * W
    rng = np.random.default_rng(1000 * W + N)
    pix = [int(v) for v in rng.integers(0, 250, N)]
    # pairs of equal depths in shuffled places, from 40/2048 up to 1940/2048 whatever N is
    z = [F(40 + int(v) * 1900 // max(N // 2, 1), 2048) for v in rng.permutation(N) // 2]
    for k in range((N + 63) // 64):  # the champions: nearer than anything the shuffle gives
        c = 64 * k + (7 * k + 3) % min(64, N - 64 * k)
        pix[c], z[c] = k, F(8 + (5 * k) % 16, 2048)

    def tie(q, a, b, zq):
        pix[a], pix[b], z[a], z[b] = q, q, zq, zq
    if N >= 65:
        tie(255, 5, 64 + (9 if N - 64 > 9 else 0), F(6, 2048))
    if N > S:
        tie(254, 11, S + (13 if N - S > 13 else 0), F(7, 2048))
    if N > 2 * S:
        tie(253, S + 17, 2 * S + (19 if N - 2 * S > 19 else 0), F(5, 2048))
    tris = []
    for i in range(N):
        px, py = BX * BIN + pix[i] % BIN, pix[i] // BIN
        wide = pix[i] < 250 and pix[i] >= 32 and i % 6 == 1 and pix[i] % BIN < BIN - 1
        tris.append((two_px if wide else one_px)(px, py, z[i]))
    return WaveScene(TW, h, tris)


WALK_KINDS = ("span", "pair", "large")


def walk_pass(kind):
    if kind == "span":
        return _pass(SPAN_PASS, 0)
    if kind == "pair":
        return _pass(PAIR_PASS, 1)
    tris = [_one(i + 5) for i in range(63)]  # one-pixel boxes and the one 64-bit-class triangle: the pair walk
    tris.insert(31, _large(2))
    return tris


def walk_passes(W, wave, first):
    """{pass: kind}: passes wave, wave + W, wave + 2W (iterations 0, 1, 2 of that wave) in the rotation that starts with
    WALK_KINDS[first]"""
    return {wave + i * W: WALK_KINDS[(first + i) % 3] for i in range(3)}


def walks_per_iteration(W, wave, first):
    """opaque: a span-walk pass, a pair-walk pass and a pass of one-pixel boxes, each with one 64-bit-class triangle in the
    middle, as three successive iterations of one wave; every other pass is 64 one-pixel triangles"""
    kinds = walk_passes(W, wave, first)
    tris = []
    for p in range(wave + 2 * W + 1):
        tris += walk_pass(kinds[p]) if p in kinds else [_one(64 * p + j) for j in range(64)]
    for t in tris:
        t.mat = None
    return WaveScene(TW, TH, tris)


def _bin_filler(k, z):
    """i32 class (34 px across at the most), box = the whole bin, covers the pixels with lx + ly below about 15 + (63 - k) / 4"""
    x0, y0, s = BX * BIN - F(1, 2), -F(1, 2), 17 + F(63 - k, 4)
    return mk([(x0, y0), (x0, y0 + s), (x0 + s, y0)], z)


def big_boxes_second_iteration(W, nfill, layout="front"):
    """opaque: pass W -- wave 0's second iteration -- holds nfill triangles whose box is the whole bin (256 pixels each) and
    64 - nfill one-pixel ones; their depths come nearer in turn, with one exact tie across two primitives.  Passes 0..W-1 and
    a short pass W + 1 are one-pixel fill.  nfill = 64: 16384 box pixels, 1024 bbox rows -- the most one pass can hold, and by
    the `spans` rule a span-walk pass.  nfill = 31: the most that still takes the pair walk, whose rounds stage a prefix of at
    most 4096 pairs each: two rounds with the big boxes in front, and with layout "split" -- 15 big, 1 small, 15 big, 1 small,
    1 big, 31 small -- three, the most any pass can need (tests/test_vis_wave_premises.py has the count)"""
    def fill(j):  # nearer than some of the big triangles, but for the corner that the first sixteen of them show in
        lx, ly = (j * 7) % 16, (j * 5 + j // 16) % 16
        return one_px(BX * BIN + lx, ly, F(250 if lx + ly >= 26 else 60 + (j * 37) % 190, 256))
    tris = [fill(j) for j in range(64 * W)]
    zs = [F(200 - 2 * k, 256) for k in range(64)]
    # a tie between two big triangles that win pixels, in two primitives (so two colours) and two rounds or sixteens of the pass
    for k in (range(27, 31) if layout == "split" else range(31, 35)):
        zs[k] = zs[k - 1]
    big = [_bin_filler(k, zs[k]) for k in range(nfill)]
    small = [fill(1000 + k) for k in range(64 - nfill)]
    if layout == "split":
        assert nfill == 31
        tris += big[:15] + small[:1] + big[15:30] + small[1:2] + big[30:] + small[2:]
    else:
        tris += big + small
    tris += [fill(2000 + j) for j in range(7)]
    return WaveScene(TW, TH, tris)


QX, QY = BX * BIN + 9, 6  # the pixel the order-list scenes stack their fragments on


def _list_scene(nfrag, nearer, h=TH):
    """mixed: nfrag translucent one-pixel fragments on pixel (QX, QY), fragment k in pass k (the last pass is a short one);
    translucent one-pixel filler on the other 255 pixels of the bin in layers -- a second fragment of a pixel is nearer than,
    level with or farther than its first in turn, a third nearer than both -- and one opaque triangle among the filler"""
    zq = [F(200 - 12 * k, 256) if nearer else F(60 + 12 * k, 256) for k in range(nfrag)]
    others = [q for q in range(BIN * BIN) if q != (QY * BIN + QX % BIN)]
    nfill = 63 * (nfrag - 1) + 4

    def filler(j):
        q, layer = others[j % 255], j // 255
        z0 = 150 + (q * 13) % 60
        zl = z0 if layer == 0 else (z0 + (-10, 0, 10)[q % 3] if layer == 1 else z0 - 20)
        return one_px(BX * BIN + q % BIN, q // BIN, F(zl, 256), None if j == 100 else "trans")
    tris, j = [], 0
    for k in range(nfrag):
        n, at = (64, (9 * k + 5) % 64) if k < nfrag - 1 else (5, 3)
        for e in range(n):
            if e == at:
                tris.append(one_px(QX, QY, zq[k], "trans"))
            else:
                tris.append(filler(j))
                j += 1
    assert j == nfill
    return WaveScene(TW, h, tris)


def lists_from_every_wave(W, h=TH):
    """pixel (QX, QY) lists exactly STAIR_K fragments, nearer and nearer, one from each of passes 0..7"""
    return _list_scene(STAIR_K, True, h)


def list_overflow_across_waves(W, nfrag):
    """nfrag > STAIR_K undominated fragments on one pixel, from nfrag passes: the bin is handed to the ordered kernel"""
    return _list_scene(nfrag, True)


def dominated_across_waves(W):
    """12 fragments on one pixel from 12 passes, farther and farther: each is dominated by the first one, if that one was
    seen before it"""
    return _list_scene(12, False)


RESOLVE_TARGETS = ((24, 12), (32, 16))
RESOLVE_KINDS = {False: ("clear", "solid", "texa", "texb"), True: ("clear", "solid", "list1", "list4", "list8")}


def resolve_pairs(w, h, mixed):
    """bin (1, 0) of a w x h target.  With two waves thread t resolves pixels t and t + 128: (lx, ly) and (lx, ly + 8).  The
    j-th such pair of the bin's visible part gets kind j mod n on its first pixel and (j div n) mod n on its second, n kinds:
    every combination.  Submitted layer by layer, so a pixel's fragments come from different passes; a list comes nearer and
    nearer, but for the second and third fragment of a list of four, which are level"""
    kinds = RESOLVE_KINDS[mixed]
    n, vw, vh = len(kinds), min(BIN, w - BIN), min(BIN, h)
    frags = {}
    for ly in range(vh):
        for lx in range(vw):
            j = (ly % 8) * vw + lx
            kind = kinds[j % n] if ly < 8 else kinds[(j // n) % n]
            px, py, q = BIN + lx, ly, ly * BIN + lx
            if kind == "clear":
                continue
            if kind.startswith("list"):
                zs = [F(220 - 20 * l - q % 7, 256) for l in range(int(kind[4:]))]
                if len(zs) == 4:
                    zs[2] = zs[1]
                frags[(px, py)] = [one_px(px, py, z, "trans") for z in zs]
            else:
                frags[(px, py)] = [one_px(px, py, F(60 + q % 100, 256), None if kind == "solid" else kind)]
    # within a layer by material, then by pixel: long runs of one material, so few primitives and few segments in the bin
    order = sorted(frags.items(), key=lambda kv: (str(kv[1][0].mat), kv[0][1], kv[0][0]))
    tris = [f[l] for l in range(STAIR_K) for _, f in order if len(f) > l]
    return WaveScene(w, h, tris, bx=1, by=0)
