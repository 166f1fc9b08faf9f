"""Scenes for the deferred-clip path of the geometry stage (k_geom defers a chunk with a triangle to clip, k_geom_clip runs
it), and a float64 model of what they rely on: which chunks of a strip mesh hold a triangle to clip, and how many
vertices a clipped triangle keeps.

The positions are (x, y, w) under M_W: clip = (x, y, 0.25 w, w).  A vertex with w < 0 lies behind the near plane (z < 0);
one with w > 0 whose x / w or y / w leaves +-2^20 px cannot be projected and is clipped against the guard band
|x| <= 64 w, |y| <= 64 w (SPEC.md 5.3).  Every product is exact in binary32 and every premise is far from its threshold, so
float64 decides them as the GPU does."""
from __future__ import annotations

import numpy as np

from mt_renderer_amd import scene
from tests.pixel_scenes import pixel_model

M_W = scene.to_f32_colmajor(np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0.25, 0], [0, 0, 1, 0]], dtype=np.float64))
CHUNK_NEW = 62      # strip positions per geometry chunk (MTR_CHUNK_NEW)
CHUNK_SLOTS = 124   # records a chunk may hold (MTR_CHUNK_SLOTS)
GUARD_PX = 1048576.0
TWO_SIDED = (0, 1, 1, 1)        # alpha blend (debug colours have alpha 1), depth write, depth test, cull none
TRANSLUCENT_ORDERED = (0, 0, 1, 1)  # alpha blend without depth write: every fragment's order counts (the ordered tile kernel's)


def grid(strips, cols, w_of=None, xs=None, ys=None, did=3, uv=False, texture=-1):
    """One primitive: `strips` triangle strips of `cols` quads joined by restarts (scene._strip_indices), vertex (r, c) at
    (xs[c], ys[r]) * w with w = w_of(r, c) (default 1): its screen position does not depend on w."""
    xs = np.linspace(-0.8, 0.8, cols + 1) if xs is None else np.asarray(xs, dtype=np.float64)
    ys = np.linspace(-0.6, 0.6, strips + 1) if ys is None else np.asarray(ys, dtype=np.float64)
    verts = []
    for r in range(strips + 1):
        for c in range(cols + 1):
            w = 1.0 if w_of is None else float(w_of(r, c))
            v = (float(xs[c]) * w, float(ys[r]) * w, w)
            verts.append(v + (c / cols, r / strips) if uv else v)
    return dict(verts=verts, indices=scene._strip_indices(strips, cols), topology=scene.TOPO_STRIP, debug_id=did, texture=texture)


def model(prims, textures=None, state=None):
    md = pixel_model(prims, textures)
    md.scene_prims = prims  # for the premises
    if state is not None:
        md.prim_states = np.array([state] * md.nprims, dtype=np.uint8)
    return md


# ---- the float64 model ----
def _strip_triangles(indices):
    """(position that completes it, (ia, ib, ic)) for every triangle of a strip with restarts, in strip order"""
    out, run = [], 0
    for p, i in enumerate(indices):
        if i == 0xFFFF:
            run = 0
            continue
        run += 1
        if run >= 3:
            a, b, c = int(indices[p - 2]), int(indices[p - 1]), int(i)
            out.append((p, (a, c, b) if (run - 3) & 1 else (a, b, c)))
    return out


def _projectable(v, w, h):
    x, y, ww = v
    if not ww > 0.0:
        return False
    return abs(x / ww * 0.5 * w + 0.5 * w) <= GUARD_PX and abs(-y / ww * 0.5 * h + 0.5 * h) <= GUARD_PX


def needs_clip(tri, w, h):
    """tri: three (x, y, w) positions under M_W.  None: trivially rejected; else whether the geometry stage clips it"""
    planes = [lambda v: v[0] < -v[2], lambda v: v[0] > v[2], lambda v: v[1] < -v[2], lambda v: v[1] > v[2], lambda v: 0.25 * v[2] < 0.0,
              lambda v: 0.25 * v[2] > v[2]]
    if any(all(pl(v) for v in tri) for pl in planes):
        return None
    return any(v[2] < 0.0 for v in tri) or not all(_projectable(v, w, h) for v in tri)


def chunks_that_clip(prim, w, h):
    """(chunks of the primitive, the set of those that hold a triangle to clip)"""
    verts = np.asarray(prim["verts"], dtype=np.float64)[:, :3]
    idx = np.asarray(prim["indices"])
    clip = set()
    for p, t in _strip_triangles(idx):
        if needs_clip([verts[i] for i in t], w, h):
            clip.add(p // CHUNK_NEW)
    return (len(idx) + CHUNK_NEW - 1) // CHUNK_NEW, clip


def clipped_polygon(tri):
    """Sutherland-Hodgman of one triangle against the near plane (w >= 0 under M_W), then the four guard-band planes"""
    poly = [np.asarray(v, dtype=np.float64) for v in tri]
    dists = [lambda v: v[2], lambda v: 64.0 * v[2] - v[0], lambda v: 64.0 * v[2] + v[0], lambda v: 64.0 * v[2] - v[1], lambda v: 64.0 * v[2] + v[1]]
    for d in dists:
        out = []
        for i, p in enumerate(poly):
            q = poly[(i + 1) % len(poly)]
            dp, dq = d(p), d(q)
            if dp >= 0.0:
                out.append(p)
            if (dp >= 0.0) != (dq >= 0.0):
                out.append(p + (q - p) * (dp / (dp - dq)))
        poly = out
        if len(poly) < 3:
            return []
    return poly


def fan_slots(prim, w, h):
    """record slots each chunk of the primitive reserves at most: a guard-clipped triangle one per fan triangle (its
    polygon's vertices - 2, culled or not), any other at most two (a near-clipped quad)"""
    verts = np.asarray(prim["verts"], dtype=np.float64)[:, :3]
    slots = {}
    for p, t in _strip_triangles(np.asarray(prim["indices"])):
        tri = [verts[i] for i in t]
        nc = needs_clip(tri, w, h)
        if nc is None:
            continue
        n = 1
        if nc:
            poly = clipped_polygon(tri)
            n = max(len(poly) - 2, 0)
        slots[p // CHUNK_NEW] = slots.get(p // CHUNK_NEW, 0) + n
    return slots


# ---- the scenes ----
W, H = 128, 96
BEHIND = -0.5  # w of a vertex behind the near plane


def one_vertex_behind(ordered=False):
    """2 strips x 40 columns = 165 strip positions = 3 chunks; the vertex (2, 0) -- the first of strip 1, in one triangle
    only, which chunk 1 owns -- lies behind the near plane: one lane of chunk 1 clips, its other lanes are ordinary.
    ordered: a translucent texture without depth write, the columns folded over each other (column c at x[c mod 21]) and
    the strips too, so that triangles of one chunk overlap and their order decides the pixel; the vertex behind the
    near plane is (2, 12), in the middle of chunk 1's overlap."""
    if not ordered:
        return model([grid(2, 40, lambda r, c: BEHIND if (r, c) == (2, 0) else 1.0)], state=TWO_SIDED)
    xs = np.linspace(-0.8, 0.8, 21)[np.arange(41) % 21]
    g = grid(2, 40, lambda r, c: BEHIND if (r, c) == (2, 12) else 1.0, xs=xs, ys=[-0.5, 0.4, -0.2], uv=True, texture=0)
    return model([g], [scene.checker_rgba8_texture(16, 16, cell=2, alpha=(255, 120))], state=TRANSLUCENT_ORDERED)


# A, B in front of the eye and inside the guard band, C behind it: what is left in front of the near plane runs off to
# infinity, and the guard band cuts it to seven vertices (clipped_polygon; found by search, rounded)
FAN_TRIANGLE = [(64.5, 50.75, 1.0), (12.25, -62.5, 1.0), (-112.25, 10.5, -1.0)]
# every vertex in front of the eye (w = 1): A and B just outside the guard-band square, C 70 000 NDC units out on the diagonal,
# 4.5 million pixels from the target and so not projectable.  The long edges pass 75 units from the centre on either side
# and cut two corners of the square, the short edge AB a third: seven vertices again, without the near plane
FAN_TRIANGLE_OUT_OF_BAND = [(0.0, 106.0, 1.0), (-106.0, 0.0, 1.0), (70000.0, -70000.0, 1.0)]


def fan_after_a_grid(tri=FAN_TRIANGLE):
    """the grid of one_vertex_behind, nothing of it clipped, and after a restart one more triangle: FAN_TRIANGLE, in the
    last chunk behind ordinary lanes.  Textured (opaque): a fan triangle in the wrong slot shows."""
    g = grid(2, 40, uv=True, texture=0)
    n = len(g["verts"])
    g["verts"] = g["verts"] + [tuple(v) + (0.1 + 0.4 * k, 0.9 - 0.3 * k) for k, v in enumerate(tri)]
    g["indices"] = np.concatenate([g["indices"], np.array([0xFFFF, n, n + 1, n + 2], dtype=np.uint16)])
    return model([g], [scene.checker_rgba8_texture(16, 16, cell=2)], state=TWO_SIDED)


def fans_that_overflow():
    """a strip between two far ends, 10^6 NDC units out on the diagonal, that turns by 150 / 10^6 rad per step: every
    triangle is a sliver whose long edges pass 75 units from the centre on either side, normal to the other diagonal --
    they cut two opposite corners off the guard-band square (corner distance 64 sqrt 2 = 90.5): six vertices, four fan
    triangles for each of the 60 triangles of chunk 0, 240 slots where 124 fit"""
    R, eps = 1.0e6, 150.0 / 1.0e6
    verts = [(R * np.cos(np.pi / 4 + i * (np.pi - eps)), R * np.sin(np.pi / 4 + i * (np.pi - eps)), 1.0) for i in range(66)]
    return model([dict(verts=verts, indices=list(range(66)), topology=scene.TOPO_STRIP, debug_id=2)], state=TWO_SIDED)


def every_chunk_clips(strips=2, cols=40):
    """the odd rows have a vertex behind the near plane every eighth column: no chunk (31 columns) without one"""
    return model([grid(strips, cols, lambda r, c: BEHIND if (r & 1) and c % 8 == 4 else 1.0)], state=TWO_SIDED)


def nothing_clips():
    return model([grid(2, 40)], state=TWO_SIDED)


def lattice_mats(nx, ny):
    """model matrices that shrink a grid() into cell (i, j) of an nx x ny lattice and keep w: the offset multiplies the
    third position component, which IS w, so every vertex moves by the same amount on the screen whatever its w, and an
    instance clips the chunks the model clips"""
    mats = np.zeros((nx * ny, 16), dtype=np.float32)
    for k in range(nx * ny):
        i, j = k % nx, k // nx
        m = np.eye(4)
        m[0, 0], m[1, 1] = 0.9 / nx, 0.9 / ny
        m[0, 2], m[1, 2] = -1.0 + (2 * i + 1) / nx, -1.0 + (2 * j + 1) / ny
        mats[k] = scene.to_f32_colmajor(m)
    return mats


def skinned_batch_two_of_four_clip(w, h):
    """four instances of a skinned capsule (8 x 20: 6 chunks), each with its own palette: instances 1 and 3 stand a quarter
    of a unit in front of the reference camera, which is then inside them (radius 0.35: the near plane cuts through),
    instances 0 and 2 two units away to its left and right"""
    md = scene.skinned_capsule_model([((0.0, 0.0, 0.0), 0.35, 1.6)], rows=8, cols=20)
    places = [(-5.6, 0.0, -1.0), (-5.0, 0.0, 0.75), (-4.4, 0.0, -1.0), (-5.05, 0.1, 0.8)]
    mats = np.stack([scene.to_f32_colmajor(scene.mat_translate(*p)) for p in places])
    pals = np.stack([scene.bone_palette(64, t=0.25 + 0.9 * k) for k in range(4)])
    vp = scene.to_f32_colmajor(scene.reference_view_proj(w, h))
    return dict(md=md, vp=vp, model_mats=mats, palettes=pals)
