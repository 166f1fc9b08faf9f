"""Scenes for the culling model (tests/cull_model.py): every edge of k_cull_instances / k_cull_chunks at the smallest
sizes that reach it.  Numpy only; the draws are dicts in the form of tests/helpers.py (a draw may also carry
``parts_disp``: the model is created with every part shown and the list is applied through set_parts_disp).

Target 320 x 200 = 20 x 13 bins, the last bin row 8 pixels tall.  Every scene is placed so that the model has no
ambiguous decision for any rank of any map in ``configs`` (tests/test_cull_model_premises.py enforces it).

Families
  a  placed edges: quads whose true rectangle edge sits 0.5 px and 1.5 px from every bin line that a band or a
     super-tile of the maps can end on, and from the four edges of the target; as instances of one batch (one-quad and
     two-quad models) and as single models
  b  rows of a wave: strips whose consecutive chunks alternate between two far-apart screen regions, with 1, 15, 16, 17,
     33 and 63 chunks
  c  skinned chunks: 1, 2, 15 and 16 joints per chunk, joints past the palette, a weight quadruple of 254, palettes with
     rotation, shear and scale, a palette whose translation cancels the model matrix's, an unskinnable primitive next
     to skinned ones, 72 joints in use
  d  24 instances against world 4 bands: most straddling, most inside (17 chunks: the mask tail), most outside, and
     the sequence of the straddler hint
  e  what cannot be bounded: behind the camera, NaN / inf in a model or palette matrix, a position of 3e38, a chunk
     without a vertex in range, a clip row down among the subnormals
  f  a hidden middle part
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, List, Optional

import numpy as np

from mt_renderer_amd import scene, sharding
from tests.pixel_scenes import pixel_model, pixel_to_ndc_matrix

W, H = 320, 200
NBX, NBY = 20, 13
WORLDS = (2, 4, 5)
UNEVEN = {2: [0, 0, 13], 4: [0, 5, 5, 9, 13], 5: [0, 2, 2, 7, 10, 13]}  # one band of each is empty
MAPS = (("bands", sharding.BANDS, 0, False), ("bands-uneven", sharding.BANDS, 0, True),
        ("supertiles1", sharding.SUPERTILES, 0, False), ("supertiles4", sharding.SUPERTILES, 2, False))
WORLD1 = "world1"  # one rank owns the target: GEOM_CULL_ALL_FRAMES on an unsharded frame


def shard_of(map_name: str, world: int, rank: int):
    """the tuple Frame.set_shard takes (None for WORLD1)"""
    if map_name == WORLD1:
        return None
    _, own_map, param, uneven = next(m for m in MAPS if m[0] == map_name)
    return (rank, world, own_map, param, UNEVEN[world] if uneven else None)


def configs(all_ranks: bool, map_name: Optional[str] = None):
    """[(map name, world, rank)]: every rank for the placed edges, ranks 0, 1 and the last otherwise"""
    out = []
    for name, *_ in MAPS:
        for world in WORLDS:
            ranks = range(world) if all_ranks else sorted({0, 1, world - 1})
            out += [(name, world, r) for r in ranks]
    out.append((WORLD1, 1, 0))
    return [c for c in out if map_name is None or c[0] == map_name]


MAP_NAMES = tuple(m[0] for m in MAPS) + (WORLD1,)


@dataclasses.dataclass
class Scene:
    name: str
    family: str
    draws: List[dict]
    all_ranks: bool = False
    tags: dict = dataclasses.field(default_factory=dict)


PIX = pixel_to_ndc_matrix(W, H)


def _translate_scale(x, y, sx=1.0, sy=1.0):
    return scene.to_f32_colmajor(scene.mat_translate(x, y, 0.0) @ scene.mat_scale(sx, sy, 1.0))


# ---------------------------------------------------------------------------------------------
# a. placed edges
# ---------------------------------------------------------------------------------------------
def _quad(x0, y0, x1, y1, z=0.5, debug_id=0, parts_no=0):
    return dict(verts=[(x0, y0, z), (x1, y0, z), (x0, y1, z), (x1, y1, z)], indices=[0, 2, 1, 1, 2, 3], topology=scene.TOPO_LIST,
                debug_id=debug_id, parts_no=parts_no)


def placed_quads():
    """[dict(rect=(x0, y0, x1, y1), bins=[(bx, by)] the bins the slack of 1 px lets it reach, border=...)]: 6 x 6 px quads
    0.5 and 1.5 px from bin lines and target edges.  border: ("h", line, side, d), ("v", line, side, d), (edge name, d)"""
    out = []
    for k in range(1, NBY):  # every horizontal bin line: the bands of every world and the super-tile rows end on them
        L, bx = 16.0 * k, (3 * k) % NBX
        xc = 16.0 * bx + 8.0
        for d in (0.5, 1.5):
            out.append(dict(rect=(xc - 3, L - d - 6, xc + 3, L - d), bins=[(bx, k - 1)] + ([(bx, k)] if d == 0.5 else []), border=("h", k, "above", d)))
            out.append(dict(rect=(xc - 3, L + d, xc + 3, L + d + 6), bins=[(bx, k)] + ([(bx, k - 1)] if d == 0.5 else []), border=("h", k, "below", d)))
    for k in (1, 4, 7, 8, 12, 16, 19):  # vertical bin lines: super-tile columns of shift 0 (all) and shift 2 (4, 8, 12, 16)
        L, by = 16.0 * k, (5 * k) % 12
        yc = 16.0 * by + 8.0
        for d in (0.5, 1.5):
            out.append(dict(rect=(L - d - 6, yc - 3, L - d, yc + 3), bins=[(k - 1, by)] + ([(k, by)] if d == 0.5 else []), border=("v", k, "left", d)))
            out.append(dict(rect=(L + d, yc - 3, L + d + 6, yc + 3), bins=[(k, by)] + ([(k - 1, by)] if d == 0.5 else []), border=("v", k, "right", d)))
    for d in (0.5, 1.5):  # off the target: reached again only through the slack
        on = d == 0.5
        out.append(dict(rect=(-d - 6, 37, -d, 43), bins=[(0, 2)] if on else [], border=("target-left", d)))
        out.append(dict(rect=(W + d, 85, W + d + 6, 91), bins=[(NBX - 1, 5)] if on else [], border=("target-right", d)))
        out.append(dict(rect=(101, -d - 6, 107, -d), bins=[(6, 0)] if on else [], border=("target-top", d)))
        out.append(dict(rect=(229, H + d, 235, H + d + 6), bins=[(14, NBY - 1)] if on else [], border=("target-bottom", d)))
    # ends exactly on fx == W and fy == H, in the last bin row (8 px tall: H is no multiple of 16)
    out.append(dict(rect=(300, 190, 320, 200), bins=[(bx, by) for bx in (18, 19) for by in (11, 12)], border=("exact-corner", 0.0)))
    out.append(dict(rect=(40, 193.5, 46, 198.5), bins=[(2, 12)], border=("last-row", 0.0)))
    return out


SINGLE_BORDERS = [("h", 6, "above"), ("h", 6, "below"), ("v", 8, "left"), ("v", 8, "right"),
                  ("target-left",), ("target-right",), ("target-top",), ("target-bottom",)]


def _family_a():
    quads = placed_quads()
    unit = pixel_model([_quad(0, 0, 1, 1)])
    mats = np.stack([_translate_scale(q["rect"][0], q["rect"][1], q["rect"][2] - q["rect"][0], q["rect"][3] - q["rect"][1]) for q in quads])
    batch = dict(md=unit, vp=PIX, model_mats=mats)
    # the two-quad model: quads at y in [0, 1] and [1.5, 2.5] (two primitives = two chunks).  Scaled by 6 its quads lie
    # 1.5 px on either side of a bin line, scaled by 2 they lie 0.5 px on either side of it
    two = pixel_model([_quad(0, 0, 1, 1), _quad(0, 1.5, 1, 2.5, debug_id=1)])
    two_inst, two_mats = [], []
    for k in (3, 6, 9, 12):
        L, bx = 16.0 * k, (7 * k) % NBX
        for sy, d in ((6.0, 1.5), (2.0, 0.5)):
            y0 = L - d - sy
            two_mats.append(_translate_scale(16.0 * bx + 5.0, y0, 6.0, sy))
            two_inst.append(dict(line=k, d=d, bx=bx))
    batch2 = dict(md=two, vp=PIX, model_mats=np.stack(two_mats))
    singles, single_tags = [], []
    for q in quads:
        if q["border"][:-1] in SINGLE_BORDERS:
            singles.append(dict(md=pixel_model([_quad(*q["rect"])]), M=PIX))
            single_tags.append(q)
    L = 96.0
    singles.append(dict(md=pixel_model([_quad(150, L - 7.5, 156, L - 1.5), _quad(150, L + 1.5, 156, L + 7.5, debug_id=1)]), M=PIX))
    singles.append(dict(md=pixel_model([_quad(170, L - 2.5, 176, L - 0.5), _quad(170, L + 0.5, 176, L + 2.5, debug_id=1)]), M=PIX))
    return [Scene("a_batch", "a", [batch, batch2], True, dict(quads=quads, two=two_inst)),
            Scene("a_single", "a", singles, True, dict(quads=single_tags))]


# ---------------------------------------------------------------------------------------------
# strips of whole chunks: 60 positions that cycle through the chunk's vertices, then two restarts, so that the two
# positions a chunk takes from before its start hold no vertex of the previous chunk
# ---------------------------------------------------------------------------------------------
def _chunk_indices(vertex_lists, tail: Optional[int] = None):
    idx = []
    for k, vl in enumerate(vertex_lists):
        n = 60 if (tail is None or k + 1 < len(vertex_lists)) else tail
        idx += [vl[i % len(vl)] for i in range(n)] + [0xFFFF, 0xFFFF]
    return idx


REGION_A, REGION_B = (18.0, 18.0), (210.0, 162.0)  # bins (1, 1) and (13, 10)


def alternating_strip(nchunks: int, debug_id=0, parts_no=0, regions=(REGION_A, REGION_B)):
    verts, lists = [], []
    for k in range(nchunks):
        ox, oy = regions[k % 2]
        x0, y0 = ox + (k % 4), oy + (k % 3)
        lists.append(list(range(len(verts), len(verts) + 4)))
        verts += [(x0, y0, 0.5), (x0 + 6, y0, 0.5), (x0, y0 + 6, 0.5), (x0 + 6, y0 + 6, 0.5)]
    return dict(verts=verts, indices=_chunk_indices(lists), topology=scene.TOPO_STRIP, debug_id=debug_id, parts_no=parts_no)


B_COUNTS = (1, 15, 16, 17, 33, 63)


def _family_b():
    models = {n: pixel_model([alternating_strip(n, debug_id=i)]) for i, n in enumerate(B_COUNTS)}
    singles = [dict(md=models[n], M=PIX) for n in B_COUNTS]
    # as instances (the composites come from k_cull_instances): at home, moved by whole bins, and off the target
    mats = np.stack([_translate_scale(0, 0), _translate_scale(48, -16), _translate_scale(-400, 0), _translate_scale(-16, 16)])
    batches = [dict(md=models[n], vp=PIX, model_mats=mats) for n in (17, 63)]
    return [Scene("b_single", "b", singles), Scene("b_batch", "b", batches)]


# ---------------------------------------------------------------------------------------------
# c. skinned chunks
# ---------------------------------------------------------------------------------------------
SKIN_LAYOUT = [(scene.SEM_POSITION, scene.IEF_F32, 3, 0), (scene.SEM_TEXCOORD, scene.IEF_F16, 2, 12),
               (scene.SEM_JOINT, scene.IEF_U8, 4, 16), (scene.SEM_WEIGHT, scene.IEF_U8N, 4, 20)]
RIGID_LAYOUT = [(scene.SEM_POSITION, scene.IEF_F32, 3, 0), (scene.SEM_TEXCOORD, scene.IEF_F16, 2, 12)]
DIST = 2.3
VP = scene.to_f32_colmajor(scene.reference_view_proj(W, H))
BASE = (-5.0, 0.0, 1.0 - DIST)  # in front of the reference camera: 1 unit is about 93 px


def skinned_model(prims) -> scene.ModelData:
    """prims: [dict(chunks=[(pos [n,3], joints [n,4] | None, weights [n,4] | None)], parts_no)]: one strip primitive
    each, one chunk per entry; a primitive whose chunks carry no joints has no joint / weight elements at all"""
    vbs, ibs, recs, lays = [], [], [], []
    vbase = iofs = 0
    for p in prims:
        rigid = p["chunks"][0][1] is None
        stride = 16 if rigid else 24
        pos = np.concatenate([np.asarray(c[0], dtype=np.float32).reshape(-1, 3) for c in p["chunks"]])
        vb = np.zeros((len(pos), stride), dtype=np.uint8)
        vb[:, 0:12] = np.ascontiguousarray(pos).view(np.uint8).reshape(-1, 12)
        if not rigid:
            vb[:, 16:20] = np.concatenate([np.asarray(c[1], dtype=np.uint8).reshape(-1, 4) for c in p["chunks"]])
            vb[:, 20:24] = np.concatenate([np.asarray(c[2], dtype=np.uint8).reshape(-1, 4) for c in p["chunks"]])
        lists, v0 = [], 0
        for c in p["chunks"]:
            n = len(np.asarray(c[0]).reshape(-1, 3))
            lists.append(list(range(v0, v0 + n)))
            v0 += n
        ib = np.array(_chunk_indices(lists), dtype=np.uint16)
        recs.append(scene.pack_primitive(vertex_num=len(pos), parts_no=p.get("parts_no", 0), weight_num=0 if rigid else 4, vertex_stride=stride,
                                         topology=scene.TOPO_STRIP, vertex_base=vbase, index_ofs=iofs, index_num=len(ib)))
        vbs.append(vb.reshape(-1)); ibs.append(ib); lays.append(list(RIGID_LAYOUT if rigid else SKIN_LAYOUT))
        vbase += vb.size
        iofs += len(ib)
    n = len(prims)
    return scene.ModelData(vertex_buf=np.concatenate(vbs), index_buf=np.concatenate(ibs), prims=np.stack(recs), layouts=lays,
                           prim_to_texture=np.full(n, -1, dtype=np.int32), prim_debug_id=np.arange(n, dtype=np.uint32),
                           parts_disp=np.ones(n, dtype=np.uint8))


def _cluster(rng, n=20, r=0.03):
    return rng.uniform(-r, r, size=(n, 3)).astype(np.float32)


def _one_joint(rng, j, n=20):
    jw = np.zeros((n, 4), dtype=np.uint8); ww = np.zeros((n, 4), dtype=np.uint8)
    jw[:, 0] = j; jw[:, 1:] = rng.integers(0, 256, size=(n, 3))  # slots of weight 0 name any joint: they do not count
    ww[:, 0] = 255
    return _cluster(rng, n), jw, ww


def _many_joints(rng, joints, n=None):
    """every vertex blends two to four of `joints`, all of them used by some vertex with a nonzero weight"""
    joints = list(joints)
    n = n or max(20, len(joints))
    jw = np.zeros((n, 4), dtype=np.uint8); ww = np.zeros((n, 4), dtype=np.uint8)
    for v in range(n):
        k = min(len(joints), 2 + v % 3)
        jw[v, :k] = [joints[(v + t) % len(joints)] for t in range(k)]
        w = np.full(k, 255 // k, dtype=np.int64)
        w[0] += 255 - w.sum()
        d = int(rng.integers(0, 255 // k - 1))
        w[0] -= d
        w[1] += d
        ww[v, :k] = w
    return _cluster(rng, n), jw, ww


def grid_palette(seed, npal, spots=None, shift=(0.0, 0.0, 0.0)) -> np.ndarray:
    """joint j sends the origin to spot j of a 6-column grid over the frame (or to spots[j]) through a linear part with
    rotation, shear and scale 0.6..1.5; `shift` is added to every translation"""
    rng = np.random.default_rng(seed)
    pal = np.zeros((npal, 16), dtype=np.float32)
    for j in range(npal):
        A = np.eye(4)
        sh = np.eye(3); sh[0, 1] = rng.uniform(-0.4, 0.4); sh[1, 2] = rng.uniform(-0.4, 0.4)
        A[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0] @ sh @ np.diag(rng.uniform(0.6, 1.5, size=3))
        t = spots[j] if spots is not None else (-1.25 + 0.5 * (j % 6), -0.78 + 0.52 * ((j // 6) % 4), 0.0)
        A[:3, 3] = np.asarray(t, dtype=np.float64) + np.asarray(shift, dtype=np.float64)
        pal[j] = scene.to_f32_colmajor(A)
    return pal


def _at(dx=0.0, dy=0.0, dz=0.0, shift=(0.0, 0.0, 0.0)):
    return scene.to_f32_colmajor(scene.mat_translate(BASE[0] + dx + shift[0], BASE[1] + dy + shift[1], BASE[2] + dz + shift[2]))


NPAL_C = 24


def _build_chunks(specs, seed, tries=()):
    """specs: [("one", joint) | ("many", joints[, n]) | ("rigid", (dx, dy))]; chunk i draws from a generator of its own,
    seeded by (seed, i, tries[i]): tries moves single chunks until no decision about them is ambiguous"""
    out = []
    for i, sp in enumerate(specs):
        rng = np.random.default_rng([seed, i, tries[i] if i < len(tries) else 0])
        if sp[0] == "one":
            out.append(_one_joint(rng, sp[1]))
        elif sp[0] == "many":
            out.append(_many_joints(rng, sp[1], *sp[2:]))
        else:
            out.append((_cluster(rng) + np.float32([sp[1][0], sp[1][1], 0.0]), None, None))
    return out


C_MAIN = ([("one", j) for j in (0, 3, 5, 6, 8, 11, 12, 14, 17, 18, 21, 23)]
          + [("many", (j, j + 1)) for j in (0, 2, 7, 9, 13, 20)]                   # neighbours on the grid
          + [("many", range(0, 15)), ("many", range(9, 24))]                       # 15 joints: a full row of lanes
          + [("many", range(0, 16)), ("many", range(8, 24))]                       # 16: over MTR_CHUNK_MAX_BOXES, kept
          + [("one", 100), ("one", 255), ("many", (22, 200))])                     # past the palette: clamped to 23
C_MIXED = [("one", j) for j in (1, 4, 9, 16, 19, 22)] + [("many", (10, 11))]
C_RIGID = [("rigid", d) for d in ((-1.1, 0.6), (0.9, -0.6), (0.1, 0.1), (1.2, 0.7))]
C_72 = [("many", range(12 * k, 12 * k + 12), 24) for k in range(6)]
# which draw of its generator each chunk takes: raised, chunk by chunk, until the model had no ambiguous decision about
# that chunk in any draw, rank and map that uses it (a chunk that never appears here keeps its first draw)
TRIES = dict(main=(0, 0, 0, 0, 20, 0, 0, 1, 0, 1, 0, 0, 0, 0, 26, 1, 3), m254=(0, 0, 0, 0, 0, 0, 0, 0, 0, 1), mixed=(0, 0, 1), rigid=(), m72=())
SUM254_CHUNK, SUM254_VERTEX = 3, 7


def _c_models(tries=None):
    t = tries or TRIES
    main = skinned_model([dict(chunks=_build_chunks(C_MAIN, 2024, t["main"]))])
    ch = _build_chunks(C_MAIN, 2025, t["m254"])
    p, jw, ww = ch[SUM254_CHUNK]
    ww = ww.copy(); ww[SUM254_VERTEX, 0] = 254
    ch[SUM254_CHUNK] = (p, jw, ww)
    m254 = skinned_model([dict(chunks=ch)])
    mixed = skinned_model([dict(chunks=_build_chunks(C_MIXED, 2026, t["mixed"])), dict(chunks=_build_chunks(C_RIGID, 2027, t["rigid"]))])
    m72 = skinned_model([dict(chunks=_build_chunks(C_72, 2028, t["m72"]))])
    return dict(main=main, m254=m254, mixed=mixed, m72=m72)


def _family_c(tries=None):
    mods = _c_models(tries)
    main, m254, mixed, m72 = mods["main"], mods["m254"], mods["mixed"], mods["m72"]
    pal0, pal1 = grid_palette(1, NPAL_C), grid_palette(2, NPAL_C)
    far = (512.0, 0.0, 0.0)
    pal_far = grid_palette(3, NPAL_C, shift=(-far[0], -far[1], -far[2]))  # cancels the model matrix of its instance
    far2 = (0.0, -1024.0, 0.0)
    pal_far2 = grid_palette(4, NPAL_C, shift=(-far2[0], -far2[1], -far2[2]))
    M = scene.to_f32_colmajor(scene.reference_view_proj(W, H) @ scene.mat_translate(*BASE))
    M_far = scene.to_f32_colmajor(scene.reference_view_proj(W, H) @ scene.mat_translate(BASE[0] + far[0], BASE[1] + far[1], BASE[2] + far[2]))
    M_far2 = scene.to_f32_colmajor(scene.reference_view_proj(W, H) @ scene.mat_translate(BASE[0] + far2[0], BASE[1] + 0.5 + far2[1], BASE[2] + far2[2]))
    mats = np.stack([_at(), _at(0.3, -0.45), _at(shift=far), _at(0.0, 0.5, shift=far2), _at(0.0, 2.6)])
    pals = np.stack([pal0, pal1, pal_far, pal_far2, pal1])
    # 72 joints in use: the instance test loops past 64 boxes.  Joints 0..63 sit in a patch at the top, 64..71 at the
    # bottom: an instance test that forgot the last eight would call the instance inside the upper band
    spots = [(-0.5 + 0.14 * (j % 8), 0.95 - 0.05 * (j // 8), 0.0) if j < 64 else (-0.5 + 0.14 * (j % 8), -0.8, 0.0) for j in range(72)]
    pal72 = grid_palette(5, 72, spots=spots)
    for j in range(72):  # small linear parts: the patches stay patches
        pal72[j].reshape(4, 4)[:3, :3] *= np.float32(0.5)
    mats72 = np.stack([_at(), _at(0.9, 0.0), _at(-0.8, 0.45), _at(0.0, 3.0)])
    return [Scene("c_single", "c", [dict(md=main, M=M, palette=pal0), dict(md=main, M=M, palette=pal1),
                                    dict(md=m254, M=M, palette=pal0), dict(md=mixed, M=M, palette=pal1),
                                    dict(md=m72, M=M, palette=pal72),
                                    dict(md=main, M=M_far, palette=pal_far), dict(md=main, M=M_far2, palette=pal_far2)]),
            Scene("c_batch", "c", [dict(md=main, vp=VP, model_mats=mats, palettes=pals),
                                   dict(md=m254, vp=VP, model_mats=mats[:2], palettes=pals[:2]),
                                   dict(md=mixed, vp=VP, model_mats=mats[:2], palettes=pals[:2]),
                                   dict(md=m72, vp=VP, model_mats=mats72, palettes=np.stack([pal72] * 4))])]


# ---------------------------------------------------------------------------------------------
# d. instances against world 4 bands (rows 0, 3, 6, 9, 13: rank 1 owns pixel rows 48..95)
# ---------------------------------------------------------------------------------------------
D_WORLD, D_RANK, D_NINST, D_NCHUNKS = 4, 1, 24, 17


def column_model():
    """17 chunks stacked in a column 34 px tall: chunk k is a 6 x 2 px quad at y = 2 k"""
    verts, lists = [], []
    for k in range(D_NCHUNKS):
        lists.append(list(range(len(verts), len(verts) + 4)))
        verts += [(0, 2.0 * k, 0.5), (6, 2.0 * k, 0.5), (0, 2.0 * k + 2, 0.5), (6, 2.0 * k + 2, 0.5)]
    return pixel_model([dict(verts=verts, indices=_chunk_indices(lists), topology=scene.TOPO_STRIP)])


def _column_mats(tops):
    return np.stack([_translate_scale(10.0 + 12.0 * i, y) for i, y in enumerate(tops)])


def d_variants():
    """instance tops (pixel row of the column's first chunk) per variant; the band of rank 1 is [48, 96)"""
    inside = [50.4 + (i % 5) * 2.0 for i in range(D_NINST)]            # rows 49.4 .. 93.4 with the slack
    straddle = [30.4 + (i % 7) * 2.0 if i % 2 else 70.4 + (i % 7) * 2.0 for i in range(D_NINST)]
    outside = [4.4 + (i % 3) * 2.0 if i % 2 else 110.4 + (i % 9) * 6.0 for i in range(D_NINST)]
    v1 = list(straddle); v1[0], v1[1], v1[2] = inside[0], outside[0], outside[1]
    v2 = list(inside); v2[3], v2[10], v2[17], v2[20] = 30.4, 80.4, 4.4, 140.4
    v3 = list(outside); v3[2], v3[9], v3[14] = 40.4, 55.4, 88.4
    few = list(inside); few[4], few[15] = 33.4, 77.4                    # two straddlers ...
    for i in range(16, 24):
        few[i] = 120.4 + i                                               # ... and some instances outside
    many = list(straddle); many[5], many[6], many[11], many[12] = inside[5], inside[6], 150.4, 160.4  # 20 straddlers
    return dict(straddle=v1, inside=v2, outside=v3, seq_few=few, seq_many=many)


def _family_d():
    md = column_model()
    v = d_variants()
    draws = [dict(md=md, vp=PIX, model_mats=_column_mats(v[k])) for k in ("straddle", "inside", "outside")]
    seq = [dict(md=md, vp=PIX, model_mats=_column_mats(v[k])) for k in ("seq_few", "seq_many")]
    return [Scene("d_batch", "d", draws), Scene("d_sequence", "d", seq)]


# ---------------------------------------------------------------------------------------------
# e. what cannot be bounded
# ---------------------------------------------------------------------------------------------
def _family_e(tries=None):
    slab = pixel_model([dict(verts=[(-0.1, -0.1, -0.05), (0.1, -0.1, -0.05), (-0.1, 0.1, 0.05), (0.1, 0.1, 0.05)],
                             indices=[0, 1, 2, 2, 1, 3], topology=scene.TOPO_LIST)])
    behind = np.stack([_at(), _at(0.4, 0.5), _at(dz=DIST + 2.0), _at(dz=DIST), _at(5.0, 0.0), _at(-0.6, -0.7)])  # 2: behind, 3: through w = 0
    bad = behind.copy()
    bad[0, 5] = np.nan          # a NaN in one model matrix
    bad[1, 12] = np.inf         # an infinity in another
    bad[2] = _at(0.8, -0.3)
    main = _c_models(tries)["main"]
    pal0 = grid_palette(1, NPAL_C)
    pals = np.stack([pal0, pal0, pal0, pal0])
    pals[1, 5, 13] = np.nan     # joint 5 of instance 1
    pals[2, 12, 0] = np.inf     # joint 12 of instance 2
    pmats = np.stack([_at(), _at(0.2, 0.3), _at(-0.3, -0.4), _at(0.0, 2.6)])
    strip = alternating_strip(3)
    strip["verts"][5] = (3e38, strip["verts"][5][1], 0.5)  # one position of chunk 1
    huge = pixel_model([strip])
    nobox = alternating_strip(4)
    nobox["indices"] = [i if not (62 <= q < 122) else 60000 for q, i in enumerate(nobox["indices"])]  # chunk 1: nothing in range
    nobox = pixel_model([nobox])
    two = np.stack([_translate_scale(0, 0), _translate_scale(32, -16)])
    # a clip row whose magnitudes lie below 2^-100: the relative margin does not cover subnormal rounding, nothing is bounded
    tiny = pixel_model([alternating_strip(2)])
    tiny_M = PIX.copy()
    tiny_M[0::4] *= np.float32(2.0 ** -110)
    return [Scene("e_unboundable", "e", [dict(md=slab, vp=VP, model_mats=behind), dict(md=slab, vp=VP, model_mats=bad),
                                         dict(md=main, vp=VP, model_mats=pmats, palettes=pals),
                                         dict(md=huge, M=PIX), dict(md=huge, vp=PIX, model_mats=two),
                                         dict(md=nobox, M=PIX), dict(md=nobox, vp=PIX, model_mats=two),
                                         dict(md=tiny, M=tiny_M)])]


# ---------------------------------------------------------------------------------------------
# f. a hidden middle part
# ---------------------------------------------------------------------------------------------
def _family_f():
    regs = [((18.0, 18.0), (100.0, 18.0)), ((60.0, 100.0), (250.0, 100.0)), ((18.0, 178.0), (210.0, 150.0))]
    make = lambda: pixel_model([alternating_strip(n, debug_id=p, parts_no=p, regions=regs[p]) for p, n in enumerate((3, 5, 4))])
    md, whole = make(), make()  # a model object of its own for the draw that shows every part
    shown = [1, 0, 1]
    two = np.stack([_translate_scale(0, 0), _translate_scale(16, -48)])
    return [Scene("f_hidden_part", "f", [dict(md=md, M=PIX, parts_disp=shown), dict(md=md, vp=PIX, model_mats=two, parts_disp=shown),
                                         dict(md=whole, M=PIX)])]


@functools.lru_cache(maxsize=None)
def scenes() -> Dict[str, Scene]:
    out = {}
    for fam in (_family_a, _family_b, _family_c, _family_d, _family_e, _family_f):
        for s in fam():
            out[s.name] = s
    return out


FAMILIES = ("a", "b", "c", "d", "e", "f")
