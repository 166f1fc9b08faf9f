"""A float64 model of geometry culling (k_cull_instances, k_cull_chunks, geom_cull.h, build_bounds), numpy only.

Written from the header comment of csrc/geom_cull.h and DESIGN.md section 4 as the specification; nothing is imported
from csrc and no GPU is needed.  For one draw (a dict in the form of tests/helpers.py), one frame size and one rank of one
ownership map it predicts how many chunks the rank culls -- the frame's ``chunks_culled`` when the draw is alone in it.

What is modelled
  * chunks: runs of 62 index positions per primitive, every chunk after the first also taking the two positions before
    its start; restart indices of strips and indices past vertex_num are skipped; only displayed parts produce chunks,
    and a chunk's box is that of its position in the model with every part shown;
  * boxes: per chunk one box of all its vertices, then one per joint that carries a nonzero weight byte; flag
    "unbounded" when a weight quadruple does not sum to 255 or more than 15 joints are used; centre rounded to binary32,
    half extent rounded up one binary32 step; a position that is not finite (|p| >= 3e38, the library's threshold for
    "cannot be bounded") gives an infinite extent; the instance boxes of the whole model likewise;
  * the interval of a box under C = M [P_j; 0 0 0 1] for clip x, y, w: v = (C (c,1)), rad = |C| e,
    m = 2^-16 (|M| |P_j| (|c| + e, 1)) -- infinite where that sum of magnitudes is below 2^-100, since the bound is a
    relative one and does not hold among the subnormals --, the joint clamped to npal - 1, the whole box going with M
    alone;
  * the screen rectangle: interval division when w_lo > 0, fx = sx W/2 + W/2, fy = H/2 - sy H/2, a slack of
    1 + 2^-20 max|f| on each side, "off the target" = fx_hi < 0 or fx_lo > W (same in y), else clamped to the bins;
    w_lo <= 0 or anything not finite means "kept";
  * ownership by brute force over sharding.owner_map (plus the documented concession for super-tiles and interleaved
    bins: narrower than `world` cells and more than 8 cell rows tall is kept), "all inside" for bands (every bin row of
    the rectangle is the rank's), for world 1 (the rectangle with its slack lies on the target) and never otherwise;
  * the decision structure: a boundable batch draw tests the instance first (culled: all its chunks count; inside:
    none; straddler: chunk by chunk), everything else goes chunk by chunk.

The certainty band
  The model does not try to reproduce the kernel's binary32 rounding.  It evaluates every rectangle twice: R_in with the
  margin m * 3/4 and the slack reduced by 1/16 px, R_out with m * 5/4 and the slack increased by 1/16 px.  Why a correct
  kernel's rectangle lies between the two:
    * the kernel's binary32 evaluation of v +- rad and of the composites C, |M||P| is about 20 operations at 2^-24,
      each relative to a partial sum of the same magnitudes that make up mag: it differs from the real value by at most
      about 2^-20 mag = m / 16, a quarter of the m / 4 the band allows;
    * its divisions, the viewport multiply-add and the cast differ from the real values by a few 2^-24 |f|: under
      2^-11 px for |f| < 2048 px, a hundredth of the 1/16 px the band allows (the 2^-20 |f| term of the slack itself is
      reproduced, not absorbed).
  So a correct kernel has a factor of four to spare on either side.  A chunk or instance whose decision differs between
  R_in and R_out is *ambiguous*; the scenes of tests/cull_scenes.py are placed so that none is
  (tests/test_cull_model_premises.py), and then culled_lo == culled_hi is the number the GPU must report.
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional

import numpy as np

from mt_renderer_amd import scene, sharding
from tests import vertex_edge_cases as vx

CHUNK_NEW = 62          # MTR_CHUNK_NEW
CHUNK_MAX_BOXES = 15    # MTR_CHUNK_MAX_BOXES
BIN_SHIFT = 4
NOT_FINITE = float(np.float32(3.0e38))  # at or above this the library treats a number as not finite
M_REL = 2.0 ** -16
MIN_MAG = 2.0 ** -100       # MTR_CULL_MIN_MAG: below it a coordinate is not bounded (infinite margin)
SLACK_PX = 1.0
SLACK_REL = 2.0 ** -20
BAND_M = (0.75, 1.25)
BAND_SLACK = (-1.0 / 16.0, 1.0 / 16.0)

CULLED, INSIDE, STRADDLE, KEPT = "culled", "inside", "straddle", "kept"


# ---------------------------------------------------------------------------------------------
# boxes
# ---------------------------------------------------------------------------------------------
class _Acc:
    """running box of binary32 points, kept in float64"""

    def __init__(self):
        self.lo = np.full(3, np.inf)
        self.hi = np.full(3, -np.inf)
        self.any = False
        self.bad = False

    def add(self, p):
        p = np.asarray(p, dtype=np.float64)
        if not (np.abs(p) < NOT_FINITE).all():  # false for NaN too
            self.bad = True
        with np.errstate(invalid="ignore"):
            self.lo = np.fmin(self.lo, p)
            self.hi = np.fmax(self.hi, p)
        self.any = True

    def merge(self, o):
        if not o.any:
            return
        self.lo = np.fmin(self.lo, o.lo)
        self.hi = np.fmax(self.hi, o.hi)
        self.any = True
        self.bad = self.bad or o.bad

    def box(self, joint):
        with np.errstate(all="ignore"):
            c = ((self.lo + self.hi) * 0.5).astype(np.float32)
            ext = np.maximum(self.hi - c.astype(np.float64), c.astype(np.float64) - self.lo)
            e = np.nextafter(ext.astype(np.float32), np.float32(np.inf))
        if self.bad:
            e = np.full(3, np.inf, dtype=np.float32)
        return Box(c.astype(np.float64), e.astype(np.float64), joint)


@dataclasses.dataclass
class Box:
    c: np.ndarray      # centre, the binary32 values
    e: np.ndarray      # half extents, rounded up
    joint: int         # -1: transformed by M alone


@dataclasses.dataclass
class Chunk:
    prim: int
    k: int                      # chunk number inside the primitive
    whole: Optional[Box]        # None: the chunk has no vertex
    joints: List[Box]
    unbounded: bool             # weights not normalised, or more than 15 joints
    skinnable: bool


@dataclasses.dataclass
class Bounds:
    chunks: List[Chunk]               # of every primitive, whatever parts_disp says
    inst_all: Optional[Box]           # an unskinned draw: the box of everything
    inst_rigid: Optional[Box]         # a skinned draw: the primitives that cannot be skinned ...
    inst_joints: List[Box]            # ... and one box per joint in use
    weights_ok: bool                  # every weight quadruple of the model sums to 255


def decode_positions(md: scene.ModelData, prim: int) -> np.ndarray:
    """float32 [vertex_num, 3]; the two position formats the scenes of the cull tests use"""
    f = scene.unpack_primitive(md.prims[prim])
    fmt, cnt, off = next((e[1], e[2], e[3]) for e in md.layouts[prim] if e[0] == scene.SEM_POSITION)
    nv, st = f["vertex_num"], f["vertex_stride"]
    vb = np.ascontiguousarray(md.vertex_buf[f["vertex_base"]:f["vertex_base"] + nv * st]).reshape(nv, st)
    if fmt == scene.IEF_F32 and cnt == 3:
        return np.ascontiguousarray(vb[:, off:off + 12]).view("<f4").reshape(nv, 3)
    if fmt == scene.IEF_S16N and cnt >= 3:
        v = np.ascontiguousarray(vb[:, off:off + 6]).view("<i2").reshape(nv, 3).astype(np.float32)
        return np.maximum(v / np.float32(32767.0), np.float32(-1.0))
    raise NotImplementedError(f"position format {fmt} x{cnt}")


def _skin_bytes(md, prim):
    """(joints, weights) uint8 [vertex_num, 4] each, or None when the primitive cannot be skinned"""
    f = scene.unpack_primitive(md.prims[prim])
    offs = {e[0]: e[3] for e in md.layouts[prim] if e[0] in (scene.SEM_JOINT, scene.SEM_WEIGHT)}
    if len(offs) < 2:
        return None
    nv, st = f["vertex_num"], f["vertex_stride"]
    vb = np.ascontiguousarray(md.vertex_buf[f["vertex_base"]:f["vertex_base"] + nv * st]).reshape(nv, st)
    return vb[:, offs[scene.SEM_JOINT]:offs[scene.SEM_JOINT] + 4], vb[:, offs[scene.SEM_WEIGHT]:offs[scene.SEM_WEIGHT] + 4]


def boxes_of_vertices(pos, joints, weights):
    """(whole box, joint boxes, unbounded) of a set of vertices: pos float32 [n, 3]; joints / weights uint8 [n, 4] or None"""
    whole, per, order, unbounded = _Acc(), {}, [], False
    for v in range(len(pos)):
        whole.add(pos[v])
        if joints is None:
            continue
        if int(weights[v].astype(np.int64).sum()) != 255:
            unbounded = True
        for t in range(4):
            if weights[v][t] == 0:
                continue
            j = int(joints[v][t])
            if j not in per:
                per[j] = _Acc()
                order.append(j)
            per[j].add(pos[v])
    if not whole.any:
        return None, [], unbounded
    return whole.box(-1), [per[j].box(j) for j in order], unbounded


_bounds_cache: Dict[int, tuple] = {}


def bounds(md: scene.ModelData) -> Bounds:
    hit = _bounds_cache.get(id(md))
    if hit is not None and hit[0] is md:
        return hit[1]
    chunks, all_acc, rigid_acc, joint_acc, weights_ok = [], _Acc(), _Acc(), {}, True
    for p in range(md.nprims):
        f = scene.unpack_primitive(md.prims[p])
        pos = decode_positions(md, p)
        skin = _skin_bytes(md, p)
        idx = np.asarray(md.index_buf[f["index_ofs"]:f["index_ofs"] + f["index_num"]], dtype=np.int64)
        for k, start in enumerate(range(0, f["index_num"], CHUNK_NEW)):
            lo, hi = max(start - 2, 0), min(f["index_num"], start + CHUNK_NEW)
            vids = []
            for q in range(lo, hi):
                if f["topology"] == scene.TOPO_STRIP and idx[q] == 0xFFFF:
                    continue
                vid = int(idx[q]) + f["index_base"]
                if vid >= f["vertex_num"]:
                    continue
                vids.append(vid)
            vids = np.asarray(vids, dtype=np.int64)
            whole, jb, unb = boxes_of_vertices(pos[vids], None if skin is None else skin[0][vids], None if skin is None else skin[1][vids])
            if unb:
                weights_ok = False
            for v in vids:
                all_acc.add(pos[v])
                if skin is None:
                    rigid_acc.add(pos[v])
                else:
                    for t in range(4):
                        if skin[1][v][t]:
                            joint_acc.setdefault(int(skin[0][v][t]), _Acc()).add(pos[v])
            if len(jb) > CHUNK_MAX_BOXES:
                unb, jb = True, []
            chunks.append(Chunk(p, k, whole, jb, unb, skin is not None))
    b = Bounds(chunks, all_acc.box(-1) if all_acc.any else None, rigid_acc.box(-1) if rigid_acc.any else None,
               [joint_acc[j].box(j) for j in sorted(joint_acc)], weights_ok)
    _bounds_cache[id(md)] = (md, b)
    return b


def visible_chunks(md: scene.ModelData, parts_disp=None) -> List[int]:
    """indices into bounds(md).chunks of the chunks a draw produces, in draw order"""
    pd = md.parts_disp if parts_disp is None else parts_disp
    out, base = [], 0
    for p in range(md.nprims):
        f = scene.unpack_primitive(md.prims[p])
        n = (f["index_num"] + CHUNK_NEW - 1) // CHUNK_NEW
        if f["parts_no"] < len(pd) and pd[f["parts_no"]]:
            out += list(range(base, base + n))
        base += n
    return out


# ---------------------------------------------------------------------------------------------
# intervals and rectangles
# ---------------------------------------------------------------------------------------------
def mat4(m16) -> np.ndarray:
    """16 column-major binary32 values -> 4 x 4 float64 (row, column)"""
    return np.asarray(m16, dtype=np.float32).astype(np.float64).reshape(4, 4).T


def pal4(p16) -> np.ndarray:
    """a palette matrix as the skinning uses it: rows 0..2 of the 16 values, last row 0 0 0 1"""
    m = mat4(p16)
    m[3] = (0.0, 0.0, 0.0, 1.0)
    return m


def composite(M: np.ndarray, P: Optional[np.ndarray]):
    """C = M [P; 0 0 0 1] and |M| |P| (P None: M itself)"""
    with np.errstate(all="ignore"):
        if P is None:
            return M, np.abs(M)
        return M @ P, np.abs(M) @ np.abs(P)


def interval_parts(box: Box, C: np.ndarray, A: np.ndarray):
    """v, rad, m (each [3]: clip x, y, w) of one box under the composite"""
    rows = [0, 1, 3]
    with np.errstate(all="ignore"):
        v = C[rows, :3] @ box.c + C[rows, 3]
        rad = np.abs(C[rows, :3]) @ box.e
        mag = A[rows, :3] @ (np.abs(box.c) + box.e) + A[rows, 3]
        m = np.where(mag >= MIN_MAG, M_REL * mag, np.inf)  # the bound is relative: near underflow nothing is bounded
    return v, rad, m


def union_interval(boxes: List[Box], M: np.ndarray, pal: Optional[np.ndarray], m_scale: float = 1.0):
    """(lo[3], hi[3]) of the union of the boxes' intervals, or None when one of them is not finite.  pal: float32
    [npal, 16] or None; a box with joint -1 (or any box without a palette) goes with M alone"""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for b in boxes:
        P = None if (pal is None or b.joint < 0) else pal4(pal[min(b.joint, len(pal) - 1)])
        v, rad, m = interval_parts(b, *composite(M, P))
        with np.errstate(all="ignore"):
            l, h = v - rad - m * m_scale, v + rad + m * m_scale
        if not ((np.abs(l) < NOT_FINITE).all() and (np.abs(h) < NOT_FINITE).all()):
            return None
        lo, hi = np.minimum(lo, l), np.maximum(hi, h)
    return lo, hi


def screen_rect(iv, W: int, H: int, slack_px: float = SLACK_PX, d_slack: float = 0.0):
    """(fx_lo, fx_hi, fy_lo, fy_hi) with the slack applied, or None: no screen bound (kept)"""
    if iv is None:
        return None
    (xlo, ylo, wlo), (xhi, yhi, whi) = iv
    if not wlo > 0.0:
        return None
    sx_lo = xlo / whi if xlo >= 0 else xlo / wlo
    sx_hi = xhi / wlo if xhi >= 0 else xhi / whi
    sy_lo = ylo / whi if ylo >= 0 else ylo / wlo
    sy_hi = yhi / wlo if yhi >= 0 else yhi / whi
    hw, hh = 0.5 * W, 0.5 * H
    fx_lo, fx_hi = sx_lo * hw + hw, sx_hi * hw + hw
    fy_lo, fy_hi = hh - sy_hi * hh, hh - sy_lo * hh
    mx = slack_px + SLACK_REL * max(abs(fx_lo), abs(fx_hi)) + d_slack
    my = slack_px + SLACK_REL * max(abs(fy_lo), abs(fy_hi)) + d_slack
    r = (fx_lo - mx, fx_hi + mx, fy_lo - my, fy_hi + my)
    return r if all(np.isfinite(r)) else None


# ---------------------------------------------------------------------------------------------
# ownership
# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Own:
    W: int
    H: int
    rank: int
    world: int
    own_map: int
    param: int
    grid: np.ndarray   # [nby, nbx]: the rank that owns each bin


_grid_cache: Dict[tuple, np.ndarray] = {}


def ownership(W, H, shard) -> Own:
    """shard: (rank, world, own_map, param, band_rows) as Frame.set_shard takes it, or None: one rank owns the target"""
    nbx, nby, _ = sharding.grid(W, H)
    if shard is None or shard[1] <= 1:
        return Own(W, H, 0, 1, sharding.INTERLEAVED, 0, np.zeros((nby, nbx), dtype=np.int64))
    rank, world, own_map = shard[0], shard[1], shard[2]
    param = shard[3] if len(shard) > 3 else 0
    bands = shard[4] if len(shard) > 4 else None
    key = (W, H, world, own_map, param, None if bands is None else tuple(bands))
    if key not in _grid_cache:
        _grid_cache[key] = sharding.owner_map(W, H, world, own_map, param, bands)[::sharding.BIN, ::sharding.BIN]
    grid = _grid_cache[key]
    assert grid.shape == (nby, nbx)  # every bin has an owner, so a rank with an empty band owns none
    return Own(W, H, rank, world, own_map, param, grid)


def bin_rect(r, own: Own):
    """inclusive bin rectangle (bx0, by0, bx1, by1) of a screen rectangle that is not off the target, else None"""
    fx_lo, fx_hi, fy_lo, fy_hi = r
    if fx_hi < 0.0 or fx_lo > own.W or fy_hi < 0.0 or fy_lo > own.H:
        return None
    nby, nbx = own.grid.shape
    cl = lambda f, top, n: min(int(min(max(f, 0.0), float(top))) >> BIN_SHIFT, n - 1)
    return cl(fx_lo, own.W, nbx), cl(fy_lo, own.H, nby), cl(fx_hi, own.W, nbx), cl(fy_hi, own.H, nby)


def may_touch(r, own: Own) -> bool:
    """r: a screen rectangle, or None (no bound: kept)"""
    if r is None:
        return True
    b = bin_rect(r, own)
    if b is None:
        return False
    if own.world <= 1:
        return True
    bx0, by0, bx1, by1 = b
    if (own.grid[by0:by1 + 1, bx0:bx1 + 1] == own.rank).any():
        return True
    if own.own_map != sharding.BANDS:  # the documented concession: tall and narrow rectangles are kept untested
        s = own.param if own.own_map == sharding.SUPERTILES else 0
        if (bx1 >> s) - (bx0 >> s) + 1 < own.world and (by1 >> s) - (by0 >> s) >= 8:
            return True
    return False


def all_inside(r, own: Own) -> bool:
    if r is None:
        return False
    if own.world <= 1:
        return r[0] >= 0.0 and r[1] <= own.W and r[2] >= 0.0 and r[3] <= own.H
    if own.own_map != sharding.BANDS:
        return False
    nby = own.grid.shape[0]
    cl = lambda f: min(int(min(max(f, 0.0), float(own.H))) >> BIN_SHIFT, nby - 1)
    return bool((own.grid[cl(r[2]):cl(r[3]) + 1, 0] == own.rank).all())


# ---------------------------------------------------------------------------------------------
# one draw
# ---------------------------------------------------------------------------------------------
def _f32_bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).reshape(-1).tolist()


def vp_model(vp16, model16) -> np.ndarray:
    """VP * Model as the library forms it for the vertex stage and the bounds alike: per element a k-ordered binary32
    fma chain from 0 (exact integer model of tests/vertex_edge_cases.py).  16 column-major binary32 values."""
    A, B = _f32_bits(vp16), _f32_bits(model16)
    out = []
    for e in range(16):
        i, c, a = e & 3, e >> 2, 0
        for k in range(4):
            a = vx.fma32(A[k * 4 + i], B[c * 4 + k], a)
        out.append(a)
    return np.array(out, dtype=np.uint32).view(np.float32)


@dataclasses.dataclass
class DrawRects:
    """what does not depend on the rank: per variant ("in", "out") the rectangles of the instances and of their chunks"""
    ninst: int
    nchunks: int
    inst_tested: bool
    inst: Dict[str, list]     # variant -> [rect or None] per instance (inst_tested only)
    chunk: Dict[str, list]    # variant -> [instance][chunk] -> rect, None (no bound: kept) or KEPT (never tested)


def draw_matrices(draw):
    """(batch?, [M 4x4 float64 per instance], palettes float32 [ninst, npal, 16] or None)"""
    if "model_mats" in draw:
        mm = np.asarray(draw["model_mats"], dtype=np.float32).reshape(-1, 16)
        Ms = [mat4(vp_model(draw["vp"], m)) for m in mm]
        pals = draw.get("palettes")
        if pals is not None:
            pals = np.asarray(pals, dtype=np.float32).reshape(len(mm), -1, 16)
        return True, Ms, pals
    pal = draw.get("palette")
    if pal is not None:
        pal = np.asarray(pal, dtype=np.float32).reshape(1, -1, 16)
    return False, [mat4(draw["M"])], pal


def draw_rects(draw, W: int, H: int, m_scales=BAND_M, d_slacks=BAND_SLACK, slack_px: float = SLACK_PX) -> DrawRects:
    md = draw["md"]
    b = bounds(md)
    vis = [b.chunks[i] for i in visible_chunks(md, draw.get("parts_disp"))]
    batch, Ms, pals = draw_matrices(draw)
    have_pal = pals is not None and pals.shape[1] > 0
    if have_pal:
        inst_boxes = ([b.inst_rigid] if b.inst_rigid is not None else []) + b.inst_joints
        inst_tested = batch and b.weights_ok and len(inst_boxes) > 0
    else:
        inst_boxes = [b.inst_all] if b.inst_all is not None else []
        inst_tested = batch and len(inst_boxes) > 0
    out = DrawRects(len(Ms), len(vis), inst_tested, {}, {})
    for name, ms, ds in zip(("in", "out"), m_scales, d_slacks):
        irects, crects = [], []
        for i, M in enumerate(Ms):
            pal = pals[i] if have_pal else None
            if inst_tested:
                irects.append(screen_rect(union_interval(inst_boxes, M, pal, ms), W, H, slack_px, ds))
            row = []
            for ch in vis:
                skinned = ch.skinnable and have_pal
                if ch.whole is None or (skinned and (ch.unbounded or len(ch.joints) < 1)):
                    row.append(KEPT)
                    continue
                boxes = ch.joints if skinned else [ch.whole]
                row.append(screen_rect(union_interval(boxes, M, pal if skinned else None, ms), W, H, slack_px, ds))
            crects.append(row)
        out.inst[name], out.chunk[name] = irects, crects
    return out


@dataclasses.dataclass
class Prediction:
    chunks: int               # what stats["chunks"] must say: nchunks * ninst
    culled_lo: int
    culled_hi: int
    n_ambiguous: int
    instances: list           # per instance (state under R_in, state under R_out); state None: not instance-tested
    chunk_kept: list          # [instance][chunk] -> (kept under R_in, kept under R_out), None where no chunk test runs

    def describe(self) -> str:
        lines = [f"chunks {self.chunks}, culled {self.culled_lo}..{self.culled_hi}, ambiguous {self.n_ambiguous}"]
        for i, (st, row) in enumerate(zip(self.instances, self.chunk_kept)):
            marks = "".join("." if c is None else ("K" if c == (True, True) else "c" if c == (False, False) else "?") for c in row)
            lines.append(f"  instance {i}: {st[0]}{'' if st[0] == st[1] else ' / ' + str(st[1])}  chunks [{marks}]")
        return "\n".join(lines)


def predict_from(dr: DrawRects, own: Own) -> Prediction:
    counts = {"in": 0, "out": 0}
    states, kept, namb = [], [], 0
    for i in range(dr.ninst):
        st, ck = {}, {}
        for v in ("in", "out"):
            if not dr.inst_tested:
                st[v] = None
            else:
                r = dr.inst[v][i]
                st[v] = STRADDLE if r is None else (CULLED if not may_touch(r, own) else (INSIDE if all_inside(r, own) else STRADDLE))
            if st[v] == CULLED:
                counts[v] += dr.nchunks
                ck[v] = None
            elif st[v] == INSIDE:
                ck[v] = None
            else:
                ck[v] = [True if r is KEPT else may_touch(r, own) for r in dr.chunk[v][i]]
                counts[v] += sum(1 for k in ck[v] if not k)
        states.append((st["in"], st["out"]))
        if st["in"] != st["out"]:
            namb += 1
            kept.append([None] * dr.nchunks)
        elif ck["in"] is None:
            kept.append([None] * dr.nchunks)
        else:
            kept.append(list(zip(ck["in"], ck["out"])))
            namb += sum(1 for a, b in kept[-1] if a != b)
    return Prediction(dr.ninst * dr.nchunks, min(counts.values()), max(counts.values()), namb, states, kept)


_rect_cache: Dict[tuple, tuple] = {}


def predict(draw, W: int, H: int, shard) -> Prediction:
    """(culled_lo, culled_hi, n_ambiguous) and the decisions behind them, for one draw alone in a W x H frame of `shard`"""
    key = (id(draw), W, H)
    hit = _rect_cache.get(key)
    if hit is None or hit[0] is not draw:
        hit = (draw, draw_rects(draw, W, H))
        _rect_cache[key] = hit
    return predict_from(hit[1], ownership(W, H, shard))


# ---------------------------------------------------------------------------------------------
# the bound itself: where a clip coordinate of a vertex lies relative to its chunk's boxes
# ---------------------------------------------------------------------------------------------
def chunk_vertex_ids(md: scene.ModelData, prim: int) -> List[np.ndarray]:
    """per chunk of the primitive, the vertex ids it holds (what its boxes were made from)"""
    f = scene.unpack_primitive(md.prims[prim])
    idx = np.asarray(md.index_buf[f["index_ofs"]:f["index_ofs"] + f["index_num"]], dtype=np.int64)
    out = []
    for start in range(0, f["index_num"], CHUNK_NEW):
        q = idx[max(start - 2, 0):min(f["index_num"], start + CHUNK_NEW)]
        if f["topology"] == scene.TOPO_STRIP:
            q = q[q != 0xFFFF]
        q = q + f["index_base"]
        out.append(np.unique(q[q < f["vertex_num"]]))
    return out


def margin_fraction(clip, boxes: List[Box], M: np.ndarray, pal: Optional[np.ndarray]):
    """For clip coordinates [n, >= 4] (x, y, z, w) that the boxes are meant to bound: per vertex the smallest s such that
    x, y and w lie in [min_b (v_b - rad_b - s m_b), max_b (v_b + rad_b + s m_b)], the union of the boxes' intervals as the
    kernels form it (a blend of several joints lies between their boxes), or None when an interval is not finite (the
    geometry is kept: nothing to hold).  s <= 1 is the bound of geom_cull.h; s = 0 is a value inside the union proper."""
    val = np.asarray(clip, dtype=np.float64)[:, [0, 1, 3]]
    above, below = np.full(val.shape, np.inf), np.full(val.shape, np.inf)
    for b in boxes:
        P = None if (pal is None or b.joint < 0) else pal4(pal[min(b.joint, len(pal) - 1)])
        v, rad, m = interval_parts(b, *composite(M, P))
        if not (np.isfinite(v).all() and np.isfinite(rad).all() and (np.abs(v) + rad + m < NOT_FINITE).all()):
            return None
        with np.errstate(all="ignore"):
            up, dn = np.maximum(val - (v + rad), 0.0), np.maximum((v - rad) - val, 0.0)
            up, dn = np.where(up == 0.0, 0.0, up / m), np.where(dn == 0.0, 0.0, dn / m)
        above = np.fmin(above, np.where(np.isnan(up), np.inf, up))
        below = np.fmin(below, np.where(np.isnan(dn), np.inf, dn))
    return np.maximum(above, below).max(axis=1)


def case_blocks(case, prim: int, skinned: bool, block: int = CHUNK_NEW):
    """A case model of tests/vertex_edge_cases.py indexes three vertices only, so blocks of 62 consecutive vertex ids
    (plus the two before, like a chunk) stand in for its chunks: [(vertex ids inside the primitive, boxes)].  Skinned:
    only the vertices whose weight bytes sum to 255 are bounded, and the boxes are the per-joint ones."""
    v0, n = case.prims[prim]
    pos = np.ascontiguousarray(case.pos_bits[v0:v0 + n]).view(np.float32)
    jw, ww = case.joints[v0:v0 + n], case.weights[v0:v0 + n]
    ids = np.arange(n)
    if skinned:
        ids = ids[ww.astype(np.int64).sum(axis=1) == 255]
    out = []
    for start in range(0, len(ids), block):
        vids = ids[max(start - 2, 0):start + block]
        whole, joints, unb = boxes_of_vertices(pos[vids], jw[vids] if skinned else None, ww[vids] if skinned else None)
        assert whole is not None and not unb
        out.append((vids, joints if skinned else [whole]))
    return out
