"""Every code of every vertex format: reference decode tables and the models that carry the codes.

Plain Python and numpy, no GPU and no oracle.  The geometry stage decodes an element in three places that are meant to be
one function -- decode_regs (geom_vertex.h; registers, after load_elem: k_vertex_stage and the main path of k_geom), decode_elem
(geom_vertex.h; memory, the clipper's re-shade only) and decode_pos_host (the host mirror behind the culling boxes).  Four parts:

* reference tables, built in integer arithmetic with ``div32`` of tests/vertex_edge_cases.py (U8N, S8N, S16N, the 10-bit
  fields of SCMP3N) and by integer construction (F16 -> binary32, all 65 536 patterns);
* ``exhaustive_case``: for every (format, count) pair the host accepts, as Position and as TexCoord, at four placements
  of the vertex in memory, a model whose vertices carry every code in every component the pair decodes, split into three
  primitives of unequal sizes that are no multiple of 64;
* ``weight_case``: every weight byte in every weight slot, in blocks the MFMA skins and in blocks the VALU redoes;
* ``clip_scenes``: small textured frames whose triangles straddle the near plane or leave the guard band, the only way to
  decode_elem, and whose local triangles let the culling boxes of the host mirror decide what a rank keeps.

NaN rule (SPEC section 2): a NaN input of a decode that computes (F16 widening, any position through the clip chain) must
give a NaN and nothing more; every other pattern is compared word for word, and so is every F32 texcoord, which is bits.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import List, Tuple

import numpy as np

from mt_renderer_amd import scene
from tests import vertex_edge_cases as vx

NAN, INF, ONE = vx.NAN, vx.INF, vx.ONE
_ABS = 0x7FFFFFFF
NEG_ONE = 0xBF800000


# ---------------------------------------------------------------------------------------------
# reference decode tables (indexed by the raw field: byte, u16, 10-bit field)
# ---------------------------------------------------------------------------------------------
def _snorm(v: int, d: int) -> int:
    return NEG_ONE if v < -d else vx.div32(v, d)  # max(v / d, -1)


def _signed(c: int, bits: int) -> int:
    return c - (1 << bits) if c >> (bits - 1) else c


def _f16_table() -> np.ndarray:
    """binary16 pattern -> binary32 pattern, exact: subnormals normalised, signed zeros, infinities and NaN payloads kept"""
    h = np.arange(65536, dtype=np.uint32)
    s, e, m = (h >> 15) << 31, (h >> 10) & 31, h & 1023
    out = s | ((e + 112) << 23) | (m << 13)                      # normal numbers
    out = np.where(e == 31, s | INF | (m << 13), out)            # inf, NaN
    out = np.where((e == 0) & (m == 0), s, out)                  # zeros
    for p in range(10):                                          # subnormal m * 2^-24 with leading bit p: 2^(p - 24) * 1.f
        sel = (e == 0) & ((m >> p) == 1)
        out = np.where(sel, s | ((p + 103) << 23) | ((m << (23 - p)) & 0x7FFFFF), out)
    return out.astype(np.uint32)


U8N_BITS = np.array([vx.div32(v, 255) for v in range(256)], dtype=np.uint32)
S8N_BITS = np.array([_snorm(_signed(c, 8), 127) for c in range(256)], dtype=np.uint32)
S16N_BITS = np.array([vx.snorm16_bits(_signed(c, 16)) for c in range(65536)], dtype=np.uint32)
SCMP_BITS = np.array([_snorm(_signed(c, 10), 511) for c in range(1024)], dtype=np.uint32)
F16_BITS = _f16_table()


# ---------------------------------------------------------------------------------------------
# the (format, count) pairs of the host's table (host_model.cpp: elem_bytes)
# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Pair:
    name: str
    fmt: int
    cnt: int
    nbytes: int    # bytes the element occupies
    ncomp: int     # components the decode produces (of x, y, z)
    bits: int      # width of one field
    signed: bool   # decoded range [-1, 1] (else [0, 1])
    flags: int = 0

    @property
    def ncodes(self) -> int:
        return 1 << self.bits

    def element(self, semantic: int, offset: int) -> tuple:
        return (semantic, self.fmt, self.cnt, offset) + ((self.flags,) if self.flags else ())

    @property
    def table(self):
        return {scene.IEF_U8N: U8N_BITS, scene.IEF_U8NL: U8N_BITS, scene.IEF_S8N: S8N_BITS, scene.IEF_S16N: S16N_BITS,
                scene.IEF_F16: F16_BITS, scene.IEF_SCMP3N: SCMP_BITS, scene.IEF_F32: None}[self.fmt]


PAIRS = {p.name: p for p in (
    Pair("u8n_x1", scene.IEF_U8N, 1, 2, 2, 8, False), Pair("u8n_x4", scene.IEF_U8N, 4, 4, 3, 8, False),
    Pair("u8nl_x3", scene.IEF_U8NL, 3, 4, 3, 8, False),
    Pair("s8n_x1", scene.IEF_S8N, 1, 2, 2, 8, True), Pair("s8n_x3", scene.IEF_S8N, 3, 4, 3, 8, True),
    Pair("s8n_x4", scene.IEF_S8N, 4, 4, 3, 8, True),
    Pair("s16n_x1", scene.IEF_S16N, 1, 4, 2, 16, True), Pair("s16n_x3", scene.IEF_S16N, 3, 8, 3, 16, True),
    Pair("f16_x2", scene.IEF_F16, 2, 4, 2, 16, True), Pair("f32_x3", scene.IEF_F32, 3, 12, 3, 32, True),
    Pair("scmp3n", scene.IEF_SCMP3N, 1, 4, 3, 10, True, flags=1))}
ROLES = ("position", "texcoord")

# the edge codes of one field, as raw fields: -max - 1, -max, -1, 0, 1, max for the signed ones
EDGE_CODES = {
    "u8": (0, 1, 127, 128, 254, 255), "s8": (0x80, 0x81, 0xFF, 0, 1, 0x7F),
    "s16": (0x8000, 0x8001, 0xFFFF, 0, 1, 0x7FFF, 0x4000, 0xC000), "s10": (0x200, 0x201, 0x3FF, 0, 1, 0x1FF),
    # +-0, smallest and largest subnormal, smallest normal, 1 - ulp, 1, 1 + ulp, 65504, +-inf, quiet and signalling NaN
    "f16": (0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x8400, 0x3BFF, 0x3C00, 0xBC00, 0x3C01, 0x7BFF, 0xFBFF,
            0x7C00, 0xFC00, 0x7E00, 0xFE00, 0x7C01, 0xFC01, 0x7DFF, 0x7FFF),
}
# binary32 is a list, not a sweep: +-0, smallest and largest subnormal, FLT_MIN, 1 -+ ulp, 1, FLT_MAX, +-inf, NaNs
F32_LIST = (0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x3F7FFFFF, 0x3F800000,
            0x3F800001, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0xFFC00001)
_F32_BENIGN = (0x3F000000, 0xBE800000, 0x3F400000)  # 0.5, -0.25, 0.75


def edge_codes(pair: Pair) -> tuple:
    if pair.fmt == scene.IEF_F32:
        return F32_LIST
    if pair.fmt == scene.IEF_F16:
        return EDGE_CODES["f16"]
    return EDGE_CODES[("s" if pair.signed else "u") + str(pair.bits)]


def decode_ref(pair: Pair, codes: np.ndarray) -> np.ndarray:
    """raw fields [n, ncomp] -> binary32 words [n, 3] of (x, y, z); a component the pair does not decode is +0"""
    out = np.zeros((len(codes), 3), dtype=np.uint32)
    out[:, :pair.ncomp] = codes if pair.table is None else pair.table[codes]
    return out


def pack(pair: Pair, codes: np.ndarray, junk: np.ndarray) -> np.ndarray:
    """raw fields [n, ncomp] -> element bytes [n, nbytes]; what the decode must not read (the w component, the top two
    bits of SCMP3N) is taken from the byte `junk` of each vertex"""
    n = len(codes)
    b = np.empty((n, pair.nbytes), dtype=np.uint8)
    b[:] = junk.astype(np.uint8)[:, None]
    c = np.ascontiguousarray(codes, dtype=np.uint32)
    if pair.bits == 8:
        b[:, :pair.ncomp] = c
    elif pair.bits == 16:
        b[:, :2 * pair.ncomp] = c.astype("<u2").view(np.uint8).reshape(n, 2 * pair.ncomp)
    elif pair.bits == 32:
        b[:, :12] = c.astype("<u4").view(np.uint8).reshape(n, 12)
    else:
        w = c[:, 0] | (c[:, 1] << 10) | (c[:, 2] << 20) | ((junk.astype(np.uint32) & 3) << 30)
        b[:] = w.astype("<u4").view(np.uint8).reshape(n, 4)
    return b


# ---------------------------------------------------------------------------------------------
# placements: where the vertex lies in memory
# ---------------------------------------------------------------------------------------------
PLACEMENTS = ("aligned", "half", "odd", "base3")
# element address mod 4 over the vertices of a model; only `aligned` sets DPrim.aligned4
PLACEMENT_RESIDUES = {"aligned": {0}, "half": {0, 2}, "odd": {0, 1, 2, 3}, "base3": {0, 2}}


def place(nb_main: int, nb_other: int, placement: str) -> Tuple[int, int, int, int]:
    """(vertex_base, offset of the element under test, offset of the other element, stride)"""
    if placement == "aligned":      # everything a multiple of four
        base, off = 8, 4
        other = off + ((nb_main + 3) & ~3) + 4
        stride = other + ((nb_other + 3) & ~3)
    elif placement == "half":       # offset 2, stride = 2 mod 4: addresses alternate between 2 and 0 mod 4
        base, off = 0, 2
        other = off + nb_main + 2
        stride = other + nb_other
        stride += (2 - stride) % 4
    elif placement == "odd":        # odd vertex_base, odd stride: every residue
        base, off = 1, 2
        other = off + nb_main + 1
        stride = (other + nb_other + 1) | 1
    else:                           # vertex_base = 3 mod 4 and an odd offset: four-byte aligned addresses on the unaligned path
        base, off = 3, 1
        other = off + nb_main + 1
        stride = other + nb_other + 1
        stride += (2 - stride) % 4
    return base, off, other, stride


def vertex_buffer(n: int, base: int, stride: int, parts) -> np.ndarray:
    """bytes 0xA5 / 0x5A everywhere, then the elements: a read of the wrong byte shows"""
    buf = np.where(np.arange(base + n * stride) & 1, 0x5A, 0xA5).astype(np.uint8)
    rows = buf[base:].reshape(n, stride)
    for off, b in parts:
        rows[:, off:off + b.shape[1]] = b
    return buf


def split(n: int) -> List[Tuple[int, int]]:
    """(first vertex, vertex_num) of three primitives: unequal sizes, none a multiple of 64 (vertex_num is a 16-bit field)"""
    a, b = n // 2 + 37, n // 4 - 11
    return [(0, a), (a, b), (a + b, n - a - b)]


def _junk(n: int) -> np.ndarray:
    return (np.arange(n) * 37 + 11) & 0xFF


# ---------------------------------------------------------------------------------------------
# exhaustive models for the vertex stage
# ---------------------------------------------------------------------------------------------
IDENTITY_M = np.eye(4, dtype=np.float32).reshape(16)


def companion(pair: Pair) -> Pair:
    """the element in the other role: two bytes, so that it fits every placement"""
    return PAIRS["s8n_x1"] if pair.name == "u8n_x1" else PAIRS["u8n_x1"]


def exhaustive_codes(pair: Pair) -> np.ndarray:
    """raw fields [n, ncomp]: component c of vertex i holds code (i + c R) mod ncodes -- every code once in every
    component, and no two components of a vertex alike, so that a swapped component cannot pass.  F32: the list, each
    value alone in each component among benign ones, then rotated through all three."""
    if pair.fmt == scene.IEF_F32:
        L, n = np.array(F32_LIST, dtype=np.uint32), len(F32_LIST)
        i = np.arange(256)
        g, k = (i // n) % 4, i % n
        out = np.tile(np.array(_F32_BENIGN, dtype=np.uint32), (256, 1))
        for c in range(3):
            out[:, c] = np.where(g == c, L[k], out[:, c])
            out[:, c] = np.where(g == 3, L[(k + (0, 5, 11)[c]) % n], out[:, c])
        return out
    i = np.arange(pair.ncodes, dtype=np.uint32)
    r = pair.ncodes // 3 + 1
    return np.stack([(i + c * r) % pair.ncodes for c in range(pair.ncomp)], axis=1).astype(np.uint32)


def identity_clip(pos: np.ndarray) -> np.ndarray:
    """clip words of M = identity: the decoded value, -0 turned into +0 by the chain's first step (fma(1, -0, +0)), w = 1;
    a component is NaN where it is NaN itself or another one is not finite (0 * inf), w is NaN where any is not finite"""
    mag = pos & _ABS
    nonfin, nan = mag >= INF, mag > INF
    out = np.zeros((len(pos), 4), dtype=np.uint32)
    for i in range(3):
        others = np.delete(nonfin, i, axis=1).any(axis=1)
        out[:, i] = np.where(others | nan[:, i], NAN, np.where(mag[:, i] == 0, 0, pos[:, i]))
    out[:, 3] = np.where(nonfin.any(axis=1), NAN, ONE)
    return out


@dataclasses.dataclass
class Expected:
    codes: np.ndarray        # raw fields of the element under test [n, ncomp]
    other_codes: np.ndarray  # raw fields of the element in the other role [n, 2]
    pos_bits: np.ndarray     # decoded position words [n, 3]
    clip: np.ndarray         # clip words under the identity [n, 4]
    uv: np.ndarray           # texcoord words [n, 2]
    sample: np.ndarray       # >= 256 vertices, those that hold an edge code in some component included


def sample_of(pair: Pair, codes: np.ndarray) -> np.ndarray:
    n = len(codes)
    edge = np.isin(codes, np.array(edge_codes(pair), dtype=np.uint32)).any(axis=1)
    rest = np.random.default_rng(pair.bits).permutation(n)[:256]
    return np.unique(np.concatenate([np.nonzero(edge)[0], rest]))


@functools.lru_cache(maxsize=None)
def expected(pair_name: str, role: str) -> Expected:
    pair = PAIRS[pair_name]
    codes = exhaustive_codes(pair)
    i = np.arange(len(codes))
    other_codes = np.stack([(i * 7 + 3) & 255, (i * 13 + 5 + (i >> 8)) & 255], axis=1).astype(np.uint32)
    main, other = decode_ref(pair, codes), decode_ref(companion(pair), other_codes)
    pos, tex = (main, other) if role == "position" else (other, main)
    return Expected(codes, other_codes, pos, identity_clip(pos), tex[:, :2].copy(), sample_of(pair, codes))


def shade_words(pos_bits: np.ndarray, M: np.ndarray, rows) -> np.ndarray:
    """the exact model of tests/vertex_edge_cases.py on the unskinned vertices `rows`: clip words [len(rows), 4]"""
    Mw = np.ascontiguousarray(M, dtype=np.float32).view(np.uint32).tolist()
    return np.array([vx.shade(p, None, None, None, Mw) for p in pos_bits[rows].tolist()], dtype=np.uint32).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def headline_clip(pair_name: str) -> np.ndarray:
    """the sample of the pair as Position under a matrix with no zero in it: exactly shade()"""
    e = expected(pair_name, "position")
    return shade_words(e.pos_bits, vx.HEADLINE_M, e.sample)


@dataclasses.dataclass
class Case:
    name: str
    pair: Pair
    role: str
    placement: str
    md: scene.ModelData
    prims: List[Tuple[int, int]]  # (first vertex, vertex_num)
    exp: Expected
    base: int
    offset: int                   # of the element under test
    stride: int

    @property
    def uv_is_bits(self) -> bool:
        """an F32 texcoord is copied, not computed: its NaNs are compared word for word too"""
        return self.role == "texcoord" and self.pair.fmt == scene.IEF_F32


def exhaustive_case(pair_name: str, role: str, placement: str) -> Case:
    pair, exp = PAIRS[pair_name], expected(pair_name, role)
    other = companion(pair)
    n = len(exp.codes)
    base, off, ooff, stride = place(pair.nbytes, other.nbytes, placement)
    junk = _junk(n)
    buf = vertex_buffer(n, base, stride, [(off, pack(pair, exp.codes, junk)), (ooff, pack(other, exp.other_codes, junk))])
    sems = (scene.SEM_POSITION, scene.SEM_TEXCOORD) if role == "position" else (scene.SEM_TEXCOORD, scene.SEM_POSITION)
    lay = [pair.element(sems[0], off), other.element(sems[1], ooff)]
    prims = split(n)
    packed = [scene.pack_primitive(vertex_num=m, vertex_stride=stride, topology=scene.TOPO_LIST, vertex_base=base + v0 * stride,
                                   index_num=3) for v0, m in prims]
    md = scene.ModelData(vertex_buf=buf, index_buf=np.zeros(3, dtype=np.uint16), prims=np.stack(packed),
                         layouts=[list(lay) for _ in prims], prim_to_texture=np.full(len(prims), -1, dtype=np.int32),
                         prim_debug_id=np.arange(len(prims), dtype=np.uint32), parts_disp=np.ones(len(prims), dtype=np.uint8))
    return Case(f"{pair_name}-{role}-{placement}", pair, role, placement, md, prims, exp, base, off, stride)


def same_words(got, ref, nan_by_class: bool = True) -> np.ndarray:
    """elementwise: words equal, or (the NaN rule) both NaN; with nan_by_class off, words equal and nothing else"""
    if nan_by_class:
        return vx.same_words(got, ref)
    return np.ascontiguousarray(got).view(np.uint32) == np.ascontiguousarray(ref).view(np.uint32)


def describe_difference(case: Case, what: str, v0: int, ok: np.ndarray, got: np.ndarray, ref: np.ndarray) -> str:
    """the first vertex of a primitive (which starts at vertex v0 of the model) with a differing word"""
    bad = np.nonzero(~ok.reshape(len(ok), -1).all(axis=1))[0]
    v = int(bad[0])
    g, r = np.ascontiguousarray(got).view(np.uint32)[v], np.ascontiguousarray(ref).view(np.uint32)[v]
    return (f"{case.name}, {what}: {len(bad)} vertices differ; first: vertex {v0 + v} (lane {v & 63} of its wave, address "
            f"{(case.base + (v0 + v) * case.stride + case.offset) & 3} mod 4), fields "
            f"{[hex(int(x)) for x in case.exp.codes[v0 + v]]}, got {[hex(int(x)) for x in g]}, expected {[hex(int(x)) for x in r]}")


# ---------------------------------------------------------------------------------------------
# every weight byte in every slot
# ---------------------------------------------------------------------------------------------
WEIGHT_NPALS = (1, 64)


@dataclasses.dataclass
class WeightCase:
    md: scene.ModelData
    prims: List[Tuple[int, int]]
    joints: np.ndarray   # uint8 [n, 4]
    weights: np.ndarray  # uint8 [n, 4]
    pal: np.ndarray      # float32 [64, 16]: entry 0 is the identity
    pos_bits: np.ndarray

    def patterns(self, prim: int) -> List[str]:
        v0, n = self.prims[prim]
        return vx.block_patterns(self.joints[v0:v0 + n], self.weights[v0:v0 + n])


@functools.lru_cache(maxsize=None)
def weight_case() -> WeightCase:
    """position (1, 0, 0); joint words in the style of alternate_blocks: the even blocks of a primitive are coherent
    (MFMA), the odd ones and the tails are not (VALU redo).  The vertices of each kind, in order, take the weight bytes
    (w, 0, 0, 0) for all 256 w, then w in each of the other slots, and then start over."""
    n = 2304
    prims = split(n)
    rng = np.random.default_rng(17)
    joints = np.concatenate([vx.alternate_blocks(rng.integers(0, 96, size=((m + 3) // 4, 4)).astype(np.uint8))[:m] for _, m in prims])
    coherent = np.concatenate([np.array(vx.block_patterns(joints[v0:v0 + m], np.ones((m, 4), dtype=np.uint8))) == "coherent" for v0, m in prims])
    weights = np.zeros((n, 4), dtype=np.uint8)
    for kind in (coherent, ~coherent):
        rows = np.nonzero(kind)[0]
        t = np.arange(len(rows)) % 1024
        weights[rows, t // 256] = t % 256
    pos = np.tile(np.array([1.0, 0.0, 0.0], dtype=np.float32), (n, 1))
    md = vx._model(pos, np.zeros((n, 2), dtype=np.float16), joints, weights, prims)
    pal = vx.rigid_palette(18)[:64].copy()
    pal[0] = IDENTITY_M
    return WeightCase(md, prims, joints, weights, pal, pos.view(np.uint32).reshape(n, 3))


@functools.lru_cache(maxsize=None)
def weight_clip(npal: int) -> np.ndarray:
    """clip words [n, 4] under the identity, from shade(); with npal = 1 clip.x is the decoded weight"""
    c = weight_case()
    pal = c.pal[:npal].view(np.uint32).tolist()
    M = IDENTITY_M.view(np.uint32).tolist()
    return np.array([vx.shade(p, j, w, pal, M) for p, j, w in zip(c.pos_bits.tolist(), c.joints.tolist(), c.weights.tolist())],
                    dtype=np.uint32).reshape(-1, 4)


# ---------------------------------------------------------------------------------------------
# frames: the clipper's decode and the host mirror
# ---------------------------------------------------------------------------------------------
CLIP_W, CLIP_H = 256, 160
CLIP_CLASSES = {"aligned": "aligned", "unaligned": "odd"}  # placement class -> placement
CLIP_NV, CLIP_LOCAL, CLIP_RANDOM = 384, 200, 300


FRAME_FLOAT_EDGES = {  # +-0, +-smallest subnormal, largest subnormal, smallest normal, 1 - ulp, +-1
    scene.IEF_F16: (0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0x0400, 0x3BFF, 0x3C00, 0xBC00),
    scene.IEF_F32: (0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x3F7FFFFF, 0x3F800000, 0xBF800000),
}


def frame_edges(pair: Pair) -> tuple:
    """the edge codes every frame model plants in every component"""
    return FRAME_FLOAT_EDGES.get(pair.fmt) or edge_codes(pair)


def _frame_fields(pair: Pair, rng, n: int) -> np.ndarray:
    """raw fields [n, ncomp] over the whole range of the format; the first rows hold each edge code in each component.
    The float formats stay inside [-1, 1] (frames with non-finite or far-away positions are not what this is about): half
    of the values uniform, half uniform in their bit pattern, so that subnormals and tiny exponents occur."""
    shape = (n, pair.ncomp)
    if pair.fmt in FRAME_FLOAT_EDGES:
        u = rng.uniform(-1.0, 1.0, size=shape)
        if pair.fmt == scene.IEF_F16:
            one, sign, vals = 0x3C00, 0x8000, u.astype(np.float16).view(np.uint16).astype(np.uint32)
        else:
            one, sign, vals = 0x3F800000, 0x80000000, u.astype(np.float32).view(np.uint32)
        pats = rng.integers(0, one + 1, size=shape).astype(np.uint32) | np.where(rng.random(shape) < 0.5, sign, 0).astype(np.uint32)
        codes = np.where(rng.random(shape) < 0.5, vals, pats).astype(np.uint32)
    else:
        codes = rng.integers(0, pair.ncodes, size=shape).astype(np.uint32)
    k = 0
    for c in range(pair.ncomp):
        for e in frame_edges(pair):
            codes[k, c] = e
            k += 1
    return codes


def _views(pair: Pair) -> dict:
    """plain: the non-clipping view of test_gpu_cases.test_vertex_formats.  near: orthographic, depth a blend of all
    decoded components (two-component formats have z = 0) that is negative for about half of the range, so most
    triangles with far-apart vertices straddle z = 0.  guard: x and y magnified until vertices away from the centre of
    the range lie beyond +-2^20 px."""
    c, h = (0.0, 1.0) if pair.signed else (0.5, 0.5)
    wt = np.array([0.4, 0.3, 0.5 if pair.ncomp == 3 else 0.0])
    wt = wt / wt.sum() / h                       # t = wt . (p - c) lies in [-1, 1]
    zrow = lambda a, b: [a * wt[0], a * wt[1], a * wt[2], b - a * c * wt.sum()]
    xy = lambda s: ([s / h, 0, 0, -s * c / h], [0, s / h, 0, -s * c / h])
    near = np.array([*xy(0.85), zrow(0.45, 0.02), [0, 0, 0, 1.0]])
    guard = np.array([*xy(1.2e4), zrow(0.4, 0.5), [0, 0, 0, 1.0]])
    plain = scene.mat_translate(0.05, -0.03, 0.5) @ scene.mat_scale(0.9, 0.9, 0.4)
    return {"plain": scene.to_f32_colmajor(plain), "near": scene.to_f32_colmajor(near), "guard": scene.to_f32_colmajor(guard)}


@dataclasses.dataclass
class ClipScene:
    name: str
    pair: Pair
    md: scene.ModelData
    views: dict  # plain, near, guard -> M

    def draws(self, view: str) -> list:
        return [dict(md=self.md, M=self.views[view])]


def _clip_scene(pair: Pair, klass: str, seed: int) -> ClipScene:
    """one triangle list: CLIP_LOCAL small triangles between neighbouring vertices, sorted by y, so that a geometry chunk
    covers a narrow band and its box (host mirror) decides whether a rank keeps it; then CLIP_RANDOM triangles between
    random vertices, which span the range and cross whatever plane a view puts through it.  The pair is Position and
    TexCoord at once; a small opaque checker shows the texcoords."""
    rng = np.random.default_rng(seed)
    nv = CLIP_NV
    pos_f, uv_f = _frame_fields(pair, rng, nv), _frame_fields(pair, rng, nv)
    base, off, uoff, stride = place(pair.nbytes, pair.nbytes, CLIP_CLASSES[klass])
    junk = rng.integers(0, 256, size=nv)
    buf = vertex_buffer(nv, base, stride, [(off, pack(pair, pos_f, junk)), (uoff, pack(pair, uv_f, junk ^ 0xFF))])
    xy = decode_ref(pair, pos_f).view(np.float32)[:, :2].astype(np.float64)
    local = []
    for a in rng.permutation(nv)[:CLIP_LOCAL]:
        d = ((xy - xy[a]) ** 2).sum(axis=1)
        d[a] = np.inf
        b, c = np.argsort(d, kind="stable")[:2]
        if (xy[b, 0] - xy[a, 0]) * (xy[c, 1] - xy[a, 1]) - (xy[c, 0] - xy[a, 0]) * (xy[b, 1] - xy[a, 1]) < 0:
            b, c = c, b  # counter-clockwise in the plain view: front-facing
        local.append((int(a), int(b), int(c)))
    local.sort(key=lambda t: xy[list(t), 1].sum())
    rand = rng.integers(0, nv, size=(CLIP_RANDOM, 3))
    nedge = pair.ncomp * len(frame_edges(pair))
    rand[:nedge, 0] = np.arange(nedge)  # every planted edge code is a vertex of a far-reaching triangle
    idx = np.concatenate([np.array(local).reshape(-1), rand.reshape(-1)]).astype(np.uint16)
    prim = scene.pack_primitive(vertex_num=nv, vertex_stride=stride, topology=scene.TOPO_LIST, index_num=len(idx), vertex_base=base)
    md = scene.ModelData(vertex_buf=buf, index_buf=idx, prims=prim[None, :],
                         layouts=[[pair.element(scene.SEM_POSITION, off), pair.element(scene.SEM_TEXCOORD, uoff)]],
                         prim_to_texture=np.array([0], dtype=np.int32), prim_debug_id=np.array([3], dtype=np.uint32),
                         parts_disp=np.ones(1, dtype=np.uint8), textures=[scene.checker_rgba8_texture(16, 16, cell=2)])
    return ClipScene(f"{pair.name}-{klass}", pair, md, _views(pair))


CLIP_SCENE_NAMES = tuple(f"{p}-{k}" for p in PAIRS for k in CLIP_CLASSES)


@functools.lru_cache(maxsize=None)
def clip_scene(name: str) -> ClipScene:
    pname, klass = name.rsplit("-", 1)
    return _clip_scene(PAIRS[pname], klass, seed=100 + CLIP_SCENE_NAMES.index(name))


def clip_scenes() -> List[ClipScene]:
    return [clip_scene(n) for n in CLIP_SCENE_NAMES]
