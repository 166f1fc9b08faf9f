"""The skinned vertex stage at its numeric edges: an exact model of the vertex shader and the inputs that probe it.

Plain Python and numpy, no GPU.  Three parts:

* ``fma32``: the exact rational a * b + c rounded ONCE to nearest-even binary32, on bit patterns, in integer arithmetic
  (subnormals kept, underflow to a zero of the exact sum's sign, overflow to +-inf, IEEE rules for inf and NaN).  On top of
  it ``shade`` is SPEC "LBS" + clip = M (q, 1) written out again: it never calls the oracle, so it pins the oracle's
  ``fmaf`` (libm or the FMA unit of whatever CPU runs the suite) as well as the GPU's two chains.  Three deliberately
  wrong variants say what the inputs can detect: ``unfused`` (round the product, then the sum), ``daz`` (subnormal A / B
  operands of the multiply-add read as zero) and ``ftz`` (subnormal results of the multiply-add written as zero).
* case models for the vertex stage alone (``cases()``): every vertex is tagged with its family, every block of four
  consecutive vertex ids with its pattern (``block_patterns``), because a block is what k_vertex_stage hands to one MFMA.
* frame models for k_geom and the tile kernels (``frame_scenes()``): finite numbers only, everything on a small target.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import List, Optional

import numpy as np

from mt_renderer_amd import scene

# ---------------------------------------------------------------------------------------------
# exact binary32 arithmetic on bit patterns
# ---------------------------------------------------------------------------------------------
NAN = 0x7FC00000
INF = 0x7F800000
ONE = 0x3F800000
NEG_ZERO = 0x80000000
_ABS = 0x7FFFFFFF


def is_nan(b: int) -> bool:
    return (b & _ABS) > INF


def is_subnormal(b: int) -> bool:
    return 0 < (b & _ABS) < 0x00800000


def _dec(b: int):
    """finite bits -> (sign, integer significand, exponent): value = (-1)^sign * significand * 2^exponent"""
    e = (b >> 23) & 0xFF
    m = b & 0x7FFFFF
    return (b >> 31, m, -149) if e == 0 else (b >> 31, m | 0x800000, e - 150)


def _round(sign: int, n: int, e: int) -> int:
    """n * 2^e (n > 0, exact) -> nearest-even binary32 bits"""
    sh = n.bit_length() - 24
    if e + sh < -149:
        sh = -149 - e  # the subnormal quantum
    if sh <= 0:
        m = n << -sh
    else:
        m = n >> sh
        rem = n & ((1 << sh) - 1)
        half = 1 << (sh - 1)
        if rem > half or (rem == half and (m & 1)):
            m += 1
    # m < 2^23: subnormal (quantum 2^-149, exponent field 0); m in [2^23, 2^24]: the hidden bit carries into the field
    bits = ((e + sh + 149) << 23) + m
    return (sign << 31) | (INF if bits >= INF else bits)


def fma32(a: int, b: int, c: int, daz: bool = False, ftz: bool = False) -> int:
    if daz:
        if is_subnormal(a):
            a &= NEG_ZERO
        if is_subnormal(b):
            b &= NEG_ZERO
    if is_nan(a) or is_nan(b) or is_nan(c):
        return NAN
    ps = (a ^ b) >> 31
    a_inf, b_inf, c_inf = (a & _ABS) == INF, (b & _ABS) == INF, (c & _ABS) == INF
    if a_inf or b_inf:
        if (a & _ABS) == 0 or (b & _ABS) == 0:
            return NAN
        if c_inf and (c >> 31) != ps:
            return NAN
        return (ps << 31) | INF
    if c_inf:
        return c
    _, ma, xa = _dec(a)
    _, mb, xb = _dec(b)
    sc, mc, xc = _dec(c)
    if ma == 0 or mb == 0:
        if mc == 0:
            return (ps << 31) if ps == sc else 0  # (+0) + (-0) = +0 to nearest
        return c
    p, xp = ma * mb, xa + xb
    if mc == 0:
        r = _round(ps, p, xp)
    else:
        x = min(xp, xc)
        v = (p << (xp - x)) * (-1 if ps else 1) + (mc << (xc - x)) * (-1 if sc else 1)
        if v == 0:
            return 0  # exact cancellation: +0 to nearest
        r = _round(1 if v < 0 else 0, abs(v), x)
    if ftz and is_subnormal(r):
        r &= NEG_ZERO
    return r


def mul32(a: int, b: int) -> int:
    return fma32(a, b, NEG_ZERO)  # x + (-0) = x for every x, zeros included


def add32(a: int, c: int) -> int:
    return fma32(a, ONE, c)


def _fma_unfused(a, b, c):
    return add32(mul32(a, b), c)


def _fma_daz(a, b, c):
    return fma32(a, b, c, daz=True)


def _fma_ftz(a, b, c):
    return fma32(a, b, c, ftz=True)


VARIANTS = {"exact": fma32, "unfused": _fma_unfused, "daz": _fma_daz, "ftz": _fma_ftz}


def div32(n: int, d: int) -> int:
    """the IEEE quotient of two integers (each exact in binary32), d > 0"""
    if n == 0:
        return 0
    q, r = divmod(abs(n) << 64, d)
    return _round(1 if n < 0 else 0, (q << 1) | (1 if r else 0), -65)  # the sticky bit keeps the rounding exact


UNORM8 = [div32(v, 255) for v in range(256)]


def snorm16_bits(v: int) -> int:
    return 0xBF800000 if v == -32768 else div32(v, 32767)  # max(v / 32767, -1)


def shade(pos, jw, ww, pal, M, fma=fma32):
    """SPEC "LBS" and clip = M (q, 1) for one vertex, all on bit patterns.  pos: 3 position words; jw, ww: the four joint
    and weight bytes; pal: list of 16-word matrices (column-major) or None; M: 16 words.  Returns the four clip words."""
    q = [pos[0], pos[1], pos[2], ONE]
    if pal is not None:
        npal = len(pal)
        pin = q
        acc = [0, 0, 0]
        for k in range(4):
            P = pal[min(jw[k], npal - 1)]
            wk = UNORM8[ww[k]]
            for c in range(4):
                s = mul32(wk, pin[c])
                for i in range(3):
                    acc[i] = fma(P[c * 4 + i], s, acc[i])
        q = [acc[0], acc[1], acc[2], ONE]
    clip = []
    for i in range(4):
        a = 0
        for c in range(4):
            a = fma(M[c * 4 + i], q[c], a)
        clip.append(a)
    return clip


# ---------------------------------------------------------------------------------------------
# case models
# ---------------------------------------------------------------------------------------------
FAMILIES = ("benign", "cancel", "subnormal", "large", "zeros", "weights", "joints")
NPALS = (None, 1, 5, 64, 256)
TAIL_VERTEX_NUMS = (1, 2, 3, 5, 63, 64, 65, 257)
F32_LAYOUT = [(scene.SEM_POSITION, scene.IEF_F32, 3, 0), (scene.SEM_TEXCOORD, scene.IEF_F16, 2, 12),
              (scene.SEM_JOINT, scene.IEF_U8, 4, 16), (scene.SEM_WEIGHT, scene.IEF_U8N, 4, 20)]
S16_LAYOUT = [(scene.SEM_POSITION, scene.IEF_S16N, 3, 0), (scene.SEM_TEXCOORD, scene.IEF_F16, 2, 8),
              (scene.SEM_JOINT, scene.IEF_U8, 4, 12), (scene.SEM_WEIGHT, scene.IEF_U8N, 4, 16)]


@dataclasses.dataclass
class Case:
    name: str
    md: scene.ModelData
    pal: np.ndarray          # float32 [256, 16]; the tests take pal[:npal]
    M: np.ndarray            # float32 [16]
    family: List[str]        # per vertex of the vertex buffer
    prims: List[tuple]       # (first vertex, vertex_num) per primitive
    pos_bits: np.ndarray     # uint32 [nv, 3]: the decoded position, exact
    joints: np.ndarray       # uint8 [nv, 4]
    weights: np.ndarray      # uint8 [nv, 4]
    uv: np.ndarray           # float32 [nv, 2]

    def patterns(self, prim: int) -> List[str]:
        v0, n = self.prims[prim]
        return block_patterns(self.joints[v0:v0 + n], self.weights[v0:v0 + n])


def block_patterns(joints: np.ndarray, weights: np.ndarray) -> List[str]:
    """per vertex, the pattern of its block of four consecutive vertex ids as k_vertex_stage sees it"""
    n = len(joints)
    out = []
    for b0 in range(0, n, 4):
        j, w = joints[b0:b0 + 4], weights[b0:b0 + 4]
        if len(j) < 4:
            tag = f"tail{len(j)}"  # inactive lanes: never coherent
        elif (j == j[0]).all():
            tag = "coherent"
        else:
            differs = (j != j[0]).any(axis=0)  # slots in which the words differ
            if (w[:, differs] == 0).all():
                tag = "zero_weight_slot"
            else:
                words = [bytes(r) for r in j]
                odd = [l for l in range(4) if sum(words[l] == x for x in words) == 1]
                tag = f"one_differs_lane{odd[0]}" if len(odd) == 1 and len(set(words)) == 2 else "mixed"
        out += [tag] * len(j)
    return out


def _f32(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def _pw(rng, e_lo, e_hi, size, sign=0):
    """+-2^e (1 + u), e uniform in [e_lo, e_hi]; sign 0: random, +1 / -1: fixed"""
    v = np.ldexp(1.0 + rng.random(size), rng.integers(e_lo, e_hi + 1, size))
    s = np.where(rng.random(size) < 0.5, -1.0, 1.0) if sign == 0 else float(sign)
    return (v * s).astype(np.float32)


def _sub(rng, size):
    """random subnormals of either sign"""
    b = rng.integers(1, 1 << 23, size).astype(np.uint32) | (rng.integers(0, 2, size).astype(np.uint32) << np.uint32(31))
    return b.view(np.float32)


def _rigid(rng, angle=1.0, shift=0.4):
    A = np.eye(4)
    q = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    A[:3, :3] = q if angle >= 1.0 else np.eye(3) + angle * (q - q.T) * 0.5
    A[:3, 3] = rng.uniform(-shift, shift, size=3)
    return scene.to_f32_colmajor(A)


def rigid_palette(seed, angle=1.0, shift=0.4) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return np.stack([_rigid(rng, angle, shift) for _ in range(256)])


def cancel_palette(seed, angle=1.0) -> np.ndarray:
    """joints 4g, 4g + 1: one linear part and translations +T, -T with |T| = 2^k on every axis, k = g % 17 (the pair
    cancels when its two weights are equal); joints 4g + 2, 4g + 3: ordinary small rigid matrices"""
    rng = np.random.default_rng(seed)
    pal = np.zeros((256, 16), dtype=np.float32)
    for g in range(64):
        a = _rigid(rng, angle, 0.0)
        t = np.ldexp(np.where(rng.random(3) < 0.5, -1.0, 1.0), g % 17)
        pal[4 * g], pal[4 * g + 1] = a, a
        pal[4 * g, 12:15], pal[4 * g + 1, 12:15] = t, -t
        pal[4 * g + 2], pal[4 * g + 3] = _rigid(rng, angle, 0.3), _rigid(rng, angle, 0.3)
    return pal


def pair_words(rng, n):
    """joint words (4g, 4g + 1, 4g' + 2, 4g'' + 3) for the cancel palette"""
    g = rng.integers(0, 64, size=(n, 3))
    return np.stack([4 * g[:, 0], 4 * g[:, 0] + 1, 4 * g[:, 1] + 2, 4 * g[:, 2] + 3], axis=1).astype(np.uint8)


def pair_weights(rng, n, rest=True):
    """(w, w, a, b) with 2 w + a + b = 255: the pair's large terms cancel"""
    w = rng.integers(1, 120, size=n)
    a = rng.integers(0, 256 - 2 * w) if rest else np.zeros(n, dtype=np.int64)
    b = 255 - 2 * w - a if rest else np.zeros(n, dtype=np.int64)
    return np.stack([w, w, a, b], axis=1).astype(np.uint8)


def normalised_weights(rng, n):
    raw = rng.integers(1, 256, size=(n, 4)).astype(np.int64)
    w = raw * 255 // raw.sum(axis=1, keepdims=True)
    w[:, 0] += 255 - w.sum(axis=1)
    return w.astype(np.uint8)


def alternate_blocks(words: np.ndarray) -> np.ndarray:
    """words [nblocks, 4] -> joints [4 nblocks, 4]: even blocks wholly coherent, odd blocks with one lane (each position in
    turn) on the next block's word, so that every family meets the MFMA chain and the VALU chain"""
    nb = len(words)
    j = np.repeat(words, 4, axis=0)
    for b in range(1, nb, 2):
        j[4 * b + (b // 2) % 4] = words[(b + 1) % nb]
    return j


HEADLINE_M = scene.to_f32_colmajor(scene.headline_transform(192, 112))


def _model(pos, uv, joints, weights, prims, s16=False):
    nv = len(joints)
    lay = S16_LAYOUT if s16 else F32_LAYOUT
    stride = 20 if s16 else 24
    vb = np.zeros((nv, stride), dtype=np.uint8)
    if s16:
        vb[:, 0:6] = np.asarray(pos, dtype="<i2").view(np.uint8).reshape(nv, 6)
        vb[:, 6:8] = 0x5A  # the w component: never read
    else:
        vb[:, 0:12] = np.ascontiguousarray(pos, dtype=np.float32).view(np.uint8).reshape(nv, 12)
    uo = lay[1][3]
    vb[:, uo:uo + 4] = np.ascontiguousarray(uv, dtype="<f2").view(np.uint8).reshape(nv, 4)
    vb[:, uo + 4:uo + 8] = joints
    vb[:, uo + 8:uo + 12] = weights
    packed = [scene.pack_primitive(vertex_num=n, weight_num=4, vertex_stride=stride, topology=scene.TOPO_LIST,
                                   vertex_base=v0 * stride, index_num=3) for v0, n in prims]
    return scene.ModelData(vertex_buf=vb.reshape(-1), index_buf=np.zeros(3, dtype=np.uint16), prims=np.stack(packed),
                           layouts=[list(lay) for _ in prims], prim_to_texture=np.full(len(prims), -1, dtype=np.int32),
                           prim_debug_id=np.arange(len(prims), dtype=np.uint32), parts_disp=np.ones(len(prims), dtype=np.uint8))


def _case(name, pos, joints, weights, pal, M, family, prims=None, s16=False) -> Case:
    nv = len(joints)
    rng = np.random.default_rng(nv)
    uv = rng.uniform(-2.0, 2.0, size=(nv, 2)).astype(np.float16)
    uv[::7, 0] = np.float16(6e-6)  # a subnormal half: exact in binary32
    prims = prims or [(0, nv)]
    if s16:
        pos_bits = np.array([[snorm16_bits(int(v)) for v in row] for row in pos], dtype=np.uint32)
    else:
        pos_bits = np.ascontiguousarray(pos, dtype=np.float32).view(np.uint32).reshape(nv, 3)
    family = [family] * nv if isinstance(family, str) else list(family)
    assert len(family) == nv and set(family) <= set(FAMILIES) and pal.shape == (256, 16) and pal.dtype == np.float32
    return Case(name, _model(pos, uv, joints, weights, prims, s16), pal, np.ascontiguousarray(M, dtype=np.float32).reshape(16),
                family, prims, pos_bits, np.asarray(joints, dtype=np.uint8), np.asarray(weights, dtype=np.uint8), uv.astype(np.float32))


def _benign():
    rng = np.random.default_rng(11)
    n = 256
    words = rng.integers(0, 256, size=(n // 4, 4)).astype(np.uint8)
    return _case("benign", rng.uniform(-1, 1, size=(n, 3)), alternate_blocks(words), normalised_weights(rng, n),
                 rigid_palette(12), HEADLINE_M, "benign")


def _s16n():
    rng = np.random.default_rng(13)
    n = 128
    pos = rng.integers(-32768, 32768, size=(n, 3))
    pos[:4] = [[-32768, 32767, 0], [-32767, 1, -1], [0, 0, 0], [32767, -32768, 16384]]
    words = rng.integers(0, 256, size=(n // 4, 4)).astype(np.uint8)
    return _case("s16n", pos, alternate_blocks(words), normalised_weights(rng, n), rigid_palette(14), HEADLINE_M, "benign", s16=True)


def _cancel():
    rng = np.random.default_rng(21)
    n = 256
    pos = rng.uniform(-1, 1, size=(n, 3)).astype(np.float32)
    wts = pair_weights(rng, n)
    # one block in eight: the pair alone on a vertex at the origin: the skinned position is exactly +0, and with no
    # translation in x (below) so is clip x
    for b in range(0, n // 4, 8):
        pos[4 * b:4 * b + 4] = 0.0
        wts[4 * b:4 * b + 4, 2:] = 0
    # one block in eight: weights one apart, so 2^k / 255 is left over
    for b in range(3, n // 4, 8):
        wts[4 * b:4 * b + 4, 1] += 1
        wts[4 * b:4 * b + 4, 2:] = 0
    M = _f32(rng.uniform(0.3, 1.0, size=16) * np.where(rng.random(16) < 0.5, -1.0, 1.0))  # every product inexact
    M[12] = 0.0
    return _case("cancel", pos, alternate_blocks(pair_words(rng, n // 4)), wts, cancel_palette(22), M, "cancel")


def _subnormal_a():
    """clip = diag(0.75, -1.25, 0.5) q, w = 1: the skinned position shows in the output.  Joints 8r .. 8r + 7 belong to
    recipe r; 32 vertices each."""
    rng = np.random.default_rng(31)
    pal = np.zeros((256, 16), dtype=np.float32)
    pos = np.zeros((128, 3), dtype=np.float32)
    for j in range(8):   # r0: subnormal matrix entries (the A operand), large positions: normal products
        pal[j, :12] = _sub(rng, 12)
    pos[0:32] = _pw(rng, 100, 120, (32, 3))
    for j in range(8, 16):  # r1: large entries, subnormal positions (the B operand, w_k p_c)
        pal[j, :12] = _pw(rng, 100, 110, 12)
    pos[32:64] = _sub(rng, (32, 3))
    for j in range(16, 24):  # r2: products and sums that are subnormal
        pal[j, :12] = _pw(rng, -72, -68, 12)
        pal[j, 12:15] = _sub(rng, 3)
    pos[64:96] = _pw(rng, -68, -62, (32, 3))
    for j in range(24, 32):  # r3: products that underflow to +-0 on a +-0 accumulator, then a subnormal translation
        pal[j, :12] = _pw(rng, -95, -90, 12)
        pal[j, 12:15] = _sub(rng, 3) if j & 1 else 0.0
    pos[96:128] = _pw(rng, -75, -70, (32, 3))
    pal[32:] = np.resize(pal[:32], (224, 16))
    words = np.concatenate([8 * r + rng.integers(0, 8, size=(8, 4)) for r in range(4)]).astype(np.uint8)
    wts = normalised_weights(rng, 128)
    wts[::5, 3] = 0
    M = scene.to_f32_colmajor(np.diag([0.75, -1.25, 0.5, 1.0]))
    return _case("subnormal_a", pos, alternate_blocks(words), wts, pal, M, "subnormal")


def _subnormal_b():
    """an ordinary positive palette; the clip chain itself (four steps, the path of unskinned draws too) works on a
    matrix whose rows are tiny: x underflows to -0 for small q, y is subnormal, z has subnormal entries"""
    rng = np.random.default_rng(32)
    pal = np.zeros((256, 16), dtype=np.float32)
    pal[:, :12] = rng.uniform(0.25, 1.0, size=(256, 12))
    pos = np.concatenate([_pw(rng, -42, -38, (64, 3), sign=1), _pw(rng, 18, 22, (64, 3), sign=1)])
    M = np.zeros(16, dtype=np.float32)
    for c in range(3):
        M[c * 4 + 0] = _pw(rng, -120, -120, 1, sign=-1)[0]
        M[c * 4 + 1] = _pw(rng, -106, -104, 1)[0]
        M[c * 4 + 2] = _sub(rng, 1)[0]
    M[12], M[13], M[14], M[15] = -0.0, 0.0, _sub(rng, 1)[0], 1.0
    words = rng.integers(0, 256, size=(32, 4)).astype(np.uint8)
    return _case("subnormal_b", pos, alternate_blocks(words), normalised_weights(rng, 128), pal, M, "subnormal")


def _large():
    rng = np.random.default_rng(41)
    n = 192
    pal = np.zeros((256, 16), dtype=np.float32)
    for j in range(256):
        pal[j, :15] = _pw(rng, 0, 0, 15) * np.float32(2.0 ** [90, 100, 110, 118, 120][j % 5])
    pos = _pw(rng, 0, 8, (n, 3))
    M = rng.uniform(0.3, 1.0, size=16) * np.where(rng.random(16) < 0.5, -1.0, 1.0)
    words = rng.integers(0, 256, size=(n // 4, 4)).astype(np.uint8)
    words[::3] = words[::3] // 5 * 5  # a third of the blocks on the 2^90 joints only: finite results
    return _case("large", pos, alternate_blocks(words), normalised_weights(rng, n), pal, _f32(M), "large")


def _zeros():
    rng = np.random.default_rng(51)
    n = 128
    vals = np.array([-0.0, 0.0, -0.0, 0.0, 1.0, -1.0, 0.5, -0.375], dtype=np.float32)
    pal = vals[rng.integers(0, 8, size=(256, 16))]
    pos = vals[rng.integers(0, 8, size=(n, 3))]
    wts = rng.integers(0, 256, size=(n, 4))
    wts[rng.random((n, 4)) < 0.4] = 0
    M = vals[rng.integers(0, 8, size=16)]
    M[12] = -0.0
    words = rng.integers(0, 256, size=(n // 4, 4)).astype(np.uint8)
    return _case("zeros", pos, alternate_blocks(words), wts.astype(np.uint8), pal, M, "zeros")


WEIGHT_WORDS = ((0, 0, 0, 0), (255, 255, 255, 255), (255, 0, 0, 0), (1, 1, 1, 252))


def _weights():
    rng = np.random.default_rng(61)
    n = 128
    wts = rng.integers(0, 256, size=(n, 4))  # un-normalised
    for i, w in enumerate(WEIGHT_WORDS):
        wts[i::8] = w  # half of the vertices on the four fixed words, each in both kinds of block
    words = rng.integers(0, 256, size=(n // 4, 4)).astype(np.uint8)
    return _case("weights", rng.uniform(-1, 1, size=(n, 3)), alternate_blocks(words), wts.astype(np.uint8), rigid_palette(62),
                 HEADLINE_M, "weights")


def _joints():
    rng = np.random.default_rng(71)
    n = 256
    edge = np.array([0, 1, 4, 5, 6, 63, 64, 65, 200, 254, 255], dtype=np.uint8)  # around every palette size, and 255
    j = np.zeros((n, 4), dtype=np.uint8)
    for b in range(n // 4):
        word = edge[rng.integers(0, len(edge), size=4)]
        kind = b % 4
        if kind == 0:    # coherent, edge indices
            j[4 * b:4 * b + 4] = word
        elif kind == 1:  # one joint in all four slots
            j[4 * b:4 * b + 4] = word[0]
        elif kind == 2:  # the same set of joints in permuted slot order: not coherent
            for l in range(4):
                j[4 * b + l] = np.roll(word, l)
        else:            # index 255 in one slot of one lane
            j[4 * b:4 * b + 4] = word
            j[4 * b + b % 4, (b // 4) % 4] = 255
    return _case("joints", rng.uniform(-1, 1, size=(n, 3)), j, normalised_weights(rng, n), rigid_palette(72), HEADLINE_M, "joints")


def _blocks():
    """one primitive per vertex_num of TAIL_VERTEX_NUMS on the cancel palette; the blocks cycle through: coherent, one
    lane differs (each position), words that differ only in a slot of weight 0, every lane on its own word"""
    rng = np.random.default_rng(81)
    prims, v0 = [], 0
    for n in TAIL_VERTEX_NUMS:
        prims.append((v0, n))
        v0 += n
    nv = v0
    pos = rng.uniform(-1, 1, size=(nv, 3))
    j = np.zeros((nv, 4), dtype=np.uint8)
    wts = pair_weights(rng, nv)
    for p0, n in prims:
        for b in range((n + 3) // 4):
            lo, hi = p0 + 4 * b, min(p0 + 4 * b + 4, p0 + n)
            word, other = pair_words(rng, 2)
            other[0], other[1] = word[0] ^ 4, word[1] ^ 4  # a different pair for certain
            kind = b % 7
            j[lo:hi] = word
            if 1 <= kind <= 4 and hi - lo == 4:
                j[lo + kind - 1] = other
            elif kind == 5:
                wts[lo:hi, 2] += wts[lo:hi, 3]
                wts[lo:hi, 3] = 0
                j[lo:hi, 3] = rng.integers(0, 256, size=hi - lo)
                j[lo, 3], j[hi - 1, 3] = 3, 7
            elif kind == 6:
                j[lo:hi] = pair_words(rng, hi - lo)
                j[lo:hi, 2] = np.arange(hi - lo) * 4 + 2
    return _case("blocks", pos, j, wts, cancel_palette(82), HEADLINE_M, "cancel", prims=prims)


def _unskinned_cancel():
    """for the clip chain alone (palette None): y within 2^-10 of x and a matrix whose x and y columns are +-K, so that
    the four-step chain cancels from thousands to order one"""
    rng = np.random.default_rng(101)
    n = 128
    pos = rng.uniform(-1, 1, size=(n, 3))
    pos[:, 1] = pos[:, 0] + rng.uniform(-1, 1, size=n) * 2.0 ** -10
    M = _M([[4099.3, -4099.3, 0.61, 0.2], [-8211.7, 8211.7, 0.3, -0.1], [1027.1, -1027.1, 0.4, 0.5], [-2053.9, 2053.9, 0.3, 1.0]])
    words = rng.integers(0, 256, size=(n // 4, 4)).astype(np.uint8)
    return _case("unskinned_cancel", pos, alternate_blocks(words), normalised_weights(rng, n), rigid_palette(102), M, "cancel")


UNSKINNED_CASES = ("unskinned_cancel", "subnormal_a", "subnormal_b")


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    return (_benign(), _s16n(), _cancel(), _unskinned_cancel(), _subnormal_a(), _subnormal_b(), _large(), _zeros(), _weights(), _joints(), _blocks())


def palette_of(case: Case, npal: Optional[int]) -> Optional[np.ndarray]:
    return None if npal is None else case.pal[:npal]


@functools.lru_cache(maxsize=None)
def _model_clip(ci: int, prim: int, npal: Optional[int], variant: str) -> np.ndarray:
    c = cases()[ci]
    v0, n = c.prims[prim]
    pal = None if npal is None else c.pal[:npal].view(np.uint32).tolist()
    M = c.M.view(np.uint32).tolist()
    fma = VARIANTS[variant]
    out = [shade(p, j, w, pal, M, fma) for p, j, w in zip(c.pos_bits[v0:v0 + n].tolist(), c.joints[v0:v0 + n].tolist(), c.weights[v0:v0 + n].tolist())]
    return np.array(out, dtype=np.uint32).reshape(n, 4)


def model_clip(case: Case, prim: int, npal: Optional[int], variant: str = "exact") -> np.ndarray:
    """clip words [vertex_num, 4] of the exact model (or one of its wrong variants); NaN is the one word NAN"""
    return _model_clip(cases().index(case), prim, npal, variant)


def same_words(got: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """elementwise: bits equal, or both NaN.  The only two classes there are."""
    got, ref = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(ref).view(np.uint32)
    nan_g, nan_r = (got & _ABS) > INF, (ref & _ABS) > INF
    return np.where(nan_r | nan_g, nan_r & nan_g, got == ref)


def describe_first_difference(case: Case, prim: int, ok: np.ndarray, got: np.ndarray, ref: np.ndarray) -> str:
    """family and block pattern of the first vertex with a differing word, so that a flush reads as one"""
    bad = np.nonzero(~ok.reshape(len(ok), -1).all(axis=1))[0]
    v = int(bad[0])
    v0, _ = case.prims[prim]
    fam = sorted({case.family[v0 + int(b)] for b in bad})
    g, r = np.ascontiguousarray(got).view(np.uint32)[v], np.ascontiguousarray(ref).view(np.uint32)[v]
    return (f"{case.name} prim {prim}: {len(bad)} vertices differ (families {fam}); first: vertex {v}, lane {v & 3}, family "
            f"{case.family[v0 + v]}, block {case.patterns(prim)[v]}, joints {case.joints[v0 + v].tolist()}, weights "
            f"{case.weights[v0 + v].tolist()}, got {[hex(int(x)) for x in g]}, expected {[hex(int(x)) for x in r]}")


# ---------------------------------------------------------------------------------------------
# frame models: k_geom and the tile kernels
# ---------------------------------------------------------------------------------------------
FRAME_W, FRAME_H = 192, 112
STRIP_LENGTHS = (3, 4, 5, 6, 7, 9, 13, 31, 61, 62, 63, 64, 125)
JOINT_PATTERNS = ("rail", "random", "zero_slot")
INDEX_BASE = 5
COLS = 64


@functools.lru_cache(maxsize=None)
def strip_runs() -> tuple:
    """the lengths between restarts, drawn from STRIP_LENGTHS until the restarts have fallen at EVERY phase of the
    62-position chunk (so also at every phase of the four-lane block, and the rails change places inside chunks): next
    comes a length whose restart falls at a phase no earlier restart had -- of those the length used least so far, then
    the shortest -- and where no length reaches a new phase, the length used least.  One last run follows the last restart."""
    runs, seen, at = [], set(), 0
    used = {L: 0 for L in STRIP_LENGTHS}
    while len(seen) < 62 or min(used.values()) == 0:
        fresh = [L for L in STRIP_LENGTHS if (at + L) % 62 not in seen]
        L = min(fresh or STRIP_LENGTHS, key=lambda n: (used[n], n))
        used[L] += 1
        runs.append(L)
        at += L + 1          # the restart index itself, at position at - 1
        seen.add((at - 1) % 62)
        assert len(runs) < 400
    return tuple(runs) + (STRIP_LENGTHS[-1],)


def frame_model(pattern: str, topology: int, z_lo=-0.9, z_hi=0.9, seed=5) -> scene.ModelData:
    """ribbons of two rails, one per run of strip_runs(), packed into rows; every index has a vertex of its own.  Joint
    words are (4g, 4g + 1, 4g' + 2, 4g'' + 3) and weights (w, w, a, b) with 2 w + a + b = 255, so that the model stands on
    a rigid palette and on the cancel palette alike."""
    assert pattern in JOINT_PATTERNS
    rng = np.random.default_rng(seed)
    runs = list(strip_runs())
    place, row, col = [], 0, 0
    for L in runs:
        ncol = (L + 1) // 2
        if col + ncol > COLS - 1:
            row, col = row + 1, 0
        place.append((row, col))
        col += ncol + 1
    nrows = row + 1
    pos, rail_of, strip_of = [], [], []
    for s, L in enumerate(runs):
        row, col = place[s]
        for i in range(L):
            c, rail = col + i // 2, i & 1
            t = (c + 0.5 * rail) / COLS
            y = 0.85 - 1.7 * row / (nrows - 1) + (-0.075 if rail else 0.075)
            z = z_lo + (z_hi - z_lo) * (0.5 + 0.5 * np.sin(5.0 * t + 0.9 * row))
            pos.append((-0.92 + 1.84 * t, y, z))
            rail_of.append(rail)
            strip_of.append(s)
    nv = len(pos)
    rail_of, strip_of = np.array(rail_of), np.array(strip_of)
    per_rail = pair_words(rng, 2 * len(runs))
    joints = per_rail[2 * strip_of + rail_of].copy()
    wts = pair_weights(rng, nv)
    if pattern == "random":
        joints = pair_words(rng, nv)
    elif pattern == "zero_slot":
        wts[:, 2] += wts[:, 3]
        wts[:, 3] = 0
        joints[:, 3] = rng.integers(0, 256, size=nv)
    junk = INDEX_BASE
    P = np.concatenate([np.full((junk, 3), 0.33), np.array(pos)]).astype(np.float32)
    J = np.concatenate([np.zeros((junk, 4), dtype=np.uint8), joints])
    Wt = np.concatenate([np.full((junk, 4), 63, dtype=np.uint8), wts])
    uv = np.zeros((nv + junk, 2), dtype=np.float16)
    # indices: local ids, the primitive's index_base puts the junk in front; three ordinary indices past vertex_num
    first = np.concatenate([[0], np.cumsum(runs)])
    strips = [np.arange(first[s], first[s + 1]) for s in range(len(runs))]
    for s, i in zip(np.argsort(runs)[-3:], (40, 17, 30)):  # inside three of the long runs
        strips[s] = strips[s].copy()
        strips[s][i] = nv + 3
    if topology == scene.TOPO_STRIP:
        idx = []
        for s, st in enumerate(strips):
            idx += list(st) + ([0xFFFF] if s != len(strips) - 1 else [])
    else:
        idx = []
        for st in strips:
            for i in range(len(st) - 2):
                idx += [st[i], st[i + 2], st[i + 1]] if i & 1 else [st[i], st[i + 1], st[i + 2]]
    md = _model(P, uv, J, Wt, [(0, nv + junk)])
    md.index_buf = np.array(idx, dtype=np.uint16)
    md.prims = scene.pack_primitive(vertex_num=nv + junk, weight_num=4, vertex_stride=24, topology=topology, index_num=len(idx),
                                    index_base=INDEX_BASE)[None, :]
    md.prim_debug_id = np.array([7], dtype=np.uint32)
    return md


def _M(rows) -> np.ndarray:
    return scene.to_f32_colmajor(np.array(rows, dtype=np.float64))


PLAIN_M = _M([[0.7, 0, 0.07, 0], [0, 0.7, 0, 0], [0, 0, 0.4, 0.5], [0, 0, 0.3, 1.0]])   # w = 1 + 0.3 z, depth in (0.1, 0.9)
NEAR_M = _M([[0.7, 0, 0.07, 0], [0, 0.7, 0, 0], [0, 0, 0.5, 0.1], [0, 0, 0.3, 1.0]])    # clip z < 0 where z < -0.2


def tiny_z_inputs():
    """the palette's z row scaled by 2^-100 and a clip matrix that scales z by 2^-40 more: clip z, and with w near 1 the
    depth buffer, hold subnormals"""
    pal = rigid_palette(91, angle=0.1, shift=0.03)
    pal[:, 2::4] *= np.float32(2.0 ** -100)   # row z of every column, the translation too
    M = _M([[0.7, 0, 0, 0], [0, 0.7, 0, 0], [0, 0, 2.0 ** -40, 2.0 ** -143], [0.2, 0, 0, 1.0]])
    return pal, M


def batch_inputs():
    """five instances, 256 matrices each, the palette rolled per instance; view_proj and the model matrices carry
    translations of thousands that cancel in their product (the chain of stage_palette).  Of the middle band of three,
    rows 32 to 63 of the target, instances 1, 2 and 3 stay clear (a rank that owns it culls them) and 0 and 4 straddle
    its two borders"""
    pal = rigid_palette(92, angle=0.1, shift=0.03)
    pals = np.stack([np.roll(pal, 51 * k, axis=0) for k in range(5)])
    t = 3334.3
    A = np.array([[0.5, 0, 0.03, 0], [0, 0.5, 0, 0], [0, 0, 0.12, 0.5], [0, 0, 0.09, 1.0]])
    vp = A @ scene.mat_translate(t, -t, 0.0)
    mats = [scene.to_f32_colmajor(scene.mat_translate(-t + dx, t + dy, 0.05 * k) @ scene.mat_scale(0.6, 0.45, 1.0))
            for k, (dx, dy) in enumerate([(0.0, 0.0), (-1.1, 1.5), (1.1, -1.5), (-1.0, -0.9), (1.1, 0.85)])]
    return scene.to_f32_colmajor(vp), np.stack(mats), pals


@functools.lru_cache(maxsize=None)
def frame_scenes() -> dict:
    """name -> list of draws for tests.helpers (render_gpu / render_oracle), all on a FRAME_W x FRAME_H target"""
    S, L = scene.TOPO_STRIP, scene.TOPO_LIST
    rigid = rigid_palette(90, angle=0.1, shift=0.03)
    out = {}
    for pattern in JOINT_PATTERNS:
        out[f"strips_{pattern}"] = [dict(md=frame_model(pattern, S), M=PLAIN_M, palette=rigid)]
        out[f"list_{pattern}"] = [dict(md=frame_model(pattern, L), M=PLAIN_M, palette=rigid)]
    out["cancel_palette"] = [dict(md=frame_model("rail", S), M=PLAIN_M, palette=cancel_palette(93, angle=0.1)),
                             dict(md=frame_model("random", L), M=PLAIN_M, palette=cancel_palette(94, angle=0.1))]
    # random joints: every block incoherent, the clip chain alone is MFMA against the clipper's VALU re-shade; then joints
    # per rail on the cancel palette: MFMA-skinned vertices of unclipped triangles meet their VALU re-shade in clipped ones
    out["near_plane_random"] = [dict(md=frame_model("random", S), M=NEAR_M, palette=rigid),
                                dict(md=frame_model("rail", S), M=NEAR_M, palette=cancel_palette(95, angle=0.1))]
    tpal, tM = tiny_z_inputs()
    out["tiny_z"] = [dict(md=frame_model("random", S, z_lo=0.1, z_hi=1.0), M=tM, palette=tpal),
                     dict(md=frame_model("rail", S, z_lo=0.1, z_hi=1.0), M=tM, palette=tpal)]
    vp, mats, pals = batch_inputs()
    out["batch_npal256"] = [dict(md=frame_model("random", S), vp=vp, model_mats=mats, palettes=pals)]
    return out
