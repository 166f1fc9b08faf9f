"""The BC7 / BC1 blocks that tests/test_bc_block_premises.py (CPU) and tests/test_gpu_bc_blocks.py (GPU) decode: every
block layout on purpose rather than whatever a few thousand random blocks happen to reach.  Deterministic; the only random
generator is scene.splitmix64.

BC7 families   coverage   K blocks for each of the 285 (mode, partition, rotation, index selection) combinations, every
                          other bit random
               extremes   per mode, at partition 0 and at the partition whose anchors lie furthest into the block: payload
                          all ones, all zeros, endpoints (0, max) and (max, 0) under all-zero and all-one indices
               mode_byte  first byte 0xFF, 0xFE .. 0x80: the lowest set bit is the mode, the bits above it are payload
               reserved   first byte 0 (SPEC.md section 8: transparent black), the other 15 bytes 0x00, 0xFF, random
BC1 families   green      every pair of 6-bit greens (c0 > c1, c0 < c1 and the diagonal c0 == c1), red and blue shared
               red, blue  every pair of 5-bit reds / blues, the other two fields shared
               edges      c0, c1 in {0, 0xFFFF} squared, under every selector word
               every BC1 block takes one of four selector words in turn; between them each texel takes each selector."""
from __future__ import annotations

import dataclasses
import math
from typing import List, Tuple

import numpy as np

from mt_renderer_amd import scene
from tests.bc_model import MODES, tables

K = 2  # blocks per combination: the smallest count (>= 2) at which test_bc_block_premises.py's conditions hold

SELECTOR_WORDS = (0xE4E4E4E4, 0x39393939, 0x4E4E4E4E, 0x93939393)


def combinations() -> List[Tuple[int, int, int, int]]:
    """the 285 (mode, partition, rotation, index selection) a BC7 block can name"""
    out = []
    for mode, (ns, pb, rb, isb) in ((m, MODES[m][:4]) for m in range(8)):
        out += [(mode, p, r, s) for p in range(1 << pb) for r in range(1 << rb) for s in range(1 << isb)]
    return out


def _rand128(seed: int, n: int) -> List[int]:
    r = scene.splitmix64(np.uint64(seed) * np.uint64(0x10001) + np.arange(2 * n, dtype=np.uint64))
    return [int(r[2 * i]) | (int(r[2 * i + 1]) << 64) for i in range(n)]


def _header(mode, part=0, rot=0, isel=0):
    """(value, bit count) of the mode bit and the fields that follow it"""
    ns, pb, rb, isb = MODES[mode][:4]
    v, n = 1 << mode, mode + 1
    for val, bits in ((part, pb), (rot, rb), (isel, isb)):
        assert 0 <= val < 1 << bits or (bits == 0 and val == 0)
        v |= val << n
        n += bits
    return v, n


def _with_header(payload: int, mode, part=0, rot=0, isel=0) -> bytes:
    v, n = _header(mode, part, rot, isel)
    return (((payload >> n) << n | v) & ((1 << 128) - 1)).to_bytes(16, "little")


def bc7_coverage(k: int = K) -> List[bytes]:
    combos = combinations()
    rnd = _rand128(7001, len(combos) * k)
    return [_with_header(rnd[ci * k + j], *c) for ci, c in enumerate(combos) for j in range(k)]


def _set_field(v, pos, bits, val):
    return (v & ~(((1 << bits) - 1) << pos)) | (val << pos)


def bc7_endpoint_block(mode, part, lo_first: bool, indices_max: bool, rot=0, isel=0) -> bytes:
    """every channel of every subset runs from 0 to its maximum (lo_first) or back, the p-bit of a zero endpoint 0 and of
    a maximal one 1 (mode 1's shared p-bits: 1), every index bit 0 or 1"""
    ns, pb, rb, isb, cb, ab, epb, spb, ib, ib2 = MODES[mode]
    v, pos = _header(mode, part, rot, isel)
    ne = 2 * ns
    for bits in [cb] * 3 + ([ab] if ab else []):
        for e in range(ne):
            v = _set_field(v, pos, bits, ((1 << bits) - 1) if (e & 1) == (1 if lo_first else 0) else 0)
            pos += bits
    if epb:
        for e in range(ne):
            v = _set_field(v, pos, 1, 1 if (e & 1) == (1 if lo_first else 0) else 0)
            pos += 1
    elif spb:
        v = _set_field(v, pos, ns, (1 << ns) - 1)
        pos += ns
    if indices_max:
        v |= ((1 << (128 - pos)) - 1) << pos
    return v.to_bytes(16, "little")


def far_anchor_partition(mode) -> int:
    """the partition of a multi-subset mode whose anchors lie furthest into the block: largest (last anchor, sum of
    anchors), the highest-numbered among equals"""
    ns, pb = MODES[mode][:2]
    T = tables()
    anch = (lambda p: (T["ANCHOR2_1"][p],)) if ns == 2 else (lambda p: (T["ANCHOR3_1"][p], T["ANCHOR3_2"][p]))
    return max(range(1 << pb), key=lambda p: (max(anch(p)), sum(anch(p)), p))


def bc7_extremes() -> List[bytes]:
    out = []
    ones = (1 << 128) - 1
    for mode in range(8):
        ns, pb, rb, isb = MODES[mode][:4]
        for part in ([0, far_anchor_partition(mode)] if ns > 1 else [0]):
            n = mode + 1 + pb  # rotation and index selection are payload here
            v = (1 << mode) | (part << (mode + 1))
            out.append((((ones >> n) << n) | v).to_bytes(16, "little"))
            out.append(v.to_bytes(16, "little"))
            out += [bc7_endpoint_block(mode, part, lo, imax) for imax in (False, True) for lo in (True, False)]
    return out


def bc7_mode_byte() -> List[bytes]:
    rnd = _rand128(7003, 128)
    return [((rnd[i] & ~0xFF) | (0xFF - i)).to_bytes(16, "little") for i in range(128)]


def bc7_reserved() -> List[bytes]:
    rnd = _rand128(7004, 4)
    return [bytes(16), bytes([0] + [0xFF] * 15)] + [(r & ~0xFF).to_bytes(16, "little") for r in rnd]


def bc7_alpha_255_blocks(n: int, seed: int = 7005) -> List[bytes]:
    """n blocks of the modes that carry alpha -- 4, 5, 6, 7 in turn -- whose alpha is 255 in every texel by VALUE: rotation
    0, both alpha endpoints of every subset at their maximum, every p-bit 1; colour, partition and indices random"""
    out = []
    for i, r in enumerate(_rand128(seed, n)):
        mode = 4 + i % 4
        ns, pb, rb, isb, cb, ab, epb, spb, ib, ib2 = MODES[mode]
        hv, hn = _header(mode, (r >> 8) & ((1 << pb) - 1), 0, (r >> 16) & ((1 << isb) - 1))
        v = ((r >> hn) << hn) | hv
        pos = hn + 3 * 2 * ns * cb
        v = _set_field(v, pos, 2 * ns * ab, (1 << (2 * ns * ab)) - 1)
        pos += 2 * ns * ab
        if epb:
            v = _set_field(v, pos, 2 * ns, (1 << (2 * ns)) - 1)
        out.append(v.to_bytes(16, "little"))
    return out


def _bc1(c0, c1, word) -> bytes:
    return (c0 | (c1 << 16) | (word << 32)).to_bytes(8, "little")


def _bc1_pairs(bits, shift, seed) -> List[bytes]:
    n = 1 << bits
    rnd = scene.splitmix64(np.uint64(seed) + np.arange(n * n, dtype=np.uint64))
    out = []
    for a in range(n):
        for b in range(n):
            shared = int(rnd[a * n + b]) & 0xFFFF & ~(((1 << bits) - 1) << shift)
            out.append(_bc1(shared | (a << shift), shared | (b << shift), SELECTOR_WORDS[(a * n + b) % 4]))
    return out


def bc1_green() -> List[bytes]:
    return _bc1_pairs(6, 5, 7011)


def bc1_red() -> List[bytes]:
    return _bc1_pairs(5, 11, 7012)


def bc1_blue() -> List[bytes]:
    return _bc1_pairs(5, 0, 7013)


def bc1_edges() -> List[bytes]:
    return [_bc1(c0, c1, w) for c0, c1 in ((0xFFFF, 0), (0, 0xFFFF), (0, 0), (0xFFFF, 0xFFFF)) for w in SELECTOR_WORDS]


BC7_FAMILIES = {"coverage": bc7_coverage, "extremes": bc7_extremes, "mode_byte": bc7_mode_byte, "reserved": bc7_reserved}
BC1_FAMILIES = {"green": bc1_green, "red": bc1_red, "blue": bc1_blue, "edges": bc1_edges}
_cache = {}


def blocks(fmt: str, family: str) -> List[bytes]:
    """the blocks of one family, built once"""
    if (fmt, family) not in _cache:
        _cache[fmt, family] = ({"bc7": BC7_FAMILIES, "bc1": BC1_FAMILIES}[fmt])[family]()
    return _cache[fmt, family]


@dataclasses.dataclass
class CaseTexture:
    fmt: str            # "bc7" or "bc1"
    family: str
    tex: scene.TextureData
    bw: int             # blocks per row
    bh: int
    nblocks: int        # the family's blocks come first, row-major; blocks from nblocks on repeat them from the start

    def block(self, bx, by) -> bytes:
        n = 16 if self.fmt == "bc7" else 8
        i = by * self.bw + bx
        return self.tex.data[i * n:(i + 1) * n]


# texels cropped off the right and the bottom: every amount from 1 to 3 on both axes over the families
CROPS = {"coverage": (3, 1), "extremes": (1, 3), "mode_byte": (2, 2), "reserved": (1, 1),
         "green": (3, 1), "red": (1, 2), "blue": (2, 3), "edges": (3, 3)}


def case_textures(fmt: str, family: str, crop: Tuple[int, int] = (0, 0)) -> List[CaseTexture]:
    """the family as textures of at most 256 x 256 texels (64 x 64 blocks), row-major in blocks, as square as the count
    allows and padded to whole rows with its own first blocks.  crop = (cx, cy), 0..3 each: the same bytes declared cx
    texels narrower and cy lower -- the block data of a 4bw x 4bh image is also that of a (4bw-cx) x (4bh-cy) one."""
    assert 0 <= crop[0] <= 3 and 0 <= crop[1] <= 3
    bl = blocks(fmt, family)
    out = []
    for start in range(0, len(bl), 64 * 64):
        part = bl[start:start + 64 * 64]
        bw = min(64, math.isqrt(len(part) - 1) + 1)
        bh = (len(part) + bw - 1) // bw
        data = b"".join(part[i % len(part)] for i in range(bw * bh))
        tex = scene.TextureData(4 * bw - crop[0], 4 * bh - crop[1], scene.TEX_BC7 if fmt == "bc7" else scene.TEX_BC1, data)
        out.append(CaseTexture(fmt, family, tex, bw, bh, len(part)))
    return out


BLEND_ALPHA, BLEND_OFF = 0, 1  # include/mtr.h: MTR_BLEND_ALPHA (the default), MTR_BLEND_OFF (replace)


def one_to_one_draws(tex: scene.TextureData, blend=None):
    """(w, h, draws): the texture on a quad of its own size, one texel per pixel; blend None leaves the default material
    state (alpha blend), BLEND_OFF stores the sampled texel as it is, so that the frame shows all four bytes of it"""
    from tests.pixel_scenes import pixel_model, pixel_to_ndc_matrix
    w, h = tex.width, tex.height
    verts = [(0, 0, 0.5, 0.0, 0.0), (0, h, 0.5, 0.0, 1.0), (w, 0, 0.5, 1.0, 0.0), (w, h, 0.5, 1.0, 1.0)]
    md = pixel_model([dict(verts=verts, indices=[0, 1, 2, 3], topology=scene.TOPO_STRIP, texture=0)], textures=[tex])
    if blend is not None:
        md.prim_states = np.array([(blend, 1, 1, 0)], dtype=np.uint8)  # depth write and test on, cull back: the default
    return w, h, [dict(md=md, M=pixel_to_ndc_matrix(w, h))]


ALL_FAMILIES =[("bc7", f) for f in BC7_FAMILIES] + [("bc1", f) for f in BC1_FAMILIES]
