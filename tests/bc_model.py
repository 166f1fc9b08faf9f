"""A plain scalar BC7 / BC1 block decoder in Python integers, written from the Khronos Data Format Specification's
BPTC chapter and SPEC.md section 8 -- not from oracle/oracle.py or the HIP decoders.  The 128 (64) bits of a block are
one ``int``; every field is a shift and a mask of it, read in the order the format lists them:

    BC7   mode (unary, lowest set bit of the first byte) | partition | rotation | index selection |
          R of every endpoint | G | B | A | p-bits | primary indices | secondary indices

Only the partition and anchor tables are not typed here: they are parsed from oracle/bc7_tables.h, and what makes them
independent is Pillow, which tests/test_bc_block_premises.py holds this model to on every case block.

``mutate=`` builds deliberately wrong decoders (never the product), in the style of tests/ideal_renderer.py: each is one
plausible misreading of the format, and the premises prove that the case blocks of tests/bc_block_cases.py tell every one
of them from the right reading.  ``only=`` restricts a mutation to the blocks whose (mode, partition, rotation, index
selection) starts with the given tuple; every other block decodes correctly."""
from __future__ import annotations

import os
import re

#             subsets, partition bits, rotation bits, index-selection bits, colour bits, alpha bits,
#             p-bit per endpoint, p-bit per subset, primary index bits, secondary index bits
MODES = {0: (3, 4, 0, 0, 4, 0, 1, 0, 3, 0),
         1: (2, 6, 0, 0, 6, 0, 0, 1, 3, 0),
         2: (3, 6, 0, 0, 5, 0, 0, 0, 2, 0),
         3: (2, 6, 0, 0, 7, 0, 1, 0, 2, 0),
         4: (1, 0, 2, 1, 5, 6, 0, 0, 2, 3),
         5: (1, 0, 2, 0, 7, 8, 0, 0, 2, 2),
         6: (1, 0, 0, 0, 7, 7, 1, 0, 4, 0),
         7: (2, 6, 0, 0, 5, 5, 1, 0, 2, 0)}
WEIGHTS = {2: (0, 21, 43, 64), 3: (0, 9, 18, 27, 37, 46, 55, 64),
           4: (0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64)}

BC7_MUTANTS = ("partition_neighbour", "rotation_next", "isel_flipped", "anchor_full_width", "anchor_order",
               "secondary_anchor_full_width", "shared_pbit_per_endpoint", "alpha_without_pbit", "mode_from_highest_bit",
               "reserved_opaque")
BC1_MUTANTS = ("bc1_ge", "bc1_third_no_round", "bc1_half_no_round", "bc1_selector_shift")

_tables = None


def tables():
    """{"PART2": [64][16], "PART3": [64][16], "ANCHOR2_1": [64], "ANCHOR3_1": [64], "ANCHOR3_2": [64]} from oracle/bc7_tables.h"""
    global _tables
    if _tables is None:
        src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle", "bc7_tables.h")).read()
        t = {}
        for name, body in re.findall(r"BC7_(\w+?)(?:\[\d+\])+\s*=\s*\{([^}]*)\}", src):
            vals = [int(x) for x in body.split(",")]
            t[name] = [vals[16 * p:16 * p + 16] for p in range(64)] if name.startswith("PART") else vals
        assert sorted(t) == ["ANCHOR2_1", "ANCHOR3_1", "ANCHOR3_2", "PART2", "PART3"] and all(len(v) == 64 for v in t.values())
        _tables = t
    return _tables


def bc7_fields(block):
    """(mode, partition, rotation, index selection) of a block, None for the reserved mode"""
    v = int.from_bytes(bytes(block), "little")
    if v & 0xFF == 0:
        return None
    mode = ((v & 0xFF) & -(v & 0xFF)).bit_length() - 1
    ns, pb, rb, isb = MODES[mode][:4]
    pos = mode + 1
    part = (v >> pos) & ((1 << pb) - 1)
    rot = (v >> (pos + pb)) & ((1 << rb) - 1)
    isel = (v >> (pos + pb + rb)) & ((1 << isb) - 1)
    return mode, part, rot, isel


def _expand(x, prec):
    x <<= 8 - prec
    return x | (x >> prec)


def decode_bc7(block, mutate=None, only=None):
    """16 bytes -> 16 (r, g, b, a) tuples, texel i = 4*y + x"""
    assert mutate is None or mutate in BC7_MUTANTS, mutate
    v = int.from_bytes(bytes(block), "little")
    assert 0 <= v < 1 << 128
    fields = bc7_fields(block)
    if only is not None and (fields is None or fields[:len(only)] != tuple(only)):
        mutate = None
    byte0 = v & 0xFF
    if byte0 == 0:  # reserved: SPEC.md section 8
        return [(0, 0, 0, 255 if mutate == "reserved_opaque" else 0)] * 16
    mode = byte0.bit_length() - 1 if mutate == "mode_from_highest_bit" else (byte0 & -byte0).bit_length() - 1
    ns, pb, rb, isb, cb, ab, epb, spb, ib, ib2 = MODES[mode]
    pos = mode + 1

    def take(n):
        nonlocal pos
        r = (v >> pos) & ((1 << n) - 1)
        pos += n
        return r

    part, rot, isel = take(pb), take(rb), take(isb)
    if mutate == "rotation_next" and rb:
        rot = (rot + 1) & 3
    if mutate == "isel_flipped" and isb:
        isel ^= 1
    ne = 2 * ns
    ep = [[0, 0, 0, 255] for _ in range(ne)]
    for c in range(3):
        for e in range(ne):
            ep[e][c] = take(cb)
    if ab:
        for e in range(ne):
            ep[e][3] = take(ab)
    cprec, aprec = cb, ab
    if epb or (spb and mutate == "shared_pbit_per_endpoint"):
        alpha_too = bool(epb and ab and mutate != "alpha_without_pbit")
        for e in range(ne):
            p = take(1)
            for c in range(3):
                ep[e][c] = (ep[e][c] << 1) | p
            if alpha_too:
                ep[e][3] = (ep[e][3] << 1) | p
        cprec += 1
        aprec += 1 if alpha_too else 0
    elif spb:
        for s in range(ns):
            p = take(1)
            for e in (2 * s, 2 * s + 1):
                for c in range(3):
                    ep[e][c] = (ep[e][c] << 1) | p
        cprec += 1
    for e in range(ne):
        for c in range(3):
            ep[e][c] = _expand(ep[e][c], cprec)
        if ab:
            ep[e][3] = _expand(ep[e][3], aprec)

    T = tables()
    sub_of = part ^ 1 if mutate == "partition_neighbour" else part
    if ns == 1:
        subset, anchors = [0] * 16, []
    elif ns == 2:
        subset, anchors = T["PART2"][sub_of], [T["ANCHOR2_1"][part]]
    else:
        subset, anchors = T["PART3"][sub_of], [T["ANCHOR3_1"][part], T["ANCHOR3_2"][part]]
    idx1, waiting = [], 0
    for i in range(16):
        if mutate == "anchor_full_width":
            short = i == 0
        elif mutate == "anchor_order":  # walks the anchor list once, in the order the tables give it
            short = i == 0 or (waiting < len(anchors) and i == anchors[waiting])
            if i > 0 and short:
                waiting += 1
        else:
            short = i == 0 or i in anchors
        idx1.append(take(ib - 1 if short else ib))
    idx2 = [take(ib2 - 1 if i == 0 and mutate != "secondary_anchor_full_width" else ib2) for i in range(16)] if ib2 else None
    assert mutate is not None or pos == 128, (mode, pos)

    out = []
    for i in range(16):
        e0, e1 = ep[2 * subset[i]], ep[2 * subset[i] + 1]
        ci, cbits, ai, abits = idx1[i], ib, idx1[i], ib
        if ib2:
            if isel:
                ci, cbits = idx2[i], ib2
            else:
                ai, abits = idx2[i], ib2
        wc, wa = WEIGHTS[cbits][ci], WEIGHTS[abits][ai]
        ch = [((64 - wc) * e0[c] + wc * e1[c] + 32) >> 6 for c in range(3)]
        ch.append(((64 - wa) * e0[3] + wa * e1[3] + 32) >> 6 if ab else 255)
        if rot:
            ch[rot - 1], ch[3] = ch[3], ch[rot - 1]
        out.append(tuple(ch))
    return out


def decode_bc1(block, mutate=None):
    """8 bytes -> 16 (r, g, b, a) tuples, texel i = 4*y + x.  SPEC.md section 8: 565 -> 888 by bit replication, then the
    /3 and /2 are integer divisions of the replicated 8-bit values."""
    assert mutate is None or mutate in BC1_MUTANTS, mutate
    v = int.from_bytes(bytes(block), "little")
    assert 0 <= v < 1 << 64
    c0, c1, sel = v & 0xFFFF, (v >> 16) & 0xFFFF, v >> 32

    def rgb(c):
        r5, g6, b5 = c >> 11, (c >> 5) & 63, c & 31
        return (r5 << 3) | (r5 >> 2), (g6 << 2) | (g6 >> 4), (b5 << 3) | (b5 >> 2)

    a, b = rgb(c0), rgb(c1)
    r3 = 0 if mutate == "bc1_third_no_round" else 1
    r2 = 0 if mutate == "bc1_half_no_round" else 1
    if c0 >= c1 if mutate == "bc1_ge" else c0 > c1:
        pal = [a + (255,), b + (255,), tuple((2 * x + y + r3) // 3 for x, y in zip(a, b)) + (255,),
               tuple((x + 2 * y + r3) // 3 for x, y in zip(a, b)) + (255,)]
    else:
        pal = [a + (255,), b + (255,), tuple((x + y + r2) // 2 for x, y in zip(a, b)) + (255,), (0, 0, 0, 0)]
    return [pal[(sel >> (i if mutate == "bc1_selector_shift" else 2 * i)) & 3] for i in range(16)]
