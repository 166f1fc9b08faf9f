"""CPU: what tests/test_gpu_bc_blocks.py rests on.  These are conditions on the case blocks of tests/bc_block_cases.py and
on the three decoders that judge them (tests/bc_model.py, the oracle, Pillow), not measurements:

* the coverage family holds every one of the 285 (mode, partition, rotation, index selection) combinations of BC7 K times,
  found by a field parser written here (not the model's, not the oracle's);
* the random texture of test_gpu_texture_blocks.py::test_every_texel_one_to_one[bc7] reaches 273 of them, and the 12 it
  misses are written down: the gap the case blocks close;
* model, oracle and Pillow agree byte for byte on every BC7 case block but the reserved ones, where SPEC.md section 8 rules
  (transparent black) and Pillow differs (it returns (0, 0, 0, 255));
* model and oracle agree on every BC1 case block, Pillow within 1 LSB (BC1's interpolation rounding is implementation-defined);
* every wrong reading bc_model can be switched to changes the decode of the case blocks it concerns -- per combination where
  the reading is per combination -- so a GPU decoder with that reading cannot pass;
* a 1:1 quad with blend OFF shows every byte of every texel, so the GPU test may compare frames with decoded images."""
import collections

import numpy as np
import pytest

from mt_renderer_amd import scene
from oracle import oracle as orc
from tests import bc_block_cases as cases
from tests import bc_model
from tests.helpers import render_oracle

# the combinations scene.random_bc7_texture(208, 132, seed=12) never draws (mode, partition; no rotation in these modes)
UNREACHED_BY_SEED_12 = {(1, 9), (1, 23), (1, 41), (1, 61), (2, 23), (2, 54), (3, 25), (7, 12), (7, 18), (7, 24), (7, 29), (7, 31)}

PARTITION_BITS = (4, 6, 6, 6, 0, 0, 0, 6)


def _parse(block):
    """(mode, partition, rotation, index selection) read byte-wise from the head of a block; None = reserved"""
    if block[0] == 0:
        return None
    mode = 0
    while not (block[0] >> mode) & 1:
        mode += 1
    bits = "".join(format(b, "08b")[::-1] for b in block[:3])[mode + 1:]  # LSB-first bit string after the mode bit
    def num(s):
        return int(s[::-1], 2) if s else 0
    pb = PARTITION_BITS[mode]
    part = num(bits[:pb])
    rot = num(bits[pb:pb + 2]) if mode in (4, 5) else 0
    isel = num(bits[pb + 2:pb + 3]) if mode == 4 else 0
    return mode, part, rot, isel


def _all_combinations():
    out = set()
    for mode in range(8):
        for part in range(1 << PARTITION_BITS[mode]):
            for rot in range(4 if mode in (4, 5) else 1):
                for isel in range(2 if mode == 4 else 1):
                    out.add((mode, part, rot, isel))
    return out


def _model7(blocks, **kw):
    return np.array([bc_model.decode_bc7(b, **kw) for b in blocks], dtype=np.uint8)


def _model1(blocks, **kw):
    return np.array([bc_model.decode_bc1(b, **kw) for b in blocks], dtype=np.uint8)


def _as_rows(blocks):
    return np.frombuffer(b"".join(blocks), dtype=np.uint8).reshape(len(blocks), -1)


@pytest.fixture(scope="module")
def bc7_right():
    """{family: (blocks, model decode)} of every BC7 family, decoded once"""
    return {f: (cases.blocks("bc7", f), _model7(cases.blocks("bc7", f))) for f in cases.BC7_FAMILIES}


@pytest.fixture(scope="module")
def bc1_right():
    return {f: (cases.blocks("bc1", f), _model1(cases.blocks("bc1", f))) for f in cases.BC1_FAMILIES}


def test_coverage_family_holds_every_combination_k_times():
    want = _all_combinations()
    assert len(want) == 285
    got = collections.Counter(_parse(b) for b in cases.blocks("bc7", "coverage"))
    assert cases.K >= 2 and got == {c: cases.K for c in want}
    assert sorted(cases.combinations()) == sorted(want)
    res = cases.blocks("bc7", "reserved")
    assert len(res) == 6 and all(_parse(b) is None for b in res)
    assert res[0] == bytes(16) and res[1] == bytes([0] + [255] * 15) and len(set(res)) == 6
    mb = cases.blocks("bc7", "mode_byte")
    assert [b[0] for b in mb] == list(range(0xFF, 0x7F, -1))
    # the lowest set bit names the mode whatever lies above it: 64 odd bytes, 32 of the form xxxxxx10, ... and 0x80 alone
    assert collections.Counter(_parse(b)[0] for b in mb) == {0: 64, 1: 32, 2: 16, 3: 8, 4: 4, 5: 2, 6: 1, 7: 1}
    ext = cases.blocks("bc7", "extremes")
    assert len(ext) == 6 * (5 * 2 + 3) and all(_parse(b) is not None for b in ext)
    assert {m for m, *_ in map(_parse, ext)} == set(range(8))
    for fmt, fam in cases.ALL_FAMILIES:  # the packing keeps every block, in order, within 256 x 256 texels
        texs = cases.case_textures(fmt, fam, cases.CROPS[fam])
        n = 16 if fmt == "bc7" else 8
        assert b"".join(t.tex.data[:t.nblocks * n] for t in texs) == b"".join(cases.blocks(fmt, fam))
        for t in texs:
            assert 4 * t.bw - 3 <= t.tex.width <= 256 and 4 * t.bh - 3 <= t.tex.height <= 256 and len(t.tex.data) == t.bw * t.bh * n


def test_what_the_random_textures_reach():
    """The shortfall of the existing GPU tests, as exact sets: changing their seed or size changes this on purpose."""
    def reached(tex):
        return {_parse(tex.data[i:i + 16]) for i in range(0, len(tex.data), 16)}
    one_to_one = reached(scene.random_bc7_texture(208, 132, seed=12))  # test_gpu_texture_blocks.py::test_every_texel_one_to_one[bc7]
    assert None not in one_to_one  # no reserved block either
    missing = _all_combinations() - one_to_one
    assert {(m, p) for m, p, r, s in missing} == UNREACHED_BY_SEED_12 and len(missing) == 12
    opaque = reached(scene.random_bc7_texture(208, 132, seed=12, opaque_modes_only=True))
    assert {c for c in missing if c[0] == 7}.isdisjoint(opaque) and {c for c in missing if c[0] < 4} <= opaque
    read_back = set()  # test_gpu_cases.py::test_texture_decode_parity[bc7]
    for w, h in [(64, 64), (52, 36), (7, 5), (4, 4)]:
        read_back |= reached(scene.random_bc7_texture(w, h, 11))
    assert len(read_back) == 125
    assert reached(cases.case_textures("bc7", "coverage")[0].tex) == _all_combinations()


def test_bc7_model_and_oracle_agree(bc7_right):
    """every BC7 case block, the reserved ones included: SPEC.md section 8 decodes those to (0, 0, 0, 0)"""
    for fam, (blocks, right) in bc7_right.items():
        got = orc.decode_bc7_blocks(_as_rows(blocks))
        bad = np.nonzero((got != right).any(axis=(1, 2)))[0]
        assert bad.size == 0, (fam, int(bad[0]), _parse(blocks[bad[0]]))
    blocks, right = bc7_right["reserved"]
    assert (right == 0).all() and (orc.decode_bc7_blocks(_as_rows(blocks)) == 0).all()


def test_bc7_pillow_agrees_on_every_block_but_the_reserved(bc7_right):
    """Pillow decodes a block whose first byte is 0 to (0, 0, 0, 255); SPEC.md section 8 says (0, 0, 0, 0) and rules, so
    those blocks -- and not one more -- are left to test_bc7_model_and_oracle_agree."""
    pytest.importorskip("PIL")
    from tools.bc7_probe_pillow import decode_bc7_blocks as pillow_bc7
    left_out = 0
    for fam, (blocks, right) in bc7_right.items():
        keep = [i for i, b in enumerate(blocks) if b[0] != 0]
        left_out += len(blocks) - len(keep)
        if keep:
            got = pillow_bc7(_as_rows([blocks[i] for i in keep]))
            bad = np.nonzero((got != right[keep]).any(axis=(1, 2)))[0]
            assert bad.size == 0, (fam, keep[int(bad[0])], _parse(blocks[keep[int(bad[0])]]))
    assert left_out == len(cases.blocks("bc7", "reserved")) == 6
    res = pillow_bc7(_as_rows(cases.blocks("bc7", "reserved")))
    assert (res[..., :3] == 0).all()  # where Pillow stands on alpha is its own affair: not asserted


def test_bc1_model_oracle_and_pillow(bc1_right):
    for fam, (blocks, right) in bc1_right.items():
        got = orc.decode_bc1_blocks(_as_rows(blocks))
        bad = np.nonzero((got != right).any(axis=(1, 2)))[0]
        assert bad.size == 0, (fam, int(bad[0]), blocks[bad[0]].hex())
    pytest.importorskip("PIL")
    import io
    from PIL import Image
    from tools.bc7_probe_pillow import dds_bc
    for fam, (blocks, right) in bc1_right.items():
        n = len(blocks)
        img = Image.open(io.BytesIO(dds_bc(b"".join(blocks), 4 * n, 4, 71)))  # DXGI_FORMAT_BC1_UNORM
        ref = np.asarray(img.convert("RGBA")).reshape(4, n, 4, 4).transpose(1, 0, 2, 3).reshape(n, 16, 4)
        assert np.abs(right.astype(int) - ref.astype(int)).max() <= 1, fam
        assert (right[..., 3] == ref[..., 3]).all(), fam


def test_bc1_selectors_and_orderings(bc1_right):
    """over green, red and blue each: c0 > c1, c0 < c1 and c0 == c1 all occur, and in each of the three every texel position
    takes every selector"""
    for fam in ("green", "red", "blue"):
        seen = collections.defaultdict(set)
        for b in bc1_right[fam][0]:
            c0, c1, sel = int.from_bytes(b[0:2], "little"), int.from_bytes(b[2:4], "little"), int.from_bytes(b[4:8], "little")
            assert sel in cases.SELECTOR_WORDS
            order = (c0 > c1) - (c0 < c1)
            for i in range(16):
                seen[order].add((i, (sel >> (2 * i)) & 3))
        assert set(seen) == {-1, 0, 1} and all(len(v) == 64 for v in seen.values()), fam
    n = {f: len(bc1_right[f][0]) for f in bc1_right}
    assert n == {"green": 64 * 64, "red": 32 * 32, "blue": 32 * 32, "edges": 16}
    diag = [b for b in bc1_right["green"][0] if b[0:2] == b[2:4]]
    assert len(diag) == 64


def _changed(blocks, right, decode, **kw):
    """indices of the blocks whose decode the mutation changes"""
    return [i for i, b in enumerate(blocks) if (np.array(decode(b, **kw), dtype=np.uint8) != right[i]).any()]


def test_bc7_wrong_readings_are_told_apart_per_combination(bc7_right):
    """K is fixed here: every combination must see, in its own K blocks, each misreading that is particular to it."""
    blocks, right = bc7_right["coverage"]
    T = bc_model.tables()
    blind = []
    for ci, combo in enumerate(cases.combinations()):
        mode, part, rot, isel = combo
        ns = bc_model.MODES[mode][0]
        mine = range(ci * cases.K, (ci + 1) * cases.K)
        assert all(_parse(blocks[i]) == combo for i in mine)
        wrong = []
        anchors = [] if ns == 1 else [T["ANCHOR2_1"][part]] if ns == 2 else [T["ANCHOR3_1"][part], T["ANCHOR3_2"][part]]
        if ns > 1:
            wrong.append(("partition_neighbour", (mode, part)))
        if any(a < 15 for a in anchors):  # an anchor at texel 15 is no case: its extra bit would be bit 128, which reads as 0
            wrong.append(("anchor_full_width", combo))
        if ns == 3 and T["ANCHOR3_1"][part] > T["ANCHOR3_2"][part]:
            wrong.append(("anchor_order", combo))
        if mode in (4, 5):
            wrong += [("rotation_next", combo), ("secondary_anchor_full_width", combo)]
        if mode == 4:
            wrong.append(("isel_flipped", combo))
        if mode == 1:
            wrong.append(("shared_pbit_per_endpoint", combo))
        if mode in (6, 7):
            wrong.append(("alpha_without_pbit", combo))
        for name, only in wrong:
            if not _changed([blocks[i] for i in mine], right[list(mine)], bc_model.decode_bc7, mutate=name, only=only):
                blind.append((combo, name))
    assert not blind, blind
    # `only` confines a mutation: applied to one combination it leaves every other block alone
    hit = _changed(blocks, right, bc_model.decode_bc7, mutate="partition_neighbour", only=(1, 9))
    assert hit and all(_parse(blocks[i])[:2] == (1, 9) for i in hit)


def test_bc7_wrong_readings_are_told_apart_by_the_other_families(bc7_right):
    blocks, right = bc7_right["mode_byte"]
    hit = {_parse(blocks[i])[0] for i in _changed(blocks, right, bc_model.decode_bc7, mutate="mode_from_highest_bit")}
    assert hit == set(range(7))  # 0x80 has one bit: both readings find mode 7
    blocks, right = bc7_right["reserved"]
    assert _changed(blocks, right, bc_model.decode_bc7, mutate="reserved_opaque") == list(range(6))
    blocks, right = bc7_right["extremes"]
    # the extremes show once more the readings that move bits or channels (not those that need subsets with endpoints of
    # their own, or an alpha endpoint that its p-bit changes: all ones is 255 and all zeros 0 with it and without)
    for name in ("rotation_next", "isel_flipped", "anchor_full_width", "secondary_anchor_full_width", "shared_pbit_per_endpoint"):
        assert _changed(blocks, right, bc_model.decode_bc7, mutate=name), name
    # weight 0 and weight 64 both meet an endpoint of 255 and one of 0, in every mode
    for mode in range(8):
        px = right[[i for i, b in enumerate(blocks) if _parse(b)[0] == mode]]
        assert {0, 255} <= set(np.unique(px[..., :3])), mode


def test_bc1_wrong_readings_are_told_apart(bc1_right):
    channel = {"red": 0, "green": 1, "blue": 2}
    for fam, ch in channel.items():
        blocks, right = bc1_right[fam]
        eq = [i for i, b in enumerate(blocks) if b[0:2] == b[2:4]]
        assert _changed(blocks, right, bc_model.decode_bc1, mutate="bc1_ge") == eq  # exactly the c0 == c1 blocks
        for name in ("bc1_third_no_round", "bc1_half_no_round"):  # the rounding of this family's own channel
            wrong = _model1(blocks, mutate=name)
            assert (wrong[..., ch] != right[..., ch]).any(), (fam, name)
        assert _changed(blocks, right, bc_model.decode_bc1, mutate="bc1_selector_shift"), fam
    blocks, right = bc1_right["edges"]
    assert len(_changed(blocks, right, bc_model.decode_bc1, mutate="bc1_ge")) == 8  # c0 = c1 = 0 and = 0xFFFF, four words each
    assert _changed(blocks, right, bc_model.decode_bc1, mutate="bc1_selector_shift")


@pytest.mark.parametrize("fmt,family", [("bc7", "coverage"), ("bc1", "green")])
def test_replace_shows_every_byte(fmt, family):
    """a 1:1 quad with blend OFF stores the texel as sampled, alpha and the colour under alpha 0 included: the oracle's frame
    IS the decoded image, so test_gpu_bc_blocks.py compares GPU frames with decoded images directly.  One 64 x 64 texture per
    format: the family's last 256 blocks (for BC7 those of modes 4 to 7, the ones with alpha)."""
    bl = cases.blocks(fmt, family)[-256:]
    tex = scene.TextureData(64, 64, scene.TEX_BC7 if fmt == "bc7" else scene.TEX_BC1, b"".join(bl))
    w, h, draws = cases.one_to_one_draws(tex, cases.BLEND_OFF)
    image = orc.decode_texture(tex.fmt, w, h, tex.data)
    assert (image[..., 3] < 255).any()  # the premise is about translucent texels
    frame = render_oracle(w, h, draws)[0]
    assert frame.shape == image.shape and (frame == image).all()
    blended = render_oracle(w, h, cases.one_to_one_draws(tex)[2])[0]
    assert (blended != image).any()  # under the default blend the same texels do not show as they are


def test_replace_shows_every_byte_at_every_case_size():
    """the same for every case texture as the GPU test draws it, full and cropped: targets that are no power of two, a last
    column and row that cut through blocks (the oracle takes milliseconds for each)"""
    for fmt, family in cases.ALL_FAMILIES:
        for crop in ((0, 0), cases.CROPS[family]):
            for ct in cases.case_textures(fmt, family, crop):
                w, h, draws = cases.one_to_one_draws(ct.tex, cases.BLEND_OFF)
                image = orc.decode_texture(ct.tex.fmt, w, h, ct.tex.data)
                assert (render_oracle(w, h, draws)[0] == image).all(), (fmt, family, crop)
