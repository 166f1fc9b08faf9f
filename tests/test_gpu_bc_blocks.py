"""Every BC7 block layout and every BC1 endpoint ordering through BOTH hand-written decoders: k_bc7_decode / k_bc1_decode
(csrc/k_texture.hip, a whole block at upload) and bc7_texel / bc1_texel (csrc/bc_sample.h, one texel per fetch when blocks
stay resident), which derive every bit offset on their own.  The blocks are those of tests/bc_block_cases.py -- all 285
(mode, partition, rotation, index selection) combinations, payload extremes, every mode byte, the reserved mode, every pair
of BC1 endpoint fields with the c0 == c1 diagonal -- and tests/test_bc_block_premises.py proves on the CPU that they tell a
list of plausible misreadings apart, that the oracle's decode of them agrees with two independent decoders, and that a 1:1
quad with blend OFF shows all four bytes of every texel, the colour under alpha 0 included (the default blend hides it)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import bc_block_cases as cases
from tests import bc_model
from tests.helpers import render_gpu, render_oracle
from tests.pixel_scenes import pixel_to_ndc_matrix
from tests.test_gpu_texture_blocks import _both_residencies, _texel_quad

pytestmark = pytest.mark.gpu

CASES = [(fmt, fam, crop) for fmt, fam in cases.ALL_FAMILIES for crop in ((0, 0), cases.CROPS[fam])]
_IDS = [f"{fmt}-{fam}-{'full' if crop == (0, 0) else 'cropped'}" for fmt, fam, crop in CASES]
_images = {}


def _case(fmt, family, crop):
    """[(case texture, the oracle's decode of it)], decoded once and shared by the tests of this module, read-only"""
    if (fmt, family, crop) not in _images:
        out = []
        for ct in cases.case_textures(fmt, family, crop):
            img = orc.decode_texture(ct.tex.fmt, ct.tex.width, ct.tex.height, ct.tex.data)
            img.setflags(write=False)
            out.append((ct, img))
        _images[fmt, family, crop] = out
    return _images[fmt, family, crop]


def _assert_image(ct, got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=-1))
    if bad[0].size:
        y, x = int(bad[0][0]), int(bad[1][0])
        blk = ct.block(x // 4, y // 4)
        where = f"{ct.fmt} family {ct.family}, block ({x // 4}, {y // 4}) = {blk.hex()}"
        if ct.fmt == "bc7":
            f = bc_model.bc7_fields(blk)
            where += " reserved mode" if f is None else f" mode {f[0]} partition {f[1]} rotation {f[2]} index selection {f[3]}"
        raise AssertionError(f"{what}: {bad[0].size} texels differ, the first at ({x}, {y}): got {got[y, x].tolist()}, "
                             f"want {want[y, x].tolist()}; {where}")


@pytest.mark.parametrize("fmt,family,crop", CASES, ids=_IDS)
def test_whole_block_decoders(gpu_device, fmt, family, crop):
    """k_bc7_decode / k_bc1_decode read back: the decoded image of every case texture, byte for byte"""
    from mt_renderer_amd import api
    for ct, want in _case(fmt, family, crop):
        t = api.Texture.new(gpu_device, ct.tex)
        try:
            got = t.read_rgba8()
        finally:
            t.close()
        _assert_image(ct, got, want, "read back")


@pytest.mark.parametrize("fmt,family,crop", CASES, ids=_IDS)
def test_per_texel_decoders_show_every_byte(gpu_device, fmt, family, crop):
    """1:1, blend OFF: the frame is the decoded image (test_bc_block_premises.py::test_replace_shows_every_byte), through the
    ordered kernel and the visibility kernel's shading alike, with blocks resident (bc7_texel / bc1_texel per fetch) and
    decoded at upload"""
    from mt_renderer_amd import api
    for ct, want in _case(fmt, family, crop):
        w, h, draws = cases.one_to_one_draws(ct.tex, cases.BLEND_OFF)
        try:
            gpu_device.set_texture_residency(api.TEXRES_BLOCKS)
            blocks = render_gpu(gpu_device, w, h, draws, tile_mode=None)
        finally:
            gpu_device.set_texture_residency(api.TEXRES_DECODED)
        decoded = render_gpu(gpu_device, w, h, draws, tile_mode=None)
        _assert_image(ct, blocks[0], want, "blocks resident")
        _assert_image(ct, decoded[0], want, "decoded at upload")


@pytest.mark.parametrize("family", ["coverage", "reserved"])
@pytest.mark.parametrize("cropped", [False, True], ids=["full", "cropped"])
def test_per_texel_decoders_default_blend(gpu_device, family, cropped):
    """the same texels through the reference's alpha blend, the oracle renderer the judge; a reserved texel blends as alpha 0:
    the clear colour stays and the stored alpha is 0"""
    for ct in cases.case_textures("bc7", family, cases.CROPS[family] if cropped else (0, 0)):
        w, h, draws = cases.one_to_one_draws(ct.tex)
        if family == "reserved":
            assert (render_oracle(w, h, draws)[0] == np.array([255, 255, 255, 0], dtype=np.uint8)).all()
        _both_residencies(gpu_device, w, h, draws, f"bc7 {family} 1:1, default blend")


def test_bilinear_taps_across_a_reserved_block(gpu_device):
    """12 x 12 texels whose centre block is reserved, magnified 3.3x: bilinear footprints mix the reserved block's zeros
    (alpha included) with texels of its eight neighbours"""
    from mt_renderer_amd import scene
    ring = cases.blocks("bc7", "coverage")[-8:]  # mode 7: colour and alpha
    assert all(bc_model.bc7_fields(b)[0] == 7 for b in ring)
    reserved = cases.blocks("bc7", "reserved")[1]  # first byte 0, fifteen bytes 0xFF: anything but zeros if it were parsed
    tex = scene.TextureData(12, 12, scene.TEX_BC7, b"".join(ring[:4] + [reserved] + ring[4:]))
    img = orc.decode_texture(tex.fmt, 12, 12, tex.data)
    assert (img[4:8, 4:8] == 0).all() and (img[..., 3] > 0).sum() > 64
    w, h = 40, 40
    draws = [dict(md=_texel_quad(tex, w, h, uv=(-0.1, -0.05, 1.1, 1.07)), M=pixel_to_ndc_matrix(w, h))]
    _both_residencies(gpu_device, w, h, draws, "bc7 reserved centre, magnified")
