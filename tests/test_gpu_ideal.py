"""-m gpu: the HIP path against the independent float64 renderer (tests/ideal_renderer.py) DIRECTLY, not through the oracle,
under the derived tolerances of tests/ideal_compare.py (SPEC.md "Accuracy against exact arithmetic"): frames through
helpers.render_gpu (both tile kernels, both bin-queue builders), Model.vertex_stage under the forward-error bound, k_pose
palettes against plain float64 products.  The scenes, the caps and the mutants that prove the rule has teeth are those of
tests/test_ideal_vs_oracle.py, whose docstring carries the measured figures."""
import pytest

from tests import ideal_compare as cmp
from tests import ideal_renderer
from tests import ideal_scenes as scenes
from tests.helpers import render_gpu

pytestmark = pytest.mark.gpu

ALL = list(scenes.SCENES)
POSED = ["lattice_poses_tree", "lattice_poses_multi_root"]


@pytest.mark.parametrize("name", ALL)
def test_gpu_frame_against_exact_arithmetic(gpu_device, name):
    w, h, draws = scenes.scene_of(name)
    ideal = scenes.ideal_of(name)
    cmp.assert_scene_caps(ideal, name)
    rep = cmp.compare(render_gpu(gpu_device, w, h, draws), ideal)
    print(f"{name}: {rep.line()}")
    if name in scenes.FRAGMENT_SCENES:
        print(f"{name}: {rep.fragment_line()}")
    assert rep.ok, (name, rep.failures)
    assert rep.compared > 0.02 * w * h


def test_gpu_block_resident_textures_against_exact_arithmetic(gpu_device):
    """the block-compressed chains once more with the blocks resident in memory and decoded per fetch (csrc/bc_sample.h),
    as tests/test_gpu_texture_blocks.py selects it; the test above rendered them decoded at upload"""
    from mt_renderer_amd import api
    name = "frag_bc_chains"
    w, h, draws = scenes.scene_of(name)
    ideal = scenes.ideal_of(name)
    try:
        gpu_device.set_texture_residency(api.TEXRES_BLOCKS)
        frame = render_gpu(gpu_device, w, h, draws)
    finally:
        gpu_device.set_texture_residency(api.TEXRES_DECODED)
    rep = cmp.compare(frame, ideal)
    print(f"{name} (blocks resident): {rep.line()}")
    print(f"{name} (blocks resident): {rep.fragment_line()}")
    assert rep.ok, (name, rep.failures)
    assert rep.textured_compared > 0.02 * w * h


def _posed_batch(dev, name):
    from mt_renderer_amd import api
    d = scenes.scene_of(name)[2][0]
    m = api.Model.new(dev, d["md"])
    try:
        m.set_skeleton(*d["skeleton"])
        b = api.Batch(dev, m, d["model_mats"])
    except Exception:
        m.close()
        raise
    return d, m, b


@pytest.mark.parametrize("name", POSED)
def test_k_pose_palettes_against_float64_products(gpu_device, name):
    d, m, b = _posed_batch(gpu_device, name)
    try:
        b.set_poses(d["poses"])
        got = b.read_palettes()
    finally:
        b.close()
        m.close()
    parents, imats = d["skeleton"]
    pal, pabs, depth = ideal_renderer.palettes_from_poses(parents, imats, d["poses"])
    assert got.shape == (pal.shape[0], pal.shape[1], 16)
    worst = cmp.palette_ratio(got, pal, pabs, depth)
    print(f"{name}: k_pose palette |err| / bound = {worst:.3f}")
    assert worst <= 1.0, (name, worst)
    wrong = ideal_renderer.palettes_from_poses(parents, imats, d["poses"], "pose_child_on_left")
    assert cmp.palette_ratio(got, *wrong) > 1.0, "the bound would not notice the product the other way round"


@pytest.mark.parametrize("name", ALL)
def test_gpu_vertex_stage_within_the_forward_error_bound(gpu_device, name):
    from mt_renderer_amd import api
    ideal = scenes.ideal_of(name)
    cases = scenes.vertex_cases(name)
    gpu_palettes = None
    if name in POSED:  # the palettes k_pose formed, not the host routine's
        d, m, b = _posed_batch(gpu_device, name)
        try:
            b.set_poses(d["poses"])
            gpu_palettes = b.read_palettes()
        finally:
            b.close()
            m.close()
    worst, models = 0.0, {}
    try:
        for (di, inst, pr, clip, uv, e_clip, e_uv) in ideal.vertex:
            md, M, pal = cases[di]
            if gpu_palettes is not None:
                pal = gpu_palettes[inst]
            if id(md) not in models:
                models[id(md)] = api.Model.new(gpu_device, md)
            m = models[id(md)]
            m.set_palette(pal)
            gc, gu = m.vertex_stage(pr, M)
            worst = max(worst, cmp.vertex_stage_ratio(gc, gu, clip, uv, e_clip, e_uv))
    finally:
        for m in models.values():
            m.close()
    print(f"{name}: vertex stage |err| / e = {worst:.3f}")
    assert worst <= 1.0, (name, worst)
