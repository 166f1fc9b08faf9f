"""-m gpu: material states (SPEC.md section 10) through the HIP path against the oracle, bit for bit:
blend off / additive, depth write off, depth test off, cull none / front, mip chains, SCMP3N positions."""
import itertools

import numpy as np
import pytest

from mt_renderer_amd import scene
from tests.helpers import assert_same, render_gpu, render_oracle
from tests.pixel_scenes import pixel_model, pixel_to_ndc_matrix

pytestmark = pytest.mark.gpu


def _quad(x0, y0, x1, y1, z, tex=-1, did=0, flip=False):
    v = [(x0, y0, z, 0.0, 0.0), (x0, y1, z, 0.0, 1.0), (x1, y1, z, 1.0, 1.0), (x1, y0, z, 1.0, 0.0)]
    idx = [0, 1, 2, 0, 2, 3] if not flip else [0, 2, 1, 0, 3, 2]
    return dict(verts=v, indices=idx, texture=tex, debug_id=did)


def _layers(rng, n, ntex):
    prims = []
    for i in range(n):
        x0, y0 = rng.uniform(-8, 40, size=2)
        w, h = rng.uniform(6, 40, size=2)
        prims.append(_quad(x0, y0, x0 + w, y0 + h, float(rng.integers(1, 15)) / 16.0, tex=int(rng.integers(-1, ntex)), did=int(rng.integers(0, 20)),
                           flip=bool(rng.integers(0, 2))))
    return prims


@pytest.mark.parametrize("seed", range(8))
def test_random_state_mixes_match_the_oracle(gpu_device, seed):
    """30 overlapping quads (debug colours, an opaque and two translucent textures), every primitive with a random
    blend / depth write / depth test / cull state: equal depths, both windings, order-dependent and order-free
    primitives side by side (visibility kernel, ordered kernel and the mixed split are all exercised)"""
    rng = np.random.default_rng(40 + seed)
    texs = [scene.checker_rgba8_texture(16, 16, cell=2, alpha=(255, 255)), scene.checker_rgba8_texture(8, 8, cell=1, alpha=(255, 90)),
            scene.random_bc7_texture(16, 16, seed=5)]
    prims = _layers(rng, 30, len(texs))
    md = pixel_model(prims, texs)
    if seed == 0:  # only order-free states: the visibility kernel must take the whole frame
        md.prim_states = np.array([(rng.integers(0, 2), 1, 1, rng.integers(0, 3)) for _ in prims], dtype=np.uint8)
        md.prim_to_texture[:] = np.where(md.prim_to_texture > 0, 0, md.prim_to_texture)  # opaque texture or none
    else:
        md.prim_states = np.array([(rng.integers(0, 3), rng.integers(0, 2), rng.integers(0, 2), rng.integers(0, 3)) for _ in prims], dtype=np.uint8)
    draws = [dict(md=md, M=pixel_to_ndc_matrix(64, 64))]
    g = render_gpu(gpu_device, 64, 64, draws)
    if seed == 0:
        assert g[2]["tile_kernel"] == 2
    assert_same(g, render_oracle(64, 64, draws), f"state mix {seed}")


@pytest.mark.parametrize("cull", [0, 1, 2])
def test_cull_modes_on_a_skinned_mesh(gpu_device, cull):
    w, h = 333, 171
    md = scene.skinned_capsule_model([((0.0, 0.0, 0.0), 0.35, 1.6)], rows=20, cols=31)
    md.prim_states = np.array([(0, 1, 1, cull)] * md.nprims, dtype=np.uint8)
    M = scene.to_f32_colmajor(scene.headline_transform(w, h))
    draws = [dict(md=md, M=M, palette=scene.bone_palette())]
    g = render_gpu(gpu_device, w, h, draws)
    ref = render_oracle(w, h, draws)
    assert_same(g, ref, f"cull {cull}")
    assert ref[2]["tris_setup"] > 100


def test_states_survive_instancing_near_clip_and_sharding(gpu_device):
    from mt_renderer_amd import api, sharding
    w, h = 320, 200
    texs = [scene.checker_rgba8_texture(32, 32, cell=4, alpha=(255, 120))]
    md = scene.skinned_capsule_model([((0.0, 0.0, 0.0), 0.35, 1.6)], rows=14, cols=24)
    md = scene.mesh50k(textured=True, textures=texs, rows=14, cols=24)
    md.prim_states = np.array([(2, 0, 1, 1)] * md.nprims, dtype=np.uint8)  # additive, no depth write, two-sided
    mats, pals = scene.instance_lattice(3, 2)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(w, h))
    near = scene.to_f32_colmajor(scene.reference_view_proj(w, h) @ scene.mat_translate(-5.0, 0.0, 1.0 - 0.25))  # through the near plane
    draws = [dict(md=md, vp=vp, model_mats=mats, palettes=pals), dict(md=md, M=near, palette=scene.bone_palette())]
    full = render_gpu(gpu_device, w, h, draws)
    assert_same(full, render_oracle(w, h, draws), "instanced states")
    owner = sharding.owner_map(w, h, 3, sharding.BANDS)
    for rank in range(3):
        part = render_gpu(gpu_device, w, h, draws, shard=(rank, 3, sharding.BANDS), tile_mode=api.TILE_AUTO)
        own = owner == rank
        assert (part[0][own] == full[0][own]).all() and (part[1].view(np.uint32)[own] == full[1].view(np.uint32)[own]).all(), rank


def _mip_texture(w, h, levels, fmt, seed):
    rng = np.random.default_rng(seed)
    data, lw, lh = b"", w, h
    for l in range(levels):
        if fmt == scene.TEX_RGBA8:
            img = rng.integers(0, 256, size=(lh, lw, 4), dtype=np.uint8)
            img[..., 3] = 255
            data += img.tobytes()
        else:
            data += scene.random_bc7_texture(lw, lh, seed=seed * 31 + l, opaque_modes_only=True).data
        lw, lh = max(1, lw >> 1), max(1, lh >> 1)
    return scene.TextureData(w, h, fmt, data, levels=levels)


@pytest.mark.parametrize("fmt", ["rgba8", "bc7"])
def test_mip_chains_match_the_oracle(gpu_device, fmt):
    """a textured, skinned capsule far enough away to minify by several levels across its surface, and a mesh whose
    texcoord scale differs per axis (anisotropic footprints: the largest derivative picks the level)"""
    w, h = 320, 200
    tex = _mip_texture(256, 128, 8, scene.TEX_RGBA8 if fmt == "rgba8" else scene.TEX_BC7, 3)
    md = scene.mesh50k(textured=True, textures=[tex], rows=30, cols=48)
    draws = []
    for dist, sx in ((2.3, 1.6), (6.0, 1.6), (12.0, 0.4)):
        M = scene.to_f32_colmajor(scene.reference_view_proj(w, h) @ scene.mat_translate(-5.0, 0.0, 1.0 - dist) @ scene.mat_scale(sx, 0.9, 1.0))
        draws.append(dict(md=md, M=M, palette=scene.bone_palette()))
    g = render_gpu(gpu_device, w, h, draws)
    assert_same(g, render_oracle(w, h, draws), f"mips {fmt}")
    # the chain matters: the same scene with level 0 only differs
    md1 = scene.mesh50k(textured=True, textures=[scene.TextureData(tex.width, tex.height, tex.fmt, tex.data, levels=1)], rows=30, cols=48)
    g1 = render_gpu(gpu_device, w, h, [dict(d, md=md1) for d in draws])
    assert (g1[0] != g[0]).any()


def test_scmp3n_positions(gpu_device):
    from mt_renderer_amd import api
    rng = np.random.default_rng(9)
    n = 300
    xyz = rng.integers(-511, 512, size=(n, 3))
    xyz[:, 2] = rng.integers(0, 400, size=n)
    packed = ((xyz[:, 0] & 0x3ff) | ((xyz[:, 1] & 0x3ff) << 10) | ((xyz[:, 2] & 0x3ff) << 20)).astype(np.uint32)
    idx = rng.integers(0, n, size=600).astype(np.uint16)

    def model(flags):
        lay = (scene.SEM_POSITION, scene.IEF_SCMP3N, 1, 0) + ((flags,) if flags else ())
        return scene.ModelData(vertex_buf=packed.view(np.uint8).copy(), index_buf=idx,
                               prims=np.stack([scene.pack_primitive(vertex_num=n, vertex_stride=4, topology=scene.TOPO_LIST, index_num=len(idx))]),
                               layouts=[[lay]], prim_to_texture=np.array([-1], dtype=np.int32),
                               prim_debug_id=np.array([6], dtype=np.uint32), parts_disp=np.ones(1, dtype=np.uint8))
    draws = [dict(md=model(1), M=np.eye(4, dtype=np.float32).reshape(16))]
    g = render_gpu(gpu_device, 96, 64, draws)
    ref = render_oracle(96, 64, draws)
    assert_same(g, ref, "scmp3n")
    assert ref[2]["tris_setup"] > 20
    with pytest.raises(api.MtrError) as e:  # not opted in: the element is skipped (src/rshader2.rs:509-512), no Position is left
        api.Model.new(gpu_device, model(0))
    assert e.value.code == api.MTR_E_UNSUPPORTED


def test_prim_state_errors(gpu_device):
    from mt_renderer_amd import api
    md = pixel_model([_quad(0, 0, 8, 8, .5)])
    m = api.Model.new(gpu_device, md)
    with pytest.raises(api.MtrError):
        m.set_prim_states(np.array([(3, 1, 1, 0)], dtype=np.uint8))  # unknown blend mode
    with pytest.raises(api.MtrError):
        m.set_prim_states(np.array([(0, 1, 1, 0), (0, 1, 1, 0)], dtype=np.uint8))  # wrong count
    m.set_prim_states(np.array([(1, 0, 0, 2)], dtype=np.uint8))
    m.set_prim_states(None)
    m.close()


def test_stage_timings_follow_the_binning_mode():
    """mtr_frame_get_timings: single-pass binning runs (and times) no scan and no fill; the two-pass queues time all four
    stages.  Sign and finiteness only: no claim about how long a stage takes."""
    from mt_renderer_amd import api
    dev = api.Device(0)
    try:
        dev.set_profiling(True)
        m = api.Model.new(dev, scene.cube_model())
        M = scene.cube_transform(64, 64)

        def frame():
            fr = api.Frame(dev, 64, 64)
            try:
                m.render(fr, M)
                fr.end()
                return fr.timings_ms(), fr.stats()
            finally:
                fr.close()

        ms, st = frame()
        assert st["binning"] == 1
        assert ms["scan"] == 0.0 and ms["fill"] == 0.0, ms
        assert np.isfinite(ms["geom"]) and np.isfinite(ms["tile"]) and ms["tile"] > 0.0, ms
        dev.set_binning(False)
        ms, st = frame()
        assert st["binning"] == 2
        assert all(np.isfinite(ms[k]) and ms[k] >= 0.0 for k in ("geom", "scan", "fill", "tile")), ms
        assert ms["tile"] > 0.0, ms
        m.close()
    finally:
        dev.close()
