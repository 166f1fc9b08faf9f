"""The scenes on which the oracle and the HIP path are compared with tests/ideal_renderer.py.  A scene is
``(width, height, draws)`` with ``draws`` in the form tests/helpers.render_oracle / render_gpu take; a posed batch carries
``skeleton`` and ``poses`` (for the HIP path and the ideal) next to the binary32 ``palettes`` of the host routine (for the
oracle)."""
from __future__ import annotations

import functools
import math

import numpy as np

from mt_renderer_amd import scene
from tests import ideal_renderer
from tests.ideal_compare import ramp_texture
from tests.pixel_scenes import pixel_model

CAPSULE = [((0.0, 0.0, 0.0), 0.35, 1.6)]


def _capsule(rows, cols, w, h, states=None, nbones=64):
    md = scene.skinned_capsule_model(CAPSULE, rows=rows, cols=cols)
    if states is not None:
        md.prim_states = np.array([states], dtype=np.uint8)
    return w, h, [dict(md=md, M=scene.to_f32_colmajor(scene.headline_transform(w, h)), palette=scene.bone_palette()[:nbones])]


def _headline():
    w, h = 480, 270
    md = scene.headline_model(rows=12, cols=20)
    return w, h, [dict(md=md, M=scene.to_f32_colmajor(scene.headline_transform(w, h)), palette=scene.bone_palette())]


def _lattice(kind):
    from tests.test_gpu_poses import SKELETONS, _bend, _model_file
    w, h = 192, 112
    parents = SKELETONS[kind]
    J = len(parents)
    md = scene.skinned_capsule_model(CAPSULE, rows=10, cols=16)
    mats, _ = scene.instance_lattice(4, 4)
    rng = np.random.default_rng(100 + J)
    imats = _bend(rng, J, angle=0.05)
    poses = _bend(rng, 16 * J).reshape(16, J, 16)
    mf = _model_file(parents, imats)
    palettes = np.stack([mf.palette(p) for p in poses]).astype(np.float32)
    vp = scene.to_f32_colmajor(scene.reference_view_proj(w, h))
    return w, h, [dict(md=md, vp=vp, model_mats=mats, palettes=palettes, skeleton=(parents, imats), poses=poses)]


def _floor():
    w, h = 320, 200
    vp = scene.reference_view_proj(w, h)
    floor = pixel_model([dict(verts=[(-60.0, -0.8, 40.0), (50.0, -0.8, 40.0), (50.0, -0.8, -60.0), (-60.0, -0.8, -60.0)],
                              indices=[0, 1, 2, 0, 2, 3], debug_id=9),
                         dict(verts=[(-60.0, 2.0, 40.0), (50.0, 2.0, 40.0), (50.0, 2.0, -60.0), (-60.0, 2.0, -60.0)],
                              indices=[0, 2, 1, 0, 3, 2], debug_id=12)])
    mesh = scene.skinned_capsule_model(CAPSULE, rows=12, cols=20)
    return w, h, [dict(md=floor, M=scene.to_f32_colmajor(vp)),
                  dict(md=mesh, M=scene.to_f32_colmajor(scene.headline_transform(w, h)), palette=scene.bone_palette())]


def _ramp_strip():
    """a ramp-textured strip on a tilted plane from behind the eye (w < 0) through the near plane to w = 8, u along it; and
    one triangle whose near corners lie far beyond the +-64 w guard band"""
    w, h = 320, 200
    P = scene.perspective_rh(math.radians(60.0), w / h, 0.1, 50.0)
    n = 12
    verts = []
    for k in range(n + 1):
        t = k / n
        # eye-space z from +0.5 (behind the eye) to -8; the first quad crosses the near plane and reaches into view
        ze = 0.5 - 8.5 * math.sqrt(t)
        ye = -0.7 + 0.12 * (-ze)        # the plane rises with distance
        verts += [(-1.2, ye, ze, k / n, 0.0), (1.2, ye, ze, k / n, 1.0)]
    strip = dict(verts=verts, indices=list(range(len(verts))), topology=scene.TOPO_STRIP, texture=0)
    big = dict(verts=[(30.0, 0.9, -0.2, 1.0, 0.0), (-30.0, 0.9, -0.2, 0.0, 0.0), (0.0, 1.6, -6.0, 0.5, 1.0)], indices=[0, 1, 2],
               texture=0)
    md = pixel_model([strip, big], textures=[ramp_texture()])
    return w, h, [dict(md=md, M=scene.to_f32_colmajor(P))]


def _assembly():
    """SPEC 1 on four bowl-shaped patches: a part switched off by parts_disp, index_base with unused vertices in front, a
    strip with an index past vertex_num (its three triangles are dropped) and a list"""
    w, h = 192, 112
    rows, cols = 6, 8

    def patch(cx, cy):
        s = np.linspace(-1.0, 1.0, cols + 1)[None, :] * np.ones((rows + 1, 1))
        t = np.linspace(-1.0, 1.0, rows + 1)[:, None] * np.ones((1, cols + 1))
        return np.stack([cx + 0.33 * s, cy + 0.3 * t, 0.25 * (s * s + t * t)], axis=-1).reshape(-1, 3)
    strip = scene._strip_indices(rows, cols).astype(np.int64)
    nv = (rows + 1) * (cols + 1)
    junk = np.full((5, 3), 7.5)
    holed = strip.copy()
    holed[2 * (cols + 1) + 8] = nv + 3          # not the restart value: an ordinary index past the end
    quads = strip[strip != 0xFFFF].reshape(rows, cols + 1, 2)
    lst = []
    for r in range(rows):
        for c in range(cols):
            b0, a0, b1, a1 = quads[r, c, 0], quads[r, c, 1], quads[r, c + 1, 0], quads[r, c + 1, 1]
            lst += [b0, a0, b1, b1, a0, a1]
    prims = [dict(verts=patch(-1.05, 0.4), indices=strip, topology=scene.TOPO_STRIP, debug_id=1),
             dict(verts=patch(-0.35, 0.4), indices=strip, topology=scene.TOPO_STRIP, debug_id=2, parts_no=1),
             dict(verts=np.concatenate([junk, patch(0.35, 0.4)]), indices=strip, topology=scene.TOPO_STRIP, debug_id=3,
                  index_base=5),
             dict(verts=patch(1.05, 0.4), indices=holed, topology=scene.TOPO_STRIP, debug_id=4),
             dict(verts=patch(-0.35, -0.4), indices=lst, topology=scene.TOPO_LIST, debug_id=25, parts_no=2)]
    md = pixel_model(prims, parts_disp=[1, 0, 1])
    return w, h, [dict(md=md, M=scene.to_f32_colmajor(scene.headline_transform(w, h) @ scene.mat_rot_y(0.3)))]


SCMP3N_FORMAT = ((scene.SEM_POSITION, scene.IEF_SCMP3N, 1, 0, 1), (scene.SEM_TEXCOORD, scene.IEF_F16, 2, 4), 8)


def _encode(el, vals):
    """values [nv, ncomp] -> bytes of one element in the format SPEC 2 decodes"""
    fmt, count = el[1], el[2]
    nv = vals.shape[0]
    if fmt == scene.IEF_F32:
        return vals[:, :3].astype("<f4").view(np.uint8).reshape(nv, 12)
    if fmt == scene.IEF_F16:
        return vals[:, :2].astype("<f2").view(np.uint8).reshape(nv, 4)
    if fmt in (scene.IEF_U8N, scene.IEF_U8NL):
        n = 2 if count == 1 else 4
        return np.clip(np.rint(vals[:, :n] * 255.0), 0, 255).astype(np.uint8)
    if fmt == scene.IEF_S8N:
        n = 2 if count == 1 else 4
        return np.clip(np.rint(vals[:, :n] * 127.0), -127, 127).astype(np.int8).view(np.uint8)
    if fmt == scene.IEF_S16N:
        n = 2 if count == 1 else 4
        return np.clip(np.rint(vals[:, :n] * 32767.0), -32767, 32767).astype("<i2").view(np.uint8).reshape(nv, 2 * n)
    if fmt == scene.IEF_SCMP3N:
        q = np.clip(np.rint(vals[:, :3] * 511.0), -511, 511).astype(np.int64) & 0x3FF
        return (q[:, 0] | (q[:, 1] << 10) | (q[:, 2] << 20)).astype("<u4").view(np.uint8).reshape(nv, 4)
    raise ValueError(fmt)


def format_model(fmt, rows=14, cols=18):
    """a curved mesh (warped outline, bowl-shaped where the format has a third component) stored in one vertex layout"""
    pos_el, uv_el, stride = fmt
    s = np.linspace(-1.0, 1.0, cols + 1)[None, :] * np.ones((rows + 1, 1))
    t = np.linspace(-1.0, 1.0, rows + 1)[:, None] * np.ones((1, cols + 1))
    x = 0.8 * s * (1.0 - 0.2 * t * t)
    y = 0.7 * t + 0.12 * np.sin(3.0 * s)
    z = 0.5 * (s * s + t * t) - 0.4
    pos = np.stack([x, y, z, np.ones_like(x)], axis=-1).reshape(-1, 4)
    unsigned = pos_el[1] in (scene.IEF_U8N, scene.IEF_U8NL)
    if unsigned:
        pos = 0.5 * (pos + 1.0)
    uv = np.stack([0.5 * (s + 1.0), 0.5 * (t + 1.0), np.zeros_like(s), np.zeros_like(s)], axis=-1).reshape(-1, 4)
    nv = pos.shape[0]
    rng = np.random.default_rng(stride)
    vb = rng.integers(0, 256, size=(nv, stride), dtype=np.uint8)   # the bytes no element reads are noise
    for el, vals in ((uv_el, uv), (pos_el, pos)):
        b = _encode(el, vals)
        vb[:, el[3]:el[3] + b.shape[1]] = b
    base = 3 if stride in (7, 19) else 0
    ib = scene._strip_indices(rows, cols)
    md = scene.ModelData(
        vertex_buf=np.concatenate([np.zeros(base, np.uint8), vb.reshape(-1)]), index_buf=ib,
        prims=scene.pack_primitive(vertex_num=nv, vertex_stride=stride, topology=scene.TOPO_STRIP, index_num=len(ib),
                                   vertex_base=base)[None, :],
        layouts=[[pos_el, uv_el]], prim_to_texture=np.array([0], np.int32), prim_debug_id=np.array([3], np.uint32),
        parts_disp=np.ones(1, np.uint8), textures=[ramp_texture()])
    model = scene.mat_translate(-1.0, -1.0, -1.0) @ scene.mat_scale(2.0, 2.0, 2.0) if unsigned else np.eye(4)
    return md, model


def _format(fmt):
    w, h = 160, 96
    md, model = format_model(fmt)
    vp = scene.reference_view_proj(w, h)
    M = vp @ scene.mat_translate(-5.0, 0.0, 1.0 - 2.2) @ scene.mat_rot_y(0.5) @ scene.mat_rot_x(-0.35) @ model
    return w, h, [dict(md=md, M=scene.to_f32_colmajor(M))]


def _vertex_formats():
    from tests.test_gpu_cases import VERTEX_FORMATS
    return list(VERTEX_FORMATS) + [SCMP3N_FORMAT]


def format_id(f):
    return f"pos{f[0][1]}x{f[0][2]}_uv{f[1][1]}x{f[1][2]}_s{f[2]}"


SCENES = {
    "capsule_12x20_160x96": lambda: _capsule(12, 20, 160, 96),
    "capsule_24x40_320x200": lambda: _capsule(24, 40, 320, 200),
    "capsule_30x48_333x171": lambda: _capsule(30, 48, 333, 171),
    "capsule_60x100_640x360": lambda: _capsule(60, 100, 640, 360),
    "capsule_short_palette": lambda: _capsule(12, 20, 160, 96, nbones=5),   # joints 5 .. 63 clamp to the last matrix
    "headline_12x20_480x270": _headline,
    "lattice_poses_tree": lambda: _lattice("tree_parents_after"),
    "lattice_poses_multi_root": lambda: _lattice("multi_root"),
    "floor_ceiling_capsule": _floor,
    "ramp_strip_w_range": _ramp_strip,
    "assembly_rules": _assembly,
    "capsule_cull_none": lambda: _capsule(24, 40, 320, 200, states=(1, 1, 1, 1)),
    "capsule_cull_front": lambda: _capsule(24, 40, 320, 200, states=(1, 1, 1, 2)),
}
for _f in _vertex_formats():
    SCENES["format_" + format_id(_f)] = functools.partial(_format, _f)


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def ideal_of(name, mutate=None):
    w, h, draws = scene_of(name)
    return ideal_renderer.render(w, h, draws, mutate=mutate)


def vertex_cases(name):
    """per draw call and instance, in the order of ideal.vertex: (md, binary32 matrix [16], binary32 palette or None)"""
    out = []
    for d in scene_of(name)[2]:
        if "model_mats" in d:
            vp = ideal_renderer.mat64(d["vp"])
            for i, mm in enumerate(np.asarray(d["model_mats"]).reshape(-1, 16)):
                M = vp @ ideal_renderer.mat64(mm)   # rounded once: inside the 4 roundings the bound grants the product
                out.append((d["md"], scene.to_f32_colmajor(M), None if d.get("palettes") is None else d["palettes"][i]))
        else:
            out.append((d["md"], np.asarray(d["M"], dtype=np.float32), d.get("palette")))
    return out
