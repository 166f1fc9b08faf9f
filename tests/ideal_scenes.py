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


# -------------------------------------------------------------------------------------------------------------------
# the fragment stage (SPEC 7, 8, 10): scenes rendered with every fragment kept (ideal_renderer.render(fragments=True))
# -------------------------------------------------------------------------------------------------------------------
FOV = math.radians(60.0)
ST_DEFAULT = (0, 1, 1, 0)     # blend ALPHA, depth write, depth test, cull BACK
ALPHA, OFF, ADD = 0, 1, 2


def _camera(w, h, dist, ry=0.0, rx=0.0, far=50.0):
    """a camera ``dist`` in front of the plane z = 0, on which one unit is ``scale`` pixels at the target's centre; the
    plane is then turned by ry, rx about its centre -> (M, scale)"""
    M = scene.perspective_rh(FOV, w / h, 0.1, far) @ scene.mat_translate(0.0, 0.0, -dist) @ scene.mat_rot_y(ry) @ scene.mat_rot_x(rx)
    return scene.to_f32_colmajor(M), (h / 2.0) / math.tan(FOV / 2.0) / dist


def _px_quad(w, h, scale, cx, cy, sx, sy, ang=0.0, z=0.0, uv=(0.0, 0.0, 1.0, 1.0), **kw):
    """a quad of sx x sy pixels (at the centre's scale) about pixel (cx, cy) of the unturned plane, turned by ang in it"""
    c, s_ = math.cos(ang), math.sin(ang)
    u0, v0, u1, v1 = uv
    verts = []
    for (x, y), (u, v) in zip(((-1, -1), (1, -1), (1, 1), (-1, 1)), ((u0, v1), (u1, v1), (u1, v0), (u0, v0))):
        x, y = 0.5 * sx * x, 0.5 * sy * y
        verts.append(((cx - w / 2.0 + c * x - s_ * y) / scale, -(cy - h / 2.0) / scale + (s_ * x + c * y) / scale, z, u, v))
    return dict(verts=verts, indices=[0, 1, 2, 0, 2, 3], **kw)


def _rgba(wt, ht, seed, alpha=None):
    img = np.random.default_rng(seed).integers(0, 256, size=(ht, wt, 4), dtype=np.uint8)
    if alpha is not None:
        img[..., 3] = alpha
    return img


def _tex(levels):
    """RGBA8 arrays, level 0 first -> TextureData"""
    return scene.TextureData(levels[0].shape[1], levels[0].shape[0], scene.TEX_RGBA8, b"".join(a.tobytes() for a in levels),
                             levels=len(levels))


def _tagged_chain(wt, ht, nlevels, seed):
    """random levels whose blue channel names the level (B = 32 l + noise below 32): a wrong level cannot pass as a
    neighbouring texel"""
    out = []
    for l in range(nlevels):
        a = _rgba(max(1, wt >> l), max(1, ht >> l), seed + l, alpha=255)
        a[..., 2] = 32 * l + (a[..., 2] & 31)
        out.append(a)
    return out


def _solid(rgba):
    return _tex([np.tile(np.array(rgba, dtype=np.uint8), (2, 2, 1))])


def _with_states(md, states):
    md.prim_states = np.array(states, dtype=np.uint8)
    return md


def _magnified_patch():
    """7 x 5 texels over about 150 x 100 pixels, turned in its plane and seen in perspective, texture coordinates from
    -0.25 to 1.25: every pixel is linear, all four clamp-to-edge borders and both x0 = -1 and x0 + 1 = W are hit"""
    w, h = 192, 112
    M, sc = _camera(w, h, 2.0, ry=0.45, rx=-0.3)
    q = _px_quad(w, h, sc, 96, 56, 150, 96, ang=0.35, uv=(-0.25, -0.25, 1.25, 1.25), texture=0)
    return w, h, [dict(md=pixel_model([q], textures=[_tex([_rgba(7, 5, 71)])]), M=M)]


def _minified_no_mips():
    """64 x 48 texels, one level, on a plane receding from below the camera: the products of SPEC 7 run from below 1 to
    about 8, and the border between linear and nearest crosses the two triangles"""
    w, h = 192, 112
    P = scene.perspective_rh(FOV, w / h, 0.1, 50.0)
    verts = [(-2.0, -0.6, -0.8, 0.0, 0.0), (2.0, -0.6, -0.8, 1.0, 0.0), (2.0, -0.6, -14.0, 1.0, 1.0), (-2.0, -0.6, -14.0, 0.0, 1.0)]
    md = pixel_model([dict(verts=verts, indices=[0, 1, 2, 0, 2, 3], texture=0)], textures=[_tex([_rgba(64, 48, 72, alpha=255)])])
    return w, h, [dict(md=md, M=scene.to_f32_colmajor(P @ scene.mat_rot_y(0.2)))]


MIP_W, MIP_H, MIP_L = 100, 60, 7


def _mip_chain():
    """100 x 60 with all 7 levels on quads squeezed along u so that the largest product sits near 1.25, 2, 4 .. 64; a
    256 x 128 texture with 3 levels whose product of about 16 asks for level 4 and is clamped to 2; a 4 x 64 texture whose
    levels 3 .. 6 are one texel wide"""
    w, h = 192, 112
    M, sc = _camera(w, h, 2.0, ry=0.2, rx=-0.1)
    prims = [_px_quad(w, h, sc, 44, 28, 80, 50, ang=0.05, texture=0), _px_quad(w, h, sc, 116, 28, 50, 45, ang=-0.1, texture=0)]
    x = 14.0
    for l in range(2, 7):
        wd = 100.0 / 2 ** l
        prims.append(_px_quad(w, h, sc, x + wd / 2, 82, wd, 45, ang=0.04 * (l - 4), texture=0))
        x += wd + 8.0
    prims.append(_px_quad(w, h, sc, 112, 82, 16, 45, ang=0.1, texture=1))
    prims.append(_px_quad(w, h, sc, 136, 82, 16, 8, ang=-0.05, texture=2))    # 64 rows on 8 px: level 3, 1 x 8 texels
    prims.append(_px_quad(w, h, sc, 165, 60, 30, 100, ang=0.08, texture=1))    # 256 texels on 30 px: product 8.5, level 2 (3 unclamped)
    texs = [_tex(_tagged_chain(MIP_W, MIP_H, MIP_L, 300)), _tex(_tagged_chain(256, 128, 3, 400)), _tex(_tagged_chain(4, 64, 7, 500))]
    return w, h, [dict(md=pixel_model(prims, textures=texs), M=M)]


LAYER_ALPHAS = (0, 1, 128, 254, 255)


def _layers(modes, states=None, extra=(), far=50.0, dark=False):
    """three clusters of eight overlapping turned quads at distinct depths, submitted back to front, front to back and
    shuffled, each with a 2 x 2 one-colour texture (alphas 0, 1, 128, 254, 255); modes[k % len(modes)] is quad k's blend.
    dark: dim colours over a dark opaque backdrop, so that additive layers do not all saturate against the white clear"""
    w, h = 192, 112
    M, sc = _camera(w, h, 2.0, ry=0.3, rx=0.1, far=far)
    rng = np.random.default_rng(11)
    texs = [_solid(tuple(rng.integers(0, 80 if dark else 256, 3)) + (LAYER_ALPHAS[t % 5],)) for t in range(10)]
    prims, st = [], []
    if dark:
        texs.append(_solid((10, 20, 30, 255)))
        prims.append(_px_quad(w, h, sc, 96, 56, 260, 150, z=-0.6, texture=10))
        st.append(ST_DEFAULT)
    for cl, order in enumerate((range(8), range(7, -1, -1), (3, 6, 0, 5, 2, 7, 1, 4))):
        for k in order:     # k = 0 is the farthest
            n = cl * 8 + k
            prims.append(_px_quad(w, h, sc, 34 + 62 * cl + 5.0 * math.cos(2.4 * k), 56 + 9.0 * math.sin(1.7 * k + cl), 52 - 2 * k, 70 - 3 * k,
                                  ang=0.37 * n, z=-0.35 + 0.1 * k, texture=(3 * n + cl) % 10))
            mode = modes[n % len(modes)]
            st.append((mode,) + (states[n % len(states)] if states else (1, 1)) + (0,))
    prims += list(extra)
    st += [ST_DEFAULT] * len(extra)
    return w, h, [dict(md=_with_states(pixel_model(prims, textures=texs), st), M=M)]


def _depth_states():
    """the layers with depth write off and depth test off mixed per primitive, and one quad behind the far plane under
    test off, which must leave nothing"""
    w, h = 192, 112
    beyond = _px_quad(w, h, 1.0, 96, 56, 4000, 3000, z=-60.0, texture=4)
    w, h, draws = _layers((ALPHA, ADD, ALPHA, OFF, ALPHA), states=((1, 1), (0, 1), (1, 0), (0, 0), (1, 1), (1, 0), (0, 1)),
                          extra=[beyond], far=6.0, dark=True)
    draws[0]["md"].prim_states[-1] = (ALPHA, 1, 0, 1)     # depth test off, cull NONE: only the 0 <= z <= 1 clip stops it
    return w, h, draws


def _translucent_over_linear():
    """a smooth, low-contrast, translucent 9 x 6 texture magnified over an opaque smooth one: sources with an error radius"""
    w, h = 192, 112
    M, sc = _camera(w, h, 2.0, ry=-0.35, rx=0.25)
    rng = np.random.default_rng(5)

    def smooth(wt, ht, base, spread, alpha):
        y, x = np.mgrid[0:ht, 0:wt]
        img = np.zeros((ht, wt, 4), dtype=np.uint8)
        for c in range(3):
            img[..., c] = base[c] + spread * np.sin(0.9 * x + c) * np.cos(0.7 * y - c) + rng.integers(0, 3, size=(ht, wt))
        img[..., 3] = alpha if np.isscalar(alpha) else alpha[0] + alpha[1] * np.sin(0.8 * x + 0.5 * y)
        return img
    texs = [_tex([smooth(6, 5, (60, 120, 200), 20, 255)]), _tex([smooth(9, 6, (200, 90, 40), 12, (120, 18))])]
    prims = [_px_quad(w, h, sc, 96, 56, 170, 100, ang=0.1, z=-0.2, texture=0),
             _px_quad(w, h, sc, 100, 52, 130, 80, ang=-0.3, z=0.1, uv=(-0.1, -0.1, 1.1, 1.1), texture=1)]
    return w, h, [dict(md=pixel_model(prims, textures=texs), M=M)]


def _bc_levels(fmt, wt, ht, nlevels, seed):
    """-> (TextureData of a random chain, its levels decoded by Pillow's DDS reader: the independent decoder of
    tests/test_bc_decode.py).  BC1 blocks use their two end-point colours and the transparent code only: SPEC 8's rounding
    of the interpolated colours is this build's own, and an independent decoder need not share it"""
    import io
    import pytest
    pytest.importorskip("PIL")
    from PIL import Image
    from tools.bc7_probe_pillow import dds_bc
    data, levels = b"", []
    for l in range(nlevels):
        lw, lh = max(1, wt >> l), max(1, ht >> l)
        bw, bh = (lw + 3) // 4, (lh + 3) // 4
        if fmt == scene.TEX_BC7:
            blocks = scene.random_bc7_texture(lw, lh, seed=seed + l).data
        else:
            rng = np.random.default_rng(seed + l)
            c = np.sort(rng.integers(0, 65536, size=(bw * bh, 2)), axis=1)              # c0 <= c1: three colours + transparent
            idx = np.array([0, 1, 3, 0])[rng.integers(0, 4, size=(bw * bh, 16))]      # never the interpolated colour
            word = (idx << (2 * np.arange(16))[None, :]).sum(axis=1)
            blocks = np.concatenate([c.astype("<u2").view(np.uint8).reshape(-1, 4), word.astype("<u4").view(np.uint8).reshape(-1, 4)],
                                    axis=1).tobytes()
        data += blocks
        img = Image.open(io.BytesIO(dds_bc(blocks, 4 * bw, 4 * bh, 98 if fmt == scene.TEX_BC7 else 71)))
        levels.append(np.asarray(img.convert("RGBA"))[:lh, :lw].copy())
    return scene.TextureData(wt, ht, fmt, data, levels=nlevels), levels


def _bc_chains():
    """BC7 and BC1 chains of a ragged size (20 x 12, 10 x 6, 5 x 3, 2 x 1, 1 x 1): a magnified quad whose bilinear
    footprints straddle blocks and the edge, and quads squeezed along u for every level; BC1 has transparent texels over a
    dark backdrop"""
    w, h = 192, 112
    M, sc = _camera(w, h, 2.0, ry=0.15, rx=-0.1)
    t7, d7 = _bc_levels(scene.TEX_BC7, 20, 12, 5, 700)
    t1, d1 = _bc_levels(scene.TEX_BC1, 20, 12, 5, 800)
    prims = [_px_quad(w, h, sc, 96, 84, 200, 58, z=-0.3, texture=2)]
    for row, cy in ((0, 28), (1, 84)):
        prims.append(_px_quad(w, h, sc, 52, cy, 92, 46, ang=0.06 - 0.1 * row, uv=(-0.1, -0.1, 1.1, 1.1), texture=row))
        x = 108.0
        for wd in (16.0, 10.0, 5.0, 2.5, 1.1):
            prims.append(_px_quad(w, h, sc, x + wd / 2, cy, wd, 40, ang=0.03 * (row + 1), texture=row))
            x += wd + 7.0
    md = pixel_model(prims, textures=[t7, t1, _solid((10, 20, 30, 255))])
    return w, h, [dict(md=md, M=M, decoded={0: d7, 1: d1})]


def _small_triangles():
    """161 x 97: a textured sheet of triangles about 1.3 px across, minified, hanging over the right and the bottom edge:
    every 2 x 2 quad holds pixels its triangle does not cover (and, at the edges, pixels the target does not have), so the
    derivatives come from extrapolation"""
    w, h = 161, 97
    M, sc = _camera(w, h, 1.0, ry=0.5, rx=-0.4)
    rows, cols = 40, 60
    c, s_ = math.cos(0.2), math.sin(0.2)
    verts = []
    for r in range(rows + 1):
        for k in range(cols + 1):
            x, y = 1.3 * (k - cols / 2), 1.3 * (r - rows / 2)
            verts.append(((135 - w / 2.0 + c * x - s_ * y) / sc, -(80 - h / 2.0) / sc + (s_ * x + c * y) / sc, 0.0, k / cols, 1.0 - r / rows))
    strip = dict(verts=verts, indices=scene._strip_indices(rows, cols), topology=scene.TOPO_STRIP, texture=0)
    md = _with_states(pixel_model([strip], textures=[_tex(_tagged_chain(160, 96, 5, 900))]), [(ALPHA, 1, 1, 1)])
    return w, h, [dict(md=md, M=M)]


def _skinned_mips():
    """the production path: the skinned capsule through k_geom with the bone palette and a mip chain"""
    w, h = 160, 96
    md = scene.mesh50k(textured=True, textures=[_tex(_tagged_chain(96, 40, 6, 1000))], rows=14, cols=24)
    return w, h, [dict(md=md, M=scene.to_f32_colmajor(scene.headline_transform(w, h)), palette=scene.bone_palette())]


def _near_plane_translucent():
    """the strip of ramp_strip_w_range, wound the other way and kept by cull NONE (SPEC 10 exchanges two vertices of every
    near-clip sub-triangle), with a translucent mipped texture"""
    w, h = 192, 112
    P = scene.perspective_rh(FOV, w / h, 0.1, 50.0)
    n = 12
    verts = []
    for k in range(n + 1):
        ze = 0.5 - 8.5 * math.sqrt(k / n)
        ye = -0.7 + 0.12 * (-ze)
        verts += [(1.2, ye, ze, k / n, 1.0), (-1.2, ye, ze, k / n, 0.0)]
    chain = _tagged_chain(64, 64, 4, 1100)
    for a in chain:
        a[..., 3] = 40 + (a[..., 0] % 200)
    strip = dict(verts=verts, indices=list(range(len(verts))), topology=scene.TOPO_STRIP, texture=0)
    md = _with_states(pixel_model([strip], textures=[_tex(chain)]), [(ALPHA, 1, 1, 1)])
    return w, h, [dict(md=md, M=scene.to_f32_colmajor(P))]


FRAGMENT_SCENES = {
    "frag_magnified_patch": _magnified_patch,
    "frag_minified_no_mips": _minified_no_mips,
    "frag_mip_chain": _mip_chain,
    "frag_layers_alpha": lambda: _layers((ALPHA,)),
    "frag_layers_off": lambda: _layers((OFF,)),
    "frag_layers_add": lambda: _layers((ADD,), dark=True),
    "frag_layers_mixed": lambda: _layers((ALPHA, OFF, ADD, ALPHA, ADD), dark=True),
    "frag_depth_states": _depth_states,
    "frag_translucent_over_linear": _translucent_over_linear,
    "frag_bc_chains": _bc_chains,
    "frag_small_triangles_161x97": _small_triangles,
    "frag_skinned_mips": _skinned_mips,
    "frag_near_plane_translucent": _near_plane_translucent,
}


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
GEOMETRY_SCENES = list(SCENES)
SCENES.update(FRAGMENT_SCENES)


def _mip_chain_is_fit(ideal):
    """every level of the 100 x 60 chain wins at least 20 compared pixels, and on the 3-level texture the clamp to L - 1
    decides at least 20 -- from the ideal alone"""
    from tests import ideal_compare
    F = ideal.frags
    ok = ideal_compare.expected(ideal).compare.reshape(-1)[F.pix] & F.passes & (F.kind == 2)
    wins = np.bincount(F.level[ok & (F.tex == 0)], minlength=MIP_L)
    assert (wins >= 20).all(), f"compared pixels per level of the full chain: {wins.tolist()}"
    clamped = int((ok & (F.tex == 1) & (F.unclamped_level > F.level)).sum())
    assert clamped >= 20, f"the clamp to L - 1 decides {clamped} pixels"
    assert int((ok & (F.tex == 2) & (F.level >= 3)).sum()) >= 20, "no pixels from the levels that are one texel wide"


CONDITIONS = {"frag_mip_chain": _mip_chain_is_fit}


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def ideal_of(name, mutate=None):
    w, h, draws = scene_of(name)
    return ideal_renderer.render(w, h, draws, mutate=mutate, fragments=name in FRAGMENT_SCENES)


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
