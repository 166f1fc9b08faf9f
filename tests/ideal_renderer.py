"""An independent reference renderer in float64 (plain numpy; nothing compiled, no oracle, no api).

Written from SPEC.md and the reference's pipeline state.  It does not imitate SPEC.md's roundings, its clipper or its
fixed-point setup: it computes what the rules mean.

* vertex fetch (SPEC 2), linear-blend skinning (3) and the transform (4) are ordinary float64 products; next to every clip
  coordinate comes the binary32 forward-error bound ``e = gamma_k * sum|terms|``: the same product evaluated on absolute
  values, ``gamma_k = k u / (1 - k u)``, ``u = 2^-24``, ``k`` the number of rounded operations on the longest path
  (4 transform fmas for a position that decodes exactly, one more for a decode division, 24 for the skinned path: 16
  skinning fmas, the weight product and division, the decode division, 4 transform fmas; 4 more when the matrix is itself
  a rounded product ``VP * Model``; ``4 (depth + 1)`` more when the palette is a rounded chain of pose products).
* rasterisation is 2-D homogeneous: for a pixel centre ``p = (x_ndc, y_ndc, 1)`` and clip-space vertices
  ``v_i = (x_i, y_i, w_i)``, ``lambda = [v0 v1 v2]^-1 p``; the pixel is inside iff every ``lambda_i > 0``; the triangle
  faces the viewer iff ``det [v0 v1 v2] > 0``.  ``z_ndc = sum lambda_i z_i`` (affine in screen space, because
  ``sum lambda_i w_i = 1``), perspective-correct attributes ``u = sum lambda_i u_i / sum lambda_i``.  No near clip, no
  guard band, no snapping; it holds with vertices behind the eye.
* depth LessEqual in submission order, fragments outside ``0 <= z <= 1`` dropped.
* ``fragments=True`` keeps every fragment of every pixel in submission order (``R.frags``) and resolves SPEC 6 and 10 on them
  literally: the ``0 <= z <= 1`` clip always, ``z <= depth`` unless the primitive's depth test is off, ``depth := z`` unless its
  depth write is off; the colour chain runs over exactly the passing fragments.  A textured fragment gets the exact
  perspective-correct ``(u, v)`` of its triangle at the pixel and at the pixels of its 2 x 2 quad (extrapolated where the
  triangle does not cover them), the four products of SPEC 7, the filter and the level they choose, and ``E_u``, ``E_v``: how far
  binary32 and the snapping of SPEC 5 may move ``u`` and ``v``.  ``nearest_at`` / ``linear_at`` / ``blend`` / ``store`` are the
  rules of SPEC 7, 8 and 10 on float64; tests/ideal_compare.py propagates intervals through them.

``mutate=`` builds deliberately wrong references (never the product) for the tests that prove the comparison has teeth.
"""
from __future__ import annotations

import math

import numpy as np

from mt_renderer_amd import scene
from tests.pixel_scenes import PALETTE  # noqa: F401  (re-exported for the comparison)

U = 2.0 ** -24
SNAP = math.sqrt(2.0) / 512.0  # a vertex snapped to the 1/256 px lattice moves by at most this many pixels
DELTA0 = 1.0 / 128.0           # constant part of the edge-ambiguity distance, pixels
Z_ROUND = 2.0 ** -21           # the binary32 roundings of SPEC 6 on values in [0, 1]

K_UV = 11                      # rounded binary32 operations on the longest path of SPEC 7's u = u' / iw
MUTANTS = ("z_perspective_weights", "uv_affine", "flip_winding", "snorm16_div_32768", "weights_div_256", "joint_clamp_n",
           "instance_model_times_vp", "pose_child_on_left", "no_y_flip", "clip_attr_from_outside",
           # the fragment stage (SPEC 7, 8, 10)
           "linear_no_half_texel", "wrap_not_clamp", "coarse_derivatives", "filter_x_only", "level_from_min_product",
           "level_plus_one", "level_unclamped", "level_size_no_max", "add_without_alpha", "alpha_premultiplied",
           "alpha_blended", "dst_unquantised", "store_truncates", "no_prefix_minima", "depth_write_off_ignored",
           "depth_test_off_ignored")
BLEND_ALPHA, BLEND_OFF, BLEND_ADD = 0, 1, 2


def gamma(k):
    return k * U / (1.0 - k * U)


def mat64(m16) -> np.ndarray:
    """16 column-major numbers -> 4x4 float64 indexed (row, column)"""
    return np.asarray(m16, dtype=np.float64).reshape(4, 4).T.copy()


# -------------------------------------------------------------------------------------------------------------------
# SPEC 12: palettes from poses
# -------------------------------------------------------------------------------------------------------------------
def palettes_from_poses(parents, imats, poses, mutate=None):
    """poses [n, J, 16], imats [J, 16] (column-major) -> (palettes [n, J, 4, 4], the same products on absolute values,
    chain depth per joint: 0 for a root).  world_j = world_parent * local_j, palette_j = world_j * imat_j."""
    parents = [int(p) for p in parents]
    J = len(parents)
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, J, 4, 4).transpose(0, 1, 3, 2)
    im = np.asarray(imats, dtype=np.float64).reshape(J, 4, 4).transpose(0, 2, 1)
    world, wabs, depth = [None] * J, [None] * J, [0] * J

    def get(j):
        if world[j] is None:
            p = parents[j]
            L = poses[:, j]
            if p == 255 or p == j:
                world[j], wabs[j], depth[j] = L, np.abs(L), 0
            else:
                get(p)
                if mutate == "pose_child_on_left":
                    world[j] = L @ world[p]
                else:
                    world[j] = world[p] @ L
                wabs[j] = wabs[p] @ np.abs(L)
                depth[j] = depth[p] + 1
        return world[j]
    pal = np.stack([get(j) @ im[j] for j in range(J)], axis=1)
    pabs = np.stack([wabs[j] @ np.abs(im[j]) for j in range(J)], axis=1)
    return pal, pabs, np.array(depth)


# -------------------------------------------------------------------------------------------------------------------
# SPEC 2: vertex fetch
# -------------------------------------------------------------------------------------------------------------------
def _fetch(vb, base, stride, nv, el, mutate):
    """one element of every vertex -> (values [nv, 4] with missing components (0, 0, 0, 1), rounded operations in the
    decode: 0 or 1), or None when the element is not bound"""
    fmt, count, off = int(el[1]), int(el[2]), int(el[3])
    flags = int(el[4]) if len(el) > 4 else 0
    start = base + stride * np.arange(nv, dtype=np.int64)[:, None] + off

    def raw(nbytes, dtype):
        b = np.ascontiguousarray(vb[start + np.arange(nbytes)[None, :]])
        return b.view(dtype).astype(np.float64)
    out = np.zeros((nv, 4))
    out[:, 3] = 1.0
    key = (fmt, count)
    if key == (scene.IEF_F32, 3):
        out[:, :3] = raw(12, "<f4")
        return out, 0
    if key == (scene.IEF_F16, 2):
        out[:, :2] = raw(4, "<f2")
        return out, 0
    if key in ((scene.IEF_U8N, 1), (scene.IEF_U8N, 4), (scene.IEF_U8NL, 3)):
        n = 2 if count == 1 else 4
        out[:, :n] = raw(n, np.uint8) / 255.0
        return out, 1
    if key in ((scene.IEF_S8N, 1), (scene.IEF_S8N, 3), (scene.IEF_S8N, 4)):
        n = 2 if count == 1 else 4
        out[:, :n] = np.maximum(raw(n, np.int8) / 127.0, -1.0)
        return out, 1
    if key in ((scene.IEF_S16N, 1), (scene.IEF_S16N, 3)):
        n = 2 if count == 1 else 4
        out[:, :n] = np.maximum(raw(2 * n, "<i2") / (32768.0 if mutate == "snorm16_div_32768" else 32767.0), -1.0)
        return out, 1
    if fmt == scene.IEF_SCMP3N:
        if not flags & 1:
            return None
        word = np.ascontiguousarray(vb[start + np.arange(4)[None, :]]).view("<u4").astype(np.int64)[:, 0]
        for c in range(3):
            f = (word >> (10 * c)) & 0x3FF
            f = np.where(f >= 512, f - 1024, f)
            out[:, c] = np.maximum(f / 511.0, -1.0)
        return out, 1
    raise ValueError(f"unsupported element {el}")


def vertex_stage(md, prim, M, palette=None, *, M_abs=None, palette_abs=None, k_extra=0, mutate=None):
    """-> clip [nv, 4], uv [nv, 2], e_clip [nv, 4], e_uv [nv, 2].  M is 4x4 (row, column), palette [n, 4, 4] or None;
    M_abs / palette_abs are those products on absolute values when M / the palette are products themselves."""
    f = scene.unpack_primitive(md.prims[prim])
    nv, stride, base = f["vertex_num"], f["vertex_stride"], f["vertex_base"]
    vb = np.asarray(md.vertex_buf, dtype=np.uint8)
    pos = tex = joint = weight = None
    for el in md.layouts[prim]:
        sem = int(el[0])
        if sem == scene.SEM_POSITION and pos is None:
            pos = _fetch(vb, base, stride, nv, el, mutate)
        elif sem == scene.SEM_TEXCOORD and tex is None:
            tex = _fetch(vb, base, stride, nv, el, mutate)
        elif sem == scene.SEM_JOINT and (int(el[1]), int(el[2])) == (scene.IEF_U8, 4):
            joint = vb[base + stride * np.arange(nv)[:, None] + int(el[3]) + np.arange(4)[None, :]].astype(np.int64)
        elif sem == scene.SEM_WEIGHT and (int(el[1]), int(el[2])) == (scene.IEF_U8N, 4):
            weight = vb[base + stride * np.arange(nv)[:, None] + int(el[3]) + np.arange(4)[None, :]].astype(np.float64)
    if pos is None:
        raise ValueError("no Position")
    p, kdec = pos
    ph = np.concatenate([p[:, :3], np.ones((nv, 1))], axis=1)
    M = np.asarray(M, dtype=np.float64)
    Ma = np.abs(M) if M_abs is None else np.asarray(M_abs, dtype=np.float64)
    if joint is not None and weight is not None and palette is not None and len(palette) >= 1:
        P = np.asarray(palette, dtype=np.float64)
        Pa = np.abs(P) if palette_abs is None else np.asarray(palette_abs, dtype=np.float64)
        n = P.shape[0]
        if mutate == "joint_clamp_n":  # clamps to n: one past the end, where this mutant finds an identity matrix
            P = np.concatenate([P, np.eye(4)[None]])
            Pa = np.concatenate([Pa, np.eye(4)[None]])
            j = np.minimum(joint, n)
        else:
            j = np.minimum(joint, n - 1)
        wk = weight / (256.0 if mutate == "weights_div_256" else 255.0)
        q = np.einsum("vk,vkic,vc->vi", wk, P[j], ph)
        qa = np.einsum("vk,vkic,vc->vi", wk, Pa[j], np.abs(ph))
        q, qa = q[:, :3], qa[:, :3]
        k = 24
    else:
        q, qa = ph[:, :3], np.abs(ph[:, :3])
        k = 4 + kdec
    qh = np.concatenate([q, np.ones((nv, 1))], axis=1)
    qah = np.concatenate([qa, np.ones((nv, 1))], axis=1)
    clip = qh @ M.T
    e_clip = gamma(k + k_extra) * (qah @ Ma.T)
    if tex is None:
        uv, e_uv = np.zeros((nv, 2)), np.zeros((nv, 2))
    else:
        uv = tex[0][:, :2].copy()
        e_uv = gamma(1) * np.abs(uv) * tex[1]
    return clip, uv, e_clip, e_uv


# -------------------------------------------------------------------------------------------------------------------
# SPEC 1: primitive assembly
# -------------------------------------------------------------------------------------------------------------------
def assemble(md, prim):
    """-> (triangles [n, 3] of vertex ids in winding order with out-of-range ones dropped, completed triangles)"""
    f = scene.unpack_primitive(md.prims[prim])
    idx = np.asarray(md.index_buf[f["index_ofs"]: f["index_ofs"] + f["index_num"]], dtype=np.int64)
    tris = []
    if f["topology"] == scene.TOPO_LIST:
        for i in range(2, len(idx), 3):
            tris.append((idx[i - 2], idx[i - 1], idx[i]))
    elif f["topology"] == scene.TOPO_STRIP:
        q = 0
        for i, v in enumerate(idx):
            if v == 0xFFFF:
                q = 0
                continue
            q += 1
            if q >= 3:
                tris.append((idx[i - 2], idx[i - 1], idx[i]) if (q - 3) % 2 == 0 else (idx[i - 2], idx[i], idx[i - 1]))
    else:
        raise ValueError("unsupported topology")
    n_in = len(tris)
    t = np.asarray(tris, dtype=np.int64).reshape(-1, 3) + f["index_base"]
    return t[(t < f["vertex_num"]).all(axis=1)], n_in


def _near_clip_wrong_end(V):
    """mutant clip_attr_from_outside: a Sutherland-Hodgman clip against z >= 0 whose intersections take uv from the wrong
    end (t measured from the other vertex).  V [3, 10] = clip xyzw, uv, four error terms.  -> list of [3, 10] triangles"""
    if (V[:, 2] >= 0).all():
        return [V]
    poly = []
    for a in range(3):
        A, B = V[a], V[(a + 1) % 3]
        if A[2] >= 0:
            poly.append(A)
        if (A[2] >= 0) != (B[2] >= 0):
            I, O = (A, B) if A[2] >= 0 else (B, A)
            t = I[2] / (I[2] - O[2])
            X = I + t * (O - I)
            X[4:6] = O[4:6] + t * (I[4:6] - O[4:6])
            poly.append(X)
    return [np.stack([poly[0], poly[k], poly[k + 1]]) for k in range(1, len(poly) - 1)]


# -------------------------------------------------------------------------------------------------------------------
# frames
# -------------------------------------------------------------------------------------------------------------------
class Ideal:
    """what render() returns; every array is [H, W]"""


def _expand(draws, mutate):
    """-> list of (md, M, M_abs, palette, palette_abs, k_extra, instance) per draw call and instance, in order"""
    out = []
    for d in draws:
        md = d["md"]
        if "model_mats" in d:
            vp = mat64(d["vp"])
            mm = np.asarray(d["model_mats"], dtype=np.float64).reshape(-1, 16)
            pal = pabs = None
            kx = 4
            if "poses" in d:
                parents, imats = d["skeleton"]
                pal, pabs, depth = palettes_from_poses(parents, imats, d["poses"], mutate)
                kx += 4 * (int(depth.max()) + 1)
            elif d.get("palettes") is not None:
                p = np.asarray(d["palettes"], dtype=np.float64)
                pal = p.reshape(mm.shape[0], -1, 4, 4).transpose(0, 1, 3, 2)
            for i in range(mm.shape[0]):
                Mo = mat64(mm[i])
                M = Mo @ vp if mutate == "instance_model_times_vp" else vp @ Mo
                out.append((md, M, np.abs(vp) @ np.abs(Mo), None if pal is None else pal[i],
                            None if pabs is None else pabs[i], kx, i))
        else:
            pal = d.get("palette")
            if pal is not None:
                pal = np.asarray(pal, dtype=np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)
            out.append((md, mat64(d["M"]), None, pal, None, 0, 0))
    return out


def render(w, h, draws, clear_depth=1.0, mutate=None, fragments=False, clear=(1.0, 1.0, 1.0, 1.0)) -> Ideal:
    """fragments: also keep every fragment of every pixel in submission order and resolve SPEC 6, 7 and 10 on them
    (R.frags, see _resolve and _sample).  A draw may carry ``decoded``: {texture index: [RGBA8 array per level]} for the
    textures this module cannot read itself (block-compressed ones)."""
    assert mutate is None or mutate in MUTANTS, mutate
    R = Ideal()
    R.w, R.h, R.clear_depth = w, h, clear_depth
    R.fragments, R.mutate, R.clear = fragments, mutate, tuple(float(c) for c in clear)
    R.sy = 1.0 if mutate == "no_y_flip" else -1.0
    R.tri_state, R.textures, R._chunks, R._sub, R._texkey = [], [], [], [], {}
    decoded = {id(d["md"]): d.get("decoded") for d in draws}
    R.depth = np.full((h, w), float(clear_depth))
    R.depth2 = np.full((h, w), float(clear_depth))   # the nearest competing fragment (or the clear depth)
    R.tri = np.full((h, w), -1, dtype=np.int64)       # winner: index into R.tris
    R.u, R.v = np.zeros((h, w)), np.zeros((h, w))
    R.grad_z, R.grad_u, R.grad_v = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))
    R.err_z = np.zeros((h, w))     # sum |lambda_i| (e_z,i + |z_ndc| e_w,i) of the winner
    R.err_u, R.err_v = np.zeros((h, w)), np.zeros((h, w))
    R.tol = np.zeros((h, w))       # the winner's depth tolerance
    R.edge_ambiguous = np.zeros((h, w), dtype=bool)
    R.z_ambiguous = np.zeros((h, w), dtype=bool)
    R.min_edge = np.full((h, w), np.inf)   # the smallest |distance| in pixels from the centre to an edge of a triangle near it
    R.tris = []                    # (draw, instance, primitive, debug id, textured)
    R.tris_in = 0
    R.vertex = []                  # (draw, instance, primitive, clip, uv, e_clip, e_uv)
    sy = 1.0 if mutate == "no_y_flip" else -1.0
    xs_all = 2.0 * (np.arange(w) + 0.5) / w - 1.0
    ys_all = sy * (2.0 * (np.arange(h) + 0.5) / h - 1.0)
    gx, gy = 2.0 / w, sy * 2.0 / h   # d x_ndc / d px, d y_ndc / d py

    for di, (md, M, M_abs, pal, pabs, kx, inst) in enumerate(_expand(draws, mutate)):
        states = getattr(md, "prim_states", None)
        for pr in range(md.nprims):
            f = scene.unpack_primitive(md.prims[pr])
            if f["parts_no"] >= len(md.parts_disp):
                raise ValueError("parts_no out of range")
            if not md.parts_disp[f["parts_no"]]:
                continue
            clip, uv, e_clip, e_uv = vertex_stage(md, pr, M, pal, M_abs=M_abs, palette_abs=pabs, k_extra=kx, mutate=mutate)
            R.vertex.append((di, inst, pr, clip, uv, e_clip, e_uv))
            tl, n_in = assemble(md, pr)
            R.tris_in += n_in
            blend, dwrite, dtest, cull = (0, 1, 1, 0) if states is None else (int(x) for x in np.asarray(states).reshape(-1, 4)[pr])
            if mutate == "depth_write_off_ignored":
                dwrite = 1
            if mutate == "depth_test_off_ignored":
                dtest = 1
            textured = bool(md.prim_to_texture[pr] >= 0 and any(int(e[0]) == scene.SEM_TEXCOORD for e in md.layouts[pr]))
            R.tris.append((di, inst, pr, int(md.prim_debug_id[pr]), textured))
            tid = len(R.tris) - 1
            tex = _texture_of(R, md, int(md.prim_to_texture[pr]), decoded[id(md)]) if textured and fragments else -1
            R.tri_state.append((blend, dwrite, dtest, tex))
            R._state = (dwrite, dtest)
            allv = np.concatenate([clip, uv, e_clip, e_uv], axis=1)  # [nv, 12]
            for t in tl:
                V = allv[t]
                if mutate == "clip_attr_from_outside":
                    for Vc in _near_clip_wrong_end(V.copy()):
                        _raster(R, Vc, tid, cull, mutate, xs_all, ys_all, gx, gy)
                else:
                    _raster(R, V, tid, cull, mutate, xs_all, ys_all, gx, gy)
    R.covered = R.tri >= 0
    R.gap = R.depth2 - R.depth
    R.ambiguous = R.edge_ambiguous | R.z_ambiguous
    if fragments:
        _resolve(R)
        _sample(R)
    return R


def _raster(R, V, tid, cull, mutate, xs_all, ys_all, gx, gy):
    w, h = R.w, R.h
    x, y, z, ww = V[:, 0], V[:, 1], V[:, 2], V[:, 3]
    uu, vv = V[:, 4], V[:, 5]
    ex, ey, ez, ew = V[:, 6], V[:, 7], V[:, 8], V[:, 9]
    eu, ev = V[:, 10], V[:, 11]
    A = np.stack([x, y, ww])          # columns = vertices
    det = float(np.linalg.det(A))
    scale = float(np.abs(A).max()) ** 3
    if scale == 0.0 or abs(det) <= 1e-14 * scale:
        return                        # degenerate (e.g. a repeated index): covers no pixel centre in any arithmetic
    front = det > 0
    if mutate == "flip_winding":
        front = not front
    kept = cull == 1 or (cull == 0 and front) or (cull == 2 and not front)
    # candidate rectangle: the projected bounding box when every vertex is in front of the eye, else the whole target
    x0, x1, y0, y1 = 0, w - 1, 0, h - 1
    if (ww > 0).all() and float(ww.min()) > 1e-6 * float(np.abs(A).max()):
        px_ = (x / ww + 1.0) * (w / 2.0) - 0.5
        py_ = (math.copysign(1.0, gy) * (y / ww) + 1.0) * (h / 2.0) - 0.5
        x0, x1 = max(0, int(math.floor(px_.min())) - 1), min(w - 1, int(math.ceil(px_.max())) + 1)
        y0, y1 = max(0, int(math.floor(py_.min())) - 1), min(h - 1, int(math.ceil(py_.max())) + 1)
        if x0 > x1 or y0 > y1:
            return
    Xn = xs_all[None, x0:x1 + 1]
    Yn = ys_all[y0:y1 + 1, None]
    Ainv = np.linalg.inv(A)           # row i: lambda_i = Ainv[i] . (x_ndc, y_ndc, 1)
    lam = Ainv[:, 0, None, None] * Xn[None] + Ainv[:, 1, None, None] * Yn[None] + Ainv[:, 2, None, None]
    gnorm = np.hypot(Ainv[:, 0] * gx, Ainv[:, 1] * gy)   # |grad lambda_i| per pixel
    dist = lam / gnorm[:, None, None]                    # signed distance to each edge line, pixels, inside positive
    alam = np.abs(lam)
    # rounding of the clip coordinates themselves, in pixels
    rx = (w / 2.0) * np.tensordot(ex, alam, 1) + (w / 2.0) * np.abs(Xn) * np.tensordot(ew, alam, 1)
    ry = (h / 2.0) * np.tensordot(ey, alam, 1) + (h / 2.0) * np.abs(Yn) * np.tensordot(ew, alam, 1)
    rpos = np.hypot(rx, ry)
    if (ww > 2.0 * ew).all():
        # an edge moves no further than its end points: outside a sliver, where the lambdas explode, the sum above
        # overstates what the rounding of three projected vertices can do
        wl = ww - ew
        cap = np.hypot((w / 2.0) * (ex + np.abs(x / ww) * ew) / wl, (h / 2.0) * (ey + np.abs(y / ww) * ew) / wl).max()
        rpos = np.minimum(rpos, cap)
    delta = DELTA0 + rpos
    dmin, dmax = dist.min(axis=0), dist.max(axis=0)
    zn = np.tensordot(z, lam, 1)
    gz = math.hypot(float(z @ Ainv[:, 0]) * gx, float(z @ Ainv[:, 1]) * gy)
    errz = np.tensordot(ez, alam, 1) + np.abs(zn) * np.tensordot(ew, alam, 1)
    tol = gz * SNAP + Z_ROUND + errz
    reach = (zn >= -2.0 * tol) & (zn <= 1.0 + 2.0 * tol)
    if kept:
        near = dmin > -delta
        sure = dmin > delta
        amb = near & ~sure & reach
    else:
        # a culled triangle can only turn up in the product if snapping reverses it: then the pixel is within delta of
        # all three edge lines
        amb = (dmin > -delta) & (dmax <= delta) & reach
    sub = (slice(y0, y1 + 1), slice(x0, x1 + 1))
    if amb.any():
        R.edge_ambiguous[sub] |= amb
    if not kept:
        return
    me = np.where(near & reach, np.abs(dist).min(axis=0), np.inf)
    R.min_edge[sub] = np.minimum(R.min_edge[sub], me)
    inside = dmin > 0
    if not inside.any():
        return
    zamb = inside & ((np.abs(zn) <= 2.0 * tol) | (np.abs(zn - 1.0) <= 2.0 * tol))
    if zamb.any():
        R.z_ambiguous[sub] |= zamb
    if mutate == "z_perspective_weights":
        with np.errstate(all="ignore"):
            zn = np.tensordot(z / ww, lam, 1) / lam.sum(axis=0)
    frag = inside & (zn >= 0.0) & (zn <= 1.0)
    if not frag.any():
        return
    dwrite, dtest = R._state
    if R.fragments:
        # every fragment, in submission order; the triangle it is a fragment of goes to R._sub
        fy, fx = np.nonzero(frag)
        vis = [float(ww[a]) for a in range(3) if z[a] >= 0]
        for a in range(3):
            b = (a + 1) % 3
            if (z[a] >= 0) != (z[b] >= 0):
                vis.append(float(ww[a] + z[a] / (z[a] - z[b]) * (ww[b] - ww[a])))
        wmin = min(vis) if vis else 0.0
        R._sub.append((Ainv, uu, vv, eu, ev, ww, 1.0 / wmin if wmin > 0 else np.inf, bool((z < 0).any() or (ww <= 0).any()), tid))
        R._chunks.append((fy + y0, fx + x0, np.full(fy.size, len(R._sub) - 1), zn[frag], tol[frag],
                          np.broadcast_to(rpos, frag.shape)[frag]))
    dep, dep2 = R.depth[sub], R.depth2[sub]
    win = frag & (zn <= dep) if dtest else frag
    if not dwrite:
        return                        # a passing fragment leaves the depth alone: it is never the depth's owner
    lose = frag & ~win
    # second-best bookkeeping: the old winner becomes the competitor where it is beaten; a loser may be the new competitor
    dep2[win] = dep[win]
    m = lose & (zn < dep2)
    dep2[m] = zn[m]
    if not win.any():
        return
    dep[win] = zn[win]
    R.tri[sub][win] = tid
    with np.errstate(all="ignore"):
        D = lam.sum(axis=0)
        if mutate == "uv_affine":
            un = np.tensordot(uu * ww, lam, 1)
            vn = np.tensordot(vv * ww, lam, 1)
        else:
            un = np.tensordot(uu, lam, 1) / D
            vn = np.tensordot(vv, lam, 1) / D
        # gradients per pixel of u = N / D: (grad N - u grad D) / D
        gD = (Ainv[:, 0].sum() * gx, Ainv[:, 1].sum() * gy)
        gNu = (float(uu @ Ainv[:, 0]) * gx, float(uu @ Ainv[:, 1]) * gy)
        gNv = (float(vv @ Ainv[:, 0]) * gx, float(vv @ Ainv[:, 1]) * gy)
        gu = np.hypot(gNu[0] - un * gD[0], gNu[1] - un * gD[1]) / np.abs(D)
        gv = np.hypot(gNv[0] - vn * gD[0], gNv[1] - vn * gD[1]) / np.abs(D)
        # attribute rounding carried to the pixel, plus the surface point moved by the position rounding
        eun = np.tensordot(eu, alam, 1) / np.abs(D) + gu * rpos
        evn = np.tensordot(ev, alam, 1) / np.abs(D) + gv * rpos
    R.u[sub][win], R.v[sub][win] = un[win], vn[win]
    R.grad_u[sub][win], R.grad_v[sub][win] = gu[win], gv[win]
    R.err_u[sub][win], R.err_v[sub][win] = eun[win], evn[win]
    R.grad_z[sub][win] = gz
    R.err_z[sub][win] = errz[win]
    R.tol[sub][win] = tol[win]


# -------------------------------------------------------------------------------------------------------------------
# SPEC 8: textures as plain arrays
# -------------------------------------------------------------------------------------------------------------------
class Texture:
    """W, H, L; flat [texels of every level, 4] uint8 with off[l], lw[l], lh[l]: level l is max(1, W >> l) x max(1, H >> l)"""


def _texture_of(R, md, index, decoded):
    key = (id(md), index)
    if key in R._texkey:
        return R._texkey[key]
    td = md.textures[index]
    T = Texture()
    T.W, T.H, T.L = int(td.width), int(td.height), int(td.levels)
    T.lw = np.array([max(1, T.W >> l) for l in range(T.L)], dtype=np.int64)
    T.lh = np.array([max(1, T.H >> l) for l in range(T.L)], dtype=np.int64)
    T.off = np.concatenate([[0], np.cumsum(T.lw * T.lh)])[:-1]
    if decoded is not None and index in decoded:
        levels = [np.asarray(a, dtype=np.uint8) for a in decoded[index]]
        assert [a.shape for a in levels] == [(int(hh), int(ww_), 4) for ww_, hh in zip(T.lw, T.lh)]
        T.flat = np.concatenate([a.reshape(-1, 4) for a in levels])
    else:
        if td.fmt != scene.TEX_RGBA8:
            raise ValueError("a block-compressed texture must come decoded")
        T.flat = np.frombuffer(td.data, dtype=np.uint8).reshape(-1, 4)
        assert T.flat.shape[0] == int((T.lw * T.lh).sum())
    T.translucent = bool((T.flat[:, 3] < 255).any())
    R.textures.append(T)
    R._texkey[key] = len(R.textures) - 1
    return R._texkey[key]


def _clampi(f, n):
    """SPEC 7: f < 0 -> 0, f > n - 1 -> n - 1, then truncate (n is at least 1 for every level that exists)"""
    return np.clip(f, 0, np.maximum(n - 1, 0)).astype(np.int64)


def _index(R, f, n):
    if R.mutate == "wrap_not_clamp":
        return np.mod(f, np.maximum(n, 1)).astype(np.int64)
    return _clampi(f, n)


def texels(R, tex, level, ix, iy):
    """bytes / 255 of texel (ix, iy) of `level` of texture `tex`, per element"""
    out = np.zeros((tex.size, 4))
    for t in np.unique(tex):
        T = R.textures[int(t)]
        m = tex == t
        l = level[m]
        stride = (T.W >> l) if R.mutate == "level_size_no_max" else T.lw[l]
        out[m] = T.flat[T.off[l] + iy[m] * stride + ix[m]] / 255.0
    return out


def nearest_at(R, i, u, v):
    """the nearest texel (SPEC 7) fragments ``i`` of R.frags read at (u, v), level as decided for them -> [n, 4] in [0, 1]"""
    F = R.frags
    tex, l, ls = F.tex[i], F.level[i], F.size_level[i]
    W = np.array([T.W for T in R.textures])[tex]
    H = np.array([T.H for T in R.textures])[tex]
    if R.mutate == "level_size_no_max":
        wl, hl = W >> ls, H >> ls
    else:
        wl, hl = np.maximum(1, W >> ls), np.maximum(1, H >> ls)
    # the level that is read; it differs from the level whose size is used only under the mutant that does not clamp
    lw = np.maximum(1, W >> l)
    lh = np.maximum(1, H >> l)
    ix = np.minimum(_index(R, np.floor(u * wl), wl), lw - 1)
    iy = np.minimum(_index(R, np.floor(v * hl), hl), lh - 1)
    return texels(R, tex, l, ix, iy)


def nearest_index(R, i, u, v):
    """the texel index after clampi, for counting candidates"""
    F = R.frags
    tex, l = F.tex[i], F.level[i]
    W = np.array([T.W for T in R.textures])[tex]
    H = np.array([T.H for T in R.textures])[tex]
    wl, hl = np.maximum(1, W >> l), np.maximum(1, H >> l)
    return _clampi(np.floor(u * wl), wl), _clampi(np.floor(v * hl), hl)


def linear_at(R, i, u, v):
    """the clamp-to-edge bilinear sample of level 0 (SPEC 7) -> [n, 4] in [0, 1]"""
    F = R.frags
    tex = F.tex[i]
    W = np.array([T.W for T in R.textures])[tex]
    H = np.array([T.H for T in R.textures])[tex]
    half = 0.0 if R.mutate == "linear_no_half_texel" else 0.5
    x, y = u * W - half, v * H - half
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    zero = np.zeros(tex.size, dtype=np.int64)
    c0, c1, r0, r1 = _index(R, x0, W), _index(R, x0 + 1, W), _index(R, y0, H), _index(R, y0 + 1, H)
    c00, c10 = texels(R, tex, zero, c0, r0), texels(R, tex, zero, c1, r0)
    c01, c11 = texels(R, tex, zero, c0, r1), texels(R, tex, zero, c1, r1)
    top = c00 + fx * (c10 - c00)
    bot = c01 + fx * (c11 - c01)
    return top + fy * (bot - top)


def blend(R, mode, s, d):
    """SPEC 10 on [n, 4] source and destination in [0, 1], mode per element -> [n, 4] before the store"""
    a = s[:, 3:4]
    mode = mode[:, None]
    over = s[:, :3] * a + d[:, :3] * (1.0 - a)
    add = s[:, :3] * a + d[:, :3]
    if R.mutate == "alpha_premultiplied":
        over = s[:, :3] + d[:, :3] * (1.0 - a)
    if R.mutate == "add_without_alpha":
        add = s[:, :3] + d[:, :3]
    rgb = np.where(mode == BLEND_OFF, s[:, :3], np.where(mode == BLEND_ADD, add, over))
    alpha = a + d[:, 3:4] * (1.0 - a) if R.mutate == "alpha_blended" else a
    return np.concatenate([rgb, alpha], axis=1)


def store(R, x255):
    """the byte a value in byte units (already clamped to [0, 255]) is stored as"""
    return np.floor(x255) if R.mutate == "store_truncates" else np.rint(x255)


def carried(R, byte, x255):
    """what the next layer reads as dst, in [0, 1]: the stored byte"""
    return x255 / 255.0 if R.mutate == "dst_unquantised" else byte / 255.0


# -------------------------------------------------------------------------------------------------------------------
# SPEC 6 and 10: the fragments of a pixel in submission order
# -------------------------------------------------------------------------------------------------------------------
class Frags:
    """every array is [number of fragments], sorted by pixel and, within a pixel, by submission order (rank 0 first)"""


def _resolve(R):
    w, h = R.w, R.h
    F = R.frags = Frags()
    if R._chunks:
        py, px, sub, z, tol, rpos = (np.concatenate([c[k] for c in R._chunks]) for k in range(6))
    else:
        py = px = sub = np.zeros(0, dtype=np.int64)
        z = tol = rpos = np.zeros(0)
    o = np.argsort(py * w + px, kind="stable")
    F.py, F.px, F.sub, F.z, F.tol, F.rpos = py[o], px[o], sub[o], z[o], tol[o], rpos[o]
    F.pix = F.py * w + F.px
    n = F.pix.size
    first = np.ones(n, dtype=bool)
    first[1:] = F.pix[1:] != F.pix[:-1]
    F.rank = np.arange(n) - np.maximum.accumulate(np.where(first, np.arange(n), 0))
    F.layers = int(F.rank.max()) + 1 if n else 0
    sub_tid = np.array([s[8] for s in R._sub], dtype=np.int64).reshape(-1)
    F.tid = sub_tid[F.sub]
    st = np.array(R.tri_state, dtype=np.int64).reshape(-1, 4)[F.tid]
    F.blend, F.dwrite, F.dtest, F.tex = st[:, 0], st[:, 1], st[:, 2], st[:, 3]
    F.did = np.array([t[3] for t in R.tris], dtype=np.int64).reshape(-1)[F.tid]
    translucent = np.array([T.translucent for T in R.textures] + [False])
    # a fragment whose effect depends on what lies under it or on the order: anything but "replace, test and write"
    F.special = (F.blend == BLEND_ADD) | (F.dwrite == 0) | (F.dtest == 0) | translucent[F.tex]
    depth = np.full(w * h, float(R.clear_depth))
    dtol = np.zeros(w * h)
    owner = np.full(w * h, -1, dtype=np.int64)
    F.passes = np.zeros(n, dtype=bool)
    tie = np.zeros(w * h, dtype=bool)
    for k in range(F.layers):
        i = np.nonzero(F.rank == k)[0]
        p = F.pix[i]
        tested = F.dtest[i] == 1
        ps = (F.z[i] <= depth[p]) | ~tested
        tie[p] |= tested & (np.abs(F.z[i] - depth[p]) <= F.tol[i] + dtol[p])
        F.passes[i] = True if R.mutate == "no_prefix_minima" else ps
        wr = ps & (F.dwrite[i] == 1)
        depth[p[wr]], dtol[p[wr]], owner[p[wr]] = F.z[i][wr], F.tol[i][wr], i[wr]
    special = np.zeros(w * h, dtype=bool)
    special[F.pix[F.special]] = True
    R.special, R.decision_tie = special.reshape(h, w), tie.reshape(h, w)
    R.chain_depth = depth.reshape(h, w)
    if R.mutate is None:
        assert (R.chain_depth == R.depth).all()


# -------------------------------------------------------------------------------------------------------------------
# SPEC 7: (u, v), fine quad derivatives, filter and level of every textured fragment
# -------------------------------------------------------------------------------------------------------------------
def _sample(R):
    F = R.frags
    n = F.pix.size
    F.kind = np.zeros(n, dtype=np.int64)          # 0 flat, 1 linear, 2 nearest
    F.level = np.zeros(n, dtype=np.int64)
    F.size_level = np.zeros(n, dtype=np.int64)
    F.decision_ambiguous = np.zeros(n, dtype=bool)
    F.u, F.v, F.Eu, F.Ev = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    F.products = np.zeros((n, 4))
    i = np.nonzero(F.tex >= 0)[0]
    if not i.size:
        return
    S = R._sub
    Ainv = np.stack([s[0] for s in S])[F.sub[i]]                 # [n, 3, 3]
    uu, vv, eu, ev, ww = (np.stack([s[k] for s in S])[F.sub[i]] for k in (1, 2, 3, 4, 5))
    iwmax = np.array([s[6] for s in S])[F.sub[i]]
    clipped = np.array([s[7] for s in S])[F.sub[i]]
    umax, vmax = np.abs(uu).max(axis=1), np.abs(vv).max(axis=1)
    gx, gy = 2.0 / R.w, R.sy * 2.0 / R.h
    rpos = F.rpos[i]

    def at(X, Y):
        """exact (u, v) of the fragment's triangle at pixel (X, Y), covered or not, and their uncertainty there"""
        xn = 2.0 * (X + 0.5) / R.w - 1.0
        yn = R.sy * (2.0 * (Y + 0.5) / R.h - 1.0)
        lam = Ainv[:, :, 0] * xn[:, None] + Ainv[:, :, 1] * yn[:, None] + Ainv[:, :, 2]
        with np.errstate(all="ignore"):
            D = lam.sum(axis=1)
            u, v = (lam * uu).sum(axis=1) / D, (lam * vv).sum(axis=1) / D
            if R.mutate == "uv_affine":
                u, v = (lam * uu * ww).sum(axis=1), (lam * vv * ww).sum(axis=1)
            aD = np.abs(D)
            gD = (Ainv[:, :, 0].sum(axis=1) * gx, Ainv[:, :, 1].sum(axis=1) * gy)
            out = [u, v]
            # screen-space barycentrics of the triangle that is set up: lam_i w_i of this one where nothing is clipped
            # away; a clipped part is taken to keep a helper pixel within |beta| sum 3
            sb = np.where(clipped, 3.0, np.abs(lam * ww).sum(axis=1))
            for a, q, e, amax in ((uu, u, eu, umax), (vv, v, ev, vmax)):
                gN = ((a * Ainv[:, :, 0]).sum(axis=1) * gx, (a * Ainv[:, :, 1]).sum(axis=1) * gy)
                g = np.hypot(gN[0] - q * gD[0], gN[1] - q * gD[1]) / aD
                out.append(g * SNAP + (e * np.abs(lam)).sum(axis=1) / aD + g * rpos
                           + gamma(K_UV) * (1.0 + 2.0 * sb) * iwmax * (amax + np.abs(q)) / aD)
        return out
    px, py = F.px[i], F.py[i]
    qx, qy = px & ~1, py & ~1
    u, v, Eu, Ev = at(px, py)
    if R.mutate == "coarse_derivatives":
        ends = ((qx, qy), (qx + 1, qy), (qx, qy), (qx, qy + 1))
    else:
        ends = ((qx, py), (qx + 1, py), (px, qy), (px, qy + 1))
    (ua, va, Eua, Eva), (ub, vb, Eub, Evb), (uc, vc, Euc, Evc), (ud, vd, Eud, Evd) = (at(X, Y) for X, Y in ends)
    Wt = np.array([T.W for T in R.textures], dtype=np.float64)[F.tex[i]]
    Ht = np.array([T.H for T in R.textures], dtype=np.float64)[F.tex[i]]
    L = np.array([T.L for T in R.textures], dtype=np.int64)[F.tex[i]]
    with np.errstate(all="ignore"):
        p = np.stack([np.abs(ub - ua) * Wt, np.abs(vb - va) * Ht, np.abs(ud - uc) * Wt, np.abs(vd - vc) * Ht], axis=1)
        e = np.stack([(Eua + Eub) * Wt, (Eva + Evb) * Ht, (Euc + Eud) * Wt, (Evc + Evd) * Ht], axis=1) + gamma(2) * p
        bad = ~np.isfinite(p).all(axis=1) | ~np.isfinite(e).all(axis=1)
        p, e = np.where(bad[:, None], 2.0, p), np.where(bad[:, None], 0.0, e)
        lo, hi = p - e, p + e
        f = slice(0, 2) if R.mutate == "filter_x_only" else slice(0, 4)
        linear = (p[:, f] <= 1.0).all(axis=1)
        sure_linear = (hi[:, f] <= 1.0).all(axis=1)
        sure_nearest = (lo[:, f] > 1.0).any(axis=1)

        def level_of(m, clamp=True):
            l = np.maximum(0, np.ceil(np.log2(np.maximum(m, 1e-300)) - 0.5)).astype(np.int64)
            if R.mutate == "level_plus_one":
                l = l + 1
            return np.minimum(l, L - 1) if clamp else l
        pick = np.min if R.mutate == "level_from_min_product" else np.max
        m, mlo, mhi = pick(p, axis=1), pick(lo, axis=1), pick(hi, axis=1)
        level = level_of(m)
        # m * m is one more rounded multiplication: gamma_1 on the square, half of it on m
        level_amb = level_of(mlo * (1.0 - gamma(1))) != level_of(mhi * (1.0 + gamma(1)))
    F.kind[i] = np.where(linear, 1, 2)
    F.level[i] = np.where(linear, 0, level)
    F.size_level[i] = np.where(linear, 0, level_of(m, clamp=R.mutate != "level_unclamped"))
    F.unclamped_level = np.zeros(n, dtype=np.int64)
    F.unclamped_level[i] = np.where(linear, 0, level_of(m, clamp=False))
    F.decision_ambiguous[i] = bad | ~(sure_linear | sure_nearest) | (~linear & level_amb)
    F.u[i], F.v[i], F.Eu[i], F.Ev[i] = u, v, Eu, Ev
    F.products[i] = p
