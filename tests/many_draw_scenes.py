"""Deterministic frames of MANY draws for the sharded, culled submit path (no GPU needed to build them).

Target 320 x 200 = 20 x 13 bins with a ragged bottom row; three even bands cut the bin rows at 4 and 8, pixel rows 64 and
128.  ``crowd(ndraws)`` returns the frame as a draw list in the dict form of tests/helpers.py (every dict also names its
``kind``), and ``Resident`` keeps the models and the persistent batches of such a list on a device, for frame loops that
render prefixes of it again and again.  The kinds, in a cycle of seven draws:

  single       a skinned model with a palette of its own (chunk culling only, no instance list): the 3-chunk capsule in
               even cycles, the 17-chunk one (two mask groups, the second with a single chunk) in odd ones
  batch        a persistent api.Batch of an ODD number of instances (3, 5, 7, 9) of the 3-chunk capsule: nx * ninst masks
               is odd, so the draw behind it starts on the padding.  Even cycles: per-instance texture override, a texture
               with alpha < 255 and an opaque one -- which also makes every frame of two or more draws a mixed one
  unboundable  a batch of the random model whose weights do not sum to 255: instance culling is skipped for it
  owned        Frame.draw_instances without palettes: a batch the frame owns, unskinned, no launch hints
  overlay      overlay cubes
  translucent  a translucent textured quad over what came before (nearer than everything) ...
  opaque       ... and an opaque quad behind it, submitted after it: which of the two is drawn first shows

Six kinds and the pair do not fit into five draws: the first five are single, batch, unboundable, owned, overlay, and every
prefix of seven or more holds every kind."""
from __future__ import annotations

import math

import numpy as np

from mt_renderer_amd import scene
from tests.pixel_scenes import pixel_model, pixel_to_ndc_matrix

W, H = 320, 200
WORLD = 3
EVEN_BANDS = [0, 4, 8, 13]
UNEVEN_BANDS = [0, 5, 5, 13]  # rank 1 owns no bin at all
CYCLE = ("single", "batch", "unboundable", "owned", "overlay", "translucent", "opaque")
KINDS = CYCLE
DIST = 2.3  # everything but the quads sits about this far in front of the reference camera
_HY = DIST * math.tan(math.radians(25.0))  # half the visible height there (fov 50), in world units
_PX = H / (2.0 * _HY)                      # pixels per world unit at that distance
# anchors of instance centres in pixel rows: inside band 0, on the 0 | 1 border, inside band 1, on the 1 | 2 border, inside band 2
ROWS = (30.0, 64.0, 96.0, 128.0, 166.0)


def _random_model(rng, normalised, many_joints):
    """strips of random quads with random joints / weights: nothing like the tidy capsule"""
    nverts, nquads = 600, 260
    pos = rng.uniform(-1, 1, size=(nverts, 3))
    pos[:, 2] *= 0.2
    stride = 24
    vb = np.zeros((nverts, stride), dtype=np.uint8)
    p16 = np.clip(np.round(pos * 32767), -32767, 32767).astype(np.int16)
    vb[:, 0:6] = p16.view(np.uint8).reshape(nverts, 6)
    vb[:, 12:16] = np.float16(rng.uniform(0, 1, size=(nverts, 2))).view(np.uint8).reshape(nverts, 4)
    joints = rng.integers(0, 40 if many_joints else 6, size=(nverts, 4)).astype(np.uint8)
    wts = rng.integers(0, 256, size=(nverts, 4)).astype(np.int64)
    wts[rng.uniform(size=nverts) < 0.3, 2:] = 0  # some vertices use two joints only
    if normalised:
        wts = np.maximum(wts, 0)
        tot = wts.sum(axis=1, keepdims=True)
        tot[tot == 0] = 1
        wts = wts * 255 // tot
        wts[:, 0] += 255 - wts.sum(axis=1)
    vb[:, 16:20] = joints
    vb[:, 20:24] = np.clip(wts, 0, 255).astype(np.uint8)
    idx = []
    for q in range(nquads):  # short strips of nearby vertices so triangles stay small
        a = int(rng.integers(0, nverts - 8))
        idx += [a, a + 1, a + 2, a + 3, a + 4, 0xFFFF]
    # make triangles local: sort vertices along x so neighbours in index are neighbours in space
    order = np.argsort(pos[:, 0] + 0.05 * pos[:, 1])
    vb = vb[order]
    index_buf = np.array(idx, dtype=np.uint16)
    prim = scene.pack_primitive(vertex_num=nverts, vertex_stride=stride, topology=scene.TOPO_STRIP, vertex_base=0, index_ofs=0,
                                index_num=len(idx), index_base=0)
    lay = [(scene.SEM_POSITION, scene.IEF_S16N, 3, 0), (scene.SEM_TEXCOORD, scene.IEF_F16, 2, 12), (scene.SEM_JOINT, scene.IEF_U8, 4, 16),
           (scene.SEM_WEIGHT, scene.IEF_U8N, 4, 20)]
    return scene.ModelData(vertex_buf=vb.reshape(-1), index_buf=index_buf, prims=np.stack([prim]), layouts=[lay],
                           prim_to_texture=np.array([-1], dtype=np.int32), prim_debug_id=np.array([5], dtype=np.uint32),
                           parts_disp=np.ones(1, dtype=np.uint8))


def chunks_of(md) -> int:
    """geometry chunks of a model: 62 index positions each, per primitive (SPEC 5.3)"""
    return sum((scene.unpack_primitive(md.prims[p])["index_num"] + 61) // 62 for p in range(md.nprims))


def view_proj():
    return scene.to_f32_colmajor(scene.reference_view_proj(W, H))


def at_pixel(px: float, py: float, size_px: float, size_world: float, yaw: float = 0.0, dist: float = DIST) -> np.ndarray:
    """model matrix (4 x 4, float64) that puts the model's origin where pixel (px, py) is, `dist` in front of the reference
    camera, and scales `size_world` model units to about `size_px` pixels"""
    k = dist / DIST
    x = -5.0 + (px - 0.5 * W) / _PX * k
    y = (0.5 * H - py) / _PX * k
    s = size_px / _PX * k / size_world
    return scene.mat_translate(x, y, 1.0 - dist) @ scene.mat_rot_y(yaw) @ scene.mat_scale(s, s, s)


def _capsule(rows, cols, debug_id, **kw):
    md = scene.skinned_capsule_model([((0.0, 0.0, 0.0), 0.35, 1.6)], rows=rows, cols=cols, **kw)
    md.prim_debug_id = np.array([debug_id], dtype=np.uint32)
    return md


class Crowd:
    """draws: the frame; kinds[i]: the kind of draws[i]; a prefix of the draw list is a frame too"""

    def __init__(self, draws):
        self.draws = draws
        self.kinds = [d["kind"] for d in draws]

    def of_kind(self, kind):
        return [d for d in self.draws if d["kind"] == kind]


def _models():
    tex = [scene.checker_rgba8_texture(16, 16, cell=2, alpha=(255, 120)), scene.checker_rgba8_texture(8, 8, cell=1)]
    quad = [(0, 0, 0.0, 0.0, 0.0), (0, 1, 0.0, 0.0, 1.0), (1, 1, 0.0, 1.0, 1.0), (1, 0, 0.0, 1.0, 0.0)]
    return dict(
        small=_capsule(6, 10, 1),                                   # 137 index positions: 3 chunks, one mask group
        big=_capsule(24, 20, 2),                                    # 1031: 17 chunks, two mask groups, the second ragged
        small_tex=_capsule(6, 10, 3, textured=True, textures=tex),  # the batches with a texture override
        owned=_capsule(4, 8, 7),
        hostile=_random_model(np.random.default_rng(4711), normalised=False, many_joints=False),
        glass=pixel_model([dict(verts=quad, indices=[0, 1, 2, 0, 2, 3], texture=0)],
                          [scene.checker_rgba8_texture(8, 8, cell=1, alpha=(230, 30))]),
        wall=pixel_model([dict(verts=[v[:3] for v in quad], indices=[0, 1, 2, 0, 2, 3], debug_id=11)]),
    )


def crowd(ndraws: int, seed: int = 0) -> Crowd:
    rng = np.random.default_rng(1000 + seed)
    md = _models()
    vp = view_proj()
    draws = []
    for di in range(ndraws):
        c, kind = divmod(di, len(CYCLE))
        kind = CYCLE[kind]
        jx = float(rng.uniform(-12.0, 12.0))  # drawn in submission order: crowd(n) is the first n draws of every larger crowd
        yaw = float(rng.uniform(0.0, 2.0 * math.pi))
        if kind == "single":
            big = c % 2 == 1
            # the big one spans both band borders; every fourth is wholly off the target
            px = -90.0 if c % 4 == 2 else 50.0 + 55.0 * (c % 5) + jx
            py = 100.0 if big else ROWS[(2 * c) % 5]
            M = scene.reference_view_proj(W, H) @ at_pixel(px, py, 150.0 if big else 44.0, 1.6, yaw)
            d = dict(md=md["big" if big else "small"], M=scene.to_f32_colmajor(M), palette=scene.bone_palette(64, t=0.25 + 0.6 * c))
        elif kind == "batch":
            n = (3, 5, 7, 9)[c % 4]
            mats, pals = [], []
            for k in range(n):
                # rows of every class for every rank over the batches; the last instance of a batch is off the target
                off = k == n - 1
                px = W + 70.0 if off and c % 2 == 0 else 24.0 + ((k * 83 + c * 47) % 272) + 0.25 * jx
                py = H + 60.0 if off and c % 2 == 1 else ROWS[(k + 2 * c) % 5] + (0.0 if (k + 2 * c) % 5 in (1, 3) else 0.2 * jx)
                mats.append(scene.to_f32_colmajor(at_pixel(px, py, 40.0, 1.6, yaw + k)))
                pals.append(scene.bone_palette(64, t=0.25 + 0.37 * (k + 10 * c)))
            d = dict(md=md["small" if c % 2 else "small_tex"], vp=vp, model_mats=np.stack(mats), palettes=np.stack(pals))
            if c % 2 == 0:
                d["tex_override"] = [k % 2 for k in range(n)]
        elif kind == "unboundable":
            npal = 8
            pal = np.zeros((npal, 16), dtype=np.float32)
            for j in range(npal):
                A = np.eye(4)
                A[:3, :3] = np.linalg.qr(rng.normal(size=(3, 3)))[0] @ np.diag(rng.uniform(0.7, 1.3, size=3))
                A[:3, 3] = rng.uniform(-0.3, 0.3, size=3)
                pal[j] = scene.to_f32_colmajor(A)
            spots = [(40.0 + 60.0 * ((c + k) % 5), ROWS[(k + c + 1) % 5]) for k in range(3)] + [(-120.0, 100.0)]
            mats = np.stack([scene.to_f32_colmajor(at_pixel(px + jx, py, 7.0, 1.0, 0.3 * k)) for k, (px, py) in enumerate(spots)])
            d = dict(md=md["hostile"], vp=vp, model_mats=mats, palettes=np.stack([np.roll(pal, k, axis=0) for k in range(len(mats))]))
        elif kind == "owned":
            spots = [(300.0 - 50.0 * ((c + k) % 6), ROWS[(k + 3 * c + 2) % 5]) for k in range(3)] + [(160.0, -80.0)]
            mats = np.stack([scene.to_f32_colmajor(at_pixel(px + jx, py, 34.0, 1.6, yaw + 0.5 * k)) for k, (px, py) in enumerate(spots)])
            d = dict(md=md["owned"], vp=vp, model_mats=mats, palettes=None, owned=True)
        elif kind == "overlay":
            spots = [(20.0 + 70.0 * ((c + k) % 4), ROWS[(k + c) % 5] + 5.0) for k in range(4)] + [(W + 40.0, 30.0)]
            cubes = np.stack([scene.to_f32_colmajor(at_pixel(px + jx, py, 9.0, 1.0, 0.4 * k)) for k, (px, py) in enumerate(spots)])
            d = dict(md=md["small"], vp=vp, overlay=cubes)
        else:
            # the translucent quad at z = 0.5 (everything else is beyond 0.99) and the opaque one behind it, shifted: swapped,
            # the opaque one shows through the translucent one where they overlap
            glass = kind == "translucent"
            x0, y0 = 30.0 + 41.0 * (c % 6), 30.0 + 23.0 * (c % 4)
            if not glass:
                x0, y0 = x0 + 16.0, y0 + 14.0
            M = np.frombuffer(pixel_to_ndc_matrix(W, H).tobytes(), dtype=np.float32).reshape(4, 4).T.astype(np.float64)
            M = M @ scene.mat_translate(x0, y0, 0.5 if glass else 0.6) @ scene.mat_scale(44.0, 64.0, 1.0)
            d = dict(md=md["glass" if glass else "wall"], M=scene.to_f32_colmajor(M))
        d["kind"] = kind
        draws.append(d)
    return Crowd(draws)


class Resident:
    """The models, textures and PERSISTENT batches of a draw list on one device, created once; frame() renders a selection
    of the draws (a prefix, a permutation) into a new api.Frame.  What render_gpu re-creates for every frame stays here
    across frames: batches keep their launch-hint slots, models their palette rings, the device's slots their counters."""

    def __init__(self, dev, draws):
        from mt_renderer_amd import api
        self.dev, self.draws, self.models, self.batches = dev, draws, {}, {}
        for i, d in enumerate(draws):
            if "overlay" in d:
                continue
            if id(d["md"]) not in self.models:
                self.models[id(d["md"])] = api.Model.new(dev, d["md"])
            if "model_mats" in d and not d.get("owned"):
                self.batches[i] = api.Batch(dev, self.models[id(d["md"])], d["model_mats"], d.get("palettes"), d.get("tex_override"))

    def frame(self, which, shard=None, w=W, h=H, submit=True, vp=None):
        """which: a draw count (that prefix) or a sequence of draw indices, in submission order; vp: a camera for every
        batch draw in place of its own"""
        from mt_renderer_amd import api
        order = range(which) if isinstance(which, int) else which
        fr = api.Frame(self.dev, w, h)
        try:
            if shard:
                fr.set_shard(*shard)
            for i in order:
                d = self.draws[i]
                if "overlay" in d:
                    fr.draw_overlay_cubes(d["vp"], d["overlay"])
                elif i in self.batches:
                    fr.draw_batch(self.batches[i], d["vp"] if vp is None else vp)
                elif "model_mats" in d:
                    fr.draw_instances(self.models[id(d["md"])], d["vp"], d["model_mats"], d.get("palettes"))
                else:
                    m = self.models[id(d["md"])]
                    m.set_palette(d.get("palette"))
                    m.render(fr, d["M"])
            if submit:
                fr.submit()
        except Exception:
            fr.close()
            raise
        return fr

    def render(self, which, shard=None, w=W, h=H, vp=None):
        fr = self.frame(which, shard, w, h, vp=vp)
        try:
            return read(fr)
        finally:
            fr.close()

    def close(self):
        for b in self.batches.values():
            b.close()
        for m in self.models.values():
            m.close()
        self.batches, self.models = {}, {}


def read(fr):
    """waits for a submitted frame: (colour, depth bits, stats)"""
    fr.wait()
    return fr.color(), fr.depth().view(np.uint32), fr.stats()
