"""Numpy model of SPEC.md section 16 (animation layers), written from that text, and the inputs its tests share.

`sample(clips, layers, njoints, masks)` carries the rules out in binary32, one rounded numpy operation per operator, and
gives the local matrices bit for bit.  `step_exact` carries every layer step out in float64, restarted from the binary32
(T, Q, S) the step starts with, the layer's own clip from its binary32 `(i0, i1, a)` or `(k, k1)` and `e` as given, and
propagates the sum of the terms on absolute values that the per-step bound of section 16 is stated against.  Position,
lerp, nlerp, `V` and `Trace` are section 14's (tests/anim_model.py); the track source is section 15's
(tests/anim_tracks_model.py).

clips: a list of uniform clips (keys [nkeys, njoints, 12] float32, flags) or of track clips (nticks, flags, tracks, times,
values); layers: an array [n, L] with the fields of api.ANIM_LAYER; masks: None or float32 [M, njoints], the user's masks
1..M.  `variant` names one deliberately wrong reading of the section (WRONG_VARIANTS)."""
import numpy as np

from tests import anim_model as am
from tests import anim_tracks_model as tm

F = np.float32
U = am.U
MAX_LAYERS = 8
OVERRIDE, ADDITIVE = 0, 1
LAYER = np.dtype([("clip", "<u4"), ("x", "<f4"), ("w", "<f4"), ("mask", "<u2"), ("mode", "<u2")])
WRONG_VARIANTS = ("mode_ignored", "qmul_reversed", "no_skip", "mask_ignored", "fused_add", "scale_product")
# rounded operations on the rotation's path through one layer step (section 16): the layer's sample, e on the lerp's
# product, qmul for ADDITIVE, the nlerp
K_STEP = {("uniform", OVERRIDE): 21, ("uniform", ADDITIVE): 25, ("tracks", OVERRIDE): 23, ("tracks", ADDITIVE): 27}


def kind_of(clips):
    return "tracks" if len(clips[0]) == 5 else "uniform"


def qmul(p, q):
    """the Hamilton product p q in section 16's operation order; p, q: (x, y, z, w)"""
    px, py, pz, pw = p
    qx, qy, qz, qw = q
    return (((pw * qx + px * qw) + py * qz) - pz * qy,
            ((pw * qy - px * qz) + py * qw) + pz * qx,
            ((pw * qz + px * qy) - py * qx) + pz * qw,
            ((pw * qw - px * qx) - py * qy) - pz * qz)


class _Source:
    """one clip at x for every instance and joint: (T, Q, S) as tuples of [n, J] values, binary32 or V"""

    def __init__(self, clips, njoints):
        self.kind, self.J, self.C = kind_of(clips), njoints, len(clips)
        if self.kind == "uniform":
            self.nkeys, self.flags, self.first, self.keys = am._clip_tables(clips, njoints)
        else:
            self.arrays = tm.concat(clips, njoints)

    def sample(self, clip, x, exact, trace, counted):
        n, J = len(x), self.J

        def num(val):
            return am.V(val) if exact else np.ascontiguousarray(val, dtype=F)

        if self.kind == "uniform":
            c = np.minimum(np.asarray(clip, dtype=np.int64), self.C - 1)
            i0, i1, a = am.position(x, self.nkeys[c], (self.flags[c] & am.CLIP_LOOP) != 0)
            k0, k1 = self.keys[self.first[c] + i0], self.keys[self.first[c] + i1]
            av = num(np.broadcast_to(a[:, None], (n, J)))
            with np.errstate(all="ignore"):
                T = tuple(am.lerp_rule(num(k0[..., i]), num(k1[..., i]), av) for i in (0, 1, 2))
                Q = am.nlerp(tuple(num(k0[..., i]) for i in (4, 5, 6, 7)), tuple(num(k1[..., i]) for i in (4, 5, 6, 7)), av, am.lerp_rule, True, trace, counted)
                S = tuple(am.lerp_rule(num(k0[..., i]), num(k1[..., i]), av) for i in (8, 9, 10))
            return T, Q, S
        _, _, tracks, _, values = self.arrays
        c, _, K0, K1, A, AX = tm._locate_states(self.arrays, np.asarray(clip), np.asarray(x, dtype=F), J)
        lo, step = tracks["lo"][c], tracks["step"][c]

        def lin(K, ch):
            wd = values[K[..., ch]]
            if exact:
                v = wd[..., :3].astype(np.float64)
                l, s = lo[:, :, ch].astype(np.float64), step[:, :, ch].astype(np.float64)
                return tuple(am.V(l[..., i] + v[..., i] * s[..., i], np.abs(l[..., i]) + v[..., i] * np.abs(s[..., i])) for i in range(3))
            d = tm.decode_lin(wd, lo[:, :, ch], step[:, :, ch])
            return tuple(num(d[..., i]) for i in range(3))

        def rot(K):
            wd = values[K[..., 1]]
            if exact:
                q = np.maximum(np.ascontiguousarray(wd).view(np.int16).astype(np.float64) / 32767.0, -1.0)
            else:
                q = tm.decode_rot(wd)
            return tuple(num(q[..., i]) for i in range(4))

        a = [num(AX[..., ch]) if exact else num(A[..., ch]) for ch in range(3)]
        with np.errstate(all="ignore"):
            T = tuple(am.lerp_rule(p, q, a[0]) for p, q in zip(lin(K0, 0), lin(K1, 0)))
            Q = am.nlerp(rot(K0), rot(K1), a[1], am.lerp_rule, True, trace, counted)
            S = tuple(am.lerp_rule(p, q, a[2]) for p, q in zip(lin(K0, 2), lin(K1, 2)))
        return T, Q, S


def effective_weight(layers_l, masks, njoints, variant=None):
    """e of one layer for every instance and joint, [n, J] float32: the clamped weight times the clamped mask's weight"""
    n = layers_l.shape[0]
    w = am.clamp_w(layers_l["w"])
    M = 0 if masks is None else len(masks)
    mi = np.minimum(layers_l["mask"].astype(np.int64), M)
    m = np.ones((n, njoints), dtype=F)
    if M and variant != "mask_ignored":
        m = np.where((mi == 0)[:, None], F(1), np.asarray(masks, dtype=F).reshape(M, njoints)[np.maximum(mi, 1) - 1]).astype(F)
    return (w[:, None] * m).astype(F)


def _step(kind, T, Q, S, Tl, Ql, Sl, e, trace, counted, variant=None):
    """one layer step on number types (binary32 arrays or V): kind OVERRIDE or ADDITIVE, everywhere"""
    with np.errstate(all="ignore"):
        if kind == OVERRIDE:
            return (tuple(am.lerp_rule(p, q, e) for p, q in zip(T, Tl)), am.nlerp(Q, Ql, e, am.lerp_rule, True, trace, counted),
                    tuple(am.lerp_rule(p, q, e) for p, q in zip(S, Sl)))
        one = am._const(e, 1)
        if variant == "fused_add":
            To = tuple((p.astype(np.float64) + e.astype(np.float64) * q.astype(np.float64)).astype(F) for p, q in zip(T, Tl))
        else:
            To = tuple(p + e * q for p, q in zip(T, Tl))
        Qo = am.nlerp(Q, qmul(Ql, Q) if variant == "qmul_reversed" else qmul(Q, Ql), e, am.lerp_rule, True, trace, counted)
        if variant == "scale_product":
            So = tuple(p * q for p, q in zip(S, Sl))
        else:
            So = tuple(p * (one + e * (q - one)) for p, q in zip(S, Sl))
        return To, Qo, So


def _pick(c, a, b):
    return tuple(am._where(c, x, y) for x, y in zip(a, b))


def local_matrix(T, Q, S):
    """section 14's local matrix from (T, Q, S): [n, J, 16]"""
    x, y, z, qw = Q
    one, zero = am._const(x, 1), am._const(x, 0)
    with np.errstate(all="ignore"):
        x2, y2, z2 = x + x, y + y, z + z
        xx, yy, zz, xy, xz, yz = x * x2, y * y2, z * z2, x * y2, x * z2, y * z2
        wx, wy, wz = qw * x2, qw * y2, qw * z2
        cols = [(one - (yy + zz)) * S[0], (xy + wz) * S[0], (xz - wy) * S[0], zero,
                (xy - wz) * S[1], (one - (xx + zz)) * S[1], (yz + wx) * S[1], zero,
                (xz + wy) * S[2], (yz - wx) * S[2], (one - (xx + yy)) * S[2], zero,
                T[0], T[1], T[2], one]
    out = np.stack(cols, axis=-1)
    assert out.dtype == F
    return out


def sample_tqs(clips, layers, njoints, masks=None, variant=None, steps=None):
    """(T, Q, S) of section 16 in binary32, tuples of [n, J] arrays.  steps: a list that receives, per layer step, a dict of
    what the step started with, its e, where it was active / additive, and what it gave"""
    assert variant is None or variant in WRONG_VARIANTS
    layers = np.asarray(layers)
    n, L = layers.shape
    assert 1 <= L <= MAX_LAYERS
    src = _Source(clips, njoints)
    everywhere = np.ones((n, njoints), dtype=bool)
    T, Q, S = src.sample(layers["clip"][:, 0], layers["x"][:, 0], False, None, everywhere)
    for l in range(1, L):
        ly = layers[:, l]
        e = effective_weight(ly, masks, njoints, variant)
        active = everywhere if variant == "no_skip" else e != 0
        add = np.broadcast_to((((ly["mode"] & 1) != 0) & (variant != "mode_ignored"))[:, None], (n, njoints))
        Tl, Ql, Sl = src.sample(ly["clip"], ly["x"], False, None, active)
        over = _step(OVERRIDE, T, Q, S, Tl, Ql, Sl, e, None, active)
        addi = _step(ADDITIVE, T, Q, S, Tl, Ql, Sl, e, None, active, variant)
        new = tuple(_pick(add, a, o) for a, o in zip(addi, over))
        before = (T, Q, S)
        T, Q, S = (_pick(active, nw, old) for nw, old in zip(new, before))
        if steps is not None:
            steps.append(dict(l=l, before=before, after=(T, Q, S), e=e, active=active, add=add))
    return T, Q, S


def sample(clips, layers, njoints, masks=None, variant=None):
    """the local matrices of section 16 in binary32: [n, njoints, 16] float32"""
    return local_matrix(*sample_tqs(clips, layers, njoints, masks, variant))


def step_exact(clips, layers, njoints, masks=None):
    """The per-step bound of section 16.  Every layer step where e != 0 is carried out in float64 from the binary32 (T, Q, S)
    it starts with, the layer's clip exactly from its binary32 (i0, i1, a) / (k, k1), e as given.  Returns a list, per
    step kind met, of dicts: kind (OVERRIDE / ADDITIVE), k, frac = the largest |binary32 - exact| / (k u sum|terms|) over
    the components of (T, Q, S) of the joints kept, calls = nlerp calls counted, left_out = those with |d| < 8 u,
    min_d = the smallest |d|."""
    layers = np.asarray(layers)
    steps = []
    sample_tqs(clips, layers, njoints, masks, steps=steps)
    src = _Source(clips, njoints)
    out = {}
    for st in steps:
        ly = layers[:, st["l"]]
        for kind, where in ((OVERRIDE, st["active"] & ~st["add"]), (ADDITIVE, st["active"] & st["add"])):
            if not where.any():
                continue
            tr = am.Trace()
            tr.near = []
            Tl, Ql, Sl = src.sample(ly["clip"], ly["x"], True, tr, where)
            T0, Q0, S0 = (tuple(am.V(c) for c in part) for part in st["before"])
            ex = _step(kind, T0, Q0, S0, Tl, Ql, Sl, am.V(st["e"]), tr, where)
            near = np.logical_or.reduce(tr.near)  # [n, J]: some nlerp call of the joint's step saw |d| < 8 u
            keep = where & ~near
            k = K_STEP[(src.kind, kind)]
            frac = 0.0
            for got, want in zip(sum(st["after"], ()), sum(ex, ())):
                err = np.abs(got.astype(np.float64) - want.val)[keep]
                if err.size:
                    frac = max(frac, float((err / (k * U * want.mag[keep] + 1e-300)).max()))
            d = tr.all_d()
            o = out.setdefault(kind, dict(kind=kind, k=k, frac=0.0, calls=0, left_out=0, min_d=np.inf))
            o["frac"] = max(o["frac"], frac)
            o["calls"] += d.size
            o["left_out"] += int((np.abs(d) < 8 * U).sum())
            o["min_d"] = min(o["min_d"], float(np.abs(d).min()))
    return list(out.values())


# ---- inputs shared by the tests -----------------------------------------------------------------------------------
W_EDGES = [float("nan"), -0.2, 0.0, 1.0, 1.2]
MODES = [0, 1, 0xFFFE, 0x8001]
N_STATES = 256
N_MASKS = 3
# (the looping 120-key clip, the clamped clip) of am.CLIP_SHAPE and of tm.CLIP_SHAPE: where EDGE_X is placed
EDGE_CLIPS = {"uniform": (2, 1), "tracks": (tm.LONG, tm.CLAMP)}


def clip_lengths(clips):
    if kind_of(clips) == "tracks":
        return [int(c[0]) for c in clips]
    return [np.asarray(k).shape[0] for k, _ in clips]


def random_masks(rng, njoints, nmasks=N_MASKS):
    """masks [nmasks, njoints]: about 40 % zeros, some exact ones, the rest in (0, 1); mask 1 (the first) is zero over the
    whole first wave of 64 joints"""
    u = rng.random((nmasks, njoints))
    m = rng.uniform(0.02, 0.98, (nmasks, njoints))
    m[u < 0.40] = 0.0
    m[u > 0.85] = 1.0
    m[0, :64] = 0.0
    return m.astype(F)


def layer_states(rng, clips, n=N_STATES, L=4, nmasks=N_MASKS, dtype=LAYER):
    """[n, L] layer records: random clips (indices past the end included), positions from half a clip before its start to
    two clips after it, weights of which a fifth is 0 and some lie outside [0, 1], mask indices up to two past the end,
    every mode word of MODES; then the edges written over the first instances: section 14's edge positions on the base
    and on layer 1 of the looping and of the clamped clip, the weights of W_EDGES, and layers on mask 1 (zero over a wave)"""
    lengths = np.array(clip_lengths(clips), dtype=np.float64)
    C = len(lengths)
    ly = np.zeros((n, L), dtype=dtype)
    clip = rng.integers(0, C + 2, (n, L))
    ly["clip"] = clip
    ly["x"] = rng.uniform(-0.5, 2.0, (n, L)) * lengths[np.minimum(clip, C - 1)]
    half = rng.random((n, L)) < 0.5  # integer positions: exactly on a key / tick
    ly["x"] = np.where(half, np.floor(ly["x"]), ly["x"])
    ly["w"] = np.where(rng.random((n, L)) < 0.2, 0.0, rng.uniform(-0.2, 1.2, (n, L)))
    ly["mask"] = rng.integers(0, nmasks + 3, (n, L))
    ly["mode"] = rng.choice(MODES, (n, L))
    loop_clip, clamp_clip = EDGE_CLIPS[kind_of(clips)]
    ex = am.EDGE_X
    i = 0
    for layer, c in ((0, loop_clip), (1, loop_clip), (0, clamp_clip), (L - 1, clamp_clip)):
        if layer >= L or i + len(ex) > n:
            continue
        ly["x"][i:i + len(ex), layer] = ex
        ly["clip"][i:i + len(ex), layer] = c
        if layer:
            ly["w"][i:i + len(ex), layer] = 0.5
            ly["mask"][i:i + len(ex), layer] = 0
        i += len(ex)
    for layer in range(1, L):
        for mode in (0, 1):
            if i + len(W_EDGES) > n:
                break
            ly["w"][i:i + len(W_EDGES), layer] = W_EDGES
            ly["mode"][i:i + len(W_EDGES), layer] = mode
            i += len(W_EDGES)
    if L > 1 and i + 8 <= n:
        ly["mask"][i:i + 8, 1:] = 1
        ly["w"][i:i + 8, 1:] = rng.uniform(0.2, 1.0, (8, L - 1))
    return ly


def crossfade_layers(states, dtype=LAYER):
    """section 14's states as two-layer stacks: (clip_a, x_a) under an OVERRIDE of (clip_b, x_b) at w over mask 0"""
    st = np.asarray(states).reshape(-1)
    ly = np.zeros((st.size, 2), dtype=dtype)
    ly["clip"][:, 0], ly["x"][:, 0] = st["clip_a"], st["x_a"]
    ly["clip"][:, 1], ly["x"][:, 1], ly["w"][:, 1] = st["clip_b"], st["x_b"], st["w"]
    return ly
