"""Numpy model of SPEC.md section 14 (animation clips), written from that text.

`sample(clips, states)` carries the rules out in binary32, one rounded numpy operation per operator (numpy never fuses,
and its float32 `/` and `sqrt` are correctly rounded), so it gives the local matrices bit for bit.  `sample_exact` carries
the same rules out in float64 from the binary32 `(i0, i1, a)` and clamped `w`, and propagates with every value the sum of
its terms on absolute values, which is what the accuracy bound of section 14 is stated against.

clips: a list of (keys [nkeys, njoints, 12] float32, flags); states: an array of api.ANIM_STATE (or any structured array
with its fields)."""
import numpy as np

F = np.float32
U = 2.0 ** -24
CLIP_LOOP = 1
K_LOCALS = 24  # rounded operations on the longest path of a local matrix element (section 14)


def position(x, nkeys, loop):
    """section 14 "Position -> keys": x float32 [n], nkeys int [n], loop bool [n] -> i0, i1 (int64) and a (float32)"""
    x = np.asarray(x, dtype=F)
    nkeys = np.asarray(nkeys, dtype=np.int64)
    nf = nkeys.astype(F)
    with np.errstate(all="ignore"):
        r_loop = x - np.floor(x / nf) * nf
        r_loop = np.where((r_loop >= F(0)) & (r_loop < nf), r_loop, F(0))
        r_clamp = np.where(x >= F(0), x, F(0))
        last = (nkeys - 1).astype(F)
        r_clamp = np.where(r_clamp > last, last, r_clamp)
    r = np.where(loop, r_loop, r_clamp).astype(F)
    i0 = np.floor(r).astype(np.int64)
    i1 = np.where(loop, np.where(i0 + 1 == nkeys, 0, i0 + 1), np.minimum(i0 + 1, nkeys - 1))
    a = r - i0.astype(F)
    assert a.dtype == F and ((i0 >= 0) & (i0 < nkeys) & (i1 >= 0) & (i1 < nkeys)).all()
    return i0, i1, a


def clamp_w(w):
    w = np.asarray(w, dtype=F)
    w = np.where(w > F(0), w, F(0))  # NaN -> 0
    return np.where(w > F(1), F(1), w).astype(F)


class V:
    """a float64 value together with the sum of its terms on absolute values (mag >= |val|)"""

    def __init__(self, val, mag=None):
        self.val = np.asarray(val, dtype=np.float64)
        self.mag = np.abs(self.val) if mag is None else np.asarray(mag, dtype=np.float64)

    def __add__(self, o):
        return V(self.val + o.val, self.mag + o.mag)

    def __sub__(self, o):
        return V(self.val - o.val, self.mag + o.mag)

    def __mul__(self, o):
        return V(self.val * o.val, self.mag * o.mag)

    def __neg__(self):
        return V(-self.val, self.mag)


def _val(v):
    return v.val if isinstance(v, V) else v


def _where(c, a, b):
    if isinstance(a, V):
        return V(np.where(c, a.val, b.val), np.where(c, a.mag, b.mag))
    return np.where(c, a, b)


def _const(like, c):
    if isinstance(like, V):
        return V(np.full(like.val.shape, float(c)))
    return np.full(like.shape, c, dtype=F)


def _rsqrt(n2):
    with np.errstate(all="ignore"):
        if isinstance(n2, V):
            # a relative error e of n2 becomes e / 2 of n2 ** -1/2; n2's own is bounded relative to mag, not to val
            val = 1.0 / np.sqrt(n2.val)
            return V(val, np.abs(val) * np.where(n2.val != 0, n2.mag / n2.val, 1.0))
        return F(1) / np.sqrt(n2)


def lerp_rule(v0, v1, a):
    return v0 + a * (v1 - v0)


def lerp_fused(v0, v1, a):
    """what a contracting compiler makes of it: the product and the sum in one rounding (binary32 only)"""
    return (v0.astype(np.float64) + a.astype(np.float64) * (v1 - v0).astype(np.float64)).astype(F)


def dot(p, q):
    return ((p[0] * q[0] + p[1] * q[1]) + p[2] * q[2]) + p[3] * q[3]


class Trace:
    """what the nlerp calls of one sample() saw: d of every call that counts (clip B's and the cross-fade's only where w != 0)"""

    def __init__(self):
        self.d = []

    def all_d(self):
        return np.concatenate([x.reshape(-1) for x in self.d])


def nlerp(q0, q1, a, lerp, flip, trace, counted):
    d = dot(q0, q1)
    neg = _val(d) < 0
    if trace is not None:
        trace.d.append(np.asarray(_val(d), dtype=np.float64)[counted])
        trace.near.append((np.abs(np.asarray(_val(d), dtype=np.float64)) < 8 * U) & counted)
    if flip:
        q1 = tuple(_where(neg, -c, c) for c in q1)
    q = tuple(lerp(c0, c1, a) for c0, c1 in zip(q0, q1))
    n2 = dot(q, q)
    rn = _rsqrt(n2)
    with np.errstate(all="ignore"):
        out = tuple(c * rn for c in q)
    bad = (_val(n2) == 0) | ~np.isfinite(_val(rn))
    ident = (0.0, 0.0, 0.0, 1.0)
    return tuple(_where(bad, _const(c, i), c) for c, i in zip(out, ident))


def _clip_tables(clips, njoints):
    nkeys = np.array([np.asarray(k).reshape(-1, njoints, 12).shape[0] for k, _ in clips], dtype=np.int64)
    flags = np.array([int(f) for _, f in clips], dtype=np.int64)
    first = np.concatenate([[0], np.cumsum(nkeys)[:-1]])
    keys = np.concatenate([np.asarray(k, dtype=F).reshape(-1, njoints, 12) for k, _ in clips])
    return nkeys, flags, first, keys


def _sample(clips, states, njoints, exact, lerp, flip, trace):
    nkeys, flags, first, keys = _clip_tables(clips, njoints)
    n = states.shape[0]
    w = clamp_w(states["w"])
    fade = np.broadcast_to((w != 0)[:, None], (n, njoints))
    everywhere = np.ones((n, njoints), dtype=bool)
    if trace is not None:
        trace.near = []

    def wrap(arr):  # [n, njoints] float32 -> the arithmetic's number type
        return V(arr) if exact else np.ascontiguousarray(arr, dtype=F)

    def one_clip(clip, x, counted):
        c = np.minimum(np.asarray(clip, dtype=np.int64), len(clips) - 1)
        i0, i1, a = position(x, nkeys[c], (flags[c] & CLIP_LOOP) != 0)
        k0, k1 = keys[first[c] + i0], keys[first[c] + i1]  # [n, njoints, 12]
        av = wrap(np.broadcast_to(a[:, None], (n, njoints)))
        T = tuple(lerp(wrap(k0[..., i]), wrap(k1[..., i]), av) for i in (0, 1, 2))
        Q = nlerp(tuple(wrap(k0[..., i]) for i in (4, 5, 6, 7)), tuple(wrap(k1[..., i]) for i in (4, 5, 6, 7)), av, lerp, flip, trace, counted)
        S = tuple(lerp(wrap(k0[..., i]), wrap(k1[..., i]), av) for i in (8, 9, 10))
        return T, Q, S

    Ta, Qa, Sa = one_clip(states["clip_a"], states["x_a"], everywhere)
    Tb, Qb, Sb = one_clip(states["clip_b"], states["x_b"], fade)  # where w == 0 the result is discarded below
    wv = wrap(np.broadcast_to(w[:, None], (n, njoints)))
    with np.errstate(all="ignore"):
        Tf = tuple(lerp(p, q, wv) for p, q in zip(Ta, Tb))
        Qf = nlerp(Qa, Qb, wv, lerp, flip, trace, fade)
        Sf = tuple(lerp(p, q, wv) for p, q in zip(Sa, Sb))
    T = tuple(_where(fade, f, p) for f, p in zip(Tf, Ta))
    Q = tuple(_where(fade, f, p) for f, p in zip(Qf, Qa))
    S = tuple(_where(fade, f, p) for f, p in zip(Sf, Sa))
    x, y, z, qw = Q
    one, zero = _const(x, 1), _const(x, 0)
    with np.errstate(all="ignore"):
        x2, y2, z2 = x + x, y + y, z + z
        xx, yy, zz, xy, xz, yz = x * x2, y * y2, z * z2, x * y2, x * z2, y * z2
        wx, wy, wz = qw * x2, qw * y2, qw * z2
        cols = [(one - (yy + zz)) * S[0], (xy + wz) * S[0], (xz - wy) * S[0], zero,
                (xy - wz) * S[1], (one - (xx + zz)) * S[1], (yz + wx) * S[1], zero,
                (xz + wy) * S[2], (yz - wx) * S[2], (one - (xx + yy)) * S[2], zero,
                T[0], T[1], T[2], one]
    if trace is not None:
        trace.near = np.logical_or.reduce(trace.near)  # [n, njoints]: some nlerp call of that joint saw |d| < 8 u
    if exact:
        return np.stack([c.val for c in cols], axis=-1), np.stack([c.mag for c in cols], axis=-1)
    out = np.stack(cols, axis=-1)
    assert out.dtype == F
    return out


def sample(clips, states, njoints, lerp=lerp_rule, flip=True, trace=None):
    """the local matrices of section 14 in binary32: [n, njoints, 16] float32"""
    return _sample(clips, np.asarray(states).reshape(-1), njoints, False, lerp, flip, trace)


def sample_exact(clips, states, njoints, trace=None):
    """the same rules in float64 from the binary32 (i0, i1, a) and w: values and sums of |terms|, each [n, njoints, 16]"""
    return _sample(clips, np.asarray(states).reshape(-1), njoints, True, lerp_rule, True, trace)


def palettes(mf, local_mats):
    """section 12 over the model's local matrices, through the host function (files.ModelFile.palette = mtr_rmodel_palette)"""
    return np.stack([mf.palette(p) for p in local_mats]).astype(F)


# ---- inputs shared by the tests -----------------------------------------------------------------------------------
EDGE_X = [0.0, -0.0, 1e-30, 119.99999, 120.0, -1e-7, float("nan"), float("inf")]
CLIP_SHAPE = [(2, CLIP_LOOP), (31, 0), (120, CLIP_LOOP), (1, 0)]


def random_clips(rng, njoints, shape=CLIP_SHAPE, noise=0.6, flip_p=0.3, trans=10.0, scale=(0.8, 1.25)):
    """clips whose neighbouring keys are related (a base quaternion per joint plus noise, normalised), 30 % of the key
    quaternions with the opposite sign"""
    clips = []
    for nk, fl in shape:
        base = rng.standard_normal((1, njoints, 4))
        q = base + noise * rng.standard_normal((nk, njoints, 4))
        q /= np.linalg.norm(q, axis=-1, keepdims=True)
        q *= np.where(rng.random((nk, njoints, 1)) < flip_p, -1.0, 1.0)
        k = np.zeros((nk, njoints, 12), dtype=F)
        k[..., 0:3] = rng.uniform(-trans, trans, (nk, njoints, 3))
        k[..., 4:8] = q
        k[..., 8:11] = rng.uniform(scale[0], scale[1], (nk, njoints, 3))
        clips.append((k, fl))
    return clips


def random_states(rng, n, dtype, nclips=4, span=300.0):
    st = np.zeros(n, dtype=dtype)
    st["clip_a"] = rng.integers(0, nclips, n)
    st["clip_b"] = rng.integers(0, nclips, n)
    st["x_a"] = rng.uniform(-span, span, n)
    st["x_b"] = rng.uniform(-span, span, n)
    st["w"] = np.where(rng.random(n) < 0.25, 0.0, rng.uniform(-0.2, 1.2, n))
    # the edge positions: on the 120-key loop as clip A, as clip B of a cross-fade, and on the 31-key clamped clip
    e = len(EDGE_X)
    for k, (field, clip_field, clip) in enumerate((("x_a", "clip_a", 2), ("x_b", "clip_b", 2), ("x_a", "clip_a", 1))):
        m = max(0, min(e, n - k * e))
        st[field][k * e:k * e + m] = EDGE_X[:m]
        st[clip_field][k * e:k * e + m] = clip
        if field == "x_b":
            st["w"][k * e:k * e + m] = 0.5
    return st


def gentle_clips(rng, njoints, shape=CLIP_SHAPE, angle=0.08, trans=0.03, scale=(0.99, 1.01)):
    """clips that keep a skinned mesh in view: rotations about z within +-angle, small translations, scale near 1"""
    clips = []
    for nk, fl in shape:
        a = rng.uniform(-angle, angle, (nk, njoints))
        k = np.zeros((nk, njoints, 12), dtype=F)
        k[..., 0:3] = rng.uniform(-trans, trans, (nk, njoints, 3))
        k[..., 6] = np.sin(a / 2)
        k[..., 7] = np.cos(a / 2)
        k[..., 4:8] *= np.where(rng.random((nk, njoints, 1)) < 0.3, -1.0, 1.0)
        k[..., 8:11] = rng.uniform(scale[0], scale[1], (nk, njoints, 3))
        clips.append((k, fl))
    return clips
