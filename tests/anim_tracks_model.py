"""Numpy model of SPEC.md section 15 (animation tracks), written from that text, and the inputs its tests share.

`sample(tclips, states, njoints)` carries the rules out in binary32, one rounded numpy operation per operator, and gives
the local matrices bit for bit.  `sample_exact` carries them out in float64 from the binary32 `r`, the binary32 choice of
`(k, k1)` per track, the clamped `w` and the integer key words (`a` and the decodes exactly), and propagates the sum of the
terms on absolute values that the accuracy bound of section 15 is stated against.  lerp, nlerp, `V` and `Trace` are section
14's (tests/anim_model.py).

A track clip is a tuple (nticks, flags, tracks, times, values): tracks a TRACK array [njoints, 3] whose `first` counts
inside the clip's own `times` (u16 [nkeys]) and `values` (u16 [nkeys, 4]); states: an array with the fields of
api.ANIM_STATE.  `variant` names one deliberately wrong reading of the section (WRONG_VARIANTS), for the tests that show
the inputs would tell it apart."""
import numpy as np

from tests import anim_model as am

F = np.float32
U = am.U
CLIP_LOOP = 1
K_LOCALS = 26  # rounded operations on the longest path of a local matrix element (section 15)
TRACK = np.dtype([("first", "<u4"), ("count", "<u4"), ("lo", "<f4", 3), ("step", "<f4", 3)])
STATE = np.dtype([("clip_a", "<u4"), ("clip_b", "<u4"), ("x_a", "<f4"), ("x_b", "<f4"), ("w", "<f4"), ("pad", "<u4")])
WRONG_VARIANTS = ("search_lt", "fused_decode", "t1_16bit", "a_without_subtraction")
PAD = 128  # tracks of at most this many keys are searched together


def position_r(x, nticks, loop):
    """section 15 "Position": section 14's r from x, N = the clip's ticks and its flag; float32 [n]"""
    x = np.asarray(x, dtype=F)
    nticks = np.asarray(nticks, dtype=np.int64)
    nf = nticks.astype(F)
    with np.errstate(all="ignore"):
        r_loop = x - np.floor(x / nf) * nf
        r_loop = np.where((r_loop >= F(0)) & (r_loop < nf), r_loop, F(0))
        r_clamp = np.where(x >= F(0), x, F(0))
        last = (nticks - 1).astype(F)
        r_clamp = np.where(r_clamp > last, last, r_clamp)
    return np.where(loop, r_loop, r_clamp).astype(F)


def concat(tclips, njoints):
    """the arrays of mtr_anim_create_tracks: nticks, flags, tracks [C, njoints, 3] with `first` rebased, times, values"""
    nticks = np.array([int(c[0]) for c in tclips], dtype=np.int64)
    flags = np.array([int(c[1]) for c in tclips], dtype=np.int64)
    tracks, times, values, base = [], [], [], 0
    for _, _, tr, tm, va in tclips:
        tr = np.array(tr, dtype=TRACK).reshape(njoints, 3)
        tr["first"] = np.minimum(tr["first"].astype(np.uint64) + np.uint64(base), np.uint64(0xFFFFFFFF))  # no wrap: an invalid first stays invalid
        base += len(tm)
        tracks.append(tr)
        times.append(np.asarray(tm, dtype=np.uint16).reshape(-1))
        values.append(np.asarray(va, dtype=np.uint16).reshape(-1, 4))
    return nticks, flags, np.stack(tracks), np.concatenate(times), np.concatenate(values)


def _largest_le(tf, first, count, r, strict):
    """per track (first, count: [m]) and position (r: [s]): the largest key index with float(time) <= r -> [s, m]"""
    out = np.zeros((r.size, first.size), dtype=np.int64)
    small = count <= PAD
    if small.any():
        f, c = first[small], count[small]
        col = np.arange(PAD)
        idx = np.minimum(f[:, None] + col[None, :], tf.size - 1)
        tp = np.where(col[None, :] < c[:, None], tf[idx], F(np.inf))  # [m, PAD]
        le = (tp[None, :, :] < r[:, None, None]) if strict else (tp[None, :, :] <= r[:, None, None])
        out[:, small] = f[None, :] + np.maximum(le.sum(axis=2) - 1, 0)
    for i in np.nonzero(~small)[0]:
        t = tf[first[i]:first[i] + count[i]]
        le = (t[None, :] < r[:, None]) if strict else (t[None, :] <= r[:, None])
        out[:, i] = first[i] + np.maximum(le.sum(axis=1) - 1, 0)
    return out


def locate(times, first, count, r, nticks, loop, variant=None):
    """section 15 "Per track" for tracks (first, count: [m]) of ONE clip at positions r [s]: k, k1 (int64 [s, m]), a in
    binary32 and a carried out exactly (float64), both [s, m]"""
    tf = times.astype(F)
    first = np.asarray(first, dtype=np.int64)
    count = np.asarray(count, dtype=np.int64)
    k = _largest_le(tf, first, count, r, variant == "search_lt")
    last = k == (first + count - 1)[None, :]
    k1 = np.where(~last, np.minimum(k + 1, times.size - 1), np.where(loop, first[None, :], k))
    tk = times[k].astype(np.int64)
    t1 = np.where(~last, times[k1].astype(np.int64), np.int64(nticks))  # N can be 65536: wider than 16 bits
    if variant == "t1_16bit":
        t1 = t1 & 0xFFFF
    same = k1 == k
    dt = np.where(same, 1, t1 - tk)
    rr = np.broadcast_to(r[:, None], k.shape)
    with np.errstate(all="ignore"):
        if variant == "a_without_subtraction":
            num = rr
            den = np.where(same, 1, t1).astype(F)
        else:
            num = rr - tk.astype(F)
            den = dt.astype(F)
        a = np.where(same, F(0), num / den).astype(F)
        a_exact = np.where(same, 0.0, (rr.astype(np.float64) - tk) / dt)
    return k, k1, a, a_exact


def decode_lin(words, lo, step, fused=False):
    """translation / scale keys: lo + float(v) * step, product then sum; words u16 [..., 4], lo / step [..., 3]"""
    v = words[..., :3].astype(F)
    if fused:
        return (lo.astype(np.float64) + v.astype(np.float64) * step.astype(np.float64)).astype(F)
    with np.errstate(all="ignore"):
        return (lo + v * step).astype(F)


def decode_rot(words):
    """rotation keys: section 2's Snorm16 of the four words (x, y, z, w)"""
    v = np.ascontiguousarray(words).view(np.int16).astype(F)
    return np.maximum(v / F(32767), F(-1)).astype(F)


def _locate_states(arrays, clip, x, J, variant=None):
    """per state, joint and channel: the clamped clip c [n], r [n], and k, k1 (indices into the concatenated arrays), a in
    binary32 and a exactly, each [n, J, 3]"""
    nticks, flags, tracks, times, _ = arrays
    n = len(x)
    c = np.minimum(np.asarray(clip, dtype=np.int64), len(nticks) - 1)
    loop = (flags[c] & CLIP_LOOP) != 0
    r = position_r(x, nticks[c], loop)
    K0 = np.zeros((n, J * 3), dtype=np.int64)
    K1 = np.zeros((n, J * 3), dtype=np.int64)
    A = np.zeros((n, J * 3), dtype=F)
    AX = np.zeros((n, J * 3), dtype=np.float64)
    for ci in np.unique(c):
        sel = np.nonzero(c == ci)[0]
        tr = tracks[ci].reshape(-1)
        K0[sel], K1[sel], A[sel], AX[sel] = locate(times, tr["first"], tr["count"], r[sel], nticks[ci], bool(flags[ci] & CLIP_LOOP), variant)
    return (c, r) + tuple(z.reshape(n, J, 3) for z in (K0, K1, A, AX))


def located(tclips, clip, x, njoints):
    """what section 15 determines before the interpolation, for the CPU harness of csrc/anim_tracks.h: r [n]; k, k1, a
    [n, J, 3]; the decoded keys k and k1 [n, J, 3, 4] (the fourth component of a translation / scale key is 0)"""
    arrays = concat(tclips, njoints)
    _, _, tracks, _, values = arrays
    c, r, K0, K1, A, _ = _locate_states(arrays, np.asarray(clip), np.asarray(x, dtype=F), njoints)
    lo, step = tracks["lo"][c], tracks["step"][c]
    dec = []
    for K in (K0, K1):
        d = np.zeros(K.shape + (4,), dtype=F)
        for ch in (0, 2):
            d[:, :, ch, :3] = decode_lin(values[K[..., ch]], lo[:, :, ch], step[:, :, ch])
        d[:, :, 1, :] = decode_rot(values[K[..., 1]])
        dec.append(d)
    return r, K0, K1, A, dec[0], dec[1]


def _sample(tclips, states, njoints, exact, lerp, flip, trace, variant):
    J = njoints
    arrays = concat(tclips, J)
    nticks, flags, tracks, times, values = arrays
    n = states.shape[0]
    w = am.clamp_w(states["w"])
    fade = np.broadcast_to((w != 0)[:, None], (n, J))
    everywhere = np.ones((n, J), dtype=bool)
    if trace is not None:
        trace.near = []

    def num(val, mag=None):  # the arithmetic's number type
        if exact:
            return am.V(val, mag)
        return np.ascontiguousarray(val, dtype=F)

    def one_clip(clip, x, counted):
        c, _, K0, K1, A, AX = _locate_states(arrays, clip, x, J, variant)
        lo, step = tracks["lo"][c], tracks["step"][c]  # [n, J, 3, 3]

        def lin(K, ch):
            wd = values[K[..., ch]]
            if exact:
                v = wd[..., :3].astype(np.float64)
                l, s = lo[:, :, ch].astype(np.float64), step[:, :, ch].astype(np.float64)
                return tuple(num(l[..., i] + v[..., i] * s[..., i], np.abs(l[..., i]) + v[..., i] * np.abs(s[..., i])) for i in range(3))
            d = decode_lin(wd, lo[:, :, ch], step[:, :, ch], fused=variant == "fused_decode")
            return tuple(num(d[..., i]) for i in range(3))

        def rot(K):
            wd = values[K[..., 1]]
            if exact:
                q = np.maximum(np.ascontiguousarray(wd).view(np.int16).astype(np.float64) / 32767.0, -1.0)
            else:
                q = decode_rot(wd)
            return tuple(num(q[..., i]) for i in range(4))

        a = [num(AX[..., ch]) if exact else num(A[..., ch]) for ch in range(3)]
        with np.errstate(all="ignore"):
            T = tuple(lerp(p, q, a[0]) for p, q in zip(lin(K0, 0), lin(K1, 0)))
            Q = am.nlerp(rot(K0), rot(K1), a[1], lerp, flip, trace, counted)
            S = tuple(lerp(p, q, a[2]) for p, q in zip(lin(K0, 2), lin(K1, 2)))
        return T, Q, S

    Ta, Qa, Sa = one_clip(states["clip_a"], states["x_a"], everywhere)
    Tb, Qb, Sb = one_clip(states["clip_b"], states["x_b"], fade)  # where w == 0 the result is discarded below
    wv = num(np.broadcast_to(w[:, None], (n, J)))
    with np.errstate(all="ignore"):
        Tf = tuple(lerp(p, q, wv) for p, q in zip(Ta, Tb))
        Qf = am.nlerp(Qa, Qb, wv, lerp, flip, trace, fade)
        Sf = tuple(lerp(p, q, wv) for p, q in zip(Sa, Sb))
    T = tuple(am._where(fade, f, p) for f, p in zip(Tf, Ta))
    Q = tuple(am._where(fade, f, p) for f, p in zip(Qf, Qa))
    S = tuple(am._where(fade, f, p) for f, p in zip(Sf, Sa))
    # the local matrix of section 14
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
    if trace is not None:
        trace.near = np.logical_or.reduce(trace.near)
    if exact:
        return np.stack([c.val for c in cols], axis=-1), np.stack([c.mag for c in cols], axis=-1)
    out = np.stack(cols, axis=-1)
    assert out.dtype == F
    return out


def sample(tclips, states, njoints, lerp=am.lerp_rule, flip=True, trace=None, variant=None):
    """the local matrices of section 15 in binary32: [n, njoints, 16] float32"""
    assert variant is None or variant in WRONG_VARIANTS
    return _sample(tclips, np.asarray(states).reshape(-1), njoints, False, lerp, flip, trace, variant)


def sample_exact(tclips, states, njoints, trace=None):
    """the same rules in float64: values and sums of |terms|, each [n, njoints, 16]"""
    return _sample(tclips, np.asarray(states).reshape(-1), njoints, True, am.lerp_rule, True, trace, None)


def validate(tclips, njoints):
    """the creation rules of section 15 "Data": None, or (clip, joint, channel, what) of the first violation"""
    nticks, _, tracks, times, _ = concat(tclips, njoints)
    for c, N in enumerate(nticks):
        if not 1 <= N <= 65536:
            return (c, None, None, "ticks")
        for j in range(njoints):
            for ch in range(3):
                f, n = int(tracks[c, j, ch]["first"]), int(tracks[c, j, ch]["count"])
                if n < 1:
                    return (c, j, ch, "count")
                if f + n > times.size:
                    return (c, j, ch, "range")
                t = times[f:f + n].astype(np.int64)
                if t[0] != 0:
                    return (c, j, ch, "first time")
                if t[-1] > N - 1:
                    return (c, j, ch, "last time")
                if (np.diff(t) <= 0).any():
                    return (c, j, ch, "increase")
    return None


# ---- inputs shared by the tests -----------------------------------------------------------------------------------
JOINT_COUNTS = {"chain64": 64, "multi_root": 40, "j256": 256, "one": 1}
CLIP_SHAPE = [(120, CLIP_LOOP), (120, 0), (65536, CLIP_LOOP), (1, 0)]  # ticks, flags
KEY_COUNTS = [1, 2, 3, 63, 64, 65, 120]
LONG, CLAMP, HUGE, ONE = 0, 1, 2, 3
N_STATES = 256


def _track_times(rng, count, nticks):
    """a random strictly increasing subset of the ticks, starting at 0"""
    count = min(count, nticks)
    if count == 1:
        return np.zeros(1, dtype=np.uint16)
    rest = np.sort(rng.choice(np.arange(1, nticks), size=count - 1, replace=False))
    return np.concatenate([[0], rest]).astype(np.uint16)


def special_tracks(njoints):
    """in the 65536-tick clip: (joint, channel) of the track with all 65536 keys (the deepest search) and of the one with 2
    keys (the widest interval, t1 = 65536 on the wrap).  Rotations of two joints; one joint alone has them on two channels."""
    return ((njoints - 1, 1) if njoints > 1 else (0, 0)), (0, 1)


def random_track_clips(rng, njoints, shape=CLIP_SHAPE, noise=0.6, flip_p=0.3, trans=10.0, scale=(0.8, 1.25)):
    """track clips whose neighbouring rotation keys are related (a base quaternion per joint plus noise, normalised, 30 % of
    them with the opposite sign); key counts from KEY_COUNTS, key times random subsets of the ticks"""
    deep, wide = special_tracks(njoints)
    clips = []
    for ci, (nticks, fl) in enumerate(shape):
        tracks = np.zeros((njoints, 3), dtype=TRACK)
        times, values, base = [], [], 0
        for j in range(njoints):
            qbase = rng.standard_normal(4)
            for ch in range(3):
                count = int(rng.choice(KEY_COUNTS))
                if ci == HUGE and (j, ch) == deep:
                    count = 65536
                if ci == HUGE and (j, ch) == wide:
                    count = 2
                if ci == HUGE and (j, ch) == wide:
                    t = np.array([0, int(rng.integers(1000, 30000))], dtype=np.uint16)
                elif count == nticks:
                    t = np.arange(nticks).astype(np.uint16)
                else:
                    t = _track_times(rng, count, nticks)
                count = t.size
                v = np.zeros((count, 4), dtype=np.uint16)
                if ch == 1:
                    q = qbase[None, :] + noise * rng.standard_normal((count, 4))
                    q /= np.linalg.norm(q, axis=-1, keepdims=True)
                    q *= np.where(rng.random((count, 1)) < flip_p, -1.0, 1.0)
                    v[:] = np.rint(q * 32767).astype(np.int16).view(np.uint16)
                else:
                    v[:, :3] = rng.integers(0, 65536, (count, 3))
                    v[:, 3] = rng.integers(0, 65536, count)  # never read
                    # translations span zero, so that neighbouring keys lie in different binades and a lerp's roundings show
                    a = np.stack([rng.uniform(-trans, -trans / 2, 3), rng.uniform(trans / 2, trans, 3)]) if ch == 0 else rng.uniform(*scale, (2, 3))
                    tracks[j, ch]["lo"] = a.min(axis=0)
                    tracks[j, ch]["step"] = (a.max(axis=0) - a.min(axis=0)) / 65535
                tracks[j, ch]["first"] = base
                tracks[j, ch]["count"] = count
                base += count
                times.append(t)
                values.append(v)
        clips.append((nticks, fl, tracks, np.concatenate(times), np.concatenate(values)))
    return clips


def _below(v):
    return np.nextafter(F(v), F(-np.inf))


def _above(v):
    return np.nextafter(F(v), F(np.inf))


def track_states(rng, tclips, njoints, n=N_STATES, dtype=STATE):
    """256 states: section 14's edge positions; every kind of r relative to a track (on a key time, its binary32
    neighbours, inside the first, the last and the LOOP wrap interval, past the end of the clamp clip); integer and
    fractional positions on every clip, cross-fades between the long and the short clips, clip indices beyond C - 1"""
    st = np.zeros(n, dtype=dtype)
    C = len(tclips)
    # random part first, then the edges written over it
    clip = rng.choice([LONG, CLAMP, HUGE, HUGE, ONE, C, C + 3], size=(2, n), p=[0.22, 0.2, 0.2, 0.2, 0.08, 0.05, 0.05])
    for f, row in (("a", 0), ("b", 1)):
        c = clip[row]
        N = np.array([tclips[min(int(k), C - 1)][0] for k in c], dtype=np.float64)
        x = rng.uniform(-0.5, 2.0, n) * N
        for i in np.nonzero(rng.random(n) < 0.7)[0]:  # exactly on a key time of some track of the clip (not its first key,
            nt, fl, tr, tm, _ = tclips[min(int(c[i]), C - 1)]  # where every reading agrees), on any lap of a LOOP clip
            t = tr.reshape(-1)[int(rng.integers(njoints * 3))]
            key = int(t["first"]) + int(rng.integers(1, t["count"])) if t["count"] > 1 else int(t["first"])
            x[i] = float(tm[key]) + (nt * int(rng.integers(0, 2)) if fl & CLIP_LOOP else 0)
        st["clip_" + f] = c
        st["x_" + f] = x
    st["w"] = np.where(rng.random(n) < 0.25, 0.0, rng.uniform(-0.2, 1.2, n))
    e = len(am.EDGE_X)
    for k, (field, clip_field, ci) in enumerate((("x_a", "clip_a", LONG), ("x_b", "clip_b", LONG), ("x_a", "clip_a", CLAMP))):
        st[field][k * e:(k + 1) * e] = am.EDGE_X
        st[clip_field][k * e:(k + 1) * e] = ci
        if field == "x_b":
            st["w"][k * e:(k + 1) * e] = 0.5
    i = 3 * e
    deep, wide = special_tracks(njoints)
    for ci, (j, ch) in ((LONG, (0, 1)), (CLAMP, (njoints - 1, 0)), (HUGE, wide), (HUGE, deep), (LONG, (njoints // 2, 2))):
        N, fl, tr, tm, _ = tclips[ci]
        f, cnt = int(tr[j, ch]["first"]), int(tr[j, ch]["count"])
        t = tm[f:f + cnt].astype(np.float64)
        mid = t[cnt // 2]
        xs = [mid, _below(mid), _above(mid), t[-1], _below(t[-1]), _above(t[-1]),
              (t[0] + t[min(1, cnt - 1)]) / 2 + 0.25,         # inside the first interval
              (t[max(cnt - 2, 0)] + t[-1]) / 2 + 0.125,       # inside the last interval
              (t[-1] + N) / 2 + 0.375, _below(N), N + mid,   # the LOOP wrap interval (or past the end of a clamp clip)
              N + 10.5, 3.0 * N + 0.5]
        for x in xs:
            for as_b in (False, True):
                if i >= n:
                    break
                if as_b:  # a cross-fade between a long and a short clip
                    st[i] = (ONE if ci != ONE else LONG, ci, 0.0, x, 0.5, 0)
                else:
                    st[i] = (ci, CLAMP, x, 7.25, 0.0 if rng.random() < 0.5 else 0.3, 0)
                i += 1
    assert i <= n
    return st


def invalid_sets(tclips, njoints):
    """every creation violation of section 15 "Data", one at a time on an otherwise valid set:
    [(what, clips, clip, joint or None, channel or None)]; the violations of a track are made on one with at least 3 keys"""
    def copy():
        return [(nt, fl, tr.copy(), tm.copy(), va.copy()) for nt, fl, tr, tm, va in tclips]

    ci = CLAMP
    tr = tclips[ci][2]
    j, ch = [(j, ch) for j in range(njoints) for ch in range(3) if tr[j, ch]["count"] >= 3][0]
    f, cnt = int(tr[j, ch]["first"]), int(tr[j, ch]["count"])
    out = []
    for what, N in (("no ticks", 0), ("too many ticks", 65537)):
        s = copy()
        s[ONE] = (N,) + s[ONE][1:]
        out.append((what, s, ONE, None, None))
    s = copy()
    s[ci][2][j, ch]["count"] = 0
    out.append(("count 0", s, ci, j, ch))
    s = copy()
    last = len(s) - 1
    s[last][2][njoints - 1, 2]["first"] = len(s[last][3])  # the last clip's last track: one past the end of all keys
    out.append(("first + count past the keys", s, last, njoints - 1, 2))
    s = copy()
    s[last][2][njoints - 1, 2]["first"] = 0xFFFFFFFF  # first + count wraps in 32 bits
    out.append(("first + count wraps", s, last, njoints - 1, 2))
    s = copy()
    s[ci][3][f] = 1
    out.append(("first time not 0", s, ci, j, ch))
    s = copy()
    s[ci][3][f + cnt - 1] = s[ci][3][f + cnt - 2]
    out.append(("times equal", s, ci, j, ch))
    s = copy()
    s[ci][3][f + 1] = s[ci][3][f + 2] + 1 if cnt > 3 else s[ci][3][f + 2]
    out.append(("times not increasing", s, ci, j, ch))
    s = copy()
    s[ci][3][f + cnt - 1] = s[ci][0]
    out.append(("last time at N", s, ci, j, ch))
    return out
