"""Root motion (SPEC.md section 19) in numpy, written from the section: per instance the blended rigid delta of S steps on the
trajectory joint of an animation set of either kind, its matrix D and M . D -- in binary32 (what k_root and csrc/root_math.h
must equal bit for bit), in float64 (what the section's properties and accuracy statement are measured against), and on
am.V values that carry the sum of the terms on absolute values (the bound) -- the generator of the cases every root-motion
test runs, and nine deliberately wrong readings of the section (WRONG_VARIANTS).

A value is a tuple of components, each an array [m] of one dtype or an am.V, as in tests/anim_layers_model.py.  A trajectory set is
a list of clips as tests/anim_model.py (keys [N, J, 12], flags) or tests/anim_tracks_model.py (ticks, flags, tracks, times,
values) make them; a root set is (joint, flags [C])."""
import numpy as np

from tests import anim_model as am
from tests import anim_tracks_model as tm
from tests.anim_ik_model import fma32
from tests.anim_layers_model import kind_of, qmul

F = np.float32
U = am.U
STEP = np.dtype([("clip", "<u4"), ("x", "<f4"), ("dx", "<f4"), ("w", "<f4")])
MAX_STEPS = 8
CYCLIC = 1
DIRECT, SEAM, IDENTITY = 0, 1, 2
WRONG_VARIANTS = ("t_unrotated", "qmul_reversed", "d_left", "seam_ignored", "period_n", "seam_swapped", "no_skip", "fused_compose", "norm_per_seam")


def k_ops(kind, S):
    """the rounded operations on the longest path of an element of D (section 19, "Accuracy"): a rotation element of a seam
    step, blended S - 1 times"""
    return (31 if kind == "tracks" else 29) + 10 * (S - 1)


# ---- positions of a step ------------------------------------------------------------------------------------------------
def clamp_pos(x, L):
    """section 14's clamp of x to [0, L]: NaN -> 0, -0 stays"""
    r = np.where(x >= 0, x, x.dtype.type(0))
    return np.where(r > L, L, r)


def positions(x, dx, N, cyc, dt=F, variant=None):
    """x, dx [m] (binary32 values), N int [m], cyc bool [m] -> r [m, 4] (r0, the first seam delta's end, the second's start,
    r1) and kind [m] (DIRECT, SEAM, IDENTITY), in dt"""
    x, dx = np.asarray(x).astype(dt), np.asarray(dx).astype(dt)
    L = (N - 1).astype(dt)
    P = N.astype(dt) if variant == "period_n" else L
    zero = np.zeros_like(x)
    with np.errstate(all="ignore"):
        # non-cyclic
        n0 = clamp_pos(x, L)
        n1 = clamp_pos(x + dx, L)
        # cyclic, N > 1
        Ps = np.where(P == 0, dt(1), P)
        r0 = x - np.floor(x / Ps) * Ps
        r0 = np.where((r0 >= 0) & (r0 < Ps), r0, zero)
        y = r0 + dx
        neg, over = y < 0, y >= Ps
        r1 = np.where(neg, y + Ps, np.where(over, y - Ps, y))
        ok = (r1 >= 0) & (r1 <= Ps)
    seam = neg | over
    kind = np.where(cyc, np.where((N == 1) | ~ok, IDENTITY, np.where(seam, SEAM, DIRECT)), DIRECT)
    if variant == "seam_ignored":
        kind = np.where(kind == SEAM, DIRECT, kind)
    dead = kind == IDENTITY
    r = np.empty(x.shape + (4,), dtype=dt)
    r[:, 0] = np.where(cyc, np.where(dead, zero, r0), n0)
    r[:, 3] = np.where(cyc, np.where(dead, zero, r1), n1)
    r[:, 1] = np.where(neg & cyc, zero, Ps if variant == "period_n" else L)  # m = +1: L, m = -1: 0
    r[:, 2] = np.where(neg & cyc, Ps if variant == "period_n" else L, zero)
    return r, kind


# ---- the trajectory joint's sample R(r) -------------------------------------------------------------------------------------
def _conv(a, dt):
    """binary32 data (or exactly known float64 data) as values of the run: arrays of dt, or am.V"""
    return am.V(np.asarray(a, dtype=np.float64)) if dt == "V" else np.asarray(a).astype(dt)


class Trace:
    """the nlerp calls of one run: d of every call that counts and whether |d| < 8u"""

    def __init__(self):
        self.d, self.near = [], []

    def fraction_near(self):
        n = sum(x.size for x in self.d)
        return (sum(int(x.sum()) for x in self.near) / n) if n else 0.0


def sample(traj, J, joint, c, r, dt, trace=None, counted=None):
    """R(r) for steps' clips c [m] (already clamped) at positions r [m] (binary32 or float64 arrays): (T, Q) tuples of [m]"""
    m = c.shape[0]
    counted = np.ones(m, dtype=bool) if counted is None else counted
    if kind_of(traj) == "uniform":
        nkeys, _, first, keys = am._clip_tables(traj, J)
        N = nkeys[c]
        pos = clamp_pos(r, (N - 1).astype(r.dtype))
        i0 = np.floor(pos).astype(np.int64)
        i1 = np.minimum(i0 + 1, N - 1)
        a = pos - i0.astype(r.dtype)  # exact
        k0, k1 = keys[first[c] + i0, joint], keys[first[c] + i1, joint]
        t0, t1, q0, q1 = k0[:, 0:3], k1[:, 0:3], k0[:, 4:8], k1[:, 4:8]
        at = aq = _conv(a, dt)
    else:
        nticks, _, tracks, times, values = tm.concat(traj, J)
        posF = clamp_pos(r.astype(F), (nticks[c] - 1).astype(F))
        K0 = np.zeros((m, 2), dtype=np.int64)
        K1 = np.zeros((m, 2), dtype=np.int64)
        A = np.zeros((m, 2), dtype=F)
        AX = np.zeros((m, 2), dtype=np.float64)
        for ci in np.unique(c):
            sel = np.nonzero(c == ci)[0]
            tr = tracks[ci, joint, :2]
            K0[sel], K1[sel], A[sel], AX[sel] = tm.locate(times, tr["first"], tr["count"], posF[sel], nticks[ci], False)
        lo, st = tracks["lo"][c, joint, 0], tracks["step"][c, joint, 0]
        if dt == F:
            t0, t1 = tm.decode_lin(values[K0[:, 0]], lo, st), tm.decode_lin(values[K1[:, 0]], lo, st)
            q0, q1 = tm.decode_rot(values[K0[:, 1]]), tm.decode_rot(values[K1[:, 1]])
            at, aq = A[:, 0], A[:, 1]
        else:  # the decodes and a carried out exactly
            def lin(K):
                v = values[K][:, :3].astype(np.float64)
                val = lo.astype(np.float64) + v * st.astype(np.float64)
                mag = np.abs(lo.astype(np.float64)) + v * np.abs(st.astype(np.float64))
                return val, mag
            (t0, t0m), (t1, t1m) = lin(K0[:, 0]), lin(K1[:, 0])
            rot = lambda K: np.maximum(np.ascontiguousarray(values[K]).view(np.int16).astype(np.float64) / 32767.0, -1.0)
            q0, q1 = rot(K0[:, 1]), rot(K1[:, 1])
            if dt == "V":
                T0 = tuple(am.V(t0[:, i], t0m[:, i]) for i in range(3))
                T1 = tuple(am.V(t1[:, i], t1m[:, i]) for i in range(3))
                at, aq = am.V(AX[:, 0]), am.V(AX[:, 1])
                T = tuple(am.lerp_rule(u, v, at) for u, v in zip(T0, T1))
                Q = am.nlerp(tuple(am.V(q0[:, i]) for i in range(4)), tuple(am.V(q1[:, i]) for i in range(4)), aq, am.lerp_rule, True, trace, counted)
                return T, Q
            at, aq = AX[:, 0], AX[:, 1]
    T0, T1 = (tuple(_conv(t[:, i], dt) for i in range(3)) for t in (t0, t1))
    Q0, Q1 = (tuple(_conv(q[:, i], dt) for i in range(4)) for q in (q0, q1))
    at, aq = (v if isinstance(v, am.V) else _conv(v, dt) for v in (at, aq))
    with np.errstate(all="ignore"):
        T = tuple(am.lerp_rule(u, v, at) for u, v in zip(T0, T1))
        Q = am.nlerp(Q0, Q1, aq, am.lerp_rule, True, trace, counted)
    return T, Q


# ---- the helpers of sections 16 and 17 on tuples ------------------------------------------------------------------------------
def conj(q):
    return (-q[0], -q[1], -q[2], q[3])


def cross(u, v):
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def qrot(q, v):
    a = q[:3]
    t = cross(a, v)
    t = tuple(c + c for c in t)
    s = cross(a, t)
    return tuple((v[i] + q[3] * t[i]) + s[i] for i in range(3))


def norm4(q):
    n2 = am.dot(q, q)
    rn = am._rsqrt(n2)
    with np.errstate(all="ignore"):
        out = tuple(c * rn for c in q)
    bad = (am._val(n2) == 0) | ~np.isfinite(am._val(rn))
    return tuple(am._where(bad, am._const(c, i), c) for c, i in zip(out, (0.0, 0.0, 0.0, 1.0)))


def _f64(c):
    return np.asarray(c, dtype=np.float64)


def delta(a, b, variant=None):
    (Ta, Qa), (Tb, Qb) = a, b
    ca = conj(Qa)
    Q = qmul(Qb, ca) if variant == "qmul_reversed" else qmul(ca, Qb)
    d = tuple(y - x for x, y in zip(Ta, Tb))
    T = d if variant == "t_unrotated" else qrot(ca, d)
    return T, Q


def compose(d1, d2, variant=None):
    if variant == "fused_compose" and not isinstance(d1[0][0], am.V) and d1[0][0].dtype == F:
        # the sum with the rotated translation in one rounding: the rotation carried out in float64 from the binary32 values
        rt = qrot(tuple(_f64(c) for c in d1[1]), tuple(_f64(c) for c in d2[0]))
        T = tuple((_f64(x) + y).astype(F) for x, y in zip(d1[0], rt))
    else:
        T = tuple(x + y for x, y in zip(d1[0], qrot(d1[1], d2[0])))
    return T, qmul(d1[1], d2[1])


def _pick(c, a, b):
    return tuple(am._where(c, x, y) for x, y in zip(a, b))


def _kind(dt):
    return "V" if dt == "V" else np.dtype(dt).type


def step_deltas(traj, root, steps, dt=F, pos_dt=F, variant=None, trace=None, counted=None):
    """D_i of every step: (T, Q) tuples of [n * S] values, and the flat clamped clips, kinds and positions"""
    dt = _kind(dt)
    joint, rflags = root
    J = _njoints(traj)
    flat = steps.reshape(-1)
    m = flat.shape[0]
    lengths = clip_lengths(traj)
    c = np.minimum(flat["clip"].astype(np.int64), len(lengths) - 1)
    N = lengths[c]
    cyc = (np.asarray(rflags, dtype=np.int64)[c] & CYCLIC) != 0
    r, kind = positions(flat["x"], flat["dx"], N, cyc, pos_dt, variant)
    counted = np.ones(m, dtype=bool) if counted is None else counted
    live = counted & (kind != IDENTITY)
    smp = [sample(traj, J, joint, c, r[:, i], dt, trace, live & ((kind == SEAM) | (i in (0, 3)))) for i in range(4)]
    with np.errstate(all="ignore"):
        direct = delta(smp[0], smp[3], variant)
        d1, d2 = delta(smp[0], smp[1], variant), delta(smp[2], smp[3], variant)
        if variant == "norm_per_seam":
            d1, d2 = (d1[0], norm4(d1[1])), (d2[0], norm4(d2[1]))
        seam = compose(d2, d1, variant) if variant == "seam_swapped" else compose(d1, d2, variant)
        T = _pick(kind == SEAM, seam[0], direct[0])
        Q = _pick(kind == SEAM, seam[1], direct[1])
        if variant != "norm_per_seam":
            Q = norm4(Q)
        else:
            Q = _pick(kind == SEAM, Q, norm4(Q))
    ident = kind == IDENTITY
    T = tuple(am._where(ident, am._const(x, 0.0), x) for x in T)
    Q = tuple(am._where(ident, am._const(x, i), x) for x, i in zip(Q, (0.0, 0.0, 0.0, 1.0)))
    return (T, Q), c, kind, r


def blended(traj, root, steps, dt=F, pos_dt=F, variant=None, trace=None):
    """the blended delta of every instance: (T, Q) tuples of [n] values.  steps: STEP [n, S]"""
    n, S = steps.shape
    e = am.clamp_w(steps["w"])  # [n, S]
    used = np.ones((n, S), dtype=bool)
    if variant != "no_skip":
        used[:, 1:] = e[:, 1:] != 0
    (T, Q), _, _, _ = step_deltas(traj, root, steps, dt, pos_dt, variant, trace, used.reshape(-1))
    at = lambda v, i: (am.V(v.val.reshape(n, S)[:, i], v.mag.reshape(n, S)[:, i]) if isinstance(v, am.V) else v.reshape(n, S)[:, i])
    accT, accQ = tuple(at(v, 0) for v in T), tuple(at(v, 0) for v in Q)
    for i in range(1, S):
        ei = _conv(e[:, i], _kind(dt))
        with np.errstate(all="ignore"):
            nT = tuple(am.lerp_rule(x, at(v, i), ei) for x, v in zip(accT, T))
            nQ = am.nlerp(accQ, tuple(at(v, i) for v in Q), ei, am.lerp_rule, True, trace, used[:, i])
        accT, accQ = _pick(used[:, i], nT, accT), _pick(used[:, i], nQ, accQ)
    return accT, accQ


def local_matrix(T, Q):
    """section 14's local matrix of (T, Q, S = (1, 1, 1)) on tuples: a list of 16 values"""
    x, y, z, w = Q
    one, zero = am._const(x, 1.0), am._const(x, 0.0)
    with np.errstate(all="ignore"):
        x2, y2, z2 = x + x, y + y, z + z
        xx, yy, zz, xy, xz, yz = x * x2, y * y2, z * z2, x * y2, x * z2, y * z2
        wx, wy, wz = w * x2, w * y2, w * z2
        return [(one - (yy + zz)) * one, (xy + wz) * one, (xz - wy) * one, zero,
                (xy - wz) * one, (one - (xx + zz)) * one, (yz + wx) * one, zero,
                (xz + wy) * one, (yz - wx) * one, (one - (xx + yy)) * one, zero,
                T[0], T[1], T[2], one]


def deltas(traj, root, steps, dt=F, pos_dt=F, variant=None, trace=None):
    """the delta matrices D [n, 16] (what mtr_anim_root_deltas writes); dt "V": (values, sums of terms on absolute values)"""
    T, Q = blended(traj, root, steps, dt, pos_dt, variant, trace)
    M = local_matrix(T, Q)
    if _kind(dt) == "V":
        return np.stack([v.val for v in M], axis=-1), np.stack([v.mag for v in M], axis=-1)
    return np.ascontiguousarray(np.stack(M, axis=-1))


def mul(A, B, dt=F):
    """A B on [n, 16] column-major, section 12's fma chain from 0"""
    A, B = A.reshape(-1, 4, 4), B.reshape(-1, 4, 4)
    r = np.zeros(A.shape, dtype=dt)
    for k in range(4):
        x, y = A[:, None, k, :], B[:, :, k, None]
        with np.errstate(all="ignore"):
            r = fma32(x, y, r) if dt == F else x * y + r
    return np.ascontiguousarray(r.reshape(-1, 16))


def root_motion(M, traj, root, steps, dt=F, variant=None):
    """M_new [n, 16] = M . D (what mtr_batch_root_motion leaves in the batch)"""
    D = deltas(traj, root, steps, dt, F, variant)
    M = np.asarray(M).astype(dt)
    return mul(D, M, dt) if variant == "d_left" else mul(M, D, dt)


# ---- the generator ------------------------------------------------------------------------------------------------------
def _njoints(traj):
    return traj[0][0].shape[1] if kind_of(traj) == "uniform" else np.asarray(traj[0][2]).reshape(-1, 3).shape[0]


def clip_lengths(traj):
    if kind_of(traj) == "uniform":
        return np.array([np.asarray(k).shape[0] for k, _ in traj], dtype=np.int64)
    return np.array([int(c[0]) for c in traj], dtype=np.int64)


def walk_clip(N=31, J=1):
    """a smooth cyclic trajectory with yaw and drift: the last key is where the next cycle's key 0 stands"""
    k = np.arange(N, dtype=np.float64)
    keys = np.zeros((N, J, 12))
    yaw = 0.9 * k / (N - 1) + 0.05 * np.sin(2 * np.pi * k / (N - 1))
    keys[:, 0, 0] = 0.3 * np.sin(2 * np.pi * k / (N - 1)) + 0.02 * k
    keys[:, 0, 1] = 0.05 * np.cos(4 * np.pi * k / (N - 1))
    keys[:, 0, 2] = 0.09 * k
    keys[:, 0, 5] = np.sin(yaw / 2)
    keys[:, 0, 7] = np.cos(yaw / 2)
    keys[:, 0, 8:11] = 1
    return [(keys.astype(F), 0)]


def device_arrays(traj, J):
    """what the set's creation call takes: uniform -> ("uniform", nkeys u32 [C], keys f32 [total, J, 12]); tracks -> ("tracks",
    nticks u32 [C], tracks TRACK [C, J, 3], times u16, values u16 [nkeys, 4])"""
    if kind_of(traj) == "uniform":
        nkeys, _, _, keys = am._clip_tables(traj, J)
        return "uniform", nkeys.astype(np.uint32), np.ascontiguousarray(keys, dtype=F)
    nticks, _, tracks, times, values = tm.concat(traj, J)
    return "tracks", nticks.astype(np.uint32), np.ascontiguousarray(tracks), np.ascontiguousarray(times), np.ascontiguousarray(values)


# the clips of every generated set: key / tick counts and the root flags; NAN_CLIP holds NaN translations and is only named by
# steps of weight 0; the last clip (what a clip index past C reads) is the long cyclic one
LENGTHS = (1, 1, 2, 2, 2, 31, 31)
ROOT_FLAGS = (0, CYCLIC, 0, CYCLIC, 0, 0, CYCLIC)
NAN_CLIP = 4
SETS = (("uniform", 1, 0), ("uniform", 3, 2), ("tracks", 1, 0), ("tracks", 3, 2))  # kind, J, joint
COUNTS = (1, 5, 17, 257)  # a partial group, a partial wave, a partial workgroup
NSTEPS = (1, 2, 8)
W_EDGES = (0.0, 1.0, float("nan"), 1.5, 0.0, -0.5)


def make_set(kind, J, seed):
    rng = np.random.default_rng(seed)
    shape = [(N, 0) for N in LENGTHS]
    if kind == "uniform":
        traj = am.random_clips(rng, J, shape=shape, noise=0.3, trans=3.0)
        traj[NAN_CLIP][0][..., 0:3] = np.nan
    else:
        # tm's generator gives the clip at index tm.HUGE two special tracks that suit a long clip only: a long one stands there
        # while the set is generated and is dropped
        traj = tm.random_track_clips(rng, J, shape=shape[:tm.HUGE] + [(30001, 0)] + shape[tm.HUGE:], noise=0.3, trans=3.0)
        del traj[tm.HUGE]
        traj[NAN_CLIP][2]["lo"][:, 0, :] = np.nan
    return traj


def edge_steps():
    """(clip, x, dx) that hit every m and every edge of the section, on the 31-key and the 2-key clips"""
    out = []
    for cyc, non, N in ((6, 5, 31), (3, 2, 2)):
        L = float(N - 1)
        over = float(np.nextafter(F(L), F(np.inf)))
        for clip in (cyc, non):
            for dx in (0.0, 0.37, -0.37, L, -L, over, -over, float("nan"), float("inf"), float("-inf")):
                out.append((clip, 0.4 * L, dx))
            for x in (-0.0, -1e-7, 1e30, float("nan"), L, L - 0.2, 0.0, 7.3 * L, -3.6 * L):
                out.append((clip, x, 0.37))
                out.append((clip, x, -0.37))
            out.append((clip, 0.0, -1e-7))  # y + L rounds to L
            out.append((clip, -1e-7, -1e-7))
    for clip in (0, 1, 7, 0xFFFFFFFF, 12):  # one key, cyclic and not; indices past C
        out.append((clip, 0.5, 0.37))
        out.append((clip, 29.9, 0.37))
    return out


EDGES = edge_steps()


def make_steps(rng, n, S, off=0):
    st = np.zeros((n, S), dtype=STEP)
    good = [i for i in range(len(LENGTHS)) if i != NAN_CLIP]
    st["clip"] = rng.choice(good, size=(n, S))
    st["x"] = rng.uniform(-40.0, 70.0, size=(n, S))
    st["dx"] = np.where(rng.random((n, S)) < 0.5, rng.choice([0.37, -0.37], size=(n, S)), rng.uniform(-3.0, 3.0, size=(n, S)))
    st["w"] = rng.uniform(-0.2, 1.2, size=(n, S))
    flat = st.reshape(-1)
    for t in range(flat.shape[0]):
        if t % 3 == 0 or n * S < 9:
            flat[t]["clip"], flat[t]["x"], flat[t]["dx"] = EDGES[(t // 3 + off) % len(EDGES)]
        if t % 2 == 1:
            flat[t]["w"] = W_EDGES[(t // 2 + off) % len(W_EDGES)]
    # NaN keys behind a step of weight 0 (never step 0, whose weight is not read)
    if S > 1:
        for i in range(0, n, 4):
            s = 1 + (i // 4) % (S - 1)
            st[i, s]["clip"], st[i, s]["w"] = NAN_CLIP, (0.0, float("nan"), -1.0)[(i // 4) % 3]
    if n >= 17:  # and one instance whose last step reads them: NaN for NaN
        st[n - 2, S - 1]["clip"], st[n - 2, S - 1]["w"] = NAN_CLIP, 0.5
    return st


def trs(rng, n, tmax=20.0):
    from tests.attach_model import trs as _trs
    return _trs(rng, n, tmax)


_CASES = None


def cases():
    """every (set, n, S) of the section's test plan: dicts of name, kind, J, traj, root (joint, flags), n, S, steps, M"""
    global _CASES
    if _CASES is None:
        out = []
        for si, (kind, J, joint) in enumerate(SETS):
            traj = make_set(kind, J, 190 + si)
            for n in COUNTS:
                for S in NSTEPS:
                    rng = np.random.default_rng(10000 * si + 10 * n + S)
                    out.append(dict(name=f"{kind}_J{J}_n{n}_S{S}", kind=kind, J=J, traj=traj, root=(joint, np.array(ROOT_FLAGS, dtype=np.uint32)), n=n, S=S,
                                    steps=make_steps(rng, n, S, off=len(out) * 5), M=trs(rng, n)))
        _CASES = out
    return _CASES


def can_show(variant, case):
    """whether a wrong reading can change an instance of the case at all (the exemptions of tests/test_root_model.py)"""
    st = case["steps"]
    lengths = clip_lengths(case["traj"])
    c = np.minimum(st["clip"].astype(np.int64), len(lengths) - 1)
    cyc = (np.asarray(ROOT_FLAGS)[c] & CYCLIC) != 0
    e = am.clamp_w(st["w"])
    used = np.ones(st.shape, dtype=bool)
    used[:, 1:] = e[:, 1:] != 0
    _, kind = positions(st["x"].reshape(-1), st["dx"].reshape(-1), lengths[c].reshape(-1), cyc.reshape(-1))
    kind = kind.reshape(st.shape)
    moving = used & (kind != IDENTITY) & (lengths[c] > 1)
    if variant in ("t_unrotated", "qmul_reversed", "d_left"):
        return bool(moving.any())
    if variant in ("seam_ignored", "seam_swapped", "fused_compose", "norm_per_seam"):  # need a step across a seam that counts
        return bool((used & (kind == SEAM)).any())
    if variant == "period_n":  # needs a cyclic clip of more than one key
        return bool((used & cyc & (lengths[c] > 1)).any())
    if variant == "no_skip":  # needs a later step of weight 0
        return bool((~used).any())
    raise KeyError(variant)


def same_bits(a, b):
    """per element: equal bits, or NaN in both (payloads are free)"""
    a, b = np.ascontiguousarray(a, dtype=F), np.ascontiguousarray(b, dtype=F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
