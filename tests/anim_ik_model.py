"""Numpy model of SPEC.md section 17 (inverse kinematics after the layer stack), written from that text, and the inputs
its tests share.

`sample(clips, layers, njoints, masks, parents, chains, targets)` carries the rule out in binary32, one rounded numpy
operation per operator, and gives the local matrices bit for bit; `dt=np.float64` carries the same operations out in
float64 from the binary32 (T, Q, S) of the stack.  The layer stack is section 16's model (tests/anim_layers_model.py).  The
world matrices are section 12's k-ordered fma chain, parent on the left, with an exact binary32 fma (`fma32`: the product is
exact in float64, the sum is rounded to odd there, and the cast to binary32 then rounds once).

chains: an array of CHAIN [K]; targets: an array of TARGET [n, K]; parents: one byte per joint, a root 255 or itself.
`variant` names one deliberately wrong reading of the section (WRONG_VARIANTS).  `probe`: a list that receives, per chain,
what the chain saw and made (positions, the guard, the re-folded joints)."""
import numpy as np

from tests import anim_layers_model as lm
from tests import anim_model as am

F = np.float32
CHAIN = np.dtype([("kind", "<u4"), ("joint", "<u4", 3), ("axis", "<f4", 3), ("flags", "<u4")])
TARGET = np.dtype([("pos", "<f4", 3), ("w", "<f4"), ("pole", "<f4", 3), ("pad", "<u4")])
TWO_BONE, AIM, POLE = 0, 1, 1
MAX_IK = 4
FLT_MAX = float(np.finfo(F).max)
WRONG_VARIANTS = ("conj_wrong_side", "local_space", "pole_ignored", "no_clamp", "stale_pb", "fused_pb", "parallel")


# ---- section 12 with an exact fma ---------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) on binary32 arrays, exactly: one rounding of the exact a * b + c"""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b  # exact: 48 bits, no underflow in float64
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)  # TwoSum: s + err == p + c exactly
        inexact = np.isfinite(s) & np.isfinite(err) & (err != 0)
        even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
        odd = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))  # the neighbour on the side of the exact sum
        return np.where(inexact & even, odd, s).astype(F)  # rounded to odd in float64, then once to binary32


def mat_mul(A, B, dt):
    """out = A B, column-major [n, 4 columns, 4 rows]: out[c][i] = the fma chain over k = 0..3 of A[k][i] * B[c][k] from 0"""
    r = np.zeros(A.shape, dtype=dt)
    for k in range(4):
        x, y = A[:, None, k, :], B[:, :, k, None]
        with np.errstate(all="ignore"):
            r = fma32(x, y, r) if dt == F else x * y + r
    return r


def paths_of(parents):
    """per joint its path, the root first and the joint last"""
    out = []
    for j in range(len(parents)):
        up = [j]
        while parents[up[-1]] != 255 and parents[up[-1]] != up[-1]:
            up.append(int(parents[up[-1]]))
        out.append(up[::-1])
    return out


def world(L, path, dt):
    """the world matrix [n, 4, 4] of the last joint of path over the local matrices L [n, J, 16]"""
    W = L[:, path[0]].reshape(-1, 4, 4)
    for j in path[1:]:
        W = mat_mul(W, L[:, j].reshape(-1, 4, 4), dt)
    return W


# ---- the helpers of section 17, on arrays [n, 3] / [n, 4] of one dtype --------------------------------------------------
def dot3(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def length(v):
    return np.sqrt(dot3(v, v))


def cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=-1)


def conj(q):
    return np.stack([-q[:, 0], -q[:, 1], -q[:, 2], q[:, 3]], axis=-1)


def qmul(p, q):
    return np.stack(lm.qmul(tuple(p[:, i] for i in range(4)), tuple(q[:, i] for i in range(4))), axis=-1)


def norm4(q):
    n2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
    rn = q.dtype.type(1) / np.sqrt(n2)
    bad = (n2 == 0) | ~np.isfinite(rn)
    ident = np.zeros_like(q)
    ident[:, 3] = 1
    return np.where(bad[:, None], ident, q * rn[:, None])


def qrot(q, v):
    t = cross(q[:, :3], v)
    t = t + t
    return (v + q[:, 3:4] * t) + cross(q[:, :3], t)


def fromto(u, v):
    w = np.sqrt(dot3(u, u) * dot3(v, v)) + dot3(u, v)
    return norm4(np.concatenate([cross(u, v), w[:, None]], axis=-1))


def nlerp(q0, q1, e):
    out = am.nlerp(tuple(q0[:, i] for i in range(4)), tuple(q1[:, i] for i in range(4)), e, am.lerp_rule, True, None, None)
    return np.stack(out, axis=-1).astype(q0.dtype)


def local_matrix(T, Q, S):
    """section 14's local matrix of (T [.., 3], Q [.., 4], S [.., 3]): [.., 16], in the arrays' dtype"""
    x, y, z, qw = (Q[..., i] for i in range(4))
    one, zero = np.ones_like(x), np.zeros_like(x)
    with np.errstate(all="ignore"):
        x2, y2, z2 = x + x, y + y, z + z
        xx, yy, zz, xy, xz, yz = x * x2, y * y2, z * z2, x * y2, x * z2, y * z2
        wx, wy, wz = qw * x2, qw * y2, qw * z2
        cols = [(one - (yy + zz)) * S[..., 0], (xy + wz) * S[..., 0], (xz - wy) * S[..., 0], zero,
                (xy - wz) * S[..., 1], (one - (xx + zz)) * S[..., 1], (yz + wx) * S[..., 1], zero,
                (xz + wy) * S[..., 2], (yz - wx) * S[..., 2], (one - (xx + yy)) * S[..., 2], zero,
                T[..., 0], T[..., 1], T[..., 2], one]
    return np.stack(cols, axis=-1)


# ---- the chains ---------------------------------------------------------------------------------------------------
def _two_bone(pa, pb, pc, P, Qa, Qb, g, pole, use_pole, e, variant, dt):
    ab, bc = pb - pa, pc - pb
    la, lb = length(ab), length(bc)
    d = g - pa
    dist = length(d)
    lo, hi = np.abs(la - lb), la + lb
    lt = dist
    if variant != "no_clamp":
        lt = np.where(lt < lo, lo, lt)
        lt = np.where(lt > hi, hi, lt)
    n = d / dist[:, None]
    u = pole - pa if use_pole and variant != "pole_ignored" else ab
    h = u - dot3(u, n)[:, None] * n
    hl = length(h)
    guard = (la > 0) & (lb > 0) & (dist > 0) & (lt > 0) & (hl > 0) & (dist <= dt(FLT_MAX))
    hh = h / hl[:, None]
    x = ((la * la - lb * lb) + lt * lt) / (lt + lt)
    y2 = la * la - x * x
    y = np.where(y2 > 0, np.sqrt(np.where(y2 > 0, y2, 0)), 0).astype(dt)
    if variant == "fused_pb":
        fused = (pa.astype(np.float64) + x.astype(np.float64)[:, None] * n.astype(np.float64)).astype(dt)
        pb1 = fused + y[:, None] * hh
    else:
        pb1 = (pa + x[:, None] * n) + y[:, None] * hh
    pc1 = pa + lt[:, None] * n
    Ra = fromto(ab, pb1 - pa)
    pcs = pa + qrot(Ra, pc - pa)
    Rb = fromto(pcs - pb1, pc1 - pb1)
    A0 = qmul(P, Qa)
    A = qmul(Ra, A0)
    if variant == "local_space":
        Qa1, Qb1 = qmul(Ra, Qa), qmul(Rb, Qb)
    else:
        Qa1 = qmul(A, conj(P)) if variant == "conj_wrong_side" else qmul(conj(P), A)
        Ab = A0 if variant == "stale_pb" else A
        Qb1 = qmul(conj(Ab), qmul(Rb, qmul(Ab, Qb)))
    return guard, nlerp(Qa, Qa1, e), nlerp(Qb, Qb1, e), dict(la=la, lb=lb, n=n, hh=hh, pc1=pc1, lt=lt, dist=dist)


def _aim(pa, P, Qa, axis, g, e, variant):
    A0 = qmul(P, Qa)
    cur = qrot(A0, axis)
    v = g - pa
    guard = (length(v) > 0) & (length(cur) > 0)
    R = fromto(cur, v)
    if variant == "local_space":
        Qa1 = qmul(R, Qa)
    elif variant == "conj_wrong_side":
        Qa1 = qmul(qmul(R, A0), conj(P))
    else:
        Qa1 = qmul(conj(P), qmul(R, A0))
    return guard, nlerp(Qa, Qa1, e), dict(v=v)


def solve(T, Q, S, parents, chains, targets, variant=None, dt=F, probe=None):
    """the chains of section 17 over (T [n, J, 3], Q [n, J, 4], S [n, J, 3]) of dtype dt: the new Q"""
    assert variant is None or variant in WRONG_VARIANTS
    chains, targets = np.asarray(chains).reshape(-1), np.asarray(targets)
    n, K = targets.shape
    assert 1 <= K <= MAX_IK and K == chains.size and Q.dtype == dt
    paths = paths_of(parents)
    Q = Q.copy()
    L = local_matrix(T, Q, S)
    Q0, L0 = Q.copy(), L.copy()
    for k in range(K):
        ch, tg = chains[k], targets[:, k]
        e32 = am.clamp_w(tg["w"])
        active = e32 != 0
        e = e32.astype(dt)
        g, pole = tg["pos"].astype(dt), tg["pole"].astype(dt)
        a, b, c = (int(j) for j in ch["joint"])
        Qs, Ls = (Q0, L0) if variant == "parallel" else (Q, L)  # what the chain sees
        with np.errstate(all="ignore"):
            Wa = world(Ls, paths[a], dt)
            pa = Wa[:, 3, :3]
            P = np.zeros((n, 4), dtype=dt)
            P[:, 3] = 1
            for i, j in enumerate(paths[a][:-1]):
                P = Qs[:, j].copy() if i == 0 else qmul(P, Qs[:, j])
            info = dict(k=k, kind=int(ch["kind"]), active=active, e=e32, pa=pa, P=P, g=g, pole=pole)
            if ch["kind"] == TWO_BONE:
                Wb = mat_mul(Wa, Ls[:, b].reshape(-1, 4, 4), dt)
                Wc = mat_mul(Wb, Ls[:, c].reshape(-1, 4, 4), dt)
                guard, Qa, Qb, more = _two_bone(pa, Wb[:, 3, :3], Wc[:, 3, :3], P, Qs[:, a], Qs[:, b], g, pole, bool(ch["flags"] & POLE), e, variant, dt)
                hit = active & guard
                Q[:, a] = np.where(hit[:, None], Qa, Q[:, a])
                Q[:, b] = np.where(hit[:, None], Qb, Q[:, b])
                changed = (a, b)
            else:
                guard, Qa, more = _aim(pa, P, Qs[:, a], np.broadcast_to(ch["axis"].astype(dt), (n, 3)), g, e, variant)
                hit = active & guard
                Q[:, a] = np.where(hit[:, None], Qa, Q[:, a])
                changed = (a,)
            for j in changed:
                L[:, j] = local_matrix(T[:, j], Q[:, j], S[:, j])
            if probe is not None:
                info.update(more, guard=guard, hit=hit, a=a, b=b, c=c, Qa=Q[:, a].copy())
                if ch["kind"] == TWO_BONE:  # the joints re-folded over the locals as they stand now
                    Wa2 = world(L, paths[a], dt)
                    Wb2 = mat_mul(Wa2, L[:, b].reshape(-1, 4, 4), dt)
                    info.update(pb_new=Wb2[:, 3, :3], pc_new=mat_mul(Wb2, L[:, c].reshape(-1, 4, 4), dt)[:, 3, :3])
                probe.append(info)
    return Q


def stack_tqs(clips, layers, njoints, masks=None):
    """section 16's (T, Q, S) in binary32 as arrays [n, J, 3], [n, J, 4], [n, J, 3]"""
    T, Q, S = lm.sample_tqs(clips, layers, njoints, masks)
    return np.stack(T, axis=-1), np.stack(Q, axis=-1), np.stack(S, axis=-1)


def sample(clips, layers, njoints, masks, parents, chains, targets, variant=None, dt=F, probe=None, tqs=None):
    """the local matrices of section 17: [n, njoints, 16] of dtype dt.  tqs: stack_tqs's result, when the caller has it"""
    T, Q, S = (v.astype(dt) for v in (tqs if tqs is not None else stack_tqs(clips, layers, njoints, masks)))
    Q = solve(T, Q, S, parents, chains, targets, variant, dt, probe)
    out = local_matrix(T, Q, S)
    assert out.dtype == dt
    return out


# ---- inputs shared by the tests -----------------------------------------------------------------------------------
W_EDGES = [float("nan"), -1.0, 0.0, 1e-30, 1.0, 2.0]
N_INST = 256


def skeleton(J):
    """parents of J joints: a chain 0 - 1 - .. for J <= 65; for more joints a chain of 210 and the rest hung onto it"""
    par = np.array([255] + list(range(J - 1)), dtype=np.uint8)
    for j in range(211, J):
        par[j] = (j * 37) % 200
    return par


def default_chains(parents, K):
    """K chains on the deepest joint c, its parent b and b's parent a: TWO_BONE with POLE on (a, b, c); AIM at a, the joint
    the first chain has just changed; TWO_BONE without POLE one joint up, (parent(a), a, b), which shares two joints with
    the first -- or, under a root a, AIM at b; AIM at c.  No chain solves a limb that an earlier one solved: a limb stretched
    straight by one chain and folded completely by the next goes through fromto of exactly antiparallel vectors, the one
    case section 17 leaves without a bound"""
    paths = paths_of(parents)
    c = max(range(len(parents)), key=lambda j: (len(paths[j]), j))
    a, b = paths[c][-3], paths[c][-2]
    rooted = len(paths[a]) == 1
    ch = np.zeros(4, dtype=CHAIN)
    ch["kind"] = [TWO_BONE, AIM, AIM if rooted else TWO_BONE, AIM]
    ch["joint"] = [(a, b, c), (a, 0, 0), (b, 0, 0) if rooted else (paths[a][-2], a, b), (c, 0, 0)]
    ch["axis"] = [(0, 0, 0), (0.3, 1.0, -0.2), (0.0, -0.5, 1.0) if rooted else (0, 0, 0), (-1.0, 0.25, 0.5)]
    ch["flags"] = [POLE, 0, 0, 0]
    return ch[:K].copy()


def make_targets(rng, tqs, parents, chains, dtype=TARGET):
    """[n, K] targets for the pose (T, Q, S): positions at 0.2 to 1.4 of the chain's reach from p_a (of the pose before any
    chain) in a random direction, poles a reach away in another direction (off the line to the target), weights of which
    a tenth is 0 and some lie outside [0, 1]; then, where n has room for them (12 K + 2 instances), the edges written over
    the first instances: every weight of W_EDGES on every chain, NaN and infinite positions and poles"""
    T, Q, S = (v.astype(np.float64) for v in tqs)
    n, K = T.shape[0], len(chains)
    paths = paths_of(parents)
    L = local_matrix(T, Q, S)
    tg = np.zeros((n, K), dtype=dtype)

    def unit(v):
        return v / np.linalg.norm(v, axis=-1, keepdims=True)
    for k, ch in enumerate(chains):
        a, b, c = (int(j) for j in ch["joint"])
        pa = world(L, paths[a], np.float64)[:, 3, :3]
        if ch["kind"] == TWO_BONE:
            pb = world(L, paths[b], np.float64)[:, 3, :3]
            pc = world(L, paths[c], np.float64)[:, 3, :3]
            reach = np.linalg.norm(pb - pa, axis=-1) + np.linalg.norm(pc - pb, axis=-1)
        else:
            reach = np.full(n, 5.0)
        d = unit(rng.normal(size=(n, 3)))
        tg["pos"][:, k] = pa + d * (reach * rng.uniform(0.2, 1.4, n))[:, None]
        side = unit(np.cross(d, rng.normal(size=(n, 3))))
        tg["pole"][:, k] = pa + (side + d * rng.uniform(-0.5, 0.5, n)[:, None]) * reach[:, None]
        tg["w"][:, k] = np.where(rng.random(n) < 0.1, 0.0, np.where(rng.random(n) < 0.5, 1.0, rng.uniform(-0.2, 1.2, n)))
    if n < 12 * K + 2:
        return tg
    i = 0
    for k in range(K):  # the edge weights, chain by chain
        tg["w"][i:i + len(W_EDGES), k] = W_EDGES
        i += len(W_EDGES)
    tg["w"][i:i + 2, :] = 0.0  # every chain at weight 0: the instance is section 16's, bit for bit
    i += 2
    for k in range(K):
        tg["w"][i:i + 6, k] = 1.0
        tg["pos"][i, k, 0] = np.nan
        tg["pos"][i + 1, k, 1] = np.inf
        tg["pos"][i + 2, k] = -np.inf
        tg["pole"][i + 3, k, 2] = np.nan
        tg["pole"][i + 4, k] = np.inf
        tg["pos"][i + 5, k] = 3e38  # finite, but the distance overflows
        i += 6
    assert i <= n
    return tg


def uniform_scale(clips):
    """the uniform clips with every key's scale made uniform (y and z take x's), which lerp and the layer steps preserve"""
    out = []
    for keys, fl in clips:
        k = np.array(keys, dtype=F, copy=True)
        k[..., 9] = k[..., 8]
        k[..., 10] = k[..., 8]
        out.append((k, fl))
    return out
