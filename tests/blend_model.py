"""The numpy model of SPEC.md section 23 (blend spaces), written from that text: blend states advanced by dt against parameter
rows, the three slots with their sequential weights, the shared phase, and the records of the frame.  binary32 throughout with
one rounded operation per numpy operation and no fused multiply-add anywhere; NaN compares false.  `fdt=np.float64` runs the same
rules in float64 (the twin the shares are held against).  Also the generator of cases that the CPU tests, the host build of
csrc/blend_math.h and the GPU tests share, a census of the branches the cases reach, and a table of wrong readings of the text
(WRONG_VARIANTS) that the cases must be able to tell apart."""
import numpy as np

from tests import player_model as pm

F = np.float32
U = 2.0 ** -24
FLT_MAX = pm.FLT_MAX
LOOP = pm.LOOP
SAMPLE = np.dtype([("clip", "<u4"), ("px", "<f4"), ("py", "<f4"), ("pad", "<u4")])
TRI = np.dtype([("v", "<u4", (3,)), ("pad", "<u4")])
STATE = np.dtype([("phase", "<f4"), ("px", "<f4"), ("py", "<f4"), ("speed", "<f4")])
LAYER = pm.LAYER
STEP = pm.STEP

WRONG_VARIANTS = ("last_tri", "e1_no_div", "rate_slot0", "pos_phi0", "step_x_after", "fused_smooth", "no_copy", "tie_later")
BRANCHES = ("1d_below", "1d_above", "1d_between", "tri_first", "tri_later", "fb_outside", "fb_crack", "om_zero", "reseed", "a_one", "wrap_fwd",
            "wrap_back", "phase_fallback")
K_SHARES = 3       # rounded operations on the longest path from (e1, e2) to a share: E0 = (1 - e1) * (1 - e2)
SUM_BOUND = K_SHARES * U / (1 - K_SHARES * U)


# ---- the set ----------------------------------------------------------------------------------------------------------------
def blend_set(tab, samples, tris=None, nparams=1, param_x=0, param_y=0, damp=np.inf):
    """tab: a player table (key counts, flag words, rates); samples: rows (clip, px[, py]); tris: rows of three indices"""
    s = np.zeros(len(samples), dtype=SAMPLE)
    for k, r in enumerate(samples):
        s["clip"][k], s["px"][k] = r[0], r[1]
        s["py"][k] = r[2] if len(r) > 2 else 0.0
    t = np.zeros(0 if tris is None else len(tris), dtype=TRI)
    if len(t):
        t["v"] = np.asarray(tris, dtype=np.uint32)
    return dict(tab=tab, samples=s, tris=t, nparams=nparams, param_x=param_x, param_y=param_y, damp=F(damp))


def area2(x0, y0, x1, y1, x2, y2):
    with np.errstate(all="ignore"):
        return (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)


def check_set(bs):
    """the creation check: None, or what mtr_anim_blend_create names"""
    nkeys, flags, rates = bs["tab"]
    C, s, t = len(nkeys), bs["samples"], bs["tris"]
    if C < 1 or not (1 <= s.size <= 32) or t.size > 64 or not (1 <= bs["nparams"] <= 16):
        return "counts"
    if bs["param_x"] >= bs["nparams"] or (t.size and bs["param_y"] >= bs["nparams"]):
        return "param"
    if not bs["damp"] > 0:
        return "damp"
    for c in range(C):
        if not (1 <= nkeys[c] <= 1 << 24) or (flags[c] & ~LOOP) or not np.isfinite(rates[c]):
            return f"clip {c} "
    for k in range(s.size):
        c = int(s["clip"][k])
        if c >= C or not (flags[c] & LOOP) or not np.isfinite(s["px"][k]) or (t.size and not np.isfinite(s["py"][k])):
            return f"sample {k} "
        if not t.size and k > 0:
            with np.errstate(all="ignore"):
                step = s["px"][k] - s["px"][k - 1]
            if not (step > 0 and np.isfinite(step)):
                return f"sample {k} "
    for k in range(t.size):
        v = [int(i) for i in t["v"][k]]
        if max(v) >= s.size or len(set(v)) != 3:
            return f"triangle {k} "
        A = area2(*(s[f][i] for i in v for f in ("px", "py")))
        if not (A > 0 and np.isfinite(A)):
            return f"triangle {k} "
    return None


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def _clamp(w):
    return pm.clamp_w(w)


def _finite(v):
    with np.errstate(all="ignore"):
        return np.abs(v) <= FLT_MAX


def smooth(p, t, a, fdt=F, variant=None):
    """step 2 for one parameter"""
    with np.errstate(all="ignore"):
        d = t - p
        if variant == "fused_smooth" and fdt is F:
            moved = (p.astype(np.float64) + a.astype(np.float64) * d.astype(np.float64)).astype(F)
        else:
            moved = p + a * d
    copy = ~_finite(p) if variant == "no_copy" else ((a == 1) | ~_finite(p))
    return np.where(copy, t, moved)


def slots_1d(p, sx, fdt=F, trace=None):
    """step 3 in a 1-D space: (slots int64 [n, 3], e1, e2)"""
    n, K = p.shape[0], sx.shape[0]
    with np.errstate(all="ignore"):
        below = ~(p > sx[0])
        above = ~below & (p >= sx[K - 1])
        mid = ~below & ~above
        j = (sx[None, 1:K - 1] <= p[:, None]).sum(axis=1) if K > 2 else np.zeros(n, dtype=np.int64)
        j1 = np.minimum(j + 1, K - 1)
        e1 = (p - sx[j]) / (sx[j1] - sx[j])
    zero = np.zeros(n, dtype=fdt)
    s0 = np.where(below, 0, np.where(above, K - 1, j))
    s1 = np.where(below, 0, np.where(above, K - 1, j1))
    if trace is not None:
        for name, m in (("1d_below", below), ("1d_above", above), ("1d_between", mid)):
            trace[name] = trace.get(name, 0) + int(m.sum())
    return np.stack([s0, s1, s0], axis=1).astype(np.int64), np.where(mid, e1, zero).astype(fdt), zero


def _dot2(ux, uy, vx, vy):
    return ux * vx + uy * vy


def slots_2d(px, py, sx, sy, tris, fdt=F, variant=None, trace=None, inside64=None):
    """step 3 in a 2-D space: (slots int64 [n, 3], e1, e2).  inside64: per instance, does the float64 twin find a triangle
    (tells a rounding crack from a point outside the hull in the census)"""
    n = px.shape[0]
    one, zero = fdt(1), np.zeros(n, dtype=fdt)
    hit = np.zeros(n, dtype=bool)
    trip = np.full(n, -1, dtype=np.int64)
    slots = np.zeros((n, 3), dtype=np.int64)
    e1, e2 = zero.copy(), zero.copy()
    omz = np.zeros(n, dtype=bool)
    with np.errstate(all="ignore"):
        for k, v in enumerate(tris):
            x0, y0, x1, y1, x2, y2 = sx[v[0]], sy[v[0]], sx[v[1]], sy[v[1]], sx[v[2]], sy[v[2]]
            A = area2(x0, y0, x1, y1, x2, y2)
            qx, qy = px - x0, py - y0
            l1 = (qx * (y2 - y0) - (x2 - x0) * qy) / A
            l2 = ((x1 - x0) * qy - qx * (y1 - y0)) / A
            l0 = (one - l1) - l2
            inside = (l0 >= 0) & (l1 >= 0) & (l2 >= 0)
            take = inside if variant == "last_tri" else inside & ~hit
            om = one - l2
            t1 = _clamp(l1) if variant == "e1_no_div" else np.where(om == 0, zero, _clamp(l1 / om))
            slots[take] = [int(v[0]), int(v[1]), int(v[2])]
            e1, e2 = np.where(take, t1, e1), np.where(take, _clamp(l2), e2)
            omz = np.where(take, om == 0, omz)
            trip = np.where(take, k, trip)
            hit |= inside
        # the fallback
        ba = np.full(n, int(tris[0][0]), dtype=np.int64)
        bb, bt, bd = ba.copy(), zero.copy(), np.full(n, np.inf, dtype=fdt)
        for v in tris:
            for ia, ib in ((v[0], v[1]), (v[1], v[2]), (v[2], v[0])):
                ax, ay = sx[ia], sy[ia]
                ex, ey = sx[ib] - ax, sy[ib] - ay
                qx, qy = px - ax, py - ay
                t = _clamp(_dot2(qx, qy, ex, ey) / _dot2(ex, ey, ex, ey)).astype(fdt)
                cx, cy = ax + t * ex, ay + t * ey
                dx, dy = px - cx, py - cy
                d2 = _dot2(dx, dy, dx, dy)
                better = (d2 <= bd) if variant == "tie_later" else (d2 < bd)
                ba, bb = np.where(better, int(ia), ba), np.where(better, int(ib), bb)
                bt, bd = np.where(better, t, bt), np.where(better, d2, bd)
    fb = ~hit
    slots[fb] = np.stack([ba, bb, ba], axis=1)[fb]
    e1, e2 = np.where(fb, bt, e1), np.where(fb, zero, e2)
    if trace is not None:
        crack = fb & (inside64 if inside64 is not None else np.zeros(n, dtype=bool))
        for name, m in (("tri_first", hit & (trip == 0)), ("tri_later", hit & (trip > 0)), ("fb_crack", crack), ("fb_outside", fb & ~crack),
                        ("om_zero", hit & omz)):
            trace[name] = trace.get(name, 0) + int(m.sum())
    return slots, e1.astype(fdt), e2.astype(fdt)


def shares_of(e1, e2):
    """E0, E1, E2 from the sequential weights: two differences and two products"""
    one = e1.dtype.type(1)
    om2, om1 = one - e2, one - e1
    return np.stack([om1 * om2, e1 * om2, e2], axis=1)


def _tables(bs, fdt):
    P, _ = pm.periods(bs["tab"], fdt)
    return P, bs["tab"][2].astype(fdt), bs["samples"]["px"].astype(fdt), bs["samples"]["py"].astype(fdt), [[int(i) for i in v] for v in bs["tris"]["v"]]


def find_slots(bs, px, py, fdt=F, variant=None, trace=None):
    """step 3 for points (px, py): (slots int64 [n, 3], e1, e2)"""
    _, _, sx, sy, tris = _tables(bs, fdt)
    if not tris:
        return slots_1d(px, sx, fdt, trace)
    inside64 = _hit64(bs, px, py) if trace is not None and fdt is F else None
    return slots_2d(px, py, sx, sy, tris, fdt, variant, trace, inside64)


def _hit64(bs, px, py):
    """does some triangle hold the point when the rule runs in float64 on the same binary32 point"""
    _, _, sx, sy, tris = _tables(bs, np.float64)
    px, py = px.astype(np.float64), py.astype(np.float64)
    hit = np.zeros(px.shape[0], dtype=bool)
    with np.errstate(all="ignore"):
        for v in tris:
            x0, y0, x1, y1, x2, y2 = sx[v[0]], sy[v[0]], sx[v[1]], sy[v[1]], sx[v[2]], sy[v[2]]
            A = area2(x0, y0, x1, y1, x2, y2)
            l1 = ((px - x0) * (y2 - y0) - (x2 - x0) * (py - y0)) / A
            l2 = ((x1 - x0) * (py - y0) - (px - x0) * (y1 - y0)) / A
            hit |= ((1.0 - l1) - l2 >= 0) & (l1 >= 0) & (l2 >= 0)
    return hit


def advance_fields(bs, st, params, dt, fdt=F, variant=None, trace=None):
    """steps 1 to 6 on a dict of state arrays: (stored state dict, frame dict)"""
    P, rate, sx, sy, tris = _tables(bs, fdt)
    two_d = bool(tris)
    dt = fdt(dt)
    n = st["phase"].shape[0]
    one, zero = fdt(1), np.zeros(n, dtype=fdt)
    with np.errstate(all="ignore"):
        # 1. target, 2. smooth
        tx, ty = params[:, bs["param_x"]].astype(fdt), params[:, bs["param_y"]].astype(fdt)
        dtp = dt if dt > 0 else fdt(0)
        a = np.full(n, _clamp(np.asarray(dtp * fdt(bs["damp"]), dtype=fdt)), dtype=fdt)
        px = smooth(st["px"], tx, a, fdt, variant)
        py = smooth(st["py"], ty, a, fdt, variant) if two_d else st["py"]
        # 3. slots
        sl, e1, e2 = find_slots(bs, px, py, fdt, variant, trace)
        clip = bs["samples"]["clip"].astype(np.int64)[sl]
        sh = shares_of(e1, e2)
        # 4. phase
        s = dt * st["speed"]
        s = np.where(_finite(s), s, zero)
        Pi = P[clip]
        fr = rate[clip] / Pi
        f = fr[:, 0]
        if variant != "rate_slot0":
            f = np.where(e1 != 0, f + e1 * (fr[:, 1] - f), f)
            f = np.where(e2 != 0, f + e2 * (fr[:, 2] - f), f)
        dphi = s * f
        ok0 = (st["phase"] >= 0) & (st["phase"] < 1)
        phi0 = np.where(ok0, st["phase"], zero)
        y = phi0 + dphi
        fl = np.floor(y)
        r = y - fl
        ok = (r >= 0) & (r < 1)
        phi = np.where(ok, r, zero)
        # 5. outputs
        pose = phi0 if variant == "pos_phi0" else phi
        x = pose[:, None] * Pi
        x0 = (phi if variant == "step_x_after" else phi0)[:, None] * Pi
        dx = dphi[:, None] * Pi
    if trace is not None:
        for name, m in (("reseed", ~_finite(st["px"]) | (two_d & ~_finite(st["py"]))), ("a_one", a == 1), ("wrap_fwd", ok & (fl >= 1)), ("wrap_back", ok & (fl <= -1)),
                        ("phase_fallback", ~ok)):
            trace[name] = trace.get(name, 0) + int(np.sum(m))
    e = np.stack([zero, e1, e2], axis=1)
    out = dict(phase=phi, px=px, py=py, speed=st["speed"])
    return out, dict(clip=clip, x=x, x0=x0, dx=dx, e=e, shares=sh, slots=sl, phi0=phi0, dphi=dphi)


def fields(states, fdt=F):
    return {k: states[k].astype(fdt) for k in STATE.names}


def advance(bs, states, params, dt, nlayers=0, layers=None, variant=None, trace=None):
    """one call on STATE records [n]: (stored states, LAYER [n, nlayers] or None, STEP [n, 3], float32 [n, 3] shares)"""
    out, fr = advance_fields(bs, fields(states), np.asarray(params, dtype=F), dt, F, variant, trace)
    n = states.shape[0]
    st = np.zeros(n, dtype=STATE)
    for k in ("phase", "px", "py"):
        st[k] = out[k]
    st["speed"] = states["speed"]  # never written: the bits stay
    ly = None
    if nlayers:
        ly = np.zeros((n, nlayers), dtype=LAYER) if layers is None else layers.copy()
        for i in range(3):
            ly["clip"][:, i], ly["x"][:, i], ly["w"][:, i], ly["mask"][:, i], ly["mode"][:, i] = fr["clip"][:, i], fr["x"][:, i], fr["e"][:, i], 0, 0
    sp = np.zeros((n, 3), dtype=STEP)
    sp["clip"], sp["x"], sp["dx"], sp["w"] = fr["clip"], fr["x0"], fr["dx"], fr["e"]
    return st, ly, sp, fr["shares"].astype(F)


def dense_shares(bs, px, py, fdt=F):
    """the shares of points as a vector over the samples, [n, K]: what each sample contributes"""
    px, py = np.asarray(px, dtype=fdt), np.asarray(py, dtype=fdt)
    sl, e1, e2 = find_slots(bs, px, py, fdt)
    sh = shares_of(e1, e2).astype(np.float64)
    out = np.zeros((px.shape[0], bs["samples"].size))
    for i in range(3):
        np.add.at(out, (np.arange(px.shape[0]), sl[:, i]), sh[:, i])
    return out


def same_bits(a, b):
    return pm.same_bits(a, b)


def same_result(a, b):
    """two lists of per-call results (states, layers, steps, shares)"""
    for ra, rb in zip(a, b):
        for xa, xb in zip(ra, rb):
            if (xa is None) != (xb is None) or (xa is not None and (xa.shape != xb.shape or not same_bits(xa, xb).all())):
                return False
    return True


# ---- the generator ------------------------------------------------------------------------------------------------------
COUNTS = pm.COUNTS
NAN, INF, DENORMAL, DT = pm.NAN, pm.INF, pm.DENORMAL, pm.DT
BIG = 1 << 24
CLIPSETS = (  # LOOP only: N of 1, 2, 30, 32 / 16 and 2^24
    pm.table([30], [LOOP], [30.0]),
    pm.table([32, 16], [LOOP, LOOP], [30.0, 30.0]),
    pm.table([1, 2, BIG], [LOOP, LOOP, LOOP], [30.0, -7.5, 1.0e6]),
    pm.table([30, 32, 16, 2], [LOOP, LOOP, LOOP, LOOP], [30.0, 32.0, 24.0, 3.0]),
)
DTS = pm.DTS
DAMPS = (INF, 4.0, DENORMAL, 30.0)
PHASE_EDGES = (-0.0, 1.0, 1e30, NAN, 0.99, 0.01, 0.5, 0.0)
SPEED_EDGES = pm.SPEED_EDGES + (-1e-9, 1e38)
P_EDGES = (NAN, INF, -INF, -0.0, DENORMAL, 1e30, -1e30)
GX, GY = (-0.7, 0.1, 1.3), (-1.1, 0.3, 0.9)  # not binary fractions: the products of the barycentric terms round
GRID = [(x, y) for y in GY for x in GX]
GRID_TRIS = [(0, 1, 4), (0, 4, 3), (1, 2, 5), (1, 5, 4), (3, 4, 7), (3, 7, 6), (4, 5, 8), (4, 8, 7)]
FAN = [(0.1, 0.2)] + [(0.1 + 1.3 * np.cos(k * np.pi / 4 + 0.3), 0.2 + 0.7 * np.sin(k * np.pi / 4 + 0.3)) for k in range(8)]
_rot = lambda t, r: t[r:] + t[:r]  # a different first vertex from triangle to triangle: a spoke is then v0-v1 of one, v1-v2 of the next
FAN_TRIS = [_rot((0, 1 + k, 1 + (k + 1) % 8), k % 3) for k in range(8)]
SPACES = (
    ("line1", [(0.5,)], None),
    ("line2", [(0.0,), (2.0,)], None),
    ("line5", [(-1.0,), (0.0,), (1.4,), (4.0,), (7.5,)], None),
    ("tri1", [(0.0, 0.0), (3.0, 0.5), (1.0, 2.0)], [(0, 1, 2)]),
    ("grid9", GRID, GRID_TRIS),
    ("fan9", FAN, FAN_TRIS),
)


def make_space(si, tab, nparams, damp):
    name, pts, tris = SPACES[si]
    C = len(tab[0])
    rows = [((k * 2 + 1) % C,) + tuple(p) for k, p in enumerate(pts)]
    return blend_set(tab, rows, tris, nparams=nparams, param_x=nparams - 1, param_y=0, damp=damp)


_CRACKS = {}


def crack_points(bs):
    """points of a 2-D space that no triangle holds in binary32 while one does in float64: found by a fixed search along the
    interior edges, [m, 2] float32 (possibly empty)"""
    key = bs["samples"].tobytes() + bs["tris"].tobytes()
    if key not in _CRACKS:
        sx, sy = bs["samples"]["px"].astype(np.float64), bs["samples"]["py"].astype(np.float64)
        edges = {}
        for v in bs["tris"]["v"]:
            for a, b in ((v[0], v[1]), (v[1], v[2]), (v[2], v[0])):
                edges.setdefault((min(a, b), max(a, b)), []).append(1)
        t = np.random.default_rng(77).uniform(0.02, 0.98, 1500)
        found = [np.zeros((0, 2), dtype=F)]
        for (a, b), uses in sorted(edges.items()):
            if len(uses) != 2:
                continue
            q = np.stack([sx[a] + t * (sx[b] - sx[a]), sy[a] + t * (sy[b] - sy[a])], axis=1).astype(F)
            tr = {}
            find_slots(bs, q[:, 0], q[:, 1], F, None, tr)
            if tr.get("fb_crack"):
                hit32 = _hit32(bs, q[:, 0], q[:, 1])
                found.append(q[~hit32 & _hit64(bs, q[:, 0], q[:, 1])])
        _CRACKS[key] = np.concatenate(found)
    return _CRACKS[key]


def _hit32(bs, px, py):
    _, _, sx, sy, tris = _tables(bs, F)
    hit = np.zeros(px.shape[0], dtype=bool)
    one = F(1)
    with np.errstate(all="ignore"):
        for v in tris:
            x0, y0, x1, y1, x2, y2 = sx[v[0]], sy[v[0]], sx[v[1]], sy[v[1]], sx[v[2]], sy[v[2]]
            A = area2(x0, y0, x1, y1, x2, y2)
            qx, qy = px - x0, py - y0
            l1 = (qx * (y2 - y0) - (x2 - x0) * qy) / A
            l2 = ((x1 - x0) * qy - qx * (y1 - y0)) / A
            hit |= ((one - l1) - l2 >= 0) & (l1 >= 0) & (l2 >= 0)
    return hit


def make_params(rng, n, bs, call):
    """parameter rows [n, NP]: per lane a point at a sample, on an edge, inside, outside each side of the hull, far outside,
    on a shared edge, in a crack, or a special value; the unused columns hold noise"""
    NP, s, t = bs["nparams"], bs["samples"], bs["tris"]
    pr = rng.uniform(-9, 9, (n, NP)).astype(F)
    K = s.size
    sx, sy = s["px"].astype(np.float64), s["py"].astype(np.float64)
    lo, hi = np.array([sx.min(), sy.min()]), np.array([sx.max(), sy.max()])
    ext = np.maximum(hi - lo, 1.0)
    pts = np.zeros((n, 2))
    cracks = crack_points(bs) if t.size else np.zeros((0, 2), dtype=F)
    for i in range(n):
        kind = (i + 3 * call) % 12
        k = int(rng.integers(0, K))
        if kind == 0:                                   # at a sample
            pts[i] = sx[k], sy[k]
        elif kind == 1 and t.size:                      # on an edge of a triangle
            v = t["v"][int(rng.integers(0, t.size))]
            a, b, u = int(v[i % 3]), int(v[(i + 1) % 3]), (i % 5) / 4.0
            pts[i] = sx[a] + u * (sx[b] - sx[a]), sy[a] + u * (sy[b] - sy[a])
        elif kind == 2 and t.size:                      # exactly at v2, v1 or v0 of a triangle
            v = t["v"][int(rng.integers(0, t.size))]
            pts[i] = sx[int(v[2 - i % 3])], sy[int(v[2 - i % 3])]
        elif kind in (3, 4, 5, 6):                      # outside, one side each
            inside = lo + rng.uniform(0.1, 0.9, 2) * (hi - lo)
            side = kind - 3
            inside[side % 2] = (lo - 0.7 * ext)[side % 2] if side < 2 else (hi + 0.7 * ext)[side % 2]
            pts[i] = inside
        elif kind == 7:                                 # far outside
            pts[i] = rng.choice([1e30, -1e30, 3e38]), rng.choice([1e30, -1e30, 0.0])
        elif kind == 8 and len(cracks):                 # in a rounding crack
            pts[i] = cracks[int(rng.integers(0, len(cracks)))]
        elif kind == 9:                                 # a special value in x, in y or in both
            pts[i] = lo + rng.uniform(0, 1, 2) * (hi - lo)
            e = P_EDGES[int(rng.integers(0, len(P_EDGES)))]
            if i % 3 != 1:
                pts[i, 0] = e
            if i % 3 != 0:
                pts[i, 1] = P_EDGES[int(rng.integers(0, len(P_EDGES)))]
        else:                                           # inside the hull's box
            pts[i] = lo + rng.uniform(0, 1, 2) * (hi - lo)
    with np.errstate(all="ignore"):
        pr[:, bs["param_x"]] = pts[:, 0].astype(F)
        if t.size:
            pr[:, bs["param_y"]] = pts[:, 1].astype(F)
    return pr


def make_states(rng, n, bs):
    st = np.zeros(n, dtype=STATE)
    pick = lambda edges, normal: np.where(rng.random(n) < 0.4, rng.choice(np.array(edges, dtype=F), n), normal.astype(F))
    st["phase"] = pick(PHASE_EDGES, rng.uniform(0, 1, n))
    st["px"] = pick((NAN, INF, 0.3, -0.0), rng.uniform(-1, 2, n))
    st["py"] = pick((NAN, -INF, 0.3, DENORMAL), rng.uniform(-1, 2, n))
    st["speed"] = pick(SPEED_EDGES, rng.uniform(0.5, 1.5, n))
    # scripted rows, as far as n reaches: a forward wrap, a backward wrap, a tiny negative step from 0 (y - floor(y) rounds to 1:
    # the fallback), a step that overflows
    script = [(0.99, 1.5), (0.01, -1.5), (0.0, -1e-9), (0.5, 1e38)]
    for i, (ph, spd) in enumerate(script[:n]):
        k = (i * 7 + 3) % n if n >= 64 else i
        st["phase"][k], st["speed"][k] = ph, spd
    return st


_CASES = None


def cases():
    """every case: name, n, set, states (STATE [n]), calls (three (dt, params [n, NP]) pairs), nlayers, layers (LAYER [n, nlayers]
    sentinels).  Deterministic."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    k = 0
    for n in COUNTS:
        for si in range(len(SPACES)):
            rng = np.random.default_rng(2300 + k)
            tab = CLIPSETS[k % len(CLIPSETS)]
            bs = make_space(si, tab, nparams=(k % 3) + 2 if k % 7 else 16, damp=DAMPS[k % len(DAMPS)])
            assert check_set(bs) is None, (SPACES[si][0], check_set(bs))
            dts = (DTS[k % len(DTS)], DTS[(k + 3) % len(DTS)], DT)
            nl = (3, 8, 5)[k % 3]
            ly = np.frombuffer(rng.bytes(n * nl * 16), dtype=LAYER).reshape(n, nl).copy()
            calls = [(dts[c], make_params(rng, n, bs, c)) for c in range(3)]
            out.append(dict(name=f"n{n}_{SPACES[si][0]}", n=n, set=bs, states=make_states(rng, n, bs), calls=calls, nlayers=nl, layers=ly))
            k += 1
    _CASES = out
    return out


def run_case(c, variant=None, trace=None, ncalls=3):
    """the model over the first ncalls calls of a case: a list of (states, LAYER, STEP, shares) after each; the layer array is
    carried from call to call as a caller's buffer would be"""
    st, ly, res = c["states"], c["layers"], []
    for dt, params in c["calls"][:ncalls]:
        st, ly, sp, sh = advance(c["set"], st, params, dt, c["nlayers"], ly, variant, trace)
        res.append((st, ly, sp, sh))
    return res


def census():
    """({branch: number of cases that reach it}, {variant: number of cases it changes}, number of cases)"""
    reach, told = {b: 0 for b in BRANCHES}, {v: 0 for v in WRONG_VARIANTS}
    cs = cases()
    for c in cs:
        tr = {}
        want = run_case(c, trace=tr)
        for b in BRANCHES:
            reach[b] += bool(tr.get(b))
        for v in WRONG_VARIANTS:
            told[v] += not same_result(run_case(c, variant=v), want)
    return reach, told, len(cs)
