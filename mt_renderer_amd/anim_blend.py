"""Sample points of a blend space (SPEC.md section 23) turned into the arrays mtr_anim_blend_create takes, and the shares of a
point for hosts that want a preview.  Helpers, not part of the rule: the rule is what the arrays say.

    IDLE, WALK, RUN = 0, 1, 2
    samples = build_1d([(0.0, IDLE), (1.4, WALK), (4.0, RUN)])                        # speed
    samples, tris = build_2d([(0, 0, IDLE), (0, 1.4, WALK), (1, 0, STRAFE_R), ...])  # (strafe, forward)
    blend = api.AnimBlend(dev, nkeys, rates, clip_flags, samples, tris, nparams=2, param_x=0, param_y=1, damp=8.0, max_instances=n)
    shares(samples, tris, (0.3, 0.9))   # -> float32 [K], what each sample contributes at that point

build_1d sorts the points by position.  build_2d keeps the order given, triangulates the points (Delaunay by a float64
Bowyer-Watson in numpy alone), orients every triangle counter-clockwise and keeps only the triangles whose doubled area is
finite and > 0 in the binary32 expression of the rule, so that what it returns always passes creation.  Two points that are
equal in binary32, fewer than three points, and a set without any such triangle (all points on a line) are errors.  A sliver
the area test drops leaves a gap of no width that the rule's closest-edge fallback covers."""
import numpy as np

from . import api

F = np.float32


def _bad(msg):
    return api.MtrError(api.MTR_E_INVALID, "anim blend build: " + msg)


def build_1d(points):
    """[(px, clip), ...] -> BLEND_SAMPLE [K], sorted by px, which must be finite and distinct in binary32"""
    rows = [tuple(r) for r in points]
    if not rows or len(rows) > 32 or any(len(r) != 2 for r in rows):
        raise _bad("1 to 32 points (px, clip)")
    s = np.zeros(len(rows), dtype=api.BLEND_SAMPLE)
    s["px"] = [r[0] for r in rows]
    s["clip"] = [r[1] for r in rows]
    if not np.isfinite(s["px"]).all():
        raise _bad("a position is not finite")
    s = s[np.argsort(s["px"], kind="stable")]
    with np.errstate(all="ignore"):
        step = s["px"][1:] - s["px"][:-1]
    if not ((step > 0) & np.isfinite(step)).all():
        raise _bad("two points share a position, or lie further apart than binary32 holds")
    return np.ascontiguousarray(s)


def area2(x0, y0, x1, y1, x2, y2):
    """the doubled area of the rule: binary32, (x1-x0)*(y2-y0) - (x2-x0)*(y1-y0), each operator rounded once"""
    x0, y0, x1, y1, x2, y2 = (np.asarray(v, dtype=F) for v in (x0, y0, x1, y1, x2, y2))
    with np.errstate(all="ignore"):
        return (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)


def _in_circle(P, t, q):
    a, b, c = P[t[0]] - q, P[t[1]] - q, P[t[2]] - q
    det = ((a[0] * a[0] + a[1] * a[1]) * (b[0] * c[1] - c[0] * b[1]) - (b[0] * b[0] + b[1] * b[1]) * (a[0] * c[1] - c[0] * a[1])
           + (c[0] * c[0] + c[1] * c[1]) * (a[0] * b[1] - b[0] * a[1]))
    return det > 0  # t is counter-clockwise


def _ccw(P, t):
    a, b, c = P[t[0]], P[t[1]], P[t[2]]
    return t if (b[0] - a[0]) * (c[1] - a[1]) - (c[0] - a[0]) * (b[1] - a[1]) > 0 else (t[0], t[2], t[1])


def _bowyer_watson(pts):
    """float64 [K, 2] -> a list of index triples.  The points are nudged by 1e-7 of their extent (a fixed sequence) for the
    circle tests only, which breaks the ties of points on one circle or one line."""
    K = len(pts)
    lo, hi = pts.min(0), pts.max(0)
    ext = max(float((hi - lo).max()), 1e-30)
    P = pts + np.random.default_rng(23).uniform(-1e-7, 1e-7, pts.shape) * ext
    c, r = (lo + hi) / 2, ext * 1e4
    P = np.vstack([P, [c[0] - 2 * r, c[1] - r], [c[0] + 2 * r, c[1] - r], [c[0], c[1] + 2 * r]])
    tris = [(K, K + 1, K + 2)]
    for i in range(K):
        bad = [t for t in tris if _in_circle(P, t, P[i])]
        count = {}
        for t in bad:
            for e in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
                key = (min(e), max(e))
                count[key] = count.get(key, 0) + 1
        tris = [t for t in tris if t not in bad] + [_ccw(P, (a, b, i)) for (a, b), k in sorted(count.items()) if k == 1]
    return [t for t in tris if max(t) < K]


def build_2d(points):
    """[(px, py, clip), ...] -> (BLEND_SAMPLE [K] in the order given, BLEND_TRI [T])"""
    rows = [tuple(r) for r in points]
    if len(rows) < 3 or len(rows) > 32 or any(len(r) != 3 for r in rows):
        raise _bad("3 to 32 points (px, py, clip)")
    s = np.zeros(len(rows), dtype=api.BLEND_SAMPLE)
    s["px"] = [r[0] for r in rows]
    s["py"] = [r[1] for r in rows]
    s["clip"] = [r[2] for r in rows]
    if not (np.isfinite(s["px"]).all() and np.isfinite(s["py"]).all()):
        raise _bad("a position is not finite")
    if len({(float(x), float(y)) for x, y in zip(s["px"], s["py"])}) != len(rows):
        raise _bad("two points share a position")
    x, y = s["px"], s["py"]
    keep = []
    for t in sorted(_bowyer_watson(np.stack([x, y], axis=1).astype(np.float64))):
        for cand in (t, (t[0], t[2], t[1])):  # whichever orientation the binary32 expression calls counter-clockwise
            A = area2(x[cand[0]], y[cand[0]], x[cand[1]], y[cand[1]], x[cand[2]], y[cand[2]])
            if A > 0 and np.isfinite(A):
                keep.append(cand)
                break
    if not keep:
        raise _bad("no triangle with an area: the points lie on one line")
    if len(keep) > 64:
        raise _bad("more than 64 triangles")
    tris = np.zeros(len(keep), dtype=api.BLEND_TRI)
    tris["v"] = np.asarray(keep, dtype=np.uint32)
    return np.ascontiguousarray(s), tris


def shares(samples, tris, point):
    """what each sample contributes at `point` (a float in 1-D, (x, y) in 2-D): float64 [K], summing to 1.  A preview in float64
    of step 3 of the rule (bracket, first triangle that holds the point, closest edge otherwise), not its binary32 twin."""
    s = np.asarray(samples)
    K = s.size
    out = np.zeros(K)
    if tris is None or len(tris) == 0:
        p, xs = float(point), s["px"].astype(np.float64)
        if not p > xs[0]:
            out[0] = 1
        elif p >= xs[-1]:
            out[-1] = 1
        else:
            j = int(np.flatnonzero(xs[:-1] <= p)[-1])
            e = (p - xs[j]) / (xs[j + 1] - xs[j])
            out[j], out[j + 1] = 1 - e, e
        return out
    px, py = float(point[0]), float(point[1])
    X, Y = s["px"].astype(np.float64), s["py"].astype(np.float64)
    for v in np.asarray(tris)["v"]:
        a, b, c = (int(i) for i in v)
        A = (X[b] - X[a]) * (Y[c] - Y[a]) - (X[c] - X[a]) * (Y[b] - Y[a])
        l1 = ((px - X[a]) * (Y[c] - Y[a]) - (X[c] - X[a]) * (py - Y[a])) / A
        l2 = ((X[b] - X[a]) * (py - Y[a]) - (px - X[a]) * (Y[b] - Y[a])) / A
        l0 = 1 - l1 - l2
        if l0 >= 0 and l1 >= 0 and l2 >= 0:
            out[a] += l0; out[b] += l1; out[c] += l2
            return out
    best = (np.inf, int(np.asarray(tris)["v"][0][0]), int(np.asarray(tris)["v"][0][0]), 0.0)
    for v in np.asarray(tris)["v"]:
        for a, b in ((int(v[0]), int(v[1])), (int(v[1]), int(v[2])), (int(v[2]), int(v[0]))):
            ex, ey = X[b] - X[a], Y[b] - Y[a]
            t = min(max(((px - X[a]) * ex + (py - Y[a]) * ey) / (ex * ex + ey * ey), 0.0), 1.0)
            d2 = (px - X[a] - t * ex) ** 2 + (py - Y[a] - t * ey) ** 2
            if d2 < best[0]:
                best = (d2, a, b, t)
    out[best[1]] += 1 - best[3]
    out[best[2]] += best[3]
    return out
