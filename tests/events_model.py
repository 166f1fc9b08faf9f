"""The numpy model of SPEC.md section 22 (animation events), written from that text: per instance and step the weight E_i, the
direction, the one or two intervals of the clip's sorted markers that the position arrives at or passes, and the list in
(instance, step, firing order) with its two counts and the per-instance masks.  binary32 throughout, one rounded operation per
numpy operation; NaN compares false.  `collect` is vectorised over instances with np.searchsorted; `brute` is its twin that
tests every marker of a clip against the interval rule one by one, the comparisons in exact rationals.  Also the generator of
cases that the CPU tests, the host build of csrc/event_math.h and the GPU tests share, a table of wrong readings of the text
(WRONG_VARIANTS) that the cases must be able to tell apart, and the census of the branches the cases reach."""
from fractions import Fraction

import numpy as np

from tests import player_model as pm

F = np.float32
MARKER = np.dtype([("x", "<f4"), ("id", "<u4")])
EVENT = np.dtype([("instance", "<u4"), ("id", "<u4"), ("where", "<u4"), ("w", "<f4")])
STEP = pm.STEP
BACKWARD = 0x80000000

WRONG_VARIANTS = ("half_open_fwd", "seam_ignored", "period_n1", "ties_reversed", "e_without_later", "bits_ored", "step_major")
BRANCHES = ("fwd_seam", "back_seam", "t_eq_P", "full_fwd", "full_back", "end_clamp", "drop_e0", "drop_minw", "truncated")


def event_set(tab, markers):
    """tab: a player set of pm (key counts, flag words, ...); markers: {clip: [(x, id), ...]} -> the set: counts, firsts and the
    MARKER array, each clip's markers sorted stably by x"""
    C = len(tab[0])
    counts = np.zeros(C, dtype=np.int64)
    parts = []
    for c in range(C):
        rows = list(markers.get(c, ()))
        m = np.zeros(len(rows), dtype=MARKER)
        m["x"], m["id"] = [r[0] for r in rows], [r[1] for r in rows]
        parts.append(m[np.argsort(m["x"], kind="stable")])
        counts[c] = len(rows)
    mk = np.concatenate(parts) if parts else np.zeros(0, dtype=MARKER)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    # for the wrong reading "ties_reversed": the index a marker swaps places with inside its run of equal positions
    mirror = np.arange(len(mk))
    for c in range(C):
        lo = int(first[c])
        while lo < first[c] + counts[c]:
            hi = lo
            while hi < first[c] + counts[c] and mk["x"][hi] == mk["x"][lo]:
                hi += 1
            mirror[lo:hi] = np.arange(lo, hi)[::-1]
            lo = hi
    return dict(tab=tab, counts=counts, first=first, markers=np.ascontiguousarray(mk), mirror=mirror)


def periods(es, variant=None):
    nkeys, flags = np.asarray(es["tab"][0], dtype=np.int64), np.asarray(es["tab"][1], dtype=np.int64)
    loop = (flags & pm.LOOP) != 0
    return np.where(loop & (variant != "period_n1"), nkeys, nkeys - 1).astype(F), loop


def weights(steps, min_weight, variant=None):
    """E [n, S] and which steps fire at all [n, S]; and the two reasons a step is dropped for"""
    n, S = steps.shape
    e = pm.clamp_w(steps["w"].astype(F))
    e[:, 0] = F(1)
    E = np.zeros((n, S), dtype=F)
    one = np.ones(n, dtype=F)
    for i in range(S):
        p = e[:, i].copy()
        if variant != "e_without_later":
            for j in range(i + 1, S):
                p = p * (one - e[:, j])
        E[:, i] = p
    e0 = e == 0
    e0[:, 0] = False
    with np.errstate(all="ignore"):
        passes = E >= F(min_weight)
    return E, ~e0 & passes, e0, ~e0 & ~passes


def spans(es, steps, live, variant=None, trace=None):
    """per (instance, step, part) the marker range [lo, hi) and per (instance, step) the backward flag and the clamped clip"""
    n, S = steps.shape
    C = len(es["counts"])
    P_t, loop_t = periods(es, variant)
    clip = np.minimum(steps["clip"].astype(np.int64), C - 1)
    x, dx = steps["x"].astype(F), steps["dx"].astype(F)
    with np.errstate(all="ignore"):
        fwd, back = live & (dx > 0), live & (dx < 0)
    lo = np.zeros((n, S, 2), dtype=np.int64)
    hi = np.zeros((n, S, 2), dtype=np.int64)
    tr = {k: np.zeros((n, S), dtype=bool) for k in ("fwd_seam", "back_seam", "t_eq_P", "full_fwd", "full_back", "end_clamp")}
    up_side = "left" if variant == "half_open_fwd" else "right"
    for c in range(C):
        sel = (clip == c) & (fwd | back)
        cnt = int(es["counts"][c])
        if not sel.any() or cnt == 0:
            continue
        xs = es["markers"]["x"][es["first"][c]:es["first"][c] + cnt]
        upper = lambda v: np.searchsorted(xs, v, side=up_side)   # how many markers do not lie above v
        lower = lambda v: np.searchsorted(xs, v, side="left")    # how many lie below v
        P = P_t[c]
        xx, dd, f_ = x[sel], dx[sel], fwd[sel]
        zero = np.zeros_like(xx)
        l0, h0, l1, h1 = (np.zeros(xx.shape, dtype=np.int64) for _ in range(4))
        with np.errstate(all="ignore"):
            if not loop_t[c]:
                a = np.where(xx >= 0, xx, zero)
                a = np.where(a > P, P, a)
                y = xx + dd
                b = np.where(y >= 0, y, zero)
                b = np.where(b > P, P, b)
                l0 = np.where(f_, upper(a), lower(b))
                h0 = np.where(f_, upper(b), lower(a))
                tr["end_clamp"][sel] = f_ & (y > P) & (a < P)
            else:
                r = xx - np.floor(xx / P) * P
                r0 = np.where((r >= 0) & (r < P), r, zero)
                y = r0 + dd
                full = np.abs(dd) >= P
                seam_f = f_ & ~full & ~(y < P)
                seam_b = ~f_ & ~full & ~(y >= 0)
                t = y + P
                k_f, k_b = upper(r0), lower(r0)
                # forward: (r0, y], or (r0, ..) then (.., y - P]; backward: [y, r0), or (.., r0) then [t, ..)
                l0 = np.where(f_, k_f, np.where(full | seam_b, 0, lower(y)))
                h0 = np.where(f_, np.where(full | seam_f, cnt, upper(y)), k_b)
                l1 = np.where(f_, 0, np.where(full, k_b, np.where(seam_b, lower(t), 0)))
                h1 = np.where(f_, np.where(full, k_f, np.where(seam_f, upper(y - P), 0)), np.where(full | seam_b, cnt, 0))
                if variant == "seam_ignored":
                    h0 = np.where(seam_f, upper(y), h0)
                    l0 = np.where(seam_b, lower(y), l0)
                    l1, h1 = np.where(seam_f | seam_b, 0, l1), np.where(seam_f | seam_b, 0, h1)
                tr["fwd_seam"][sel], tr["back_seam"][sel] = seam_f, seam_b
                tr["t_eq_P"][sel] = seam_b & (t == P)
                tr["full_fwd"][sel], tr["full_back"][sel] = f_ & full, ~f_ & full
        h0, h1 = np.maximum(h0, l0), np.maximum(h1, l1)  # an inverted interval is empty
        base = int(es["first"][c])
        lo[sel, 0], hi[sel, 0], lo[sel, 1], hi[sel, 1] = l0 + base, h0 + base, l1 + base, h1 + base
    if trace is not None:
        trace.update(tr)
    return lo, hi, back, clip


def collect(es, steps, min_weight, capacity, out_prev=None, bits_prev=None, variant=None, trace=None):
    """one call on STEP [n, S]: (EVENT [capacity] -- out_prev behind the records written --, uint32 [2], uint32 [n])"""
    steps = np.asarray(steps)
    n, S = steps.shape
    E, live, drop_e0, drop_mw = weights(steps, min_weight, variant)
    tr = {}
    lo, hi, back, clip = spans(es, steps, live, variant, tr)
    where = (clip | (np.arange(S, dtype=np.int64)[None, :] << 24) | np.where(back, BACKWARD, 0)).astype(np.uint32)
    inst = np.broadcast_to(np.arange(n, dtype=np.uint32)[:, None], (n, S))
    order = (1, 0, 2) if variant == "step_major" else (0, 1, 2)
    flat = lambda a3: np.ascontiguousarray(np.transpose(a3, order)).reshape(-1)
    rep2 = lambda a2: flat(np.repeat(a2[:, :, None], 2, axis=2))
    lo_f, hi_f = flat(lo), flat(hi)
    cnt = hi_f - lo_f
    total = int(cnt.sum())
    owner = np.repeat(np.arange(cnt.size), cnt)
    pos = np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    bk = rep2(back)[owner]
    idx = np.where(bk, hi_f[owner] - 1 - pos, lo_f[owner] + pos)
    if variant == "ties_reversed":
        idx = np.where(bk, idx, es["mirror"][idx])
    ev = np.zeros(total, dtype=EVENT)
    ev["instance"], ev["id"], ev["where"], ev["w"] = rep2(inst)[owner], es["markers"]["id"][idx], rep2(where)[owner], rep2(E)[owner]
    written = min(total, capacity)
    out = np.zeros(capacity, dtype=EVENT) if out_prev is None else np.array(out_prev, dtype=EVENT).reshape(capacity)
    out[:written] = ev[:written]
    bits = np.zeros(n, dtype=np.uint32)
    np.bitwise_or.at(bits, ev["instance"], (np.uint32(1) << (ev["id"] & np.uint32(31))).astype(np.uint32))
    if variant == "bits_ored" and bits_prev is not None:
        bits |= np.asarray(bits_prev, dtype=np.uint32)
    if trace is not None:
        trace.update({k: bool(v.any()) for k, v in tr.items()})
        trace.update(drop_e0=bool(drop_e0.any()), drop_minw=bool(drop_mw.any()), truncated=total > capacity, fired=total)
    return out, np.array([total, written], dtype=np.uint32), bits


def end_position(es, steps):
    """where the rule ends on a LOOP clip with |dx| < P, per (instance, step): y, y - P across the forward seam, or t = y + P
    across the backward one with the fallback to 0 -- for a start inside [0, P) the x' that section 20 stores.  NaN elsewhere."""
    steps = np.asarray(steps)
    C = len(es["counts"])
    P_t, loop_t = periods(es)
    clip = np.minimum(steps["clip"].astype(np.int64), C - 1)
    P, x, dx = P_t[clip], steps["x"].astype(F), steps["dx"].astype(F)
    zero = np.zeros_like(x)
    with np.errstate(all="ignore"):
        r = x - np.floor(x / P) * P
        r0 = np.where((r >= 0) & (r < P), r, zero)
        y = r0 + dx
        t = y + P
        t = np.where((t >= 0) & (t < P), t, zero)
        end = np.where(y < 0, t, np.where(y < P, y, y - P))
        return np.where(loop_t[clip] & (np.abs(dx) < P), end, F(NAN)).astype(F), r0, y


# ---- the brute-force twin ---------------------------------------------------------------------------------------------------
def _clamp(v, P):
    r = v if v >= 0 else F(0)
    return P if r > P else r


def brute(es, steps, min_weight, capacity, out_prev=None, bits_prev=None):
    """the same call instance by instance, step by step, marker by marker: each marker of the step's clip is tested against the
    interval rule with exact rational comparisons, in array order forward and in reverse order backward"""
    steps = np.asarray(steps)
    n, S = steps.shape
    C = len(es["counts"])
    P_t, loop_t = periods(es)
    mw = F(min_weight)
    fr = [[(Fraction(float(m["x"])), int(m["id"])) for m in es["markers"][es["first"][c]:es["first"][c] + es["counts"][c]]] for c in range(C)]
    events, bits = [], np.zeros(n, dtype=np.uint32)
    Q = lambda v: Fraction(float(v))
    with np.errstate(all="ignore"):
        for inst in range(n):
            e = [F(1)] + [F(pm.clamp_w(np.array([steps["w"][inst, i]], dtype=F))[0]) for i in range(1, S)]
            for i in range(S):
                p = e[i]
                for j in range(i + 1, S):
                    p = F(p * F(F(1) - e[j]))
                if (i >= 1 and e[i] == 0) or not (p >= mw):
                    continue
                c = min(int(steps["clip"][inst, i]), C - 1)
                x, dx, P = F(steps["x"][inst, i]), F(steps["dx"][inst, i]), P_t[c]
                if not (dx > 0 or dx < 0):
                    continue
                fwd = bool(dx > 0)
                # the parts of the step, each (above, or_equal, below, or_equal): above < m (<=) and m < below (<=); None: no bound
                if not loop_t[c]:
                    a, b = _clamp(x, P), _clamp(F(x + dx), P)
                    parts = [(Q(a), False, Q(b), True)] if fwd else [(Q(b), True, Q(a), False)]
                else:
                    r = F(x - F(F(np.floor(F(x / P))) * P))
                    r0 = r if (r >= 0 and r < P) else F(0)
                    y = F(r0 + dx)
                    if abs(dx) >= P:
                        parts = [(Q(r0), False, None, False), (None, False, Q(r0), True)] if fwd else [(None, False, Q(r0), False), (Q(r0), True, None, False)]
                    elif fwd:
                        parts = [(Q(r0), False, Q(y), True)] if y < P else [(Q(r0), False, None, False), (None, False, Q(F(y - P)), True)]
                    else:
                        parts = [(Q(y), True, Q(r0), False)] if y >= 0 else [(None, False, Q(r0), False), (Q(F(y + P)), True, None, False)]
                where = c | (i << 24) | (0 if fwd else BACKWARD)
                for above, a_eq, below, b_eq in parts:
                    for mx, mid in (fr[c] if fwd else reversed(fr[c])):
                        if above is not None and not (mx > above or (a_eq and mx == above)):
                            continue
                        if below is not None and not (mx < below or (b_eq and mx == below)):
                            continue
                        events.append((inst, mid, where, p))
                        bits[inst] |= np.uint32(1 << (mid & 31))
    total = len(events)
    written = min(total, capacity)
    out = np.zeros(capacity, dtype=EVENT) if out_prev is None else np.array(out_prev, dtype=EVENT).reshape(capacity)
    for k in range(written):
        out[k] = events[k]
    return out, np.array([total, written], dtype=np.uint32), bits


def same_bits(a, b):
    return pm.same_bits(a, b)


def same_result(a, b):
    return all(x.shape == y.shape and same_bits(x, y).all() for x, y in zip(a, b))


# ---- the generator ------------------------------------------------------------------------------------------------------
COUNTS = pm.COUNTS
NAN, INF, DENORMAL = float("nan"), float("inf"), 1e-41
STEP_COUNTS = (1, 2, 8)
MIN_WEIGHTS = (0.0, 0.5, 0.0, 1.0, 0.0, NAN)
W_EDGES = (0.0, 1.0, NAN, 1.5, 0.5, 0.25)
KINDS = ("empty", "at_zero", "ties", "at_end", "many")


def pred(v):
    return F(np.nextafter(F(v), F(-INF)))


def succ(v):
    return F(np.nextafter(F(v), F(INF)))


def make_markers(rng, kind, P, loop):
    """one clip's list of (x, id) of the named kind, valid for the clip: inside [0, P) on a LOOP clip, [0, P] otherwise"""
    P = F(P)
    top = pred(P) if loop else P  # the last position a marker may have
    rid = lambda: int(rng.integers(0, 1 << 32))
    inside = lambda u: F(min(max(F(u * float(P)), F(0)), top))
    if kind == "empty":
        return []
    if kind == "at_zero":
        return [(F(0), rid())]
    if kind == "ties":
        t = inside(0.4)
        return [(inside(0.1), rid()), (t, 1), (t, 2), (t, 3), (inside(0.9), rid()), (top, 4), (top, 5)]
    if kind == "at_end":
        return [(inside(0.25), rid()), (inside(0.7), rid()), (top, rid())]
    return [(inside((k + 0.5) / 65.0), rid() if k % 3 else k) for k in range(65)]  # 65: a search takes more than six turns


def make_steps(rng, n, S, es):
    C = len(es["counts"])
    P_t, loop_t = periods(es)
    st = np.zeros((n, S), dtype=STEP)
    clip = np.where(rng.random((n, S)) < 0.15, rng.choice([C, 0xFFFFFFFF], (n, S)), rng.integers(0, C, (n, S)))
    st["clip"] = clip
    cc = np.minimum(clip, C - 1)
    P = P_t[cc]
    # positions: the special values, a marker of the clip and its two neighbours, the ends of the clip, or anywhere inside
    x = (rng.random((n, S)) * P.astype(np.float64)).astype(F)
    has = es["counts"][cc] > 0
    mk = es["markers"]["x"][np.minimum(es["first"][cc] + (rng.integers(0, 1 << 30, (n, S)) % np.maximum(es["counts"][cc], 1)), max(len(es["markers"]) - 1, 0))] \
        if len(es["markers"]) else np.zeros((n, S), dtype=F)
    u = rng.random((n, S))
    for lo_, hi_, val in ((0.00, 0.03, F(-0.0)), (0.03, 0.06, F(-1e-7)), (0.06, 0.09, F(1e30)), (0.09, 0.12, F(NAN))):
        x = np.where((u >= lo_) & (u < hi_), val, x)
    x = np.where((u >= 0.12) & (u < 0.20) & has, mk, x)
    x = np.where((u >= 0.20) & (u < 0.25) & has, np.nextafter(mk, F(-INF)), x)
    x = np.where((u >= 0.25) & (u < 0.30) & has, np.nextafter(mk, F(INF)), x)
    x = np.where((u >= 0.30) & (u < 0.38), P - F(0.1), x)
    x = np.where((u >= 0.38) & (u < 0.44), F(0.05), x)
    st["x"] = x.astype(F)
    dx = rng.uniform(-2, 2, (n, S)).astype(F)
    v = rng.random((n, S))
    edges = [F(0.0), F(-0.0), F(NAN), F(INF), F(-INF), F(DENORMAL), F(-DENORMAL), F(0.37), F(-0.37)]
    for k, val in enumerate(edges):
        dx = np.where((v >= 0.03 * k) & (v < 0.03 * (k + 1)), val, dx)
    b = 0.03 * len(edges)
    pp, sp = np.nextafter(P, F(-INF)), np.nextafter(P, F(INF))
    for k, val in enumerate((pp, -pp, P, -P, sp, -sp)):
        dx = np.where((v >= b + 0.03 * k) & (v < b + 0.03 * (k + 1)), val, dx)
    st["dx"] = dx.astype(F)
    w = rng.uniform(0, 1, (n, S)).astype(F)
    st["w"] = np.where(rng.random((n, S)) < 0.5, rng.choice(np.array(W_EDGES, dtype=F), (n, S)), w)
    # scripted rows on the first LOOP clip, as far as n reaches: a forward and a backward seam, the tiny negative y whose t rounds
    # to P, a full cycle each way; on the first one-shot clip: into the end and beyond
    loops, shots = np.flatnonzero(loop_t), np.flatnonzero(~loop_t)
    script = []
    if len(loops):
        c, Pc = int(loops[0]), P_t[loops[0]]
        script += [(c, Pc - F(0.1), 0.37), (c, 0.05, -0.37), (c, -0.0, -DENORMAL), (c, 0.3, float(Pc)), (c, 0.3, -INF)]
    if len(shots):
        c, Pc = int(shots[0]), P_t[shots[0]]
        script += [(c, Pc - F(0.1), 0.37), (c, float(Pc), 0.37)]
    for i, (c, xv, dv) in enumerate(script[:n]):
        k = (i * 7 + 3) % n if n >= 64 else i
        st["clip"][k, 0], st["x"][k, 0], st["dx"][k, 0] = c, xv, dv
    return st


_CASES = None


def cases():
    """every case: name, n, S, set (event_set), steps (STEP [n, S]), min_weight, capacity, out_prev (EVENT [capacity] sentinels),
    bits_prev (uint32 [n]).  Deterministic."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out, k = [], 0
    for n in COUNTS:
        for si, tab in enumerate(pm.CLIPSETS):
            rng = np.random.default_rng(2200 + k)
            P_t, loop_t = ctrl_periods(tab)
            C = len(tab[0])
            kinds = [KINDS[(k + 2 * j + (k // 6)) % len(KINDS)] for j in range(C)]
            es = event_set(tab, {j: make_markers(rng, kinds[j], P_t[j], loop_t[j]) for j in range(C)})
            S = STEP_COUNTS[(k + k // 6) % 3]
            steps = make_steps(rng, n, S, es)
            mw = MIN_WEIGHTS[(k + k // 6) % len(MIN_WEIGHTS)]
            fired = int(collect(es, steps, mw, 0)[1][0])
            mode = (k // 2) % 3  # 0: no list, 1: one short of the total, 2: ample
            cap = 0 if mode == 0 else max(fired - 1, 0) if mode == 1 else fired + 9
            prev = np.frombuffer(rng.bytes(cap * 16), dtype=EVENT).copy()
            out.append(dict(name=f"n{n}_set{si}_s{S}", n=n, S=S, set=es, steps=steps, min_weight=mw, capacity=cap, out_prev=prev,
                            bits_prev=rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), kinds=kinds))
            k += 1
    _CASES = out
    return out


def ctrl_periods(tab):
    nkeys, flags = np.asarray(tab[0], dtype=np.int64), np.asarray(tab[1], dtype=np.int64)
    loop = (flags & pm.LOOP) != 0
    return np.where(loop, nkeys, nkeys - 1).astype(F), loop


def run_case(c, variant=None, trace=None, fn=collect):
    if fn is brute:
        return brute(c["set"], c["steps"], c["min_weight"], c["capacity"], c["out_prev"], c["bits_prev"])
    return collect(c["set"], c["steps"], c["min_weight"], c["capacity"], c["out_prev"], c["bits_prev"], variant, trace)


def census():
    """(in how many cases each branch is reached, in how many cases each wrong variant changes something), from the model alone"""
    reach = {k: 0 for k in BRANCHES}
    changed = {v: 0 for v in WRONG_VARIANTS}
    for c in cases():
        tr = {}
        want = run_case(c, trace=tr)
        for k in reach:
            reach[k] += int(tr[k])
        for v in WRONG_VARIANTS:
            changed[v] += int(not same_result(run_case(c, variant=v), want))
    return reach, changed
