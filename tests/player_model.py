"""The numpy model of SPEC.md section 20 (players), written from that text: play states advanced by dt, at most one command per
instance (the last in array order), and the records of the frame.  binary32 throughout with one rounded operation per numpy
operation and no fused multiply-add; NaN compares false.  `fdt=np.float64` runs the same rules in float64 (the drift figure).
Also the generator of cases that the CPU tests, the host build of csrc/play_math.h and the GPU tests share, and a table of
wrong readings of the text (WRONG_VARIANTS) that the cases must be able to tell apart."""
import numpy as np

F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
LOOP = 1
ENDED = 1
PLAY = np.dtype([("clip_a", "<u4"), ("clip_b", "<u4"), ("x_a", "<f4"), ("x_b", "<f4"), ("w", "<f4"), ("fade", "<f4"), ("speed", "<f4"),
                 ("flags", "<u4")])
CMD = np.dtype([("instance", "<u4"), ("clip", "<u4"), ("x", "<f4"), ("seconds", "<f4")])
STATE = np.dtype([("clip_a", "<u4"), ("clip_b", "<u4"), ("x_a", "<f4"), ("x_b", "<f4"), ("w", "<f4"), ("pad", "<u4")])
LAYER = np.dtype([("clip", "<u4"), ("x", "<f4"), ("w", "<f4"), ("mask", "<u2"), ("mode", "<u2")])
STEP = np.dtype([("clip", "<u4"), ("x", "<f4"), ("dx", "<f4"), ("w", "<f4")])

WRONG_VARIANTS = ("period_n1", "fma", "b_always", "first_dup", "out_after_swap", "step_x_after", "w_neg_dt", "swap_gt")


def table(nkeys, flags, rates):
    """a player set: key counts, flag words, rates (positions per second)"""
    return (np.asarray(nkeys, dtype=np.int64), np.asarray(flags, dtype=np.int64), np.asarray(rates, dtype=F))


def periods(tab, fdt=F, variant=None):
    nkeys, flags, _ = tab
    loop = (flags & LOOP) != 0
    P = np.where(loop & (variant != "period_n1"), nkeys, nkeys - 1)
    return P.astype(fdt), loop


def clamp_w(w):
    """section 14's clamp: NaN -> 0, then [0, 1]"""
    with np.errstate(all="ignore"):
        w = np.where(w > 0, w, np.zeros_like(w))
        return np.where(w > 1, np.ones_like(w), w)


def adv(y, P, loop):
    """x' from y = x + dx: section 14's wrap with its fallback on a LOOP clip, the clamp to [0, P] otherwise"""
    zero = np.zeros_like(y)
    with np.errstate(all="ignore"):
        q = y / P
        fl = np.floor(q)
        pr = fl * P
        r = y - pr
        wrapped = np.where((r >= 0) & (r < P), r, zero)
        c = np.where(y >= 0, y, zero)
        clamped = np.where(c > P, P, c)
    return np.where(loop, wrapped, clamped)


def fields(st, fdt=F):
    """a PLAY array as a dict of arrays (positions and weights in fdt)"""
    d = {k: st[k].astype(np.int64) for k in ("clip_a", "clip_b")}
    d.update({k: st[k].astype(fdt) for k in ("x_a", "x_b", "w", "fade", "speed")})
    d["flags"] = st["flags"].astype(np.uint32)
    return d


def records(d):
    st = np.zeros(d["x_a"].shape[0], dtype=PLAY)
    for k in PLAY.names:
        st[k] = d[k]
    return st


def select(cmds, n, variant=None):
    """per instance the index of the command that reaches it, or -1: the last in array order that names it"""
    sel = np.full(n, -1, dtype=np.int64)
    for i in range(0 if cmds is None else len(cmds)):
        inst = int(cmds["instance"][i])
        if inst >= n:
            continue
        if variant == "first_dup" and sel[inst] >= 0:
            continue
        sel[inst] = i
    return sel


def advance_fields(d, dt, tab, cmds=None, fdt=F, variant=None, trace=None):
    """steps 1 to 8 on a dict of fields; returns (stored fields, frame): frame holds clip_a, clip_b, x_a, x_b, w (the state
    and layer records), x0_a, dx_a, x0_b, dx_b (the steps)"""
    nkeys, tflags, rates = tab
    C = len(nkeys)
    P_t, loop_t = periods(tab, fdt, variant)
    rate_t = rates.astype(fdt)
    n = d["x_a"].shape[0]
    zero, one = np.zeros(n, dtype=fdt), np.ones(n, dtype=fdt)
    # 1. clamp
    ca, cb = np.minimum(d["clip_a"], C - 1), np.minimum(d["clip_b"], C - 1)
    xa, xb, w, fade, speed = d["x_a"], d["x_b"], d["w"], d["fade"], d["speed"]
    # 2. command
    sel = select(cmds, n, variant)
    has = sel >= 0
    tr = {}
    with np.errstate(all="ignore"):
        if has.any():
            pick = np.where(has, sel, 0)
            cc = np.minimum(cmds["clip"].astype(np.int64)[pick], C - 1)
            cx = cmds["x"][pick].astype(fdt)
            sec = cmds["seconds"][pick].astype(fdt)
            r = one / sec
            isfade = has & (sec > 0) & (r > 0) & (r <= FLT_MAX)
            cut = has & ~isfade
            running0 = fade > 0
            promote = isfade & running0 & (clamp_w(w) >= 0.5)
            ca, xa = np.where(promote, cb, ca), np.where(promote, xb, xa)
            cb, xb = np.where(isfade, cc, cb), np.where(isfade, cx, xb)
            ca, xa = np.where(cut, cc, ca), np.where(cut, cx, xa)
            w = np.where(has, zero, w)
            fade = np.where(isfade, r, np.where(cut, zero, fade))
            tr.update(cut=cut, fade_start=isfade, above=promote, below=isfade & running0 & ~promote)
            named = np.array([int(i) < n for i in cmds["instance"]])
            tr["dup_lost"] = int(named.sum()) > int(has.sum())
        else:
            f0 = np.zeros(n, dtype=bool)
            tr.update(cut=f0, fade_start=f0, above=f0, below=f0, dup_lost=False)
        running = fade > 0
        # 3. time
        dtf = fdt(dt)
        s = dtf * speed
        s = np.where(np.abs(s) <= FLT_MAX, s, zero)
        dtp = dtf if dt > 0 else fdt(0)
        # 4. advance A
        Pa, la = P_t[ca], loop_t[ca]
        dx_a = s * rate_t[ca]
        x0_a = xa
        ya = (xa.astype(np.float64) + s.astype(np.float64) * rate_t[ca].astype(np.float64)).astype(fdt) if variant == "fma" else xa + dx_a
        xa1 = adv(ya, Pa, la)
        # 5. advance B
        Pb, lb = P_t[cb], loop_t[cb]
        dx_b_all = s * rate_t[cb]
        yb = (xb.astype(np.float64) + s.astype(np.float64) * rate_t[cb].astype(np.float64)).astype(fdt) if variant == "fma" else xb + dx_b_all
        moves_b = running | (variant == "b_always")
        xb1 = np.where(moves_b, adv(yb, Pb, lb), xb)
        dx_b = np.where(moves_b, dx_b_all, zero)
        x0_b = xb
        # 6. weight
        w1 = clamp_w(w) + (dtf if variant == "w_neg_dt" else dtp) * fade
        w_out = np.where(running, np.where(w1 > 1, one, w1), zero)
        complete = running & ((w1 > 1) if variant == "swap_gt" else (w1 >= 1))
    frame = dict(clip_a=ca, clip_b=cb, x_a=xa1, x_b=xb1, w=w_out, x0_a=x0_a, dx_a=dx_a, x0_b=x0_b, dx_b=dx_b)
    if variant == "step_x_after":
        frame["x0_a"], frame["x0_b"] = ya, np.where(moves_b, yb, xb)
    # 8. store
    out = dict(clip_a=np.where(complete, cb, ca), clip_b=cb, x_a=np.where(complete, xb1, xa1),
               x_b=np.where(moves_b & ~complete, xb1, xb), w=np.where(complete, zero, np.where(running, w1, w)),
               fade=np.where(complete, zero, fade), speed=speed)
    with np.errstate(all="ignore"):
        ended = ~loop_t[out["clip_a"]] & (out["x_a"] >= P_t[out["clip_a"]])
    out["flags"] = (d["flags"] & np.uint32(0xFFFFFFFE)) | ended.astype(np.uint32)
    if variant == "out_after_swap":
        frame.update(clip_a=out["clip_a"], x_a=out["x_a"], x_b=out["x_b"], w=np.where(complete, zero, w_out))
    if trace is not None:
        with np.errstate(all="ignore"):
            tr.update(fwd_wrap=la & (ya >= Pa) & (xa1 < Pa) & (ya <= FLT_MAX), back_wrap=la & (ya < 0) & (xa1 > 0), complete=complete,
                      running=running, ended=ended, end_clamp=~la & (ya > Pa), exact_one=running & (w1 == 1), loop_a=la,
                      moved=(s != 0) & (dx_a != 0), has=has)
        trace.append(tr)
    return out, frame


def frame_records(frame, nlayers=0, layers=None):
    """the three outputs of a frame: STATE [n], LAYER [n, nlayers] or None (layers 2.. as `layers` holds them), STEP [n, 2]"""
    n = frame["x_a"].shape[0]
    st = np.zeros(n, dtype=STATE)
    for k in ("clip_a", "clip_b", "x_a", "x_b", "w"):
        st[k] = frame[k]
    ly = None
    if nlayers:
        ly = np.zeros((n, nlayers), dtype=LAYER) if layers is None else np.array(layers, dtype=LAYER).reshape(n, nlayers)
        ly[:, 0] = np.zeros(n, dtype=LAYER)
        ly[:, 1] = np.zeros(n, dtype=LAYER)
        ly["clip"][:, 0], ly["x"][:, 0] = frame["clip_a"], frame["x_a"]
        ly["clip"][:, 1], ly["x"][:, 1], ly["w"][:, 1] = frame["clip_b"], frame["x_b"], frame["w"]
    sp = np.zeros((n, 2), dtype=STEP)
    sp["clip"][:, 0], sp["x"][:, 0], sp["dx"][:, 0] = frame["clip_a"], frame["x0_a"], frame["dx_a"]
    sp["clip"][:, 1], sp["x"][:, 1], sp["dx"][:, 1], sp["w"][:, 1] = frame["clip_b"], frame["x0_b"], frame["dx_b"], frame["w"]
    return st, ly, sp


def advance(states, dt, tab, cmds=None, nlayers=0, layers=None, variant=None, trace=None):
    """one call on PLAY records [n]: (stored states, STATE [n], LAYER [n, nlayers] or None, STEP [n, 2])"""
    out, frame = advance_fields(fields(states), dt, tab, cmds, F, variant, trace)
    return (records(out),) + frame_records(frame, nlayers, layers)


def same_bits(a, b):
    """element by element: the same bits, or NaN for NaN (payloads are free); structured arrays field by field"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.names:
        ok = np.ones(a.shape, dtype=bool)
        for k in a.dtype.names:
            ok &= same_bits(a[k], b[k])
        return ok
    if a.dtype.kind == "f":
        return (a.view("<u4") == b.view("<u4")) | (np.isnan(a) & np.isnan(b))
    return a == b


# ---- the host recipe the player replaces (INTEGRATION.md "Characters that walk", before players) --------------------------
def host_recipe(x, dt, speed, rate, N):
    """binary32: x := (x + dt * speed * rate) wrapped at the LOOP period N"""
    x, P = F(x), F(N)
    dx = F(F(dt) * F(speed)) * F(rate)
    y = F(x + dx)
    r = F(y - F(np.floor(F(y / P)) * P))
    return (r if 0 <= r < P else F(0)), dx


# ---- the generator ------------------------------------------------------------------------------------------------------
COUNTS = (1, 5, 63, 64, 65, 257)
BIG = 1 << 24
CLIPSETS = (
    table([30], [LOOP], [30.0]),
    table([30], [0], [24.0]),
    table([1], [LOOP], [30.0]),
    table([30, 2, BIG], [LOOP, 0, LOOP], [30.0, 2.5, 60.0]),
    table([1, 2, BIG], [0, LOOP, 0], [30.0, -7.5, 1.0e6]),
    table([30, 30, 2], [LOOP, 0, LOOP], [30.0, 30.0, 3.0]),
)
DT = float(F(1.0) / F(30.0))
DTS = (DT, 0.0, -DT, float("nan"), float("inf"), DT, 0.5, DT)
NAN = float("nan")
INF = float("inf")
DENORMAL = 1e-41
X_EDGES = (-0.0, -1e-7, 1e30, NAN, 0.2, 29.8, 28.95, 1.0, 16777215.5, 0.0)
SPEED_EDGES = (-1.0, -0.0, NAN, 1.0, 0.5, INF, 1.5, -1.25)
W_EDGES = (NAN, -0.5, INF, 0.3, 0.7, 0.97, 0.5, 0.0)
FADE_EDGES = (NAN, -1.0, INF, 0.0, 2.0, 15.0, 30.0, 1.0, 0.0, 0.0)
SEC_EDGES = (0.0, -1.0, NAN, INF, DENORMAL, 0.05, 0.5, 1.0 / 15.0)


def make_states(rng, n, C):
    st = np.zeros(n, dtype=PLAY)
    pick = lambda edges, normal: np.where(rng.random(n) < 0.45, rng.choice(np.array(edges, dtype=F), n), normal.astype(F))
    st["clip_a"] = np.where(rng.random(n) < 0.15, rng.choice([C, 0xFFFFFFFF], n), rng.integers(0, C, n))
    st["clip_b"] = np.where(rng.random(n) < 0.15, rng.choice([C, 0xFFFFFFFF], n), rng.integers(0, C, n))
    st["x_a"] = pick(X_EDGES, rng.uniform(0, 30, n))
    st["x_b"] = pick(X_EDGES, rng.uniform(0, 30, n))
    st["w"] = pick(W_EDGES, rng.uniform(0, 1, n))
    st["fade"] = pick(FADE_EDGES, np.zeros(n))
    st["speed"] = pick(SPEED_EDGES, rng.uniform(0.5, 1.5, n))
    st["flags"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    # scripted rows, as far as n reaches: a forward wrap, a backward wrap, the end of a one-shot clip, fades that complete
    # (one of them at w' == 1 exactly for dt = 1/30 and for dt = 0.5), fades to interrupt below and above one half
    script = [(0, 0, 29.8, 0.0, 0.0, 0.0, 1.0), (0, 0, 0.2, 0.0, 0.0, 0.0, -1.0), (C - 1, 0, 28.95, 0.0, 0.0, 0.0, 1.5),
              (0, C - 1, 3.0, 1.0, 0.0, 30.0, 1.0), (0, C - 1, 3.0, 1.0, 0.5, 1.0, 1.0), (0, C - 1, 5.0, 2.0, 0.2, 2.0, 1.0),
              (0, C - 1, 5.0, 2.0, 0.7, 2.0, 1.0), (min(1, C - 1), 0, 0.5, 0.0, 0.0, 0.0, 1.0)]
    for i, row in enumerate(script[:n]):
        k = (i * 7 + 3) % n if n >= 64 else i
        for name, v in zip(("clip_a", "clip_b", "x_a", "x_b", "w", "fade", "speed"), row):
            st[name][k] = v
    return st


def make_cmds(rng, n, C, m, scripted):
    """m random commands (duplicates, instances >= n, edges of every field), then the scripted ones"""
    cm = np.zeros(m + len(scripted), dtype=CMD)
    cm["instance"][:m] = np.where(rng.random(m) < 0.2, rng.choice([n, n + 7, 0xFFFFFFFF], m), rng.integers(0, n, m))
    cm["clip"][:m] = np.where(rng.random(m) < 0.2, rng.choice([C, 0xFFFFFFFF], m), rng.integers(0, C, m))
    cm["x"][:m] = np.where(rng.random(m) < 0.4, rng.choice(np.array(X_EDGES, dtype=F), m), rng.uniform(0, 30, m).astype(F))
    cm["seconds"][:m] = rng.choice(np.array(SEC_EDGES, dtype=F), m)
    for j, row in enumerate(scripted):
        cm[m + j] = row
    return cm


_CASES = None


def cases():
    """every case: name, n, tab (the player set), states (PLAY [n]), calls (three (dt, CMD array) pairs), nlayers, layers (LAYER
    [n, nlayers] sentinels).  Deterministic."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    k = 0
    for n in COUNTS:
        for si, tab in enumerate(CLIPSETS):
            rng = np.random.default_rng(2000 + k)
            C = len(tab[0])
            st = make_states(rng, n, C)
            rows = lambda i: ((i * 7 + 3) % n if n >= 64 else i) if i < n else None
            dts = (DTS[k % len(DTS)], DTS[(k + 3) % len(DTS)], DT)
            # call 0: a crowd of commands with duplicates; call 1: none (even cases) or one; call 2: a cut on the instance
            # that reached its end, fades onto the two running fades, and a duplicate pair whose first entry must lose
            s2 = []
            if rows(2) is not None:
                s2.append((rows(2), 0, 1.5, 0.0))
            for i in (5, 6):
                if rows(i) is not None:
                    s2.append((rows(i), min(1, C - 1), 0.25, 0.5))
            s2 += [(0, C - 1, 2.0, 0.0), (0, 0, 7.0, 0.25)]
            c0 = make_cmds(rng, n, C, 0 if k % 5 == 4 else max(1, n // 3), [])
            if k % 5 != 4:  # not on the scripted rows in call 0: they play out first
                keep = ~np.isin(c0["instance"], [rows(i) for i in range(8) if rows(i) is not None])
                c0 = c0[keep] if n >= 64 else c0
            c1 = make_cmds(rng, n, C, 0, [] if k % 2 == 0 else [(n - 1, 0, 1.0, 0.05)])
            c2 = make_cmds(rng, n, C, n // 8, s2)
            nl = 8 if k % 2 else 2
            ly = np.frombuffer(rng.bytes(n * nl * 16), dtype=LAYER).reshape(n, nl).copy()
            out.append(dict(name=f"n{n}_set{si}", n=n, tab=tab, states=st, calls=[(dts[0], c0), (dts[1], c1), (dts[2], c2)], nlayers=nl, layers=ly))
            k += 1
    _CASES = out
    return out


def run_case(c, variant=None, trace=None, ncalls=3):
    """the model over the first ncalls calls of a case: a list of (states, STATE, LAYER, STEP) after each; the layer array is
    carried from call to call as the device buffer is"""
    st, ly, res = c["states"], c["layers"], []
    for dt, cm in c["calls"][:ncalls]:
        st, os_, ly, sp = advance(st, dt, c["tab"], cm, c["nlayers"], ly, variant, trace)
        res.append((st, os_, ly, sp))
    return res


def can_show(variant, traces, calls):
    """whether a case (the traces of its calls from the model as the text reads) can tell the wrong reading apart at all"""
    any_ = lambda key: any(np.any(t[key]) for t in traces)
    if variant == "period_n1":
        return any_("loop_a")
    if variant == "fma":
        return any_("moved")
    if variant == "b_always":
        return any(np.any(~t["running"]) for t in traces)
    if variant == "first_dup":
        return any(t["dup_lost"] for t in traces)
    if variant == "out_after_swap":
        return any_("complete")
    if variant == "step_x_after":
        return any_("moved")
    if variant == "w_neg_dt":
        return any(not dt >= 0 and np.any(t["running"]) for t, (dt, _) in zip(traces, calls))  # negative or NaN
    if variant == "swap_gt":
        return any_("exact_one")
    raise ValueError(variant)


def drift(steps=20000, speed=0.37, rate=30.0, N=30):
    """20 000 accumulated binary32 advances of a LOOP clip (the scalar form of steps 3 and 4, which test_player_model holds equal
    to the model) against the same advances in float64 from the same binary32 dt, speed and rate: (largest distance on the
    circle of period N, the distance at the end, wraps)"""
    x32, x64, P32, P64 = F(0), 0.0, F(N), float(N)
    dx32 = F(F(DT) * F(speed)) * F(rate)
    dx64 = float(F(DT)) * float(F(speed)) * float(F(rate))
    worst, wraps, e = 0.0, 0, 0.0
    for _ in range(steps):
        y = F(x32 + dx32)
        r = F(y - F(np.floor(F(y / P32)) * P32))
        r = r if 0 <= r < P32 else F(0)
        wraps += int(r < x32)
        x32 = r
        y = x64 + dx64
        x64 = y - np.floor(y / P64) * P64
        e = abs(float(x32) - x64)
        e = min(e, N - e)
        worst = max(worst, e)
    return worst, e, wraps
