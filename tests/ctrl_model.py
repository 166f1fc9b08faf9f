"""The numpy model of SPEC.md section 21 (controllers), written from that text: per instance the node is clamped, the lead of
the play state gives the built-in values, the any-state transitions and then the node's own are tried in array order, the
first that is not skipped and whose conditions hold fires and writes command slot i; otherwise the slot holds a command the
player ignores.  binary32 throughout, one rounded operation per numpy operation; NaN compares false and NE is IEEE !=.
Also the generator of cases that the CPU tests, the host build of csrc/ctrl_math.h and the GPU tests share (each case three
steps chained through tests/player_model.py), a table of wrong readings of the text (WRONG_VARIANTS) that the cases must be
able to tell apart, and the locomotion graph of the stated consequences."""
import numpy as np

from tests import player_model as pm

F = np.float32
NODE = np.dtype([("clip", "<u4"), ("first", "<u4"), ("count", "<u4"), ("pad", "<u4")])
COND = np.dtype([("param", "<u2"), ("op", "<u2"), ("value", "<f4")])
TRANS = np.dtype([("target", "<u4"), ("flags", "<u4"), ("seconds", "<f4"), ("x", "<f4"), ("ncond", "<u4"), ("pad", "<u4"), ("cond", COND, (3,))])
STATE = np.dtype([("node", "<u4"), ("t", "<f4"), ("fired", "<u4"), ("user", "<u4")])
LT, LE, GT, GE, EQ, NE = range(6)
INTERRUPT, SELF, SYNC, CONSUME = 1, 2, 4, 8
TIME, POS, PHASE, ENDED, FADING = 0xFFFF, 0xFFFE, 0xFFFD, 0xFFFC, 0xFFFB
BUILTINS = (TIME, POS, PHASE, ENDED, FADING)
NONE = 0xFFFFFFFF

WRONG_VARIANTS = ("last_passes", "own_first", "lead_a", "t_first", "t_kept", "ne_nan_false", "consume_evaluated", "sync_ratio", "dtp_keeps_neg_zero")
BRANCHES = ("fire_any", "fire_own", "skip_fade", "skip_self", "interrupt", "sync", "consume", "no_fire")


def graph(nodes, trans, nany, nparams):
    return dict(nodes=np.ascontiguousarray(nodes, dtype=NODE), trans=np.ascontiguousarray(trans, dtype=TRANS), nany=int(nany), nparams=int(nparams))


def periods(nkeys, flags):
    """P = float(N) for a LOOP clip, float(N - 1) otherwise; and which clips are LOOP"""
    nkeys, flags = np.asarray(nkeys, dtype=np.int64), np.asarray(flags, dtype=np.int64)
    loop = (flags & pm.LOOP) != 0
    return np.where(loop, nkeys, nkeys - 1).astype(F), loop


def _compare(op, v, value, variant):
    with np.errstate(all="ignore"):
        ne = ((v < value) | (v > value)) if variant == "ne_nan_false" else (v != value)
        res = [v < value, v <= value, v > value, v >= value, v == value, ne]
    out = np.zeros(v.shape, dtype=bool)
    for k in range(6):
        out = np.where(op == k, res[k], out)
    return out


def step(g, tab, states, play, params, dt, counts=None, variant=None, trace=None):
    """one step on STATE [n], pm.PLAY [n] and float32 [n, NP]: (states', params', pm.CMD [n], counts' or None).  tab: the player
    set's (nkeys, flags, ...)."""
    nodes, trans, nany, NP = g["nodes"], g["trans"], g["nany"], g["nparams"]
    n, S, C = len(states), len(nodes), len(tab[0])
    P_t, loop_t = periods(tab[0], tab[1])
    rows = np.arange(n)
    zero, one = np.zeros(n, dtype=F), np.ones(n, dtype=F)
    params = np.zeros((n, 0), dtype=F) if params is None else np.array(params, dtype=F).reshape(n, NP)
    # 1. node
    node = np.minimum(states["node"].astype(np.int64), S - 1)
    # 2. lead
    ca, cb = np.minimum(play["clip_a"].astype(np.int64), C - 1), np.minimum(play["clip_b"].astype(np.int64), C - 1)
    with np.errstate(all="ignore"):
        running = play["fade"] > 0
        lead_b = running & (variant != "lead_a")
        cl, xl = np.where(lead_b, cb, ca), np.where(lead_b, play["x_b"], play["x_a"]).astype(F)
        Pl = P_t[cl]
        phase = xl / Pl
        ended = np.where(~loop_t[cl] & (xl >= Pl), one, zero)
        dtp = F(dt) if dt > 0 else F(0)
        if variant == "dtp_keeps_neg_zero" and dt == 0:  # max(dt, 0) written so that it hands -0 through
            dtp = F(dt)
        t0 = states["t"].astype(F)
        t_seen = t0 + dtp if variant == "t_first" else t0
    fading = np.where(running, one, zero)
    builtin = {TIME: t_seen, POS: xl, PHASE: phase, ENDED: ended, FADING: fading}
    # 3. candidates: per instance the any-state transitions, then the node's own (own_first: the other way round)
    count = nodes["count"].astype(np.int64)[node]
    first = nodes["first"].astype(np.int64)[node]
    K = int(count.max()) if n else 0
    own_idx = first[:, None] + np.arange(K)[None, :]
    own_ok = np.arange(K)[None, :] < count[:, None]
    any_idx = np.broadcast_to(np.arange(nany)[None, :], (n, nany))
    parts = [(any_idx, np.ones((n, nany), dtype=bool), True), (own_idx, own_ok, False)]
    if variant == "own_first":
        parts.reverse()
    fired = np.full(n, -1, dtype=np.int64)
    tr_ = {k: np.zeros(n, dtype=bool) for k in BRANCHES}
    p0_phase = np.zeros(n, dtype=bool)
    for idx_m, ok_m, is_any in parts:
        for k in range(idx_m.shape[1]):
            live = ok_m[:, k] & ((fired < 0) | (variant == "last_passes"))
            if not live.any():
                continue
            idx = np.where(live, idx_m[:, k], 0)
            t = trans[idx]
            fl = t["flags"].astype(np.int64)
            skip_fade = live & running & ((fl & INTERRUPT) == 0)
            skip_self = live & ~skip_fade & is_any & (t["target"].astype(np.int64) == node) & ((fl & SELF) == 0)
            tr_["skip_fade"] |= skip_fade
            tr_["skip_self"] |= skip_self
            ev = live & ~skip_fade & ~skip_self
            ok = ev.copy()
            for c in range(3):
                use = ev & (c < t["ncond"].astype(np.int64))
                p = t["cond"]["param"][:, c].astype(np.int64)
                v = zero.copy()
                for code, val in builtin.items():
                    v = np.where(p == code, val, v)
                user = use & (p < NP)
                if NP:
                    v = np.where(user, params[rows, np.minimum(p, NP - 1)], v)
                p0_phase |= use & (p == PHASE) & (Pl == 0)
                ok &= ~use | _compare(t["cond"]["op"][:, c].astype(np.int64), v, t["cond"]["value"][:, c].astype(F), variant)
                if variant == "consume_evaluated":  # a store for what was only evaluated
                    st_ = user & ((fl & CONSUME) != 0)
                    params[rows[st_], p[st_]] = F(0)
            fired = np.where(ok, idx, fired)
    # 4. fire, 5. no fire
    has = fired >= 0
    t = trans[np.where(has, fired, 0)] if len(trans) else np.zeros(n, dtype=TRANS)
    fl = t["flags"].astype(np.int64)
    g_ = t["target"].astype(np.int64)
    c_ = nodes["clip"].astype(np.int64)[np.where(has, g_, 0)]
    with np.errstate(all="ignore"):
        if variant == "sync_ratio":
            xs = xl * (P_t[c_] / Pl)
        else:
            xs = (xl / Pl) * P_t[c_]
        x = np.where((fl & SYNC) != 0, xs, t["x"].astype(F))
        t_no = t0 + dtp
    cmds = np.zeros(n, dtype=pm.CMD)
    cmds["instance"] = np.where(has, rows, NONE)
    cmds["clip"] = np.where(has, c_, 0)
    cmds["x"] = np.where(has, x, zero)
    cmds["seconds"] = np.where(has, t["seconds"].astype(F), zero)
    consumed = np.zeros(n, dtype=bool)
    for c in range(3):
        p = t["cond"]["param"][:, c].astype(np.int64)
        st_ = has & ((fl & CONSUME) != 0) & (c < t["ncond"].astype(np.int64)) & (p < NP)
        params[rows[st_], p[st_]] = F(0)
        consumed |= st_
    out = np.zeros(n, dtype=STATE)
    out["node"] = np.where(has, g_, node)
    out["t"] = np.where(has, t_no if variant == "t_kept" else zero, t_no)
    out["fired"] = np.where(has, fired, NONE)
    out["user"] = states["user"]
    if counts is not None:
        counts = np.array(counts, dtype=np.uint32)
        np.add.at(counts, fired[has], 1)
    if trace is not None:
        tr_["fire_any"], tr_["fire_own"] = has & (fired < nany), has & (fired >= nany)
        tr_["interrupt"] = has & running
        tr_["sync"], tr_["consume"], tr_["no_fire"] = has & ((fl & SYNC) != 0), consumed, ~has
        tr_["p0_phase"], tr_["p0_sync"] = p0_phase, tr_["sync"] & (Pl == 0)
        trace.append(tr_)
    return out, params, cmds, counts


def same_bits(a, b):
    return pm.same_bits(a, b)


# ---- the generator ------------------------------------------------------------------------------------------------------
COUNTS = pm.COUNTS
NAN, INF, DENORMAL = float("nan"), float("inf"), 1e-41
T_EDGES = (NAN, INF, -INF, -0.0, DENORMAL, 0.0, 0.5, 1.0)
P_EDGES = (NAN, INF, -INF, -0.0, DENORMAL, 0.0, 1.0, 0.5)
V_EDGES = (NAN, INF, -INF, -0.0, DENORMAL, 0.0, 1.0, 0.5, 0.25, 15.0)
# what the player's generator does not hold: dt of -0, a denormal and -inf; positions of +-inf and a denormal; fades of -0, a
# denormal (a fade that runs only where denormals are kept) and -inf
DTS = (pm.DT, 0.0, -pm.DT, NAN, INF, -0.0, DENORMAL, -INF, 0.5, pm.DT, -0.0)
X_MORE = (INF, -INF, DENORMAL, -DENORMAL)
FADE_MORE = (-0.0, DENORMAL, -INF, DENORMAL)
KINDS = (("single", 0), ("mixed0", 1), ("mixed2", 5), ("mixed2", 16), ("mixed0", 0), ("mixed2", 1), ("mixed0", 16), ("mixed2", 0))


def make_trans(rng, S, NP, target=None):
    t = np.zeros(1, dtype=TRANS)[0]
    t["target"] = rng.integers(0, S) if target is None else target
    t["flags"] = rng.integers(0, 16)
    t["seconds"] = rng.choice(np.array(pm.SEC_EDGES, dtype=F))
    t["x"] = rng.choice(np.array(pm.X_EDGES, dtype=F)) if rng.random() < 0.5 else F(rng.uniform(0, 30))
    nc = int(rng.choice([0, 1, 1, 2, 3]))
    t["ncond"] = nc
    for c in range(3):  # the unused ones hold junk that must not be looked at
        if c >= nc:
            t["cond"][c] = (rng.integers(0, 1 << 16), rng.integers(0, 1 << 16), F(rng.uniform(-1, 1)))
            continue
        if NP and rng.random() < 0.6:
            p = int(rng.integers(0, NP))
        else:
            p = int(rng.choice(BUILTINS))
        # comparisons that pass about every other time: the values the generator puts into parameters and states
        v = rng.choice(np.array(V_EDGES, dtype=F)) if rng.random() < 0.5 else F(rng.uniform(0, 1))
        t["cond"][c] = (p, rng.integers(0, 6), v)
    return t


def make_graph(rng, kind, NP, C):
    if kind == "single":
        return graph(np.array([(C - 1, 0, 0, 0)], dtype=NODE), np.zeros(0, dtype=TRANS), 0, NP)
    nany = 2 if kind == "mixed2" else 0
    counts = (0, 1, 7, 1)  # side by side: lanes of one wave loop differently
    S = len(counts)
    trans = [make_trans(rng, S, NP) for _ in range(nany)]
    nodes = []
    for s, cnt in enumerate(counts):
        nodes.append((int(rng.integers(0, C)), len(trans), cnt, int(rng.integers(0, 1 << 32))))
        trans += [make_trans(rng, S, NP) for _ in range(cnt)]
    tr = np.array(trans, dtype=TRANS)
    if nany:  # scripted: an any-state transition into node 0 without SELF and with no condition, behind a conditional one
        tr[1]["target"], tr[1]["flags"], tr[1]["ncond"] = 0, int(tr[1]["flags"]) & ~SELF, 0
    # scripted: the node with 7 transitions ends on one that always passes, with SYNC and CONSUME over a user parameter
    last = nodes[2][1] + 6
    tr[last]["flags"] = SYNC | CONSUME | INTERRUPT
    tr[last]["ncond"] = 1
    tr[last]["cond"][0] = (0, NE, F(-2.0)) if NP else (ENDED, NE, F(-2.0))
    return graph(np.array(nodes, dtype=NODE), tr, nany, NP)


def make_states(rng, n, S):
    st = np.zeros(n, dtype=STATE)
    st["node"] = np.where(rng.random(n) < 0.15, rng.choice([S, 0xFFFFFFFF], n), rng.integers(0, S, n))
    st["t"] = np.where(rng.random(n) < 0.4, rng.choice(np.array(T_EDGES, dtype=F), n), rng.uniform(0, 2, n).astype(F))
    st["fired"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    st["user"] = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return st


def make_params(rng, n, NP):
    p = rng.uniform(0, 1, (n, NP)).astype(F)
    return np.where(rng.random((n, NP)) < 0.4, rng.choice(np.array(P_EDGES, dtype=F), (n, NP)), p).astype(F)


_CASES = None


def cases():
    """every case: name, n, tab (a player set of pm), graph, states (STATE [n]), play (pm.PLAY [n]), params (float32 [n, NP]),
    dts (three).  Deterministic."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out, k = [], 0
    for n in COUNTS:
        for kind, NP in KINDS:
            rng = np.random.default_rng(2100 + k)
            tab = pm.CLIPSETS[(k * 5 + 4) % len(pm.CLIPSETS)]
            C = len(tab[0])
            g = make_graph(rng, kind, NP, C)
            play = pm.make_states(rng, n, C)
            play["fade"] = np.where(rng.random(n) < 0.5, F(0), play["fade"])  # half the crowd can fire without INTERRUPT
            for name, more in (("x_a", X_MORE), ("x_b", X_MORE), ("fade", FADE_MORE)):
                play[name] = np.where(rng.random(n) < 0.12, rng.choice(np.array(more, dtype=F), n), play[name])
            dts = (DTS[k % len(DTS)], DTS[(k + 3) % len(DTS)], pm.DT)
            out.append(dict(name=f"n{n}_{kind}_p{NP}", n=n, tab=tab, graph=g, states=make_states(rng, n, len(g["nodes"])), play=play,
                            params=make_params(rng, n, NP), dts=dts))
            k += 1
    _CASES = out
    return out


def run_case(c, variant=None, trace=None, nsteps=3, counts=True):
    """the model over the first nsteps steps of a case, the commands of each step consumed by the player model before the next:
    a list of (states, params, cmds, counts, play after the advance) after each"""
    st, pr, play, res = c["states"], c["params"], c["play"], []
    ct = np.zeros(len(c["graph"]["trans"]), dtype=np.uint32) if counts else None
    for dt in c["dts"][:nsteps]:
        st, pr, cm, ct = step(c["graph"], c["tab"], st, play, pr, dt, ct, variant, trace)
        play = pm.advance(play, dt, c["tab"], cm)[0]
        res.append((st, pr, cm, ct, play))
    return res


def same_result(a, b):
    """two run_case results: the same states, parameters, commands and counts, NaN for NaN"""
    return all(same_bits(x[0], y[0]).all() and same_bits(x[1], y[1]).all() and same_bits(x[2], y[2]).all() and (x[3] == y[3]).all()
               for x, y in zip(a, b))


def census():
    """(in how many cases each branch is reached, in how many cases each wrong variant changes something), from the model alone"""
    reach = {k: 0 for k in BRANCHES + ("p0_phase", "p0_sync")}
    changed = {v: 0 for v in WRONG_VARIANTS}
    for c in cases():
        tr = []
        want = run_case(c, trace=tr)
        for k in reach:
            reach[k] += int(any(t[k].any() for t in tr))
        for v in WRONG_VARIANTS:
            changed[v] += int(not same_result(run_case(c, variant=v), want))
    return reach, changed


# ---- the locomotion graph of the stated consequences -----------------------------------------------------------------------
LOCO_TAB = pm.table([30, 32, 16, 12], [pm.LOOP, pm.LOOP, pm.LOOP, 0], [30.0, 32.0, 24.0, 24.0])  # idle, walk, run, jump
IDLE, WALK, RUN, JUMP = range(4)
SPEED, TRIGGER = 0, 1


def _t(target, flags, seconds, conds, x=0.0):
    t = np.zeros(1, dtype=TRANS)[0]
    t["target"], t["flags"], t["seconds"], t["x"], t["ncond"] = target, flags, seconds, x, len(conds)
    for i, cnd in enumerate(conds):
        t["cond"][i] = cnd
    return t


def locomotion(interrupt=True):
    """idle, walk and run (LOOP) on speed thresholds with hysteresis, walk <-> run with SYNC; an any-state jump on a trigger
    parameter (INTERRUPT unless told otherwise, CONSUME) that returns to idle when the one-shot clip has ENDED"""
    trans = [
        _t(JUMP, (INTERRUPT if interrupt else 0) | CONSUME, 0.0, [(TRIGGER, GT, 0.5)]),
        _t(WALK, 0, 0.2, [(SPEED, GT, 0.6)]),                       # idle ->
        _t(IDLE, 0, 0.2, [(SPEED, LT, 0.4)]),                       # walk ->
        _t(RUN, SYNC, 0.2, [(SPEED, GT, 2.2)]),
        _t(WALK, SYNC, 0.2, [(SPEED, LT, 1.8)]),                    # run ->
        _t(IDLE, 0, 0.1, [(ENDED, GE, 1.0)]),                       # jump ->
    ]
    nodes = np.array([(IDLE, 1, 1, 0), (WALK, 2, 2, 0), (RUN, 4, 1, 0), (JUMP, 5, 1, 0)], dtype=NODE)
    return graph(nodes, np.array(trans, dtype=TRANS), 1, 2)
