"""The numpy model of SPEC.md section 25 (motion matching), written from the text: binary32 throughout, every fma exact
(anim_ik_model.fma32), every other operator one rounding, NaN compares false.  `search` is one call on n instances; its
variants are wrong readings of the rule that the tests must be able to tell from the right one.  `search64` is the same
search with scores in float64, for the accuracy paragraph.  `cases()` is the generator every match test shares."""
import numpy as np

from tests import player_model as pm
from tests.anim_ik_model import fma32

F = np.float32
ROW = np.dtype([("clip", "<u4"), ("x", "<f4"), ("bias", "<f4"), ("tags", "<u4")])
FILTER = np.dtype([("require", "<u4"), ("exclude", "<u4")])
RESULT = np.dtype([("row", "<u4"), ("cur", "<u4"), ("score", "<f4"), ("cur_score", "<f4")])
PLAY, CMD = pm.PLAY, pm.CMD
NONE = 0xFFFFFFFF
QNAN = 0x7FC00000
INTERRUPT = 1
WRONG_VARIANTS = ("unfused", "reverse", "c_last", "tie_high", "nan_wins", "neg_zero_less", "no_filter", "pose_raw", "cur_lt", "near_any_clip", "no_margin",
                  "cur_filtered_skip")


def periods(nkeys, flags):
    nkeys, flags = np.asarray(nkeys, dtype=np.int64), np.asarray(flags, dtype=np.int64)
    loop = (flags & pm.LOOP) != 0
    return np.where(loop, nkeys, nkeys - 1).astype(F), loop


def c_of(feats, bias):
    """c_r = -(0.5 * n2 + bias_r), n2 the fma chain of f_d * f_d from 0 in d order"""
    feats = np.asarray(feats, dtype=F)
    n2 = np.zeros(feats.shape[0], dtype=F)
    for d in range(feats.shape[1]):
        n2 = fma32(feats[:, d], feats[:, d], n2)
    with np.errstate(all="ignore"):
        return -((F(0.5) * n2).astype(F) + np.asarray(bias, dtype=F)).astype(F)


def make_set(nkeys, clip_flags, rows, feats, pose_dims=0, flags=0, seconds=0.2, near=0.0, margin=0.0, mean=None, scale=None):
    rows, feats = np.ascontiguousarray(rows, dtype=ROW), np.ascontiguousarray(feats, dtype=F)
    D = feats.shape[1]
    P, loop = periods(nkeys, clip_flags)
    return dict(nkeys=np.asarray(nkeys, dtype=np.uint32), clip_flags=np.asarray(clip_flags, dtype=np.uint32), P=P, loop=loop, rows=rows, feats=feats, D=D,
                pose_dims=int(pose_dims), flags=int(flags), seconds=F(seconds), near=F(near), margin=F(margin),
                mean=np.zeros(D, dtype=F) if mean is None else np.asarray(mean, dtype=F), scale=np.ones(D, dtype=F) if scale is None else np.asarray(scale, dtype=F),
                has_norm=mean is not None, c=c_of(feats, rows["bias"]))


def lead(s, play):
    """step 1: the lead clip L (clamped), its position p, and whether a fade runs"""
    running = play["fade"] > 0
    top = len(s["nkeys"]) - 1
    L = np.minimum(np.where(running, play["clip_b"], play["clip_a"]).astype(np.int64), top)
    p = np.where(running, play["x_b"], play["x_a"]).astype(F)
    return L, p, running


def current_rows(s, L, p, variant=None):
    """step 1: the row of clip L with the largest x <= p, or NONE"""
    rows = s["rows"]
    cur = np.full(len(L), NONE, dtype=np.int64)
    for i in range(len(L)):
        idx = np.flatnonzero(rows["clip"] == L[i])
        if idx.size == 0:
            continue
        with np.errstate(invalid="ignore"):
            k = int(np.count_nonzero(rows["x"][idx] < p[i] if variant == "cur_lt" else rows["x"][idx] <= p[i]))
        if k:
            cur[i] = idx[k - 1]
    return cur


def query(s, cur, raw, variant=None):
    """step 2: a difference and then a product; pose dimensions from the current row where there is one"""
    n, D = len(cur), s["D"]
    raw = np.zeros((n, D), dtype=F) if raw is None else np.asarray(raw, dtype=F).reshape(n, D)
    with np.errstate(all="ignore"):
        q = ((raw - s["mean"][None, :]).astype(F) * s["scale"][None, :]).astype(F)
    if variant != "pose_raw":
        have = cur != NONE
        for d in range(D):
            if (s["pose_dims"] >> d) & 1:
                q[have, d] = s["feats"][cur[have], d]
    return q


def canon(S):
    """-0 counts as +0"""
    return np.where(S == 0, F(0.0), S).astype(F)


def scores(s, q, variant=None):
    """step 3: the chain in d order from c_r, [n, R]"""
    f, c = s["feats"], s["c"]
    n, R, D = q.shape[0], f.shape[0], s["D"]
    S = np.zeros((n, R), dtype=F) if variant == "c_last" else np.broadcast_to(c[None, :], (n, R)).astype(F)
    order = range(D - 1, -1, -1) if variant == "reverse" else range(D)
    with np.errstate(all="ignore"):
        for d in order:
            if variant == "unfused":
                S = ((q[:, d, None] * f[None, :, d]).astype(F) + S).astype(F)
            else:
                S = fma32(q[:, d, None], f[None, :, d], S)
        if variant == "c_last":
            S = (S + c[None, :]).astype(F)
    return S if variant == "neg_zero_less" else canon(S)


def order_key(S, variant=None):
    """the order of scores as unsigned words: 0 for NaN, else increasing with s"""
    u = np.ascontiguousarray(S, dtype=F).view(np.uint32).astype(np.int64)
    k = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(S), 0xFFFFFFFF if variant == "nan_wins" else 0, k)


def candidates(s, filt, n, variant=None):
    tags = s["rows"]["tags"].astype(np.int64)[None, :]
    if filt is None or variant == "no_filter":
        return np.ones((n, tags.shape[1]), dtype=bool)
    req, exc = filt["require"].astype(np.int64)[:, None], filt["exclude"].astype(np.int64)[:, None]
    return ((tags & req) == req) & ((tags & exc) == 0)


def decide(s, play, cur, S, cand, base, variant=None):
    """steps 5 to 7 from the score matrix"""
    n, R = S.shape
    L, p, running = lead(s, play)
    key = np.where(cand, order_key(S, variant), 0)
    win = (R - 1 - np.argmax(key[:, ::-1], axis=1)) if variant == "tie_high" else np.argmax(key, axis=1)
    ar = np.arange(n)
    have = key[ar, win] > 0
    rows = s["rows"]
    have_cur = cur != NONE
    curc = np.where(have_cur, cur, 0)
    s_win, s_cur = canon(S[ar, win]), S[ar, curc]
    cur_ok = have_cur & ~np.isnan(s_cur)
    with np.errstate(all="ignore"):
        near_hit = have_cur & (np.abs((rows["x"][win] - p).astype(F)) <= s["near"])
        if variant != "near_any_clip":
            near_hit &= rows["clip"][win].astype(np.int64) == L
        weak = cur_ok & ~((s_win - s_cur).astype(F) > s["margin"])
    if variant == "no_margin":
        weak[:] = False
    if variant == "cur_filtered_skip":
        weak &= cand[ar, curc]
    ignore = ~have | (running & (not s["flags"] & INTERRUPT)) | near_hit | weak
    cmds = np.zeros(n, dtype=CMD)
    cmds["instance"] = np.where(ignore, 0xFFFFFFFF, (base + ar) & 0xFFFFFFFF)
    cmds["clip"] = np.where(ignore, 0, rows["clip"][win])
    cmds["x"] = np.where(ignore, F(0), rows["x"][win])
    cmds["seconds"] = np.where(ignore, F(0), s["seconds"])
    res = np.zeros(n, dtype=RESULT)
    res["row"] = np.where(have, win, NONE)
    res["cur"] = cur
    res["score"] = np.where(have, s_win.view(np.uint32), QNAN).astype(np.uint32).view(F)
    res["cur_score"] = np.where(cur_ok, canon(s_cur).view(np.uint32), QNAN).astype(np.uint32).view(F)
    return cmds, res


def search(s, play, raw, filt=None, base=0, variant=None):
    """one call: (commands [n], results [n], scores [n, R])"""
    play = np.asarray(play, dtype=PLAY)
    L, p, _ = lead(s, play)
    cur = current_rows(s, L, p, variant)
    S = scores(s, query(s, cur, raw, variant), variant)
    cmds, res = decide(s, play, cur, S, candidates(s, filt, len(play), variant), base, variant)
    return cmds, res, S


def costs64(s, play, raw):
    """float64: the exact score sum q_d f_d + c_r of every row from the binary32 query, features and c_r, [n, R] (its negative is
    the cost 0.5 |q - f_r|^2 + bias_r up to a term that does not depend on r), and the bound of section 25 on a binary32
    score's distance from it: gamma_{D+2} (sum |q_d f_d| + |c_r|), plus (D + 2) 2^-150 for results that underflow"""
    play = np.asarray(play, dtype=PLAY)
    L, p, _ = lead(s, play)
    q = query(s, current_rows(s, L, p), raw).astype(np.float64)
    f, c = s["feats"].astype(np.float64), s["c"].astype(np.float64)
    with np.errstate(all="ignore"):
        S = q @ f.T + c[None, :]
        mag = np.abs(q) @ np.abs(f).T + np.abs(c)[None, :]
    u = 2.0 ** -24
    k = s["D"] + 2
    return S, (k * u / (1 - k * u)) * mag + k * 2.0 ** -150


def same_bits(a, b):
    """equal bit for bit, field by field; a NaN must be a NaN, payloads are free"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.names:
        ok = np.ones(a.shape, dtype=bool)
        for name in a.dtype.names:
            ok &= same_bits(a[name], b[name])
        return ok
    if a.dtype.kind == "f":
        return (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return a == b


# ---- the generator --------------------------------------------------------------------------------------------------
NS = (1, 31, 32, 33, 65, 257)
RS = (1, 31, 32, 33, 127, 1025)
DS = (4, 8, 36, 64)
FAMILIES = ("benign", "cancel", "subnormal", "large")
NKEYS, CLIP_FLAGS = (30, 32, 16, 12), (pm.LOOP, pm.LOOP, 0, 0)  # clip 2 gets no rows
NAN, INF = float("nan"), float("inf")
P_EDGES = (NAN, -1.0, 1e9, 0.0, -0.0, INF, -INF, 0.25)
FADE_EDGES = (0.0, 0.0, 2.0, 0.0, NAN, -1.0, 15.0, 0.0, INF, 0.0)
PAIR_BIT = 0x100
ZERO_BIT = 0x4000


def make_rows(R):
    """R rows over clips 0, 1 and 3, x strictly increasing within a clip from 0.5 on; tags: one of 8 group bits"""
    P, _ = periods(NKEYS, CLIP_FLAGS)
    use = [c for c in (0, 1, 3)][:max(1, min(3, R))]
    share = [R // len(use) + (1 if k < R % len(use) else 0) for k in range(len(use))]
    rows = np.zeros(R, dtype=ROW)
    r = 0
    for c, k in zip(use, share):
        rows["clip"][r:r + k] = c
        rows["x"][r:r + k] = (0.5 + np.arange(k) * ((float(P[c]) - 1.0) / k)).astype(F)
        r += k
    rows["tags"] = 1 << (np.arange(R) % 8)
    assert all(np.all(np.diff(rows["x"][rows["clip"] == c]) > 0) for c in use)
    return rows


def dup_pairs(R):
    """(source, copy) rows whose features and bias are made equal, across tile (32) boundaries and at both ends.  At the
    generator's sizes (R <= 1025, n <= 257) the default grid gives every slab one tile, so a tile boundary is a slab boundary
    too, no wave meets a second tile, and only wave 0 of a SHARE workgroup has work: what these pairs join is two registers of
    one lane or two slabs.  tests/match_grid_cases.py places pairs by the plan of a forced grid for everything else."""
    return [(a, b) for a, b in ((0, 1), (31, 32), (63, 64), (95, 97), (R - 2, R - 1), (31, R - 1)) if 0 <= a < b < R]


def pair_bit(k):
    """the tag bit of duplicated pair k: six below ZERO_BIT, as ever, and from the seventh on above it"""
    return PAIR_BIT << k if k < 6 else ZERO_BIT << (k - 5)


def grid(n, R, scores=False, share_groups=32, target=1024):
    """the search grid of csrc/match_launch.h for n instances and R rows (tests/test_match_launch_plan.py holds the two
    together): the layout, the workgroups in x (instance groups) and y (slabs), the tiles of a slab, and the counts it is made of"""
    ngroups, ntiles = (n + 31) // 32, (R + 31) // 32
    share = (not scores) and ngroups <= share_groups
    gx = ngroups if share else (ngroups + 3) // 4
    gy = min((target + gx - 1) // gx, ntiles)
    tps = (ntiles + gy - 1) // gy
    return dict(share=share, gx=gx, gy=(ntiles + tps - 1) // tps, tiles_per_slab=tps, ngroups=ngroups, ntiles=ntiles, n=n, R=R)


def wave_tiles(plan, slab):
    """the tiles [t0, t1) of each wave that walks slab `slab`: four waves and a quarter each under SHARE (a wave may have
    none), otherwise one entry, every wave of the workgroup walking the whole slab for its own instances"""
    tps = plan["tiles_per_slab"]
    t0, t1 = slab * tps, min(slab * tps + tps, plan["ntiles"])
    if not plan["share"]:
        return [(t0, t1)]
    quarter = (tps + 3) // 4
    return [(t0 + w * quarter, max(t0 + w * quarter, min(t0 + w * quarter + quarter, t1))) for w in range(4)]


def owner(row, plan):
    """(slab, wave, tile, half, register) of a row under a plan: the wave among those the slab's tiles are split over (always 0
    in the wave-owned layout), and the half-wave and accumulator register of the 32 x 32 result that hold the row: lane l has
    rows 8 (i >> 2) + 4 (l >> 5) + (i & 3), i = 0..15, of a tile"""
    tile = row // 32
    slab = tile // plan["tiles_per_slab"]
    wave = next(w for w, (t0, t1) in enumerate(wave_tiles(plan, slab)) if t0 <= tile < t1)
    r = row % 32
    return slab, wave, tile, (r >> 2) & 1, 4 * (r >> 3) + (r & 3)


def make_case(rng, n, R, D, family, idx, pairs=None):
    """one case; `pairs` is the list of duplicated (source, copy) rows, dup_pairs(R) where none is given"""
    rows = make_rows(R)
    if family == "benign":
        feats, qamp = rng.standard_normal((R, D)).astype(F), 1.0
    elif family == "cancel":  # large nearly equal terms: scores are small differences of large products
        feats, qamp = (1000.0 + rng.standard_normal((R, D))).astype(F), 1.0
    elif family == "subnormal":  # subnormal features, queries and products; rows of zeroes give c = -0
        feats, qamp = (rng.standard_normal((R, D)) * 10.0 ** rng.integers(-44, -18, (R, D))).astype(F), 1e-20
        feats[::7] = 0.0
    else:  # scores reach +-inf, and inf - inf gives NaN
        feats, qamp = (rng.standard_normal((R, D)) * 1e17).astype(F), 1e21
    raw = (feats[rng.integers(0, R, n)] + rng.standard_normal((n, D)).astype(F) * F(0.1) * np.abs(feats).max()).astype(F) if family != "large" else \
        (rng.standard_normal((n, D)) * qamp).astype(F)
    if family == "subnormal":
        raw = (rng.standard_normal((n, D)) * qamp * 10.0 ** rng.integers(-20, 1, (n, D))).astype(F)
    if family == "large" and n > 1:
        raw[1::8] = F(NAN)  # every score NaN: no winner
        raw[2::8, 0] = F(INF)
    rows["bias"] = (rng.random(R) * 0.01 * (1.0 if family in ("benign", "cancel") else (1e-30 if family == "subnormal" else 1e30))).astype(F)
    if family == "subnormal":
        # rows of zeroes have c = -0 and score -0 against a query of negative components; the row behind each has one feature
        # so small that its product with such a query rounds to +0: the two tie, and only if -0 counts as +0
        feats[1::7] = 0.0
        feats[1::7, 0] = F(-1.4e-45)
        rows["bias"][::7] = rows["bias"][1::7] = 0.0
        rows["tags"][::7] |= ZERO_BIT
        rows["tags"][1::7] |= ZERO_BIT
        raw[5::16] = (-1e-19 * (1.0 + rng.random(raw[5::16].shape))).astype(F)
    # duplicated rows win for the instances whose filter admits them: a bias below every other row's cost
    big = {"benign": 1e3, "cancel": 1e9, "subnormal": 1e-15, "large": 1e37}[family]
    for k, (a, b) in enumerate(dup_pairs(R) if pairs is None else pairs):
        feats[b] = feats[a]
        rows["bias"][a] = rows["bias"][b] = F(-big * (1.0 + k))
        rows["tags"][a] |= pair_bit(k)
        rows["tags"][b] |= pair_bit(k)
    mode = ("all", "none", "mixed")[idx % 3]
    pose = {"all": (1 << D) - 1, "none": 0, "mixed": sum(1 << d for d in range(0, D, 3))}[mode]
    norm = idx % 2 == 1
    mean = (rng.standard_normal(D) * 0.1 * qamp).astype(F) if norm else None
    scale = (1.0 + rng.random(D)).astype(F) if norm else None
    s = make_set(NKEYS, CLIP_FLAGS, rows, feats, pose_dims=pose, flags=INTERRUPT if idx % 4 < 2 else 0, seconds=0.2, mean=mean, scale=scale)
    # play states: every clip index (one past the end too), positions inside, on and outside the clips, fades of every kind
    play = np.zeros(n, dtype=PLAY)
    play["clip_a"], play["clip_b"] = rng.integers(0, len(NKEYS) + 2, n), rng.integers(0, len(NKEYS) + 2, n)
    play["x_a"], play["x_b"] = (rng.random(n) * 34.0 - 1.0).astype(F), (rng.random(n) * 34.0 - 1.0).astype(F)
    edge = np.arange(n) % 5 == 3
    play["x_a"][edge] = np.resize(np.array(P_EDGES, dtype=F), n)[edge]
    play["x_b"][edge] = np.resize(np.array(P_EDGES[::-1], dtype=F), n)[edge]
    exact = np.arange(n) % 5 == 1  # exactly on a row's x: <= against <
    ri = rng.integers(0, R, n)
    play["x_a"][exact], play["clip_a"][exact] = rows["x"][ri][exact], rows["clip"][ri][exact]
    play["fade"] = np.resize(np.array(FADE_EDGES, dtype=F), n)
    play["w"], play["speed"] = rng.random(n).astype(F), F(1.0)
    # filters: none, one group required, duplicated pairs excluded, everything excluded (no candidate), the current row out
    filt = np.zeros(n, dtype=FILTER)
    kind = rng.integers(0, 6, n)
    kind[0] = 0  # instance 0 admits every row: the duplicated rows tie at every size
    filt["require"] = np.where(kind == 1, 1 << rng.integers(0, 8, n), 0)
    filt["exclude"] = np.select([kind == 2, kind == 3, kind == 4, kind == 5], [PAIR_BIT, PAIR_BIT * 0x3F, 0xFFFFFFFF, 1 << rng.integers(0, 8, n)], 0)
    if family == "subnormal":
        filt["exclude"] |= ZERO_BIT  # the rows of zeroes are for the instances that ask for them
        filt["require"][5::16], filt["exclude"][5::16] = ZERO_BIT, PAIR_BIT * 0x3F
    c = dict(name=f"{family}-n{n}-R{R}-D{D}-{mode}", n=n, R=R, D=D, family=family, set=s, play=play, raw=raw, filt=filt, base=(0, 7, 4096)[idx % 3])
    # near and margin exactly on their thresholds for two instances of the case, found by the rule itself at near = margin = 0
    _, res, S = search(s, play, raw, filt, c["base"])
    L, p, _ = lead(s, play)
    ok = (res["row"] != NONE) & (res["cur"] != NONE)
    win = np.where(ok, res["row"], 0)
    with np.errstate(all="ignore"):
        dist = np.abs((rows["x"][win] - p).astype(F))
        gain = (res["score"] - res["cur_score"]).astype(F)
    j = np.flatnonzero(ok & (rows["clip"][win].astype(np.int64) == L) & np.isfinite(dist) & (dist > 0))
    if j.size:
        s["near"] = dist[j[len(j) // 2]]
    k = np.flatnonzero(ok & np.isfinite(gain) & (gain > 0) & ~((rows["clip"][win].astype(np.int64) == L) & (dist <= s["near"])))
    if k.size:
        s["margin"] = gain[k[len(k) // 2]]
    if mode == "all" and idx % 2 == 0:
        c["raw"] = None
    return c


_CASES = None


def cases():
    """24 cases: every n, every R and every D with every value family"""
    global _CASES
    if _CASES is None:
        _CASES, idx = [], 0
        for fi, family in enumerate(FAMILIES):
            for k in range(6):
                rng = np.random.default_rng(2500 + idx)
                _CASES.append(make_case(rng, NS[k], RS[(k + fi) % 6], DS[(k + 2 * fi + idx // 6) % 4], family, idx))
                idx += 1
    return _CASES
