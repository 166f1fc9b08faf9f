"""Numpy model of SPEC.md section 24 (spring bones after the IK chains), written from that text, its float64 twin and the
cases its tests share.

`step(T, Q, S, parents, springs, states, h, motion)` carries the rule out over the (T, Q, S) the chains left, in binary32,
one rounded numpy operation per operator, and gives the new rotations and the new state records bit for bit;
`dt=np.float64` carries the same operations out in float64 from the same binary32 inputs (its states come back as float64
arrays).  `sample(...)` puts section 16's stack (tests/anim_layers_model.py) and section 17's chains
(tests/anim_ik_model.py) in front and gives the local matrices.

springs: an array of SPRING [K]; states: an array of STATE [n, K]; motion: [n, 16] float32 or None; parents: one byte per
joint, a root 255 or itself.  `variant` names one deliberately wrong reading of the section (WRONG_VARIANTS).  `probe`: a
list that receives, per spring, which branch every instance took."""
import functools

import numpy as np

from tests import anim_ik_model as ik
from tests import anim_layers_model as lm
from tests import anim_model as am
from tests import anim_tracks_model as tm

F = np.float32
SPRING = np.dtype([("joint", "<u4"), ("flags", "<u4"), ("stiffness", "<f4"), ("drag", "<f4"), ("tail", "<f4", 3), ("pad0", "<f4"),
                   ("gravity", "<f4", 3), ("pad1", "<f4")])
STATE = np.dtype([("cur", "<f4", 3), ("live", "<u4"), ("prev", "<f4", 3), ("pad", "<u4")])
MAX_SPRINGS = 16
FLT_MAX = ik.FLT_MAX
WRONG_VARIANTS = ("carry_R", "prev_not_carried", "before_ik", "stale_parent", "old_length", "fresh_keeps_prev", "drag_inverted",
                  "paused_integrates", "list_order")


def rounds_of(parents, springs):
    """per spring its round: the spring joints among its joint's ancestors"""
    paths = ik.paths_of(parents)
    joints = {int(j) for j in springs["joint"]}
    return [sum(1 for a in paths[int(j)][:-1] if a in joints) for j in springs["joint"]]


def _finite(x, dt):
    with np.errstate(all="ignore"):
        return np.abs(x) <= dt(FLT_MAX)  # NaN compares false


def _carry(D, p, variant):
    """R^T (p - t) of the column-major rigid D [n, 16]"""
    u = p - D[:, 12:15]
    if variant == "carry_R":
        return (D[:, 0:3] * u[:, 0:1] + D[:, 4:7] * u[:, 1:2]) + D[:, 8:11] * u[:, 2:3]
    return np.stack([ik.dot3(D[:, 0:3], u), ik.dot3(D[:, 4:7], u), ik.dot3(D[:, 8:11], u)], axis=-1)


def step(T, Q, S, parents, springs, states, h, motion=None, variant=None, dt=F, probe=None, states64=None):
    """the springs of section 24 over (T [n, J, 3], Q [n, J, 4], S [n, J, 3]) of dtype dt: (the new Q, the new states).  h: the
    call's dt, any binary32.  The states come back as a STATE array (dt binary32) or as (cur, prev) [n, K, 3] float64.
    states64: such a pair from the float64 twin's previous step, read instead of the records' cur and prev (a chained run)"""
    assert variant is None or variant in WRONG_VARIANTS
    springs, states = np.asarray(springs).reshape(-1), np.asarray(states)
    n, K = states.shape
    assert 1 <= K <= MAX_SPRINGS and K == springs.size and Q.dtype == dt and states.dtype == STATE
    paths = ik.paths_of(parents)
    rounds = rounds_of(parents, springs)
    order = list(range(K)) if variant == "list_order" else sorted(range(K), key=lambda k: (rounds[k], k))
    Q = Q.copy()
    L = ik.local_matrix(T, Q, S)
    Q0, L0 = Q.copy(), L.copy()
    h32 = F(h)
    with np.errstate(all="ignore"):
        hh = dt(h32) if (h32 > 0 and h32 <= F(FLT_MAX)) else dt(0)
    paused = not hh > 0
    if variant == "paused_integrates":
        paused = False
    D = None if motion is None else np.asarray(motion, dtype=F).reshape(n, 16).astype(dt)
    cur_out, prev_out = np.zeros((n, K, 3), dtype=dt), np.zeros((n, K, 3), dtype=dt)
    for k in order:
        sp = springs[k]
        a = int(sp["joint"])
        Qs, Ls = (Q0, L0) if variant == "stale_parent" else (Q, L)
        with np.errstate(all="ignore"):
            pa = ik.world(Ls, paths[a], dt)[:, 3, :3]
            P = np.zeros((n, 4), dtype=dt)
            P[:, 3] = 1
            for i, j in enumerate(paths[a][:-1]):
                P = Qs[:, j].copy() if i == 0 else ik.qmul(P, Qs[:, j])
            qa = Q[:, a]
            tail = np.broadcast_to(sp["tail"].astype(dt), (n, 3))
            grav = np.broadcast_to(sp["gravity"].astype(dt), (n, 3))
            A0 = ik.qmul(P, qa)
            d0 = ik.qrot(A0, tail)
            Ln = ik.length(d0)
            r = pa + d0
            cur32, prev32 = (states["cur"][:, k], states["prev"][:, k]) if states64 is None else (states64[0][:, k], states64[1][:, k])
            dead = states["live"][:, k] == 0
            fresh = dead | ~(_finite(cur32, cur32.dtype.type).all(axis=-1) & _finite(prev32, cur32.dtype.type).all(axis=-1))
            c, p = cur32.astype(dt), prev32.astype(dt)
            if D is not None:
                c = _carry(D, c, variant)
                if variant != "prev_not_carried":
                    p = _carry(D, p, variant)
            c_old = c
            kk = dt(sp["stiffness"]) * hh
            clamped = not kk < 1
            kk = dt(1) if clamped else kk
            if not paused:
                drag = dt(sp["drag"]) if variant == "drag_inverted" else dt(1) - dt(sp["drag"])
                v = drag * (c - p)
                nn = ((c + v) + kk * (r - c)) + hh * grav
                p, c = c, nn
            if variant == "fresh_keeps_prev":  # the particle at rest, the record's prev: a kick
                cf, pf = r, prev32.astype(dt)
                if not paused:
                    vf = (dt(1) - dt(sp["drag"])) * (cf - pf)
                    cf, pf = ((cf + vf) + kk * (r - cf)) + hh * grav, cf
            else:
                cf, pf = r, r
            c = np.where(fresh[:, None], cf, c)
            p = np.where(fresh[:, None], pf, p)
            u = c - pa
            ul = ik.length(u)
            ref_len = ik.length(c_old - pa) if variant == "old_length" else Ln
            ref_len = np.where(fresh, Ln, ref_len)
            ok = (ul > 0) & (ul <= dt(FLT_MAX)) & (Ln > 0)
            c = np.where(ok[:, None], pa + (ref_len / ul)[:, None] * u, r)
            cur_out[:, k], prev_out[:, k] = c, p
            guard, qa1, _ = ik._aim(pa, P, qa, tail, c, np.ones(n, dtype=dt), None)
            Q[:, a] = np.where(guard[:, None], qa1, qa)
            L[:, a] = ik.local_matrix(T[:, a], Q[:, a], S[:, a])
        if probe is not None:
            probe.append(dict(k=k, joint=a, round=rounds[k], dead=dead, fresh=fresh, nonfinite=fresh & ~dead, paused=paused, carried=D is not None,
                              clamped=clamped and not paused, ul_zero=~(ul > 0) & np.isfinite(ul), L_zero=~(Ln > 0), guard=guard, pa=pa, r=r, L=Ln,
                              plain=~fresh & guard & (not paused)))
    if dt != F:
        return Q, (cur_out, prev_out)
    out = np.zeros((n, K), dtype=STATE)
    out["cur"], out["prev"], out["live"] = cur_out, prev_out, 1
    return Q, out


def sample(clips, layers, njoints, masks, parents, springs, states, h, motion=None, chains=None, targets=None, variant=None, dt=F, probe=None,
           tqs=None, states64=None):
    """the local matrices [n, njoints, 16] of dtype dt and the new states of section 24: the stack, the chains (chains None:
    none), the springs.  tqs: ik.stack_tqs's result, when the caller has it"""
    T, Q, S = (v.astype(dt) for v in (tqs if tqs is not None else ik.stack_tqs(clips, layers, njoints, masks)))
    if variant == "before_ik":
        Q, st = step(T, Q, S, parents, springs, states, h, motion, None, dt, probe)
        if chains is not None:
            Q = ik.solve(T, Q, S, parents, chains, targets, None, dt)
    else:
        if chains is not None:
            Q = ik.solve(T, Q, S, parents, chains, targets, None, dt)
        Q, st = step(T, Q, S, parents, springs, states, h, motion, variant, dt, probe, states64)
    out = ik.local_matrix(T, Q, S)
    assert out.dtype == dt
    return out, st


# ---- inputs shared by the tests -----------------------------------------------------------------------------------
def make_springs(joints, tails, stiffness=30.0, drag=0.2, gravity=(0.0, -2.0, 0.0), dtype=SPRING):
    sp = np.zeros(len(joints), dtype=dtype)
    sp["joint"] = joints
    sp["tail"] = tails
    sp["stiffness"], sp["drag"] = stiffness, drag
    sp["gravity"] = gravity
    return sp


def rigid(rng, n, angle=0.2, trans=0.5):
    """n rigid deltas [n, 16] float32, column-major: a rotation of up to `angle` about a random axis, a translation"""
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=-1, keepdims=True)
    th = rng.uniform(-angle, angle, n)
    x, y, z = ax.T
    c, s = np.cos(th), np.sin(th)
    C = 1 - c
    R = np.stack([np.stack([c + x * x * C, y * x * C + z * s, z * x * C - y * s], -1),  # column 0
                  np.stack([x * y * C - z * s, c + y * y * C, z * y * C + x * s], -1),
                  np.stack([x * z * C + y * s, y * z * C - x * s, c + z * z * C], -1)], 1)
    D = np.zeros((n, 4, 4))
    D[:, :3, :3] = R
    D[:, 3, :3] = rng.uniform(-trans, trans, (n, 3))
    D[:, 3, 3] = 1
    return D.reshape(n, 16).astype(F)


# name: (J, parents, spring joints in list order, IK chains or None)
def _skeletons():
    strands = np.array([255, 0, 1, 2, 0, 4, 5, 0, 7], dtype=np.uint8)  # 0 - 1 - 2 - 3, 0 - 4 - 5 - 6, 0 - 7 - 8
    aim = np.zeros(2, dtype=ik.CHAIN)
    aim["kind"] = [ik.AIM, ik.TWO_BONE]
    aim["joint"] = [(1, 0, 0), (4, 5, 6)]
    aim["axis"] = [(0.2, 1.0, 0.1), (0, 0, 0)]
    return {
        "chain4": (4, ik.skeleton(4), [1, 2, 3], None),                 # one strand, 3 rounds
        "strands9": (9, strands, [3, 2, 6, 5], None),                   # two strands, child first: 2 rounds
        "waves70": (70, ik.skeleton(70), [66, 30, 60], None),           # 66's spring parent 60 lies in the other wave
        "ik9": (9, strands, [2, 3, 6, 8], aim),                         # chains on an ancestor (1) and on a spring joint's limb
    }


SKELETONS = _skeletons()
H_PAUSED = [0.0, -1.0 / 60.0, float("nan"), float("inf")]


def make_case(name, seed, n=24, h=1.0 / 60.0, with_motion=True, stiffness=30.0, tiny_tail=False, kind="uniform", dtype_spring=SPRING,
              dtype_state=STATE, dtype_layer=lm.LAYER, dtype_target=ik.TARGET):
    """One call on states two warm-up steps old, with the edges written over the first instances (0 always, the others where
    n >= 5): 0: a zeroed record; 1: live but cur NaN; 2: prev +inf; 3: a user-written state (finite, far off); 4 (paused calls
    without motion, round-0 springs): cur exactly at the joint, so that ul == 0.  The rest is the plain path."""
    J, parents, joints, chains = SKELETONS[name]
    rng = np.random.default_rng(seed)
    clips = ik.uniform_scale(am.random_clips(rng, J, trans=2.0)) if kind == "uniform" else tm.random_track_clips(rng, J, trans=2.0)
    masks = lm.random_masks(rng, J)
    ly0 = lm.layer_states(rng, clips, n=n, L=2, dtype=dtype_layer)
    ly0["x"] = rng.uniform(0.0, 30.0, ly0["x"].shape).astype(F)
    ly0["clip"] %= len(clips)
    tails = rng.uniform(0.3, 1.5, (len(joints), 3)) * rng.choice([-1.0, 1.0], (len(joints), 3))
    if tiny_tail:
        tails[0] = (1e-12, 0.0, 0.0)  # L > 0, but pa + (L / ul) u rounds to pa: the aim's guard fails
    springs = make_springs(joints, tails, stiffness=stiffness, drag=0.2, gravity=(0.0, -2.0, 0.5), dtype=dtype_spring)
    springs["stiffness"] = stiffness * rng.uniform(0.5, 1.5, len(joints))
    springs["drag"] = rng.uniform(0.05, 0.5, len(joints))
    targets = None
    if chains is not None:
        tqs0 = ik.stack_tqs(clips, ly0, J, masks)
        targets = ik.make_targets(rng, tqs0, parents, chains, dtype=dtype_target)
        targets["w"] = np.where(np.isfinite(targets["w"]) & (targets["w"] > 0.3), targets["w"], 1.0)
        targets["pos"] = np.nan_to_num(targets["pos"], nan=1.0, posinf=2.0, neginf=-2.0)
        targets["pole"] = np.nan_to_num(targets["pole"], nan=1.0, posinf=2.0, neginf=-2.0)
    st = np.zeros((n, len(joints)), dtype=STATE)
    ly = ly0
    for _ in range(2):  # the warm-up: the clips move on by a third of a key per frame
        _, st = sample(clips, ly, J, masks, parents, springs.astype(SPRING), st, 1.0 / 60.0, None, chains, targets)
        ly = ly.copy()
        ly["x"] += F(1.0 / 3.0)
    motion = rigid(rng, n) if with_motion else None
    st = st.astype(dtype_state)
    st[0] = np.zeros((), dtype=dtype_state)
    if n >= 5:
        st["cur"][1, :, 1] = np.nan
        st["prev"][2, :, 0] = np.inf
        st["cur"][3] += F(3.0)
        st["prev"][3] -= F(1.0)
        st["pad"][3] = 0xDEADBEEF
    with np.errstate(all="ignore"):
        paused = not (F(h) > 0 and F(h) <= F(FLT_MAX))
    if paused and not with_motion and n >= 5:
        probe = []
        sample(clips, ly, J, masks, parents, springs.astype(SPRING), st.astype(STATE), h, None, chains, targets, probe=probe)
        for pr in probe:
            if pr["round"] == 0:
                st["cur"][4, pr["k"]] = pr["pa"][4]
    return dict(name=name, kind=kind, J=J, parents=parents, springs=springs, chains=chains, clips=clips, masks=masks, layers=ly, targets=targets, states=st,
                motion=motion, h=F(h), n=n)


def run(case, variant=None, dt=F, probe=None, states=None, motion="case", h=None):
    return sample(case["clips"], case["layers"], case["J"], case["masks"], case["parents"], case["springs"].astype(SPRING),
                  (case["states"] if states is None else states).astype(STATE), case["h"] if h is None else h,
                  case["motion"] if isinstance(motion, str) else motion, case["chains"], case["targets"], variant, dt, probe)


@functools.lru_cache(maxsize=None)
def cases():
    """the generator's cases; nobody writes into them"""
    out = []
    seed = 2400
    for name in SKELETONS:
        for with_motion in (True, False):
            out.append(make_case(name, seed, with_motion=with_motion))
            out.append(make_case(name, seed + 1, h=1.0 / 30.0, with_motion=with_motion, stiffness=45.0))  # kk clamps on some springs
            seed += 2
    for i, h in enumerate(H_PAUSED):
        out.append(make_case(list(SKELETONS)[i % len(SKELETONS)], seed + i, h=h, with_motion=i % 2 == 0))
    out.append(make_case("strands9", seed + 10, h=0.0, with_motion=False))
    out.append(make_case("chain4", seed + 11, tiny_tail=True))
    out.append(make_case("ik9", seed + 12, tiny_tail=True, with_motion=False))
    return tuple(out)
