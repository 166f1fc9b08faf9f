"""CPU: the numpy model of SPEC.md section 17 (tests/anim_ik_model.py) against the section's own statements.

On the float64 version of the rule, from (T, Q, S) whose rotations are renormalised in float64 and whose scales are
uniform (what "exact" is stated for: the world matrices are then similarities and P is their rotation), for every chain
whose guard holds and whose weight is 1: the re-folded end joint lies within 1e-9 (la + lb) of p_c'; with POLE the middle
joint lies in the half plane of p_a, g and the pole; with AIM the rotated axis is parallel to v.  Measured here, 256
instances, J = 65, K = 4: end joint 3.9e-15 (la + lb), out of the pole's plane 2.3e-15, sine of the aim's angle 5.3e-15.

binary32 against float64 from the same binary32 (T, Q, S), a figure that is printed and not asserted (fromto has no bound near
antiparallel vectors): the median end-joint distance is 1.9e-7 (la + lb) at J = 3, 2.6e-6 at J = 65 and 3.1e-5 at J = 256
(depth 210, median reach 5.6e3); the largest are single ill-conditioned instances, 2.1e-4, 0.43 and 1.97 (la + lb).

Every weight 0 is section 16 bit for bit; chains the guard stops are untouched bit for bit; every wrong reading of the
section changes some instance."""
from fractions import Fraction

import numpy as np
import pytest

from tests import anim_ik_model as ik
from tests import anim_layers_model as lm
from tests import anim_model as am

F = np.float32
N = ik.N_INST


def _inputs(J, K, uniform=False, L=3):
    rng = np.random.default_rng(170 + J + K)
    clips = am.random_clips(rng, J)
    if uniform:
        clips = ik.uniform_scale(clips)
    masks = lm.random_masks(rng, J)
    ly = lm.layer_states(rng, clips, n=N, L=L)
    parents = ik.skeleton(J)
    chains = ik.default_chains(parents, K)
    tqs = ik.stack_tqs(clips, ly, J, masks)
    tg = ik.make_targets(rng, tqs, parents, chains)
    return clips, masks, ly, parents, chains, tqs, tg


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_fma32_is_the_exact_fma():
    rng = np.random.default_rng(3)
    a, b, c = ((rng.normal(size=3000) * 10.0 ** rng.integers(-18, 18, 3000)).astype(F) for _ in range(3))
    c[:1500] = -(a[:1500].astype(np.float64) * b[:1500]).astype(F)  # cancellation: the sum is the product's rounding error
    a[-3:], b[-3:], c[-3:] = [0.0, -0.0, 1e-30], [-1.0, 0.0, 1e-30], [0.0, 0.0, -0.0]
    got = ik.fma32(a, b, c)
    for i in range(a.size):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        g = got[i]
        lo, hi = np.nextafter(g, F(-np.inf)), np.nextafter(g, F(np.inf))
        err = abs(exact - Fraction(float(g)))
        assert err <= abs(exact - Fraction(float(lo))) and err <= abs(exact - Fraction(float(hi))), (a[i], b[i], c[i], g)
    assert (_bits(got[-3:]) == 0).all(), "-0 + 0, and an underflow to zero, are +0"


@pytest.mark.filterwarnings("ignore::RuntimeWarning")  # the generator's infinite targets meet np.cross below
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("J", [3, 65])
def test_float64_properties(J, K):
    clips, masks, ly, parents, chains, tqs, tg = _inputs(J, K, uniform=True)
    T, Q, S = (v.astype(np.float64) for v in tqs)
    assert (S[..., 0] == S[..., 1]).all() and (S[..., 0] == S[..., 2]).all() and (S > 0).all()
    Q = Q / np.sqrt((Q * Q).sum(-1, keepdims=True))
    probe = []
    Qn = ik.solve(T, Q, S, parents, chains, tg, dt=np.float64, probe=probe)
    assert np.isfinite(Qn).all()
    worst = dict(end=0.0, plane=0.0, aim=0.0)
    for p in probe:
        full = p["hit"] & (p["e"] == 1) & np.isfinite(p["g"]).all(-1)  # AIM's guard lets an infinite target through: no direction
        assert full.sum() > N // 4
        if p["kind"] == ik.TWO_BONE:
            reach = p["la"] + p["lb"]
            end = np.linalg.norm(p["pc_new"] - p["pc1"], axis=-1) / reach
            assert (end[full] <= 1e-9).all(), f"chain {p['k']}: end joint {end[full].max():.3e} (la + lb) from p_c'"
            worst["end"] = max(worst["end"], float(end[full].max()))
            if chains[p["k"]]["flags"] & ik.POLE:
                rel = p["pb_new"] - p["pa"]
                normal = np.cross(p["n"], p["hh"])
                off = np.abs((rel * normal).sum(-1)) / reach
                side = (rel * p["hh"]).sum(-1) / reach
                toward = ((p["pole"] - p["pa"]) * p["hh"]).sum(-1)
                assert (off[full] <= 1e-9).all() and (side[full] >= -1e-9).all() and (toward[full] > 0).all(), "the pole's half plane"
                worst["plane"] = max(worst["plane"], float(off[full].max()))
        else:
            axis = np.broadcast_to(chains[p["k"]]["axis"].astype(np.float64), (N, 3))
            cur = ik.qrot(ik.qmul(p["P"], p["Qa"]), axis)
            v = p["v"]
            sin = np.linalg.norm(np.cross(cur, v), axis=-1) / (np.linalg.norm(cur, axis=-1) * np.linalg.norm(v, axis=-1))
            assert (sin[full] <= 1e-9).all() and ((cur * v).sum(-1)[full] > 0).all(), f"chain {p['k']}: the axis is off v by {sin[full].max():.3e}"
            worst["aim"] = max(worst["aim"], float(sin[full].max()))
    print(f"float64, J = {J}, K = {K}: end joint {worst['end']:.3e} (la + lb), out of the pole's plane {worst['plane']:.3e}, aim {worst['aim']:.3e}")


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("J", [3, 65, 256])
def test_binary32_model(J, K):
    clips, masks, ly, parents, chains, tqs, tg = _inputs(J, K)
    probe, probe64 = [], []
    out = ik.sample(clips, ly, J, masks, parents, chains, tg, tqs=tqs, probe=probe)
    assert out.dtype == F and np.isfinite(out).all()
    stack = lm.sample(clips, ly, J, masks)
    # every weight 0 (on all instances, and on the two instances the generator leaves so): section 16, bit for bit
    zero = tg.copy()
    zero["w"] = np.where(np.arange(N)[:, None] % 2 == 0, np.float32(0), np.float32("nan"))
    zero["pos"][::3] = np.nan
    assert (_bits(ik.sample(clips, ly, J, masks, parents, chains, zero, tqs=tqs)) == _bits(stack)).all()
    idle = (am.clamp_w(tg["w"]) == 0).all(axis=1)
    assert idle.sum() >= 2 and (_bits(out[idle]) == _bits(stack[idle])).all()
    # the guard: under 1 % of the chains with e > 0 and finite targets are left untouched; what it stops is untouched bit
    # for bit (an instance none of whose chains is solved is section 16's)
    active = stopped = 0
    solved = np.zeros(N, dtype=bool)
    for p in probe:
        finite = np.isfinite(p["g"]).all(-1) & np.isfinite(p["pole"]).all(-1)
        active += int((p["active"] & finite).sum())
        stopped += int((p["active"] & finite & ~p["guard"]).sum())
        unusable = np.isnan(p["g"]).any(-1) if p["kind"] == ik.AIM else ~np.isfinite(p["g"]).all(-1)
        assert not (p["guard"] & unusable).any(), "a NaN target stops the chain, an infinite one a TWO_BONE chain"
        solved |= p["hit"]
    assert stopped < 0.01 * active, f"{stopped} of {active} chains stopped by the guard"
    assert (~solved).sum() >= (2 if K == 4 else 20) and (_bits(out[~solved]) == _bits(stack[~solved])).all()
    # binary32 against float64 from the same (T, Q, S)
    ik.sample(clips, ly, J, masks, parents, chains, tg, tqs=tqs, dt=np.float64, probe=probe64)
    dist = []
    for p, q in zip(probe, probe64):
        if p["kind"] == ik.TWO_BONE:
            both = p["hit"] & q["hit"]
            dist.append((np.linalg.norm(p["pc_new"].astype(np.float64) - q["pc_new"], axis=-1) / (q["la"] + q["lb"]))[both])
    dist = np.concatenate(dist)
    print(f"binary32 against float64, J = {J}, K = {K}: the end joints differ by at most {dist.max():.3e} (la + lb), "
          f"median {np.median(dist):.3e}, 99th percentile {np.percentile(dist, 99):.3e}")
    # every wrong reading shows
    for v in ik.WRONG_VARIANTS:
        if v == "parallel" and K == 1 or v == "conj_wrong_side" and J == 3 and K == 1:
            continue  # one chain has no order; under a root a, P is the identity, which commutes
        wrong = ik.sample(clips, ly, J, masks, parents, chains, tg, variant=v, tqs=tqs)
        assert (_bits(wrong) != _bits(out)).any(axis=(1, 2)).sum() >= 1, v
