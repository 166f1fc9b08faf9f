"""CPU: properties of the root-motion rule (SPEC.md section 19) on its numpy model, tests/root_model.py.

In float64: a run of steps composes to the one long step, inside a cycle and across the seam in both directions, and a run of
whole cycles is a power of the cycle's own delta -- the seam rule telescopes.  Binary32 against float64 per call: the section's
bound k u sum|terms|.  Recorded, not bounded: the drift of 20 000 accumulated binary32 steps.  And nine wrong readings of the
section each change the generated cases."""
import numpy as np
import pytest

from tests import root_model as rm

F = np.float32
CASES = rm.cases()


TRAJ = rm.walk_clip()
ROOT = (0, np.array([rm.CYCLIC], dtype=np.uint32))
L = 30.0


def steps_of(x, dx):
    st = np.zeros((len(x), 1), dtype=rm.STEP)
    st["x"][:, 0], st["dx"][:, 0] = x, dx
    assert np.array_equal(st["x"][:, 0].astype(np.float64), x, equal_nan=True) and np.array_equal(st["dx"][:, 0].astype(np.float64), dx, equal_nan=True), "exact in binary32"
    return st


def d64(x, dx):
    return rm.deltas(TRAJ, ROOT, steps_of(np.atleast_1d(np.asarray(x, dtype=np.float64)), np.atleast_1d(np.asarray(dx, dtype=np.float64))), np.float64, np.float64)


def chain(D):
    out = np.eye(4).T.reshape(1, 16).copy()
    for d in D:
        out = rm.mul(out, d[None, :], np.float64)
    return out[0]


@pytest.mark.parametrize("x0,dx,k", [(10.25, 0.375, 8), (27.5, 0.375, 16), (1.5, -0.375, 16), (0.0, 0.375, 80), (0.0, -0.375, 80), (29.625, 0.375, 1)])
def test_steps_telescope_in_float64(x0, dx, k):
    """k steps of dx compose to the one step of k dx (at most one cycle long), inside a cycle and across the seam in both
    directions; the host wraps x or not, as it likes"""
    x = x0 + dx * np.arange(k)
    path = abs(dx) * k
    one = d64(x0, dx * k)[0]
    for xs in (x, x - L * np.floor(x / L), x + 7 * L):
        got = chain(d64(xs, np.full(k, dx)))
        err = np.abs(got - one).max()
        print(f"x0 {x0} dx {dx} k {k}: {err:.2e} over a path of {path}")
        assert err <= 1e-9 * max(path, 1.0)


@pytest.mark.parametrize("cycles,dx", [(3, 7.5), (5, -7.5), (246, 3.75)])
def test_whole_cycles_are_a_power_of_the_cycle_delta(cycles, dx):
    per = int(round(L / abs(dx)))
    G = d64(0.0, np.copysign(L, dx))[0]  # the one step of a whole cycle: delta(0 -> L), or delta(L -> 0) backwards
    assert np.abs(G - np.eye(4).reshape(16)).max() > 0.1, "the cycle moves"
    x = dx * np.arange(per * cycles)
    got = chain(d64(x, np.full(per * cycles, dx)))
    want = chain(np.repeat(G[None, :], cycles, axis=0))
    path = L * cycles
    err = np.abs(got - want).max()
    print(f"{cycles} cycles: {err:.2e} over a path of {path}, position {np.abs(want[12:15]).max():.2f}")
    assert err <= 1e-9 * path


def test_two_seams_and_not_finite_move_nothing():
    """the guard: a step that would cross a second seam (r1 outside [0, L]), a NaN and an infinite dx move nothing; a step of up
    to one cycle never does, and one just over a cycle that crosses one seam is the cycle and a bit"""
    D = d64([3.0, 3.0, 3.0, 3.0, 3.0], [58.0, -34.0, np.nan, np.inf, -np.inf])
    assert (D == np.eye(4).reshape(16)).all()
    over = float(np.nextafter(F(L), F(np.inf)))
    got = d64([3.0], [over])[0]
    want = chain(np.concatenate([d64([3.0], [27.0]), d64([0.0], [3.0]), d64([3.0], [over - L])]))
    assert np.abs(got - want).max() <= 1e-9 * L


def _per_instance(mask, n):
    return mask.reshape(n, -1).any(axis=1)


def test_binary32_stays_inside_the_bound():
    """|binary32 - exact| <= k u sum|terms| per element of D, k = rm.k_ops (section 19); instances with an nlerp call of
    |d| < 8u, a NaN or an overflow are left out; the calls left out for |d| < 8u stay under 1 % of the calls"""
    worst, calls, near_calls, compared = 0.0, 0, 0, 0
    for c in CASES:
        n, S = c["n"], c["S"]
        got = rm.deltas(c["traj"], c["root"], c["steps"]).astype(np.float64)
        tr = rm.Trace()
        val, mag = rm.deltas(c["traj"], c["root"], c["steps"], "V", F, trace=tr)
        near = np.zeros(n, dtype=bool)
        for m in tr.near:
            near |= _per_instance(m, n)
        calls += sum(x.size for x in tr.d)
        near_calls += sum(int(m.sum()) for m in tr.near)
        ok = ~near & np.isfinite(got).all(axis=1) & np.isfinite(val).all(axis=1) & np.isfinite(mag).all(axis=1)
        bound = rm.k_ops(c["kind"], S) * rm.U * mag[ok]
        err = np.abs(got[ok] - val[ok])
        with np.errstate(all="ignore"):
            frac = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
        compared += int(ok.sum())
        if frac.size:
            worst = max(worst, float(frac.max()))
    print(f"binary32 model: at most {worst:.3f} of the bound over {compared} instances; {near_calls} of {calls} nlerp calls with |d| < 8u ({near_calls / calls:.4%})")
    assert compared > 2000
    assert near_calls < 0.01 * calls
    assert worst <= 1.0


def test_drift_of_20000_binary32_steps_is_recorded():
    """not a bound: what 20 000 accumulated binary32 steps of dx = 0.37 leave, against the same walk in float64 (x accumulated
    in binary32 by the host and wrapped at L, part of the difference)"""
    n, dx = 20000, F(0.37)
    xs = np.empty(n, dtype=F)
    x = F(0)
    for i in range(n):
        xs[i] = x
        x = F(x + dx)
        if x >= F(L):
            x = F(x - F(L))
    st = np.zeros((n, 1), dtype=rm.STEP)
    st["x"][:, 0], st["dx"][:, 0] = xs, dx
    D32 = rm.deltas(TRAJ, ROOT, st)
    M = np.eye(4, dtype=F).reshape(1, 16)
    for i in range(n):
        M = rm.mul(M, D32[i:i + 1], F)
    ideal = 0.37 * np.arange(n)
    r64 = ideal - L * np.floor(ideal / L)
    (T, Q), _, _, _ = rm.step_deltas(TRAJ, ROOT, _steps64(r64, 0.37), np.float64, np.float64)  # positions past what a binary32 record holds
    W = np.eye(4).reshape(1, 16)
    D64 = np.stack(rm.local_matrix(T, Q), axis=-1)
    for i in range(n):
        W = rm.mul(W, D64[i:i + 1], np.float64)
    M, W = M[0].astype(np.float64).reshape(4, 4), W[0].reshape(4, 4)
    pos = np.abs(M[3, :3] - W[3, :3]).max()
    rot = np.abs(M[:3, :3] - W[:3, :3]).max()
    R = M[:3, :3]
    orth = np.abs(R @ R.T - np.eye(3)).max()
    print(f"20 000 steps: position error {pos:.2e} at a position of magnitude {np.abs(W[3, :3]).max():.1f}, rotation error {rot:.2e}, off orthonormal by {orth:.2e}")
    assert np.isfinite([pos, rot, orth]).all()
    assert pos < 1.0 and rot < 0.1 and orth < 0.01, "a gross error, not rounding"


class _Steps64:
    """steps whose x and dx are float64 arrays: what rm.step_deltas reads of a STEP array"""

    def __init__(self, x, dx):
        self.f = {"clip": np.zeros(len(x), dtype=np.uint32), "x": x, "dx": np.full(len(x), dx), "w": np.zeros(len(x))}

    def reshape(self, *_):
        return self

    @property
    def shape(self):
        return (len(self.f["x"]),)

    def __getitem__(self, k):
        return self.f[k]


def _steps64(x, dx):
    return _Steps64(x, dx)


def test_wrong_readings_change_the_cases():
    """each of the nine wrong readings changes at least one case that can show it; the shares of instances go into SPEC.md"""
    lines = []
    for v in rm.WRONG_VARIANTS:
        changed_cases = able = 0
        changed = total = 0
        for c in CASES:
            if not rm.can_show(v, c):
                continue
            able += 1
            want = rm.root_motion(c["M"], c["traj"], c["root"], c["steps"])
            wrong = rm.root_motion(c["M"], c["traj"], c["root"], c["steps"], variant=v)
            diff = ~rm.same_bits(want, wrong).all(axis=1)
            changed += int(diff.sum())
            total += c["n"]
            changed_cases += bool(diff.any())
        lines.append(f"{v}: {changed_cases} of {able} cases, {100.0 * changed / max(total, 1):.0f} % of their instances")
        assert able and changed_cases >= 1, v
    print("\n".join(lines))
