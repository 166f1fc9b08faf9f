"""-m gpu: k_match_search at every feature width, in both layouts, with several tiles per wave and several slabs, on the grid
cases of tests/match_grid_cases.py; everything is compared bit for bit with tests/match_model.py.  tests/test_gpu_match.py is
careful about values but runs three of the eight G = Dp / 8, and under the default tuning its sizes give every wave one tile.

In process, under the default tuning: all 16 widths D = 4 .. 64 at n = 33, R = 97 (SHARE, two groups, the second with one
live lane; four one-tile slabs, the last tile with one row), and the widths 8 g also at n = 1025, R = 65 (wave-owned, 33
groups: the last workgroup's last three waves return).  Each runs the scores call, the search with filters and the search
without.

In child processes, one per tuning and one at a time: MTR_MATCH_TUNE is read once per process, so a forced grid needs a
fresh interpreter (tests/match_grid_child.py, started by subprocess.run with the variable in its environment, never by
exec).  At n = 65, R = 300 -- three instance groups, the third with one live lane, and ten tiles, the last with 12 rows --
  32,1  SHARE, one slab of ten tiles: the waves get 3, 3, 3 and 1
  0,1   wave-owned, one slab: three waves pipeline ten tiles each, the fourth returns
  32,6  SHARE, two slabs of five: the waves get 2, 2, 1 and 0 tiles per slab, the slab winners meet in atomicMax
  0,2   wave-owned, two slabs of five
each with the four value families at eight widths, one per G, padded under two tunings and not under the other two, with a
tie of every kind the plan has (tests/test_match_grid_premises.py asserts all of this from the plan and the model, without
a device).  A child that times out, ends on a signal or returns any non-zero status fails its test and every later
parametrization of this module at once: nothing more is started on a GPU that may have faulted, and nothing is tried again.
The time limit is five times a child's measured wall time on an MI355X, rounded up: at most 3.7 s with the interpreter's
start and the cases' generation, of which 0.2 s lie between creating the device and closing it.

All tunings give the same answers by design, so no output can show that a forced tuning reached the launcher:
tests/test_match_launch_plan.py pins the parse of the string and the grid rule (csrc/match_launch.h) on the CPU, and the
launcher is the few lines that call them."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import match_grid_cases as gc
from tests import match_model as mm
from tests import player_model as pm
from tests.match_grid_child import run_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 20  # seconds
_child_failed = []  # the first child that did not end well: (tune, how)


def compare(c, got):
    """the raw outputs of one case against the model, the scores computed once"""
    S, with_filter, without = got
    s, n = c["set"], c["n"]
    L, p, _ = mm.lead(s, c["play"])
    cur = mm.current_rows(s, L, p)
    want = mm.scores(s, mm.query(s, cur, c["raw"]))
    bad = ~mm.same_bits(S, want)
    assert S.shape == want.shape and not bad.any(), f"{c['name']}: {int(bad.sum())} of {bad.size} scores differ, first at {np.argwhere(bad)[0]}"
    for what, filt, (cmds, res) in (("with filters", c["filt"], with_filter), ("without filters", None, without)):
        want_c, want_r = mm.decide(s, c["play"], cur, want, mm.candidates(s, filt, n), c["base"])
        for name, a, b in (("commands", cmds, want_c), ("results", res, want_r)):
            bad = np.flatnonzero(~mm.same_bits(a, b))
            assert a.shape == b.shape and bad.size == 0, \
                f"{c['name']} {what}: {bad.size} {name} differ, first at instance {bad[0]}: got {a[bad[0]]}, want {b[bad[0]]}; pairs {c['pairs']}"
    return want


@pytest.mark.parametrize("D", range(4, 68, 4))
def test_every_width_under_the_default_tuning(gpu_device, D):
    cases = [c for c in gc.width_cases() if c["D"] == D]
    assert len(cases) == (2 if D % 8 == 0 else 1)
    for c in cases:
        compare(c, run_case(gpu_device, c))


@pytest.mark.parametrize("tune", gc.TUNES)
def test_forced_grid_in_a_child_process(tmp_path, tune):
    if _child_failed:
        pytest.fail(f"not started: the child of tuning {_child_failed[0][0]} {_child_failed[0][1]}")
    out = tmp_path / "out.npz"
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, "-m", "tests.match_grid_child", tune, str(out)], cwd=ROOT, env={**os.environ, "MTR_MATCH_TUNE": tune},
                           capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired:
        _child_failed.append((tune, f"did not end within {CHILD_TIMEOUT} s"))
        pytest.fail(f"the child of tuning {tune} did not end within {CHILD_TIMEOUT} s")
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        _child_failed.append((tune, f"ended with status {r.returncode}"))
        pytest.fail(f"the child of tuning {tune} ended with status {r.returncode}:\n{r.stdout[-2000:]}{r.stderr[-4000:]}")
    cases = gc.forced_cases(tune)
    with np.load(out) as z:
        print(f"child {tune}: {wall:.2f} s, of which {float(z['gpu_seconds']):.2f} s from device create to close")
        nan = inf = zero = 0
        for k, c in enumerate(cases):
            got = (z[f"scores{k}"], (z[f"cmds_f{k}"].view(pm.CMD), z[f"res_f{k}"].view(mm.RESULT)), (z[f"cmds_n{k}"].view(pm.CMD), z[f"res_n{k}"].view(mm.RESULT)))
            S = compare(c, got)
            nan, inf, zero = nan + int(np.isnan(S).sum()), inf + int(np.isinf(S).sum()), zero + int((S == 0).sum())
    assert nan and inf and zero, "NaN, infinite and zero scores went through the forced grid"
