"""CPU: the grid of k_match_search and the reading of MTR_MATCH_TUNE (csrc/match_launch.h): tests/cpp/match_launch_plan.cpp, a
stand-alone program built by g++ with AddressSanitizer and UBSan, prints the parse of a list of tuning strings and, for the
default tuning and the four that tests/test_gpu_match_grid.py forces, the plan of every n in 1..1100 and 2040..2060 at eight
row counts, for a search and for a scores call.  The text must equal tests/golden/match_launch_plan.txt, which was recorded
from the launcher's own lines before match_launch.h replaced them and is not regenerated: every grid gives the same winners,
so a changed rule, or a string read differently, is a difference here and nowhere else.  The Python model's grid(), which the
grid cases are placed by, is held to the same text for every n of every run."""
import difflib
import os
import re
import subprocess

import pytest

from tests import cpp_build
from tests import match_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNES = ("none", "32,1", "0,1", "32,6", "0,2")
RS = (1, 31, 32, 33, 300, 1025, 4100, 65536)
NS = list(range(1, 1101)) + list(range(2040, 2061))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "match_launch_plan.txt")) as f:
        return f.read()


def test_match_launch_plan_matches_the_recorded_one(tmp_path, golden):
    exe = cpp_build.build("match_launch_plan", tmp_path, cpp_build.HOST_ASAN)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-6000:]
    if r.stdout != golden:
        diff = "\n".join(list(difflib.unified_diff(golden.splitlines(), r.stdout.splitlines(), "golden", "now", lineterm="", n=6))[:200])
        pytest.fail("the grid plans differ from tests/golden/match_launch_plan.txt:\n" + diff)


def test_the_recording_holds_what_it_is_for(golden):
    """a recording of defaults only, or of one layout, would pin nothing"""
    tune = dict(re.findall(r'^tune (none|".*"): (\d+ \d+)$', golden, re.M))
    assert tune["none"] == tune['""'] == tune['"32"'] == tune['"32,0"'] == tune['"32,65536"'] == tune['"x32,6"'] == "32 1024"
    assert (tune['"32,1"'], tune['"0,1"'], tune['"32,6"'], tune['"0,2"'], tune['"32,65535"'], tune['"32,6x"']) == ("32 1", "0 1", "32 6", "0 2", "32 65535", "32 6")
    heads = re.findall(r"^plan tune=(\S+) share_groups=(\d+) target=(\d+) scores=(\d) R=(\d+)$", golden, re.M)
    assert len(heads) == len(set(heads)) == len(TUNES) * 2 * len(RS) and {h[0] for h in heads} == set(TUNES) and {int(h[4]) for h in heads} == set(RS)
    runs = re.findall(r"^  n=\d+\.\.\d+: share=(\d) gx=\d+ gy=(\d+) tiles_per_slab=(\d+)$", golden, re.M)
    assert {r[0] for r in runs} == {"0", "1"} and any(int(r[1]) > 1 and int(r[2]) > 1 for r in runs), "both layouts, several slabs of several tiles"


def test_the_models_grid_is_the_launchers_for_every_n(golden):
    seen, head = {}, None
    for line in golden.splitlines():
        m = re.match(r"plan tune=(\S+) share_groups=(\d+) target=(\d+) scores=(\d) R=(\d+)$", line)
        if m:
            head = (m[1], int(m[2]), int(m[3]), m[4] == "1", int(m[5]))
            continue
        m = re.match(r"  n=(\d+)\.\.(\d+): share=(\d) gx=(\d+) gy=(\d+) tiles_per_slab=(\d+)$", line)
        if not m:
            assert line.startswith("tune "), line
            continue
        name, share_groups, target, scores, R = head
        want = dict(share=m[3] == "1", gx=int(m[4]), gy=int(m[5]), tiles_per_slab=int(m[6]))
        for n in range(int(m[1]), int(m[2]) + 1):
            g = mm.grid(n, R, scores, share_groups, target)
            assert {k: g[k] for k in want} == want, (head, n, g, want)
            assert (name, scores, R, n) not in seen
            seen[name, scores, R, n] = True
    assert len(seen) == len(TUNES) * 2 * len(RS) * len(NS) and all((t, s, R, n) in seen for t in TUNES for s in (False, True) for R in RS for n in (NS[0], NS[1099], NS[1100], NS[-1]))
    # the defaults of grid() are the defaults of the parse
    assert mm.grid(993, 4100) == mm.grid(993, 4100, False, 32, 1024) and mm.grid(1025, 4100)["share"] is False
