"""CPU: the launch decisions of k_anim.hip's four launchers (csrc/anim_launch.h): tests/cpp/anim_launch_plan.cpp, a
stand-alone program over the stand-in HIP runtime (tests/cpp/hip_stub) built by g++ with AddressSanitizer and UBSan, builds
one valid parameter block for each of the sixteen (stage, tracks, fold) combinations and prints `ok threads lds` for it and
for every single violation of it: each pointer null in turn, each count at 0, at its maximum and one above, the path bytes
at 0, at their maximum and a word above, unequal path bytes, misaligned spring states and motion, a mask count without
masks.  The text must equal tests/golden/anim_launch_plan.txt, which was recorded from the predicates and the sixteen
launcher bodies that k_anim.hip ended in before anim_launch.h replaced them and is not regenerated: a launcher whose
decision says no launches nothing and reports nothing, so a dropped term is a difference here and nowhere else."""
import difflib
import os
import re
import subprocess

import pytest

from tests import cpp_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_anim_launch_plan_matches_the_recorded_one(tmp_path):
    exe = cpp_build.build("anim_launch_plan", tmp_path, cpp_build.HOST_ASAN)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-6000:]
    with open(os.path.join(ROOT, "tests", "golden", "anim_launch_plan.txt")) as f:
        want = f.read()
    # every combination's valid block launches, in the golden itself: a recording of sixteen refusals would pin nothing
    assert len(set(re.findall(r"^(\w+) valid: 1 \d+ \d+$", want, re.M))) == 16, want[:2000]
    if r.stdout != want:
        diff = "\n".join(list(difflib.unified_diff(want.splitlines(), r.stdout.splitlines(), "golden", "now", lineterm="", n=6))[:200])
        pytest.fail("the launch plans differ from tests/golden/anim_launch_plan.txt:\n" + diff)
