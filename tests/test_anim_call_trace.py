"""CPU: the stream traffic of every animation entry point (SPEC.md sections 13 to 24): tests/cpp/anim_call_trace.cpp, a
stand-alone program over the stand-in HIP runtime (tests/cpp/hip_stub) built by g++ with AddressSanitizer and UBSan, makes
each call once and prints every wait, record, copy, sync and launch with its streams, events and buffers named by first
appearance.  The text must equal tests/golden/anim_call_trace.txt, which was recorded before the animation host code was
moved into csrc/host_anim.cpp and is not regenerated (the controllers, event sets, blend sets and spring sets were appended
behind it later, recorded before their host code was changed, the earlier lines left as they were): a reordered wait, a lost record or a changed offset in a set's device
image is a difference here, not a wrong pose on the GPU."""
import difflib
import os
import re
import subprocess

import pytest

from tests import cpp_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_anim_call_trace_matches_the_recorded_one(tmp_path):
    exe = cpp_build.build("anim_call_trace", tmp_path, cpp_build.HOST_ASAN)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-6000:]
    # two such lines: where the first recording ended (598 operations, 34 rejected calls), and the whole run's, the last
    m = re.findall(r"anim_call_trace: ops=(\d+) rejected=(\d+) failed=(\d+)", r.stdout)
    assert len(m) == 2 and int(m[-1][0]) >= 792 and int(m[-1][1]) >= 70 and int(m[-1][2]) == 0, r.stdout[-2000:]
    with open(os.path.join(ROOT, "tests", "golden", "anim_call_trace.txt")) as f:
        want = f.read()
    if r.stdout != want:
        diff = "\n".join(list(difflib.unified_diff(want.splitlines(), r.stdout.splitlines(), "golden", "now", lineterm="", n=6))[:200])
        pytest.fail("the trace differs from tests/golden/anim_call_trace.txt:\n" + diff)
