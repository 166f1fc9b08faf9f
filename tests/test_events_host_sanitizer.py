"""CPU: the HOST side of animation events (mtr_anim_events_create / _destroy, mtr_anim_events_collect_device and
mtr_anim_events_collect_host: csrc/host_events.cpp) compiled by g++ with AddressSanitizer and UBSan over the stand-in HIP runtime
(tests/cpp/hip_stub), as a stand-alone program with its own main whose k_events launcher runs csrc/event_math.h on exactly the
words it is handed: every rejected creation and call of SPEC.md section 22 launches nothing and leaves the list, the count and
the bits as they were (the error names the clip and the marker), the valid calls equal a second run of the rule on copies --
through the device call on two streams and through the host hook on unaligned memory --, and sets are created and destroyed
with calls queued."""
import re
import subprocess

from tests import cpp_build


def test_events_host_side_under_asan_ubsan(tmp_path):
    exe = cpp_build.build("events_host_asan", tmp_path, cpp_build.HOST_ASAN)
    r = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"collected=(\d+) rejected=(\d+) launches=(\d+) failed=(\d+)", r.stdout)
    assert m, r.stdout
    collected, rejected, launches, failed = map(int, m.groups())
    # per iteration: 7 + 1 + 2 rejected creations (more with markers), 19 rejected calls; 3 valid calls and 3 on sets that are
    # destroyed right after; and at the end the one call whose worst case passes 2^32 - 1 events
    assert failed == 0 and rejected >= 40 * 29 + 1 and launches == collected == 40 * 6, r.stdout
