"""CPU: the HOST side of controllers (mtr_anim_ctrl_create / _destroy, mtr_anim_ctrl_step_device and mtr_anim_ctrl_step_host:
csrc/host_ctrl.cpp) compiled by g++ with AddressSanitizer and UBSan over the stand-in HIP runtime (tests/cpp/hip_stub), as a
stand-alone program with its own main whose k_ctrl launcher runs csrc/ctrl_math.h on exactly the words it is handed: every
rejected creation and step of SPEC.md section 21 launches nothing and leaves states, parameters, commands and counts as they
were (the error names the clip, node or transition), the valid calls equal a second run of the rule on copies -- through the
device call on two streams and through the host hook on unaligned memory --, and controllers are created and destroyed with
steps queued."""
import re
import subprocess

from tests import cpp_build


def test_ctrl_host_side_under_asan_ubsan(tmp_path):
    exe = cpp_build.build("ctrl_host_asan", tmp_path, cpp_build.HOST_ASAN)
    r = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"stepped=(\d+) rejected=(\d+) launches=(\d+) failed=(\d+)", r.stdout)
    assert m, r.stdout
    stepped, rejected, launches, failed = map(int, m.groups())
    # per iteration: 12 + 2 + 4 rejected creations (5 more with transitions, 1 more with any-state ones), 16 rejected steps
    # (2 more with parameters); 3 valid steps and 3 on controllers that are destroyed right after
    assert failed == 0 and rejected >= 40 * 34 + 20 * 5 and launches == stepped == 40 * 6, r.stdout
