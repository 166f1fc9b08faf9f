"""CPU: the HOST side of blend spaces (mtr_anim_blend_create / _destroy, mtr_anim_blend_advance_device and
mtr_anim_blend_advance_host: csrc/host_blend.cpp) compiled by g++ with AddressSanitizer and UBSan over the stand-in HIP runtime
(tests/cpp/hip_stub), as a stand-alone program with its own main whose k_blend launcher runs csrc/blend_math.h on exactly the
words it is handed: every rejected creation and call of SPEC.md section 23 launches nothing and leaves the states, the layers,
the steps and the shares as they were (the error names the clip, the sample or the triangle), the valid calls equal a second
run of the rule on copies -- through the device call on two streams and through the host hook on unaligned memory --, and sets
are created and destroyed with calls queued."""
import re
import subprocess

from tests import cpp_build


def test_blend_host_side_under_asan_ubsan(tmp_path):
    exe = cpp_build.build("blend_host_asan", tmp_path, cpp_build.HOST_ASAN)
    r = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"advanced=(\d+) rejected=(\d+) launches=(\d+) failed=(\d+)", r.stdout)
    assert m, r.stdout
    advanced, rejected, launches, failed = map(int, m.groups())
    # per iteration: 19 + 3 + 4 rejected creations (more with triangles or several 1-D samples), 19 rejected calls; 3 valid calls
    # and 3 on sets that are destroyed right after
    assert failed == 0 and rejected >= 40 * 45 and launches == advanced == 40 * 6, r.stdout
