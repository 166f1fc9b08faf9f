"""CPU: the HOST side of spring bones (mtr_anim_spring_create / _destroy, mtr_batch_animate_spring_device,
mtr_anim_sample_spring: csrc/host_spring.cpp, csrc/host_anim.cpp, csrc/host_batch.cpp) compiled by g++ with AddressSanitizer
and UBSan over the stand-in HIP runtime (tests/cpp/hip_stub), as a stand-alone program whose launchers check the set's
device image and run csrc/spring_math.h on the state words they are handed: every rejected creation and call of SPEC.md
section 24 launches nothing, leaves the states untouched and names the spring (or the joint whose parent differs); valid
calls on two streams, with and without an IK set, motion and masks, equal a second run of the rule; the host hook works on
memory one byte off every alignment; spring sets are destroyed with their calls queued and frames in flight."""
import re
import subprocess

from tests import cpp_build


def test_spring_host_side_under_asan_ubsan(tmp_path):
    exe = cpp_build.build("spring_host_asan", tmp_path, cpp_build.HOST_ASAN)
    r = subprocess.run([exe, "60"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"animated=(\d+) rejected=(\d+) launches=(\d+) state_steps=(\d+) path_reads=(\d+)", r.stdout)
    assert m, r.stdout
    animated, rejected, launches, state_steps, path_reads = map(int, m.groups())
    assert animated == 60 * 13 and launches == animated - 60 and state_steps > 0 and path_reads > 0, r.stdout  # one layered call an iteration
    assert rejected == 60 * 53, r.stdout
