"""CPU: the HOST side of inverse kinematics (mtr_anim_ik_create / _destroy and the four IK entry points: csrc/host_anim.cpp, csrc/host_batch.cpp)
compiled by g++ with AddressSanitizer and UBSan over the stand-in HIP runtime (tests/cpp/hip_stub), as a stand-alone
program whose launchers read the first and last layer and target of every instance, every chain of the set and the path of
every chain's first joint: every invalid call and every creation rule of SPEC.md section 17 (the error names the chain, or
the first joint whose parent differs), both kinds of set with host and device targets, and one batch animated by every kind
of pose call with frames in flight while IK sets are created and destroyed between them."""
import re
import subprocess

from tests import cpp_build


def test_anim_ik_host_side_under_asan_ubsan(tmp_path):
    exe = cpp_build.build("anim_ik_host_asan", tmp_path, cpp_build.HOST_ASAN)
    r = subprocess.run([exe, "60"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"animated=(\d+) rejected=(\d+) target_reads=(\d+) chain_reads=(\d+) path_reads=(\d+)", r.stdout)
    assert m, r.stdout
    animated, rejected, target_reads, chain_reads, path_reads = map(int, m.groups())
    assert animated == 60 * 19 and target_reads > 0 and chain_reads > 0 and path_reads > 0, r.stdout
    assert rejected == 60 * 57, r.stdout
