"""CPU: the HOST side of root motion (mtr_anim_root_create / _destroy, mtr_batch_root_motion(_device) and
mtr_anim_root_deltas(_device): csrc/host_anim.cpp, csrc/host_batch.cpp) compiled by g++ with AddressSanitizer and UBSan over the stand-in HIP
runtime (tests/cpp/hip_stub), as a stand-alone program with its own main whose launchers read the first and last word of
everything k_root is handed: every rejected call of SPEC.md section 19 (the error names the clip with unknown flag bits, and the
LOOP clip of a trajectory set) leaves the batch's version ring as it was, both kinds of set with host and device steps, root
sets created and destroyed with calls queued and frames in flight, and the event order of a root-motion call between an
animate call and an attach call on the same batch."""
import re
import subprocess

from tests import cpp_build


def test_root_host_side_under_asan_ubsan(tmp_path):
    exe = cpp_build.build("root_host_asan", tmp_path, cpp_build.HOST_ASAN)
    r = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"moved=(\d+) rejected=(\d+) root_launches=(\d+) delta_launches=(\d+) step_reads=(\d+) failed=(\d+)", r.stdout)
    assert m, r.stdout
    moved, rejected, root_launches, delta_launches, step_reads, failed = map(int, m.groups())
    assert failed == 0 and moved == 40 * 11 and rejected == 40 * 55, r.stdout
    assert root_launches == 40 * 7 + 2 and delta_launches == 40 * 4 and step_reads == 2 * (root_launches + delta_launches), r.stdout
