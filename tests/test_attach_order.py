"""CPU: the cross-batch ordering of attachments (SPEC.md section 18): tests/cpp/attach_order.cpp, a stand-alone program over
the stand-in HIP runtime (tests/cpp/hip_stub) built by g++ with AddressSanitizer and UBSan, asserts the logged sequence of
stream waits, launches and event records for an attach followed by two updates of the source, an attach followed by the
source's destruction, and a batch attached to itself, and that every invalid call leaves `cur` and the version rings
untouched."""
import re
import subprocess

from tests import cpp_build


def test_attach_ordering_under_asan_ubsan(tmp_path):
    exe = cpp_build.build("attach_order", tmp_path, cpp_build.HOST_ASAN)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-6000:]
    m = re.search(r"attach_order: launches=(\d+) failed=(\d+) sink=ok", r.stdout)
    assert m and int(m.group(1)) >= 8 and int(m.group(2)) == 0, r.stdout
