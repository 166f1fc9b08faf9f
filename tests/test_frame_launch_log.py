"""CPU: the launch sequence of a frame.  The host side of libmtr.so (csrc/host_*.cpp) compiled by g++ with AddressSanitizer
and UBSan over the stand-in HIP runtime (tests/cpp/hip_stub), with kernel launchers that log what they are asked to launch
and a trace hook that logs the memsets, uploads, waits, event records and stream syncs in between; the expected logs --
which kernels run in which order for direct / two-pass binning, visibility / mixed / ordered tile kernels, sharded draws,
overflow re-runs, an empty band, profiling, frames of several draws on one slot (with every draw's share of the culling
buffers checked) -- are written out in tests/cpp/frame_launch_log.cpp."""
import subprocess

import pytest

from tests import cpp_build


@pytest.fixture(scope="module")
def launch_log_exe(tmp_path_factory):
    exe = cpp_build.build("frame_launch_log", tmp_path_factory.mktemp("frame_launch_log"), cpp_build.HOST_ASAN)
    return exe


def test_launch_sequences(launch_log_exe):
    r = subprocess.run([launch_log_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "failed=0" in r.stdout, (r.returncode, r.stdout[-300:], r.stderr[-6000:])


def test_a_failed_allocation_never_leaves_a_null_buffer(launch_log_exe):
    """hipMalloc fails at each allocation of a submit in turn, on a fresh slot and on one that has already served a smaller
    frame: MTR_E_NOMEM, and the frame submitted next succeeds or fails the same way without a launcher seeing a null buffer."""
    r = subprocess.run([launch_log_exe, "nomem"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "first_frame_bad=0 grown_slot_bad=0:" in r.stdout, (r.returncode, r.stdout[-300:], r.stderr[-6000:])
