"""CPU: the HOST side of the animation entry points (mtr_anim_*, mtr_*_animate*: csrc/host_anim.cpp, csrc/host_batch.cpp) compiled by g++ with
AddressSanitizer and UBSan over the stand-in HIP runtime (tests/cpp/hip_stub), with launchers that read the first and last
key of every clip a state names and write the last output word: clip tables, key offsets, staged state counts, every
invalid call of include/mtr.h's list, and an animation set destroyed while frames that were animated from it are in flight."""
import subprocess

from tests import cpp_build


def test_anim_host_side_under_asan_ubsan(tmp_path):
    exe = cpp_build.build("anim_host_asan", tmp_path, cpp_build.HOST_ASAN)
    r = subprocess.run([exe, "300"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "animated=900 rejected=6300" in r.stdout, r.stdout
