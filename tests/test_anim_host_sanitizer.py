"""CPU: the HOST side of the animation entry points (mtr_anim_*, mtr_*_animate*: csrc/host_anim.cpp, csrc/host_batch.cpp) compiled by g++ with
AddressSanitizer and UBSan over the stand-in HIP runtime (tests/cpp/hip_stub), with launchers that read the first and last
key of every clip a state names and write the last output word: clip tables, key offsets, staged state counts, every
invalid call of include/mtr.h's list, and an animation set destroyed while frames that were animated from it are in flight."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_anim_host_side_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "anim_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "anim_host_asan.cpp"), "-o", exe, "-lz"])
    r = subprocess.run([exe, "300"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "animated=900 rejected=6300" in r.stdout, r.stdout
