"""CPU: the HOST side of animation tracks (mtr_anim_create_tracks and the section-14 entry points on a track set:
csrc/host_anim.cpp, csrc/host_batch.cpp) compiled by g++ with AddressSanitizer and UBSan over the stand-in HIP runtime (tests/cpp/hip_stub),
as a stand-alone program whose four launchers read the first and last descriptor, time and value of every clip a state
names: every invalid creation, sets of both kinds created and destroyed around animate calls and frames in flight, and one
batch animated alternately from a uniform and a track set."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_anim_tracks_host_side_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "anim_tracks_host_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "tests", "cpp", "hip_stub"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "anim_tracks_host_asan.cpp"), "-o", exe, "-lz"])
    r = subprocess.run([exe, "60"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"animated=(\d+) rejected=(\d+) key_reads=(\d+) track_reads=(\d+)", r.stdout)
    assert m, r.stdout
    animated, rejected, key_reads, track_reads = map(int, m.groups())
    assert animated == 60 * 13 and rejected >= 60 * 24 and key_reads > 0 and track_reads > 0, r.stdout
