"""CPU: the HOST side of animation tracks (mtr_anim_create_tracks and the section-14 entry points on a track set:
csrc/host_anim.cpp, csrc/host_batch.cpp) compiled by g++ with AddressSanitizer and UBSan over the stand-in HIP runtime (tests/cpp/hip_stub),
as a stand-alone program whose four launchers read the first and last descriptor, time and value of every clip a state
names: every invalid creation, sets of both kinds created and destroyed around animate calls and frames in flight, and one
batch animated alternately from a uniform and a track set."""
import re
import subprocess

from tests import cpp_build


def test_anim_tracks_host_side_under_asan_ubsan(tmp_path):
    exe = cpp_build.build("anim_tracks_host_asan", tmp_path, cpp_build.HOST_ASAN)
    r = subprocess.run([exe, "60"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"animated=(\d+) rejected=(\d+) key_reads=(\d+) track_reads=(\d+)", r.stdout)
    assert m, r.stdout
    animated, rejected, key_reads, track_reads = map(int, m.groups())
    assert animated == 60 * 13 and rejected >= 60 * 24 and key_reads > 0 and track_reads > 0, r.stdout
