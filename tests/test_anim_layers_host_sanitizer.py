"""CPU: the HOST side of animation layers (mtr_anim_masks_create / _destroy and the four layered entry points:
csrc/host_anim.cpp, csrc/host_batch.cpp) compiled by g++ with AddressSanitizer and UBSan over the stand-in HIP runtime (tests/cpp/hip_stub),
as a stand-alone program whose launchers read the first and last layer of every instance and the first and last mask
weight and clip entry each layer names: every invalid call, both kinds of set with and without masks, and one batch
animated by all kinds of call with frames in flight while mask sets come and go."""
import re
import subprocess

from tests import cpp_build


def test_anim_layers_host_side_under_asan_ubsan(tmp_path):
    exe = cpp_build.build("anim_layers_host_asan", tmp_path, cpp_build.HOST_ASAN)
    r = subprocess.run([exe, "60"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    m = re.search(r"animated=(\d+) rejected=(\d+) layer_reads=(\d+) mask_reads=(\d+) clip_reads=(\d+)", r.stdout)
    assert m, r.stdout
    animated, rejected, layer_reads, mask_reads, clip_reads = map(int, m.groups())
    assert animated == 60 * 15 and rejected == 60 * 38 and layer_reads > 0 and mask_reads > 0 and clip_reads > 0, r.stdout
