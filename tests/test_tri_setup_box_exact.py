"""CPU: csrc/tri_setup.h's tri_setup_box -- the set-up k_tile_vis.hip stages its flat walks from, with a small-class
triangle's edge constants taken at the bbox's first pixel inside the bin -- against tri_setup (tests/cpp/tri_setup_box_exact.cpp)
on the cases tests/test_tri_setup_exact.py draws from tests/cpp/tri_gen.h (same counts, same seed): A, B, the flags, the
area, rcpA, the z plane and the bbox are tri_setup's bit for bit; the small class's C_i equal tri_edge(C_i, A_i, B_i, ox,
oy) of tri_setup's -- the rebase the kernel used to do for every staged triangle -- and the int64 edge value at that pixel;
the 64-bit class's C stays where the whole-wave walk reads it."""
import subprocess

from tests import cpp_build


def test_box_setup_matches_rebased_shared_setup(tmp_path):
    exe = cpp_build.build("tri_setup_box_exact", tmp_path, cpp_build.BARE, extra=["-ffp-contract=off"])
    out = subprocess.run([exe, "1000000", "30000", "20261018"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    small, large, moved, bad = (int(v) for v in out.stdout.split())
    assert small >= 1000000 and large >= 30000 and bad == 0
    # teeth: a bbox that starts inside the bin is where the two entry points differ at all
    assert moved > small // 4, out.stdout
