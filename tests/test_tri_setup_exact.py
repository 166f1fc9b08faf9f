"""CPU: csrc/tri_setup.h -- the triangle set-up and edge evaluation that k_tile.hip and k_tile_vis.hip share -- against a
plain int64 reference (tests/cpp/tri_setup_exact.cpp) on >= 10^6 small-class triangles of the span test's generator
(tests/cpp/tri_gen.h) and 3 x 10^4 of the 64-bit class: every coefficient, top-left bit, the area, the bbox; every edge
value and inside decision at all 256 pixels of the bin; and the absolute-coordinate E1 / E2 of deferred shading against
the bin-relative integers at every covered pixel.

The small class multiplies with v_mul_i32_i24, which the header's host macro models.  Its widest operand is
A = 256 * dy, a signed 24-bit value iff |256 * dy| < 2^23 (the positive side), i.e. dy <= 32767.  A class limit L admits
dy = L, so L = 32768 is the first limit at which A (= 2^23, read back as -2^23) no longer fits: the mutant build."""
import subprocess

from tests import cpp_build

MUTANT_LIMIT = 32768  # 256 * 32768 = 2^23: one past the largest positive 24-bit operand


def _build(tmp_path, name, *defs):
    return cpp_build.build("tri_setup_exact", tmp_path, cpp_build.BARE, extra=["-ffp-contract=off", *defs], exe=f"tri_setup_exact_{name}")


def test_shared_setup_matches_int64_reference(tmp_path):
    exe = _build(tmp_path, "exact")
    out = subprocess.run([exe, "1000000", "30000", "20261018"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    small, large, covered, bad = (int(v) for v in out.stdout.split())
    assert small >= 1000000 and large >= 30000 and bad == 0
    # teeth: the covered pixels are where the inside decision and the E1 / E2 identity are exercised
    assert covered > small, out.stdout


def test_operand_beyond_24_bits_is_caught(tmp_path):
    assert 256 * (MUTANT_LIMIT - 1) < 2 ** 23 <= 256 * MUTANT_LIMIT
    exe = _build(tmp_path, "mutant", f"-DMTR_TRI_CLASS_LIMIT={MUTANT_LIMIT}")
    out = subprocess.run([exe, "200000", "0", "7"], capture_output=True, text=True)
    assert out.returncode == 1 and int(out.stdout.split()[3]) > 0, out.stdout
