"""CPU: the multiply-high divisions of the tile kernels (csrc/tile_common.h: udiv_make / udiv_apply, row_magic) against
`/` and `%`, exhaustively: bin / nbx and bin % nbx for every bins-per-row count and every bin index a frame can have,
blockIdx.x >> 3 by every run length the host accepts for every block of such a launch, and the pair walks' k / iw.  A
multiplier one too small must be caught."""
import subprocess

import pytest

from tests import cpp_build


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return cpp_build.build("bin_magic_exact", tmp_path_factory.mktemp("bin_magic"), cpp_build.BARE, extra=["-pthread"])


def _run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True)
    divisors, dividends, bad = (int(v) for v in out.stdout.split())
    return out.returncode, divisors, dividends, bad


def test_bin_by_nbx_is_exact(exe):
    rc, divisors, dividends, bad = _run(exe, "nbx")
    assert rc == 0 and bad == 0
    assert divisors == 1024 and dividends == 1024 * sum(range(1, 1025))  # every bin of every grid up to 1024 x 1024


def test_block_by_run_is_exact(exe):
    rc, divisors, dividends, bad = _run(exe, "run")
    assert rc == 0 and bad == 0
    assert divisors == 65536 and dividends >= 65536 * (1 << 17)  # at least the 2^17 blocks per XCD of the largest frame


def test_row_magic_is_exact(exe):
    rc, divisors, dividends, bad = _run(exe, "magic")
    assert rc == 0 and bad == 0 and divisors == 16 and dividends == 16 * 256


@pytest.mark.parametrize("mode", ["nbx", "run", "magic"])
def test_multiplier_one_too_small_is_caught(exe, mode):
    rc, _, _, bad = _run(exe, mode, "-1")
    assert rc == 1 and bad > 0
