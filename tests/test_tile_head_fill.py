"""CPU: tile_fill_head (csrc/tile_common.h), which both tile launchers call on their copy of the parameters.  The head of
TileParams is what the kernels fetch first and read instead of the fields it mirrors, so every mirrored field must equal its
source, the grid must be the whole runs of the launch, the divisor words must still give `/` and `%`, and nothing outside the
head may change -- over unsharded and sharded parameter sets, own_list null and set, a rank without a bin, xcd_run 0 / 1 /
16 / 65536, both queue layouts (tests/cpp/tile_head_fill.cpp).  A head with two fields swapped must be caught."""
import subprocess

import pytest

from tests import cpp_build


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return cpp_build.build("tile_head_fill", tmp_path_factory.mktemp("tile_head"), cpp_build.HOST_ASAN)


def _run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True)
    sets, checks, bad = (int(v) for v in out.stdout.split())
    return out.returncode, sets, checks, bad, out.stderr


def test_every_mirrored_field_equals_its_source(exe):
    rc, sets, checks, bad, err = _run(exe)
    assert rc == 0 and bad == 0, err
    assert sets == 4 * 9 and checks >= sets * 28  # 4 run lengths x 9 parameter sets, 28 or more checks each


def test_swapped_fields_are_caught(exe):
    rc, sets, _, bad, _ = _run(exe, "mutant")
    assert rc == 1 and bad == 2 * sets  # bin_start and seg_start, in every set
