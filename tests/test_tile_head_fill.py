"""CPU: tile_fill_head (csrc/tile_common.h), which both tile launchers call on their copy of the parameters.  The head of
TileParams is what the kernels fetch first and read instead of the fields it mirrors, so every mirrored field must equal its
source, the grid must be the whole runs of the launch, the divisor words must still give `/` and `%`, and nothing outside the
head may change -- over unsharded and sharded parameter sets, own_list null and set, a rank without a bin, xcd_run 0 / 1 /
16 / 65536, both queue layouts (tests/cpp/tile_head_fill.cpp).  A head with two fields swapped must be caught."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "tile_head_fill.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = str(tmp_path_factory.mktemp("tile_head") / "tile_head_fill")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(HERE, "cpp", "hip_stub"), SRC, "-o", out])
    return out


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
