"""CPU: csrc/root_math.h (the scalar rule of SPEC.md section 19: the positions of a step with the seam and the guard, the sample
of the trajectory joint from uniform keys and from tracks, delta, composition, the step blend, the delta matrix) compiled by g++
with -ffp-contract=off over the HIP stub, put together as k_root puts it together and compared bit for bit with the numpy model
on every case of the generator: the GPU bit-exactness test's rehearsal on a machine without a GPU.  An element that is NaN in
the model must be NaN in the result; payloads are free."""
import subprocess

import numpy as np
import pytest

from tests import cpp_build
from tests import root_model as rm

CASES = rm.cases()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = cpp_build.build("root_exact", tmp_path_factory.mktemp("root_exact"), cpp_build.EXACT, extra=["-Wno-unused-function", "-Wno-unknown-pragmas"])
    return out


def run(exe, tmp_path, c):
    blob, res = tmp_path / "in.bin", tmp_path / "out.bin"
    arrays = rm.device_arrays(c["traj"], c["J"])
    lengths = arrays[1]
    C = len(lengths)
    table = np.zeros((C, 4), dtype="<u4")
    table[:, 1] = lengths
    with open(blob, "wb") as f:
        if arrays[0] == "uniform":
            table[:, 0] = np.concatenate([[0], np.cumsum(lengths)[:-1]])
            f.write(np.array([0, c["J"], C, c["root"][0], c["n"], c["S"], 0, 0], dtype="<u4").tobytes())
            f.write(table.tobytes())
            f.write(c["root"][1].astype("<u4").tobytes())
            f.write(arrays[2].tobytes())
        else:
            _, _, tracks, times, values = arrays
            f.write(np.array([1, c["J"], C, c["root"][0], c["n"], c["S"], len(times), 0], dtype="<u4").tobytes())
            f.write(table.tobytes())
            f.write(c["root"][1].astype("<u4").tobytes())
            f.write(tracks.tobytes())
            f.write(values.tobytes())
            f.write(times.tobytes())
            if len(times) % 2:
                f.write(b"\0\0")
        f.write(c["steps"].tobytes())
        f.write(c["M"].tobytes())
    subprocess.check_call([exe, str(blob), str(res)], timeout=60)
    out = np.fromfile(res, dtype="<f4").reshape(2, c["n"], 16)
    return out[0], out[1]


@pytest.mark.parametrize("kind,J", [(k, j) for k, j, _ in rm.SETS])
def test_header_equals_the_model_bit_for_bit(exe, tmp_path, kind, J):
    nan_seen = False
    for c in (c for c in CASES if c["kind"] == kind and c["J"] == J):
        got_d, got_m = run(exe, tmp_path, c)
        want_d = rm.deltas(c["traj"], c["root"], c["steps"])
        want_m = rm.root_motion(c["M"], c["traj"], c["root"], c["steps"])
        for what, got, want in (("D", got_d, want_d), ("M . D", got_m, want_m)):
            bad = ~rm.same_bits(got, want)
            assert not bad.any(), f"{c['name']} {what}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0]}"
        nan_seen |= bool(np.isnan(want_m).any())
        # and the harness would notice a wrong reading: the same comparison fails against every wrong variant of the model
        # that changes the case
        for v in rm.WRONG_VARIANTS:
            if rm.can_show(v, c):
                wrong = rm.root_motion(c["M"], c["traj"], c["root"], c["steps"], variant=v)
                if not rm.same_bits(wrong, want_m).all():
                    assert not rm.same_bits(got_m, wrong).all(), (c["name"], v)
    assert nan_seen, "the special steps reach the comparison"
