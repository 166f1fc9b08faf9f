"""CPU: csrc/attach_math.h (the scalar rule of SPEC.md section 18: the two clamps, a row of the joint matrix, an element of
A * O) compiled by g++ with -ffp-contract=off over the HIP stub, put together as k_attach puts it together and compared bit
for bit with the numpy model on every case of the generator: the GPU bit-exactness test's rehearsal on a machine without a
GPU.  An element that is NaN in the model must be NaN in the result; payloads are free."""
import subprocess

import numpy as np
import pytest

from tests import attach_model as am
from tests import cpp_build

CASES = am.cases()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = cpp_build.build("attach_exact", tmp_path_factory.mktemp("attach_exact"), cpp_build.EXACT, extra=["-Wno-unused-function", "-Wno-unknown-pragmas"])
    return out


def run(exe, tmp_path, c):
    blob, res = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(blob, "wb") as f:
        f.write(np.array([c["n"], c["n_src"], c["npal"], 0], dtype="<u4").tobytes())
        f.write(c["M_src"].tobytes())
        if c["npal"]:
            f.write(c["P_src"].tobytes())
        f.write(c["recs"].tobytes())
    subprocess.check_call([exe, str(blob), str(res)], timeout=60)
    return np.fromfile(res, dtype="<f4").reshape(c["n"], 16)


@pytest.mark.parametrize("n_src,npal", [(s, p) for s in am.N_SRC for p in am.NPAL])
def test_header_equals_the_model_bit_for_bit(exe, tmp_path, n_src, npal):
    nan_seen = False
    for c in (c for c in CASES if c["n_src"] == n_src and c["npal"] == npal):
        got = run(exe, tmp_path, c)
        want = am.attach(c["M_src"], c["P_src"], c["recs"])
        bad = ~am.same_bits(got, want)
        assert not bad.any(), f"{c['name']}: {int(bad.sum())} of {bad.size} elements differ, first at {np.argwhere(bad)[0]}"
        nan_seen |= bool(np.isnan(want).any())
        # and the harness would notice a wrong reading: the same comparison fails against every wrong variant of the model
        for v in am.WRONG_VARIANTS:
            if am.can_show(v, c):
                wrong = am.attach(c["M_src"], c["P_src"], c["recs"], variant=v)
                assert not am.same_bits(got, wrong).all(), (c["name"], v)
    assert nan_seen, "the special records reach the comparison"
