"""CPU: csrc/spring_math.h (the scalar rule of SPEC.md section 24), csrc/anim_blend.h's local matrix and
csrc/pose_common.h's pose_mul chain, compiled by g++ with -ffp-contract=off, put together as the k_anim_spring kernels put
them together and compared bit for bit -- local matrices and state records -- with the numpy model of section 24 on the
generator's cases: the GPU bit-exactness test's rehearsal on a machine without a GPU.  The (T, Q, S) the springs start from
come from the models of sections 16 and 17."""
import subprocess

import numpy as np
import pytest

from tests import anim_ik_model as ik
from tests import cpp_build
from tests import spring_model as sm

F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = cpp_build.build("spring_exact", tmp_path_factory.mktemp("spring_exact"), cpp_build.EXACT, extra=["-Wno-unused-function", "-Wno-unknown-pragmas"])
    return out


def _header(case, tqs):
    """(got locals, got states) of the compiled header on the case's call"""
    n, J, K = case["n"], case["J"], len(case["springs"])
    T, Q, S = tqs
    if case["chains"] is not None:
        Q = ik.solve(T, Q, S, case["parents"], case["chains"], case["targets"])
    packed = np.zeros((n, J, 12), dtype=F)
    packed[..., 0:3], packed[..., 4:8], packed[..., 8:11] = T, Q, S
    return n, J, K, packed


@pytest.mark.parametrize("i", range(len(sm.cases())))
def test_header_equals_the_model_bit_for_bit(exe, tmp_path, i):
    case = sm.cases()[i]
    tqs = ik.stack_tqs(case["clips"], case["layers"], case["J"], case["masks"])
    n, J, K, packed = _header(case, tqs)
    blob, res = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(blob, "wb") as f:
        f.write(np.array([n, J, K, case["motion"] is not None], dtype="<u4").tobytes())
        f.write(np.array([case["h"], 0, 0, 0], dtype="<f4").tobytes())
        f.write(case["parents"].tobytes() + b"\0" * (-J % 4))
        f.write(case["springs"].astype(sm.SPRING).tobytes())
        f.write(np.ascontiguousarray(case["states"].astype(sm.STATE)).tobytes())
        if case["motion"] is not None:
            f.write(np.ascontiguousarray(case["motion"], dtype=F).tobytes())
        f.write(packed.tobytes())
    subprocess.check_call([exe, str(blob), str(res)], timeout=120)
    raw = np.fromfile(res, dtype="<u4")
    got, got_st = raw[:n * J * 16].reshape(n, J, 16), raw[n * J * 16:].reshape(n, K, 8)
    want, want_st = sm.run(case)
    bad = got != want.view(np.uint32)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} local matrix elements differ, first at {np.argwhere(bad)[0]}"
    bad = got_st != np.ascontiguousarray(want_st).view(np.uint32).reshape(n, K, 8)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} state words differ, first at {np.argwhere(bad)[0]}"
    # and the harness would notice a wrong reading where the case can tell it apart
    told = 0
    for v in sm.WRONG_VARIANTS:
        wrong, wrong_st = sm.run(case, variant=v)
        told += bool((wrong.view(np.uint32) != got).any() or (np.ascontiguousarray(wrong_st).view(np.uint32).reshape(n, K, 8) != got_st).any())
    assert told >= 3, "the case tells wrong readings apart"
