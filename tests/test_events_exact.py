"""CPU: csrc/event_math.h (the scalar rule of SPEC.md section 22: the weights, the clamp and the wrap of a position, and per step
the ranges of sorted markers found by lower / upper bound searches) compiled by g++ with -ffp-contract=off over the HIP stub,
put together as k_events puts it together (count, scan of block sums, fill) and compared bit for bit with the numpy model on
every case of the generator: the GPU bit-exactness test's rehearsal on a machine without a GPU.  A NaN in the model must be a
NaN in the result; payloads are free."""
import subprocess

import numpy as np
import pytest

from tests import cpp_build
from tests import events_model as em

CASES = em.cases()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = cpp_build.build("events_exact", tmp_path_factory.mktemp("events_exact"), cpp_build.EXACT, extra=["-Wno-unused-function", "-Wno-unknown-pragmas"])
    return out


def blob_of(es, steps, min_weight, capacity, out_prev, bits_prev):
    n, S = steps.shape
    C, M = len(es["counts"]), len(es["markers"])
    P, _ = em.periods(es)
    t = np.zeros((C, 4), dtype="<u4")
    t[:, 0], t[:, 1], t[:, 3] = P.astype("<f4").view("<u4"), es["tab"][1], es["tab"][0]
    r = np.zeros((C, 2), dtype="<u4")
    r[:, 0], r[:, 1] = es["first"], es["counts"]
    return (np.array([n, C, S, M, capacity, 0], dtype="<u4").tobytes() + np.array([min_weight], dtype="<f4").tobytes() + b"\0\0\0\0" + t.tobytes()
            + r.tobytes() + es["markers"].tobytes() + np.ascontiguousarray(steps).tobytes() + np.ascontiguousarray(out_prev).tobytes()
            + np.ascontiguousarray(bits_prev, dtype="<u4").tobytes())


def run(exe, tmp_path, c):
    blob, res = tmp_path / "in.bin", tmp_path / "out.bin"
    blob.write_bytes(blob_of(c["set"], c["steps"], c["min_weight"], c["capacity"], c["out_prev"], c["bits_prev"]))
    subprocess.check_call([exe, str(blob), str(res)], timeout=60)
    raw = np.fromfile(res, dtype="<u4")
    cap, n = c["capacity"], c["n"]
    return raw[:cap * 4].view(em.EVENT), raw[cap * 4:cap * 4 + 2], raw[cap * 4 + 2:]


@pytest.mark.parametrize("n", em.COUNTS)
def test_header_equals_the_model_bit_for_bit(exe, tmp_path, n):
    fired = told = 0
    for c in (c for c in CASES if c["n"] == n):
        want = em.run_case(c)
        got = run(exe, tmp_path, c)
        for a, b, what in zip(got, want, ("list", "count", "bits")):
            bad = ~em.same_bits(a, b)
            assert a.shape == b.shape and not bad.any(), f"{c['name']} {what}: {int(bad.sum())} differ, first at {np.argwhere(bad)[0]}"
        fired += int(want[1][0])
        # and the harness would notice a wrong reading: the same comparison fails against every wrong variant of the model
        # that changes this case
        for v in em.WRONG_VARIANTS:
            wrong = em.run_case(c, variant=v)
            if not em.same_result(wrong, want):
                assert not em.same_result(got, wrong), (c["name"], v)
                told += 1
    assert fired and told, "no marker fires, or no wrong reading changes a case, at this size"
