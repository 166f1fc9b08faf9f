"""CPU: csrc/blend_math.h (the scalar rule of SPEC.md section 23: the smoothing of the parameters, the bracket of a 1-D space, the
first triangle that holds the point and the closest-edge fallback of a 2-D space, the shared phase and the records) compiled by
g++ with -ffp-contract=off over the HIP stub, put together as k_blend puts it together and compared bit for bit with the numpy
model on every case of the generator, three chained calls each: the GPU bit-exactness test's rehearsal on a machine without a
GPU.  A NaN in the model must be a NaN in the result; payloads are free."""
import subprocess

import numpy as np
import pytest

from tests import blend_model as bm
from tests import cpp_build

CASES = bm.cases()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = cpp_build.build("blend_exact", tmp_path_factory.mktemp("blend_exact"), cpp_build.EXACT, extra=["-Wno-unused-function", "-Wno-unknown-pragmas"])
    return out


def blob_of(bs, states, params, dt, nlayers, layers):
    n = states.shape[0]
    nkeys, flags, rates = bs["tab"]
    C, K, T = len(nkeys), bs["samples"].size, bs["tris"].size
    P, _ = bm.pm.periods(bs["tab"])
    t = np.zeros((C, 4), dtype="<u4")
    t[:, 0], t[:, 1], t[:, 2], t[:, 3] = P.astype("<f4").view("<u4"), flags, rates.astype("<f4").view("<u4"), nkeys
    head = np.array([n, C, K, T, bs["nparams"], bs["param_x"], bs["param_y"], nlayers], dtype="<u4").tobytes()
    head += np.array([bs["damp"], dt], dtype="<f4").tobytes() + b"\0" * 8
    return (head + t.tobytes() + bs["samples"].tobytes() + bs["tris"].tobytes() + np.ascontiguousarray(states).tobytes()
            + np.ascontiguousarray(params, dtype="<f4").tobytes() + np.ascontiguousarray(layers).tobytes())


def run(exe, tmp_path, c):
    """the three chained calls of a case through the host build: a list of (states, layers, steps, shares)"""
    st, ly, res = c["states"], c["layers"], []
    n, nl = c["n"], c["nlayers"]
    for dt, params in c["calls"]:
        blob, out = tmp_path / "in.bin", tmp_path / "out.bin"
        blob.write_bytes(blob_of(c["set"], st, params, dt, nl, ly))
        subprocess.check_call([exe, str(blob), str(out)], timeout=60)
        raw = np.fromfile(out, dtype="<u4")
        a, b, d = n * 4, n * 4 + n * nl * 4, n * 4 + n * nl * 4 + n * 12
        st, ly = raw[:a].view(bm.STATE), raw[a:b].view(bm.LAYER).reshape(n, nl)
        res.append((st, ly, raw[b:d].view(bm.STEP).reshape(n, 3), raw[d:].view("<f4").reshape(n, 3)))
    return res


@pytest.mark.parametrize("n", bm.COUNTS)
def test_header_equals_the_model_bit_for_bit(exe, tmp_path, n):
    told = 0
    for c in (c for c in CASES if c["n"] == n):
        want = bm.run_case(c)
        got = run(exe, tmp_path, c)
        for call, (g, w) in enumerate(zip(got, want)):
            for a, b, what in zip(g, w, ("states", "layers", "steps", "shares")):
                bad = ~bm.same_bits(a, b)
                assert a.shape == b.shape and not bad.any(), f"{c['name']} call {call} {what}: {int(bad.sum())} differ, first at {np.argwhere(bad)[0]}"
        # and the harness would notice a wrong reading: the same comparison fails against every wrong variant of the model
        # that changes this case
        for v in bm.WRONG_VARIANTS:
            wrong = bm.run_case(c, variant=v)
            if not bm.same_result(wrong, want):
                assert not bm.same_result(got, wrong), (c["name"], v)
                told += 1
    assert told, "no wrong reading changes a case at this size"
