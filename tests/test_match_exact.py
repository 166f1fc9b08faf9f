"""CPU: csrc/match_math.h (the scalar rule of SPEC.md section 25: the tile-major slot, the lead, the current row, the query, the
chain, the order key and the decision) compiled by g++ with -ffp-contract=off over the HIP stub, put together as k_match puts
it together and compared bit for bit with the numpy model on every case of the generator, for scores, winners, commands and
results: the GPU bit-exactness test's rehearsal on a machine without a GPU.  A NaN in the model must be a NaN in the result;
payloads are free."""
import subprocess

import numpy as np
import pytest

from tests import cpp_build
from tests import match_model as mm

CASES = mm.cases()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = cpp_build.build("match_exact", tmp_path_factory.mktemp("match_exact"), cpp_build.EXACT, extra=["-Wno-unused-function", "-Wno-unknown-pragmas"])
    return out


def run(exe, tmp_path, c, filt):
    s, n, R, D = c["set"], c["n"], c["R"], c["D"]
    blob, res = tmp_path / "in.bin", tmp_path / "out.bin"
    t = np.zeros((len(s["nkeys"]), 4), dtype="<u4")
    t[:, 0], t[:, 1], t[:, 3] = s["P"].astype("<f4").view("<u4"), s["clip_flags"], s["nkeys"]
    head = np.zeros(16, dtype="<u4")
    head[:10] = [n, len(s["nkeys"]), R, D, s["flags"], c["base"], c["raw"] is not None, filt is not None, s["pose_dims"] & 0xFFFFFFFF, s["pose_dims"] >> 32]
    head[10:13] = np.array([s["seconds"], s["near"], s["margin"]], dtype="<f4").view("<u4")
    with open(blob, "wb") as f:
        f.write(head.tobytes() + t.tobytes() + s["rows"].tobytes() + s["feats"].tobytes() + s["mean"].tobytes() + s["scale"].tobytes() + c["play"].tobytes())
        if c["raw"] is not None:
            f.write(np.ascontiguousarray(c["raw"], dtype="<f4").tobytes())
        if filt is not None:
            f.write(filt.tobytes())
    subprocess.check_call([exe, str(blob), str(res)], timeout=120)
    raw = np.fromfile(res, dtype="<u4")
    return raw[n * R:n * R + n * 4].view(mm.CMD), raw[n * R + n * 4:].view(mm.RESULT), raw[:n * R].view("<f4").reshape(n, R)


@pytest.mark.parametrize("family", mm.FAMILIES)
def test_header_equals_the_model_bit_for_bit(exe, tmp_path, family):
    nan_seen = none_seen = jumps = told = 0
    for c in (c for c in CASES if c["family"] == family):
        for filt in (c["filt"], None):
            want = mm.search(c["set"], c["play"], c["raw"], filt, c["base"])
            got = run(exe, tmp_path, c, filt)
            for a, b, what in zip(got, want, ("commands", "results", "scores")):
                bad = ~mm.same_bits(a, b)
                assert a.shape == b.shape and not bad.any(), f"{c['name']} {what}: {int(bad.sum())} differ, first at {np.argwhere(bad)[0]}"
            nan_seen += int(np.isnan(want[2]).any())
            none_seen += int((want[1]["row"] == mm.NONE).sum())
            jumps += int((want[0]["instance"] != 0xFFFFFFFF).sum())
            # and the harness would notice a wrong reading: the same comparison fails against every wrong variant of the model
            # that changes this case
            for v in mm.WRONG_VARIANTS:
                wrong = mm.search(c["set"], c["play"], c["raw"], filt, c["base"], variant=v)
                if not all(mm.same_bits(a, b).all() for a, b in zip(wrong, want)):
                    assert not all(mm.same_bits(a, b).all() for a, b in zip(got, wrong)), (c["name"], v)
                    told += 1
    assert nan_seen or family != "large", "the special values reach the comparison"
    assert none_seen and jumps and told, "no instance without a winner, no command, or no wrong reading changes a case, in this family"
