"""CPU: csrc/ctrl_math.h (the scalar rule of SPEC.md section 21: the clamp of the node, the lead and its built-in values, the
candidates with their skips, the conditions, the fire and the store) compiled by g++ with -ffp-contract=off over the HIP stub,
put together as k_ctrl puts it together and compared bit for bit with the numpy model on every step of every case of the
generator: the GPU bit-exactness test's rehearsal on a machine without a GPU.  A NaN in the model must be a NaN in the result;
payloads are free."""
import subprocess

import numpy as np
import pytest

from tests import cpp_build
from tests import ctrl_model as cm
from tests import player_model as pm

CASES = cm.cases()


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = cpp_build.build("ctrl_exact", tmp_path_factory.mktemp("ctrl_exact"), cpp_build.EXACT, extra=["-Wno-unused-function", "-Wno-unknown-pragmas"])
    return out


def run(exe, tmp_path, g, tab, states, play, params, dt, counts):
    blob, res = tmp_path / "in.bin", tmp_path / "out.bin"
    n, C, S, T, NP = len(states), len(tab[0]), len(g["nodes"]), len(g["trans"]), g["nparams"]
    P, _ = cm.periods(tab[0], tab[1])
    t = np.zeros((C, 4), dtype="<u4")
    t[:, 0], t[:, 1], t[:, 3] = P.astype("<f4").view("<u4"), tab[1], tab[0]
    with open(blob, "wb") as f:
        f.write(np.array([n, C, S, T, g["nany"], NP], dtype="<u4").tobytes() + np.array([dt], dtype="<f4").tobytes() + b"\0\0\0\0")
        f.write(t.tobytes() + g["nodes"].tobytes() + g["trans"].tobytes() + states.tobytes() + play.tobytes())
        f.write(np.ascontiguousarray(params, dtype="<f4").tobytes() + np.ascontiguousarray(counts, dtype="<u4").tobytes())
    subprocess.check_call([exe, str(blob), str(res)], timeout=60)
    raw = np.fromfile(res, dtype="<u4")
    a, b, c = n * 4, n * 4 + n * NP, n * 8 + n * NP
    return raw[:a].view(cm.STATE), raw[a:b].view("<f4").reshape(n, NP), raw[b:c].view(pm.CMD), raw[c:]


@pytest.mark.parametrize("n", cm.COUNTS)
def test_header_equals_the_model_bit_for_bit(exe, tmp_path, n):
    nan_seen = told = fired = 0
    for c in (c for c in CASES if c["n"] == n):
        g, tab = c["graph"], c["tab"]
        st, pr, play, ct = c["states"], c["params"], c["play"], np.zeros(len(g["trans"]), dtype=np.uint32)
        for dt in c["dts"]:
            want = cm.step(g, tab, st, play, pr, dt, ct)
            got = run(exe, tmp_path, g, tab, st, play, pr, dt, ct)
            for a, b, what in zip(got, want, ("states", "params", "commands", "counts")):
                bad = ~cm.same_bits(a, b)
                assert a.shape == b.shape and not bad.any(), f"{c['name']} {what}: {int(bad.sum())} differ, first at {np.argwhere(bad)[0]}"
            nan_seen += int(np.isnan(want[0]["t"]).any() or np.isnan(want[2]["x"]).any())
            fired += int((want[0]["fired"] != cm.NONE).sum())
            # and the harness would notice a wrong reading: the same comparison fails against every wrong variant of the
            # model that changes this step
            for v in cm.WRONG_VARIANTS:
                wrong = cm.step(g, tab, st, play, pr, dt, ct, variant=v)
                if not all(cm.same_bits(a, b).all() for a, b in zip(wrong, want)):
                    assert not all(cm.same_bits(a, b).all() for a, b in zip(got, wrong)), (c["name"], v)
                    told += 1
            st, pr, ct = want[0], want[1], want[3]
            play = pm.advance(play, dt, tab, want[2])[0]
    assert nan_seen or n < 63, "the special values reach the comparison"
    assert fired and told, "no transition fires, or no wrong reading changes a step, at this size"
