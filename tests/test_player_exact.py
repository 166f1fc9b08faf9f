"""CPU: csrc/play_math.h (the scalar rule of SPEC.md section 20: clamp, command, time, the advance on a LOOP and on a one-shot
clip, the weight, the records of the frame and the store) compiled by g++ with -ffp-contract=off over the HIP stub, put together
as k_play puts it together and compared bit for bit with the numpy model on every call of every case of the generator: the GPU
bit-exactness test's rehearsal on a machine without a GPU.  A NaN in the model must be a NaN in the result; payloads are free."""
import subprocess

import numpy as np
import pytest

from tests import cpp_build
from tests import player_model as pm

CASES = pm.cases()
F32 = np.float32
FRAME = ("clip_a", "clip_b", "x_a", "x_b", "w", "x0_a", "dx_a", "x0_b", "dx_b")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = cpp_build.build("play_exact", tmp_path_factory.mktemp("play_exact"), cpp_build.EXACT, extra=["-Wno-unused-function", "-Wno-unknown-pragmas"])
    return out


def run(exe, tmp_path, tab, states, dt, cmds):
    blob, res = tmp_path / "in.bin", tmp_path / "out.bin"
    n, C = len(states), len(tab[0])
    P, _ = pm.periods(tab)
    t = np.zeros((C, 4), dtype="<u4")
    t[:, 0], t[:, 1], t[:, 2], t[:, 3] = P.astype("<f4").view("<u4"), tab[1], tab[2].astype("<f4").view("<u4"), tab[0]
    with open(blob, "wb") as f:
        f.write(np.array([n, C, len(cmds)], dtype="<u4").tobytes() + np.array([dt], dtype="<f4").tobytes())
        f.write(t.tobytes() + states.tobytes() + cmds.tobytes())
    subprocess.check_call([exe, str(blob), str(res)], timeout=60)
    raw = np.fromfile(res, dtype="<u4")
    st = raw[:n * 8].view(pm.PLAY)
    fr = raw[n * 8:].reshape(n, 9)
    frame = {k: (fr[:, i].astype(np.int64) if i < 2 else fr[:, i].copy().view("<f4")) for i, k in enumerate(FRAME)}
    return st, frame


@pytest.mark.parametrize("n", pm.COUNTS)
def test_header_equals_the_model_bit_for_bit(exe, tmp_path, n):
    nan_seen = told = 0
    for c in (c for c in CASES if c["n"] == n):
        st = c["states"]
        for dt, cm in c["calls"]:
            want_f, want_frame = pm.advance_fields(pm.fields(st), dt, c["tab"], cm)
            want = pm.records(want_f)
            got, got_frame = run(exe, tmp_path, c["tab"], st, dt, cm)
            bad = ~pm.same_bits(got, want)
            assert not bad.any(), f"{c['name']} states: {int(bad.sum())} of {n} differ, first at {np.argwhere(bad)[0]}"
            for k in FRAME:
                a, b = got_frame[k], want_frame[k]
                bad = ~(pm.same_bits(a, b.astype(F32)) if k not in ("clip_a", "clip_b") else a == b)
                assert not bad.any(), f"{c['name']} frame {k}: {int(bad.sum())} of {n} differ, first at {np.argwhere(bad)[0]}"
            nan_seen += int(np.isnan(want["x_b"]).any() or np.isnan(want["w"]).any())
            # and the harness would notice a wrong reading: the same comparison fails against every wrong variant of the
            # model that changes this call
            for v in pm.WRONG_VARIANTS:
                wrong = pm.records(pm.advance_fields(pm.fields(st), dt, c["tab"], cm, variant=v)[0])
                if not pm.same_bits(wrong, want).all():
                    assert not pm.same_bits(got, wrong).all(), (c["name"], v)
                    told += 1
            st = want
    assert nan_seen or n < 63, "the special values reach the comparison"
    assert told, "no wrong reading changes a stored state at this size"
