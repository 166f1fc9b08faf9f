"""CPU: csrc/anim_ik.h (the scalar solve of SPEC.md section 17: dot3, cross, qrot, fromto, the two-bone reach and the aim),
csrc/anim_blend.h's local matrix and csrc/pose_common.h's pose_mul chain, compiled by g++ with -ffp-contract=off, put
together as the k_anim_ik kernels put them together and compared bit for bit with the numpy model of section 17: the GPU
bit-exactness test's rehearsal on a machine without a GPU.  The (T, Q, S) the chains start from come from the model of
section 16."""
import subprocess

import numpy as np
import pytest

from tests import anim_ik_model as ik
from tests import anim_layers_model as lm
from tests import anim_model as am
from tests import cpp_build

F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = cpp_build.build("anim_ik_exact", tmp_path_factory.mktemp("anim_ik_exact"), cpp_build.EXACT, extra=["-Wno-unused-function", "-Wno-unknown-pragmas"])
    return out


@pytest.mark.parametrize("J,K", [(3, 1), (3, 4), (65, 1), (65, 4)])
def test_header_equals_the_model_bit_for_bit(exe, tmp_path, J, K):
    rng = np.random.default_rng(17 * J + K)
    clips = am.random_clips(rng, J)
    masks = lm.random_masks(rng, J)
    ly = lm.layer_states(rng, clips, L=3)
    parents = ik.skeleton(J)
    chains = ik.default_chains(parents, K)
    tqs = ik.stack_tqs(clips, ly, J, masks)
    tg = ik.make_targets(rng, tqs, parents, chains)
    n = ly.shape[0]
    packed = np.zeros((n, J, 12), dtype=F)
    packed[..., 0:3], packed[..., 4:8], packed[..., 8:11] = tqs
    blob, res = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(blob, "wb") as f:
        f.write(np.array([n, J, K, 0], dtype="<u4").tobytes())
        f.write(parents.tobytes() + b"\0" * (-J % 4))
        f.write(chains.tobytes())
        f.write(np.ascontiguousarray(tg).tobytes())
        f.write(packed.tobytes())
    subprocess.check_call([exe, str(blob), str(res)], timeout=120)
    got = np.fromfile(res, dtype="<u4").reshape(n, J, 16)
    probe = []
    want = ik.sample(clips, ly, J, masks, parents, chains, tg, tqs=tqs, probe=probe)
    assert all(p["hit"].sum() > n // 2 for p in probe), "most instances are solved"
    bad = got != want.view(np.uint32)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} local matrix elements differ, first at {np.argwhere(bad)[0]}"
    # and the harness would notice a wrong reading: the same comparison fails against every wrong variant of the model
    for v in ik.WRONG_VARIANTS:
        if v == "parallel" and K == 1 or v in ("conj_wrong_side",) and J == 3 and K == 1:
            continue  # one chain has no order; under a root a, P is the identity and commutes
        wrong = ik.sample(clips, ly, J, masks, parents, chains, tg, variant=v, tqs=tqs)
        assert (wrong.view(np.uint32) != got).any(), v
