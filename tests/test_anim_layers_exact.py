"""CPU: csrc/anim_blend.h, the source k_anim.hip's blends are made of (lerp, the dot product, nlerp, the Hamilton product,
the layer weight and the two layer steps), compiled by g++ with -ffp-contract=off and compared bit for bit with the numpy
model of SPEC.md section 16 on the inputs the GPU tests use: the GPU bit-exactness test's rehearsal on a machine without a
GPU.  The keys and fractions each layer blends come from the models of sections 14 and 15."""
import subprocess

import numpy as np
import pytest

from tests import anim_layers_model as lm
from tests import anim_model as am
from tests import anim_tracks_model as tm
from tests import cpp_build

F = np.float32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = cpp_build.build("anim_layers_exact", tmp_path_factory.mktemp("anim_layers_exact"), cpp_build.EXACT)
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _layer_keys(clips, ly, J):
    """per instance and joint of one layer: a [n, J, 3], key 0 and key 1 [n, J, 12] in binary32"""
    n = ly.shape[0]
    if lm.kind_of(clips) == "tracks":
        _, _, _, a, d0, d1 = tm.located(clips, ly["clip"], ly["x"], J)
        keys = []
        for d in (d0, d1):
            k = np.zeros((n, J, 12), dtype=F)
            k[..., 0:3], k[..., 4:8], k[..., 8:11] = d[:, :, 0, :3], d[:, :, 1, :], d[:, :, 2, :3]
            keys.append(k)
        return a.astype(F), keys[0], keys[1]
    nkeys, flags, first, allk = am._clip_tables(clips, J)
    c = np.minimum(ly["clip"].astype(np.int64), len(clips) - 1)
    i0, i1, a = am.position(ly["x"], nkeys[c], (flags[c] & am.CLIP_LOOP) != 0)
    return np.broadcast_to(a[:, None, None], (n, J, 3)).astype(F), allk[first[c] + i0], allk[first[c] + i1]


@pytest.mark.parametrize("kind", ["uniform", "tracks"])
@pytest.mark.parametrize("J,L", [(1, 2), (65, 2), (65, 8)])
def test_header_equals_the_model_bit_for_bit(exe, tmp_path, kind, J, L):
    rng = np.random.default_rng(16)
    clips = am.random_clips(rng, J) if kind == "uniform" else tm.random_track_clips(rng, J)
    masks = lm.random_masks(rng, J)
    ly = lm.layer_states(rng, clips, L=L)
    n = ly.shape[0]
    head = np.zeros((n, L, 2), dtype="<u4")
    head[..., 0] = ly["w"].view(np.uint32)
    head[..., 1] = ly["mode"]
    per = np.zeros((n, L, J, 28), dtype=F)
    M = len(masks)
    for l in range(L):
        mi = np.minimum(ly["mask"][:, l].astype(np.int64), M)
        per[:, l, :, 0] = np.where((mi == 0)[:, None], F(1), masks[np.maximum(mi, 1) - 1])
        per[:, l, :, 1:4], per[:, l, :, 4:16], per[:, l, :, 16:28] = _layer_keys(clips, ly[:, l], J)
    blob, res = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(blob, "wb") as f:
        f.write(np.array([n, J, L, 0], dtype="<u4").tobytes())
        f.write(head.tobytes())
        f.write(per.tobytes())
    subprocess.check_call([exe, str(blob), str(res)], timeout=120)
    raw = np.fromfile(res, dtype="<u4")
    got = raw[:n * J * 12].reshape(n, J, 12)
    e = raw[n * J * 12:].reshape(n, L, J)
    for l in range(1, L):
        assert (e[:, l] == _bits(lm.effective_weight(ly[:, l], masks, J))).all(), f"layer {l}: e"
    T, Q, S = lm.sample_tqs(clips, ly, J, masks)
    want = np.zeros((n, J, 12), dtype=F)
    for i in range(3):
        want[..., i], want[..., 8 + i] = T[i], S[i]
    for i in range(4):
        want[..., 4 + i] = Q[i]
    bad = got != _bits(want)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} components of (T, Q, S) differ, first at {np.argwhere(bad)[0]}"
    # and the harness would notice a wrong reading: the same comparison fails against every wrong variant of the model
    for v in lm.WRONG_VARIANTS:
        Tv, Qv, Sv = lm.sample_tqs(clips, ly, J, masks, variant=v)
        wrong = np.stack(list(Tv) + list(Qv) + list(Sv), axis=-1)
        right = np.stack(list(T) + list(Q) + list(S), axis=-1)
        assert J == 1 or (_bits(wrong) != _bits(right)).any(), v
