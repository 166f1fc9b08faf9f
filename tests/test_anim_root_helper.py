"""CPU: mt_renderer_amd/anim_root.py::split_root (a helper of SPEC.md section 19, not part of the rule) on 24-joint walks made
from the generators of tests/anim_model.py: in float64, the trajectory key composed with the in-place clip's root local
reproduces the source's root local at every key; the other joints are untouched; a looping source loses its duplicated end
key in the in-place clip and keeps it in the trajectory."""
import numpy as np
import pytest

from mt_renderer_amd.anim_root import split_root
from tests import anim_model as anm
from tests.anim_ik_model import local_matrix

J, N = 24, 31


def _walk(rng):
    """a 24-joint clip whose root strides forward, sways, bobs, turns and leans; the last key is the first a cycle later"""
    keys = anm.gentle_clips(rng, J, shape=[(N, 0)], angle=0.3, trans=0.2, scale=(0.8, 1.25))[0][0].astype(np.float64)
    k = np.arange(N) / (N - 1)
    yaw, lean = 0.8 * k + 0.1 * np.sin(2 * np.pi * k), 0.15 * np.sin(4 * np.pi * k)
    keys[:, 0, 0:3] = np.stack([0.4 * np.sin(2 * np.pi * k) + 0.5 * k, 0.9 + 0.05 * np.cos(4 * np.pi * k), 2.5 * k], axis=-1)
    qy = np.stack([np.zeros(N), np.sin(yaw / 2), np.zeros(N), np.cos(yaw / 2)], axis=-1)
    qx = np.stack([np.sin(lean / 2), np.zeros(N), np.zeros(N), np.cos(lean / 2)], axis=-1)
    from mt_renderer_amd.anim_root import _qmul
    keys[:, 0, 4:8] = _qmul(qy, qx) * np.where(rng.random((N, 1)) < 0.3, -1.0, 1.0)
    return keys.astype(np.float32)


def _mat(key):
    """[n, 12] keys -> mathematical matrices [n][row][column], float64"""
    k = key.astype(np.float64)
    return local_matrix(k[:, 0:3], k[:, 4:8], k[:, 8:11]).reshape(-1, 4, 4).transpose(0, 2, 1)


@pytest.mark.parametrize("rotate", ["twist", "all", "none"])
def test_trajectory_times_in_place_root_is_the_source_root(rotate):
    # measured over the 8 seeds below: the worst element error relative to the largest element of the source's root matrix is
    # 2.9e-8 for "twist", 2.6e-8 for "all", 2.0e-8 for "none" (the three sets of keys are binary32, and a source rotation is
    # unit only to 2^-24); the margin is 4 x the largest
    TOL = 4 * 2.9e-8
    worst = 0.0
    for seed in range(8):
        keys = _walk(np.random.default_rng(seed))
        inplace, traj = split_root(keys, 0, rotate=rotate)
        assert inplace.dtype == traj.dtype == np.float32 and inplace.shape == keys.shape and traj.shape == (N, 1, 12)
        assert (inplace[:, 1:] == keys[:, 1:]).all() and (inplace[:, 0, 8:11] == keys[:, 0, 8:11]).all(), "the other joints and the scale are untouched"
        assert (traj[:, 0, 1] == 0).all() and (inplace[:, 0, 1] != 0).all(), "the height stays in the pose"
        assert (traj[:, 0, 8:11] == 1).all()
        if rotate == "twist":
            assert (traj[:, 0, 4] == 0).all() and (traj[:, 0, 6] == 0).all() and (np.abs(traj[:, 0, 5]) > 0).any(), "a rotation about up"
        if rotate == "none":
            assert (traj[:, 0, 4:8] == (0, 0, 0, 1)).all()
        want = _mat(keys[:, 0])
        got = _mat(traj[:, 0]) @ _mat(inplace[:, 0])
        rel = np.abs(got - want).max(axis=(1, 2)) / np.abs(want).max(axis=(1, 2))
        worst = max(worst, float(rel.max()))
    print(f"split_root ({rotate}): worst relative error {worst:.2e}")
    assert worst <= TOL


def test_looping_source_and_arguments():
    keys = _walk(np.random.default_rng(11))
    inplace, traj = split_root(keys, 0, loop=True)
    full, _ = split_root(keys, 0)
    assert inplace.shape == (N - 1, J, 12) and traj.shape == (N, 1, 12) and (inplace == full[:-1]).all()
    side, t2 = split_root(keys, 0, translate=(1, 1, 1), up=(0, 2, 0))
    assert (side[:, 0, 0:3] == 0).all() and (t2[:, 0, 0:3] == keys[:, 0, 0:3]).all()
    for bad in (lambda: split_root(keys, J), lambda: split_root(keys[0], 0), lambda: split_root(keys, 0, rotate="yaw"), lambda: split_root(keys, 0, up=(0, 0, 0)),
                lambda: split_root(keys[:1], 0, loop=True)):
        with pytest.raises(ValueError):
            bad()
