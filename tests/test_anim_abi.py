"""CPU: the animation-clip entry points (SPEC.md section 14) are declared in include/mtr.h, exported by libmtr.so and bound by
api.py with the argument count of their prototype; the two structs have their stated sizes; and the numpy model of
section 14 (tests/anim_model.py), which the GPU tests pin the kernel to, gives the answers the section's rules imply."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import anim_model as am
from tests.abi_header import prototypes as _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mtr_anim_create", "mtr_anim_destroy", "mtr_model_animate", "mtr_batch_animate", "mtr_batch_animate_device", "mtr_anim_sample"]
F = np.float32


def test_anim_prototypes_declared_exported_and_bound():
    from mt_renderer_amd import api
    protos = _prototypes()
    lib = ctypes.CDLL(api.LIB_PATH)
    for name in NEW:
        assert name in protos, f"include/mtr.h does not declare {name}"
        assert hasattr(lib, name), f"libmtr.so does not export {name}"
        assert name in api.EXPORTED_SYMBOLS, name
        fn = getattr(api.lib, name)
        assert fn.restype is (None if name == "mtr_anim_destroy" else ctypes.c_int32), name
        assert len(fn.argtypes) == protos[name], (name, len(fn.argtypes), protos[name])
    assert api.lib.mtr_abi_version() == 2


def test_struct_sizes(tmp_path):
    from mt_renderer_amd import api
    assert api.ANIM_KEY.itemsize == 48 and api.ANIM_STATE.itemsize == 24
    assert api.ANIM_STATE.names == ("clip_a", "clip_b", "x_a", "x_b", "w", "pad")
    assert [api.ANIM_STATE.fields[n][1] for n in api.ANIM_STATE.names] == [0, 4, 8, 12, 16, 20]
    assert [api.ANIM_KEY.fields[n][1] for n in ("t", "q", "s")] == [0, 16, 32]
    assert api.CLIP_LOOP == 1
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include "mtr.h"\n'
                   '_Static_assert(sizeof(mtr_anim_key) == 48, "mtr_anim_key");\n'
                   '_Static_assert(sizeof(mtr_anim_state) == 24, "mtr_anim_state");\n'
                   '_Static_assert(MTR_CLIP_LOOP == 1u && MTR_ABI_VERSION == 2, "constants");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["g++", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_handles_are_rejected_without_a_device():
    from mt_renderer_amd import api
    L = api.lib
    out = ctypes.c_void_p(1)
    assert L.mtr_anim_create(None, 1, 1, None, None, None, ctypes.byref(out)) == api.MTR_E_INVALID
    assert L.mtr_anim_destroy(None) is None
    assert L.mtr_model_animate(None, None, None) == api.MTR_E_INVALID
    assert L.mtr_batch_animate(None, None, None) == api.MTR_E_INVALID
    assert L.mtr_batch_animate_device(None, None, None, None) == api.MTR_E_INVALID
    assert L.mtr_anim_sample(None, None, 0, None, 0) == api.MTR_E_INVALID
    assert api.lib.mtr_abi_version() == 2


def test_state_conversion():
    from mt_renderer_amd import api
    st = api.anim_states(dict(clip_a=[0, 1, 2], x_a=[0.5, 1.5, 2.5], w=0.25))
    assert st.dtype == api.ANIM_STATE and st.shape == (3,)
    assert list(st["clip_a"]) == [0, 1, 2] and list(st["clip_b"]) == [0, 0, 0] and (st["w"] == F(0.25)).all()
    assert api.anim_states(st, 3) is not None
    with pytest.raises(api.MtrError):
        api.anim_states(st, 4)
    with pytest.raises(api.MtrError):
        api.anim_states(np.zeros((3, 6), dtype=np.float32))
    with pytest.raises(api.MtrError):
        api.anim_states(dict(clip_a=[0], x_a=[0.0], speed=[1.0]))


# ---- the model's own known answers -------------------------------------------------------------------------------
STATE = np.dtype([("clip_a", "<u4"), ("clip_b", "<u4"), ("x_a", "<f4"), ("x_b", "<f4"), ("w", "<f4"), ("pad", "<u4")])


def _states(**cols):
    n = max(np.atleast_1d(v).size for v in cols.values())
    st = np.zeros(n, dtype=STATE)
    for k, v in cols.items():
        st[k] = v
    return st


def _matrix(t, q, s):
    """from_scale_rotation_translation in float64, column-major 16"""
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    M = np.eye(4)
    M[:3, :3] = R * np.asarray(s)[None, :]
    M[:3, 3] = t
    return M.T.reshape(16)


def _key(t, q, s):
    return np.array([*t, 0.0, *q, *s, 0.0], dtype=F)


def _clips():
    rng = np.random.default_rng(7)
    return am.random_clips(rng, 3)


def test_position_rules():
    N = np.array([120] * 10)
    loop = np.ones(10, dtype=bool)
    x = np.array([0.0, -0.0, 119.5, 120.0, -1e-7, np.nan, np.inf, -np.inf, 3e38, 119.99999], dtype=F)
    i0, i1, a = am.position(x, N, loop)
    assert list(i0) == [0, 0, 119, 0, 0, 0, 0, 0, 0, 119]
    assert list(i1) == [1, 1, 0, 1, 1, 1, 1, 1, 1, 0]
    assert a[2] == F(0.5) and a[4] == 0 and a[3] == 0 and 0 < a[9] < 1
    # the rounding case the r == Nf clause exists for: -1e-7 wraps to exactly 120.0 in binary32
    assert F(-1e-7) - np.floor(F(-1e-7) / F(120)) * F(120) == F(120)
    # clamp mode holds the ends
    x = np.array([-5.0, 0.0, 29.25, 30.0, 31.0, 1e30, np.nan, np.inf, -np.inf], dtype=F)
    i0, i1, a = am.position(x, np.array([31] * 9), np.zeros(9, dtype=bool))
    assert list(i0) == [0, 0, 29, 30, 30, 30, 0, 30, 0]
    assert list(i1) == [1, 1, 30, 30, 30, 30, 1, 30, 1]
    assert list(a) == [0, 0, 0.25, 0, 0, 0, 0, 0, 0]
    # a fraction is exact: r - float(i0) never rounds
    xs = np.random.default_rng(1).uniform(0, 120, 1000).astype(F)
    i0, _, a = am.position(xs, np.array([120] * 1000), np.ones(1000, dtype=bool))
    assert (a.astype(np.float64) == xs.astype(np.float64) - i0).all()


def test_a_zero_returns_the_key_with_a_renormalised_quaternion():
    q = np.array([0.3, -0.2, 0.5, 0.7])  # not of unit length: the rule normalises also at a == 0
    k0 = _key((1.0, 2.0, 3.0), q, (1.0, 1.5, 0.5))
    k1 = _key((4.0, 5.0, 6.0), (0.0, 0.0, 0.0, 1.0), (1.0, 1.0, 1.0))
    clips = [(np.stack([k0, k1]).reshape(2, 1, 12), 0)]
    got = am.sample(clips, _states(clip_a=0, x_a=0.0), 1)[0, 0]
    want = _matrix((1.0, 2.0, 3.0), q / np.linalg.norm(q), (1.0, 1.5, 0.5))
    assert np.abs(got - want).max() < 1e-6
    assert got[12] == 1.0 and got[13] == 2.0 and got[14] == 3.0 and got[15] == 1.0 and got[3] == 0.0
    col0 = got[0:3].astype(np.float64)
    assert abs(np.linalg.norm(col0) - 1.0) < 1e-6, "a rotation column of unit length: the quaternion was renormalised"
    # a zero quaternion cannot be normalised: identity rotation
    clips = [(np.stack([_key((0, 0, 0), (0, 0, 0, 0), (1, 1, 1))] * 2).reshape(2, 1, 12), 0)]
    got = am.sample(clips, _states(clip_a=0, x_a=0.5), 1)[0, 0]
    assert (got == np.eye(4, dtype=F).reshape(16)).all()


def test_one_key_clip_is_constant_and_modes_wrap_or_hold():
    clips = _clips()  # 2 loop, 31 clamp, 120 loop, 1 clamp
    xs = np.array([0.0, -3.5, 0.75, 1e9, -1e9, np.nan, np.inf, 17.0], dtype=F)
    one = am.sample(clips, _states(clip_a=3, x_a=xs), 3)
    assert (one.view(np.uint32) == one[:1].view(np.uint32)).all(), "a one-key clip is the same for every x"
    # LOOP at N - 0.5 interpolates last -> first: equal to a two-key clip (last, first) at 0.5
    k = clips[2][0]
    pair = [(np.stack([k[119], k[0]]), 0)]
    a = am.sample(clips, _states(clip_a=2, x_a=119.5), 3)
    b = am.sample(pair, _states(clip_a=0, x_a=0.5), 3)
    assert (a.view(np.uint32) == b.view(np.uint32)).all()
    # clamp mode holds the ends
    lo = am.sample(clips, _states(clip_a=1, x_a=[-7.0, 0.0]), 3)
    hi = am.sample(clips, _states(clip_a=1, x_a=[30.0, 44.0]), 3)
    assert (lo[0].view(np.uint32) == lo[1].view(np.uint32)).all() and (hi[0].view(np.uint32) == hi[1].view(np.uint32)).all()
    # -1e-7 on the 120-key loop is key 0, not key 120
    z = am.sample(clips, _states(clip_a=2, x_a=[-1e-7, 0.0]), 3)
    assert (z[0].view(np.uint32) == z[1].view(np.uint32)).all()
    # clip indices are clamped
    c = am.sample(clips, _states(clip_a=[3, 4, 0xFFFFFFFF], x_a=0.0), 3)
    assert (c.view(np.uint32) == c[:1].view(np.uint32)).all()


def test_w_zero_ignores_clip_b():
    clips = _clips()
    a = am.sample(clips, _states(clip_a=2, x_a=17.25, clip_b=0xFFFFFFFF, x_b=np.nan, w=0.0), 3)
    b = am.sample(clips, _states(clip_a=2, x_a=17.25, clip_b=1, x_b=3.0, w=0.0), 3)
    c = am.sample(clips, _states(clip_a=2, x_a=17.25, clip_b=1, x_b=3.0, w=[-0.5, np.nan, -0.0]), 3)
    assert np.isfinite(a).all()
    assert (a.view(np.uint32) == b.view(np.uint32)).all() and (c.view(np.uint32) == a.view(np.uint32)).all()
    # w == 1 goes through the formulas: clip B's pose up to the roundings of the cross-fade, w > 1 is w == 1
    one = am.sample(clips, _states(clip_a=2, x_a=17.25, clip_b=1, x_b=3.0, w=[1.0, 7.0]), 3)
    only_b = am.sample(clips, _states(clip_a=1, x_a=3.0), 3)
    assert (one[0].view(np.uint32) == one[1].view(np.uint32)).all()
    assert np.abs(one[0] - only_b[0]).max() < 1e-5


def test_exact_model_agrees_with_the_rule_within_the_bound():
    """the float64 version against the binary32 one on the CPU: the bound of section 14 holds for the model itself"""
    rng = np.random.default_rng(14)
    clips = am.random_clips(rng, 64)
    st = am.random_states(rng, 256, STATE)
    tr = am.Trace()
    got = am.sample(clips, st, 64)
    val, mag = am.sample_exact(clips, st, 64, trace=tr)
    keep = ~tr.near
    assert (~keep).sum() < 0.01 * keep.size
    frac = np.abs(got.astype(np.float64) - val)[keep] / (am.K_LOCALS * am.U * mag[keep] + 1e-300)
    print("largest fraction of the bound:", frac.max(), "left out:", int((~keep).sum()), "min |d|:", np.abs(tr.all_d()).min())
    assert frac.max() <= 1.0
