"""CPU: the entry points of inverse kinematics (SPEC.md section 17) are declared in include/mtr.h, exported by libmtr.so and
bound by api.py with the argument counts of their prototypes; mtr_ik_chain and mtr_ik_target have their stated sizes and
field offsets; NULL arguments are rejected without a GPU; the ABI version stays 2."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.abi_header import prototypes as _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mtr_anim_ik_create": 6, "mtr_anim_ik_destroy": 1, "mtr_model_animate_ik": 7, "mtr_batch_animate_ik": 7,
         "mtr_batch_animate_ik_device": 8, "mtr_anim_sample_ik": 9}


def test_prototypes_declared_exported_and_bound():
    from mt_renderer_amd import api
    protos = _prototypes()
    so = ctypes.CDLL(api.LIB_PATH)
    hpp = open(os.path.join(ROOT, "include", "mtr.hpp")).read()
    rs = open(os.path.join(ROOT, "rust", "mtr-sys", "src", "lib.rs")).read()
    for name, nargs in NAMES.items():
        assert protos.get(name) == nargs, f"include/mtr.h: {name} with {nargs} arguments"
        assert hasattr(so, name), f"libmtr.so does not export {name}"
        assert name in api.EXPORTED_SYMBOLS
        fn = getattr(api.lib, name)
        assert len(fn.argtypes) == nargs and fn.restype is (None if name.endswith("_destroy") else ctypes.c_int32)
        assert name in hpp, f"mtr.hpp: {name}"
        assert name in rs, f"mtr-sys: {name}"
    assert "mtr_ik_chain" in rs and "mtr_ik_target" in rs and "mtr_anim_ik" in rs and "MTR_ANIM_MAX_IK" in rs
    assert api.lib.mtr_abi_version() == 2


def test_record_layouts(tmp_path):
    from mt_renderer_amd import api
    from tests import anim_ik_model as ik
    for dt in (api.ANIM_IK_CHAIN, ik.CHAIN):
        assert dt.itemsize == 32 and dt.names == ("kind", "joint", "axis", "flags")
        assert [dt.fields[n][1] for n in dt.names] == [0, 4, 16, 28]
    for dt in (api.ANIM_IK_TARGET, ik.TARGET):
        assert dt.itemsize == 32 and dt.names == ("pos", "w", "pole", "pad")
        assert [dt.fields[n][1] for n in dt.names] == [0, 12, 16, 28]
    assert (api.ANIM_MAX_IK, api.IK_TWO_BONE, api.IK_AIM, api.IK_POLE) == (4, 0, 1, 1) == (ik.MAX_IK, ik.TWO_BONE, ik.AIM, ik.POLE)
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "mtr.h"\n'
                   '_Static_assert(sizeof(mtr_ik_chain) == 32 && sizeof(mtr_ik_target) == 32, "sizes");\n'
                   '_Static_assert(offsetof(mtr_ik_chain, kind) == 0 && offsetof(mtr_ik_chain, joint) == 4, "kind, joint");\n'
                   '_Static_assert(offsetof(mtr_ik_chain, axis) == 16 && offsetof(mtr_ik_chain, flags) == 28, "axis, flags");\n'
                   '_Static_assert(offsetof(mtr_ik_target, pos) == 0 && offsetof(mtr_ik_target, w) == 12, "pos, w");\n'
                   '_Static_assert(offsetof(mtr_ik_target, pole) == 16 && offsetof(mtr_ik_target, pad) == 28, "pole, pad");\n'
                   '_Static_assert(MTR_ANIM_MAX_IK == 4 && MTR_IK_TWO_BONE == 0 && MTR_IK_AIM == 1 && MTR_IK_POLE == 1, "constants");\n'
                   '_Static_assert(MTR_ABI_VERSION == 2, "ABI version");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["g++", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_arguments_are_rejected_without_a_device():
    from mt_renderer_amd import api
    L = api.lib
    par = np.array([255, 0, 1], dtype=np.uint8)
    ch = np.zeros(1, dtype=api.ANIM_IK_CHAIN)
    ch["joint"][0] = (0, 1, 2)
    ly = np.zeros(2, dtype=api.ANIM_LAYER)
    tg = np.zeros(1, dtype=api.ANIM_IK_TARGET)
    out = np.zeros(48, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    h = ctypes.c_void_p(1)
    assert L.mtr_anim_ik_create(None, 3, p(par), 1, p(ch), ctypes.byref(h)) == api.MTR_E_INVALID
    assert L.mtr_anim_ik_destroy(None) is None
    assert L.mtr_model_animate_ik(None, None, None, p(ly), 2, None, p(tg)) == api.MTR_E_INVALID
    assert L.mtr_batch_animate_ik(None, None, None, p(ly), 2, None, p(tg)) == api.MTR_E_INVALID
    assert L.mtr_batch_animate_ik_device(None, None, None, p(ly), 2, None, p(tg), None) == api.MTR_E_INVALID
    assert L.mtr_anim_sample_ik(None, None, None, p(ly), 2, p(tg), 1, p(out), out.size) == api.MTR_E_INVALID
    assert api.lib.mtr_abi_version() == 2


def test_python_builds_targets():
    from mt_renderer_amd import api
    tg = api.ik_targets(dict(pos=np.ones((4, 2, 3)), pole=np.zeros((4, 2, 3))), 4, 2)
    assert tg.shape == (4, 2) and tg.dtype == api.ANIM_IK_TARGET and tg.flags.c_contiguous
    assert (tg["w"] == 1).all() and (tg["pos"] == 1).all() and (tg["pad"] == 0).all()
    flat = np.zeros(12, dtype=api.ANIM_IK_TARGET)
    assert api.ik_targets(flat, 4, 3).shape == (4, 3) and api.ik_targets(flat, None, 2).shape == (6, 2)
    for bad in (lambda: api.ik_targets(flat, 5, 3), lambda: api.ik_targets(dict(w=1.0), 1, 1), lambda: api.ik_targets(dict(pos=[0, 0, 0], x=1), 1, 1),
                lambda: api.ik_targets(np.zeros(4, dtype=api.ANIM_LAYER), 4, 1), lambda: api.ik_targets(flat[:5], None, 2)):
        with pytest.raises(api.MtrError):
            bad()
