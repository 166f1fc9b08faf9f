"""CPU: the entry points of spring bones (SPEC.md section 24) are declared in include/mtr.h, exported by libmtr.so and bound
by api.py with the argument counts of their prototypes, and mirrored in mtr.hpp and mtr-sys; mtr_spring and
mtr_spring_state have their stated sizes and field offsets; NULL arguments are rejected without a GPU; the ABI version stays
2; anim_spring.chain builds the records of a strand."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import cpp_build
from tests.abi_header import prototypes as _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mtr_anim_spring_create": 6, "mtr_anim_spring_destroy": 1, "mtr_batch_animate_spring_device": 12, "mtr_anim_sample_spring": 13}


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
    assert "mtr_spring_state" in rs and "pub struct mtr_spring " in rs and "mtr_anim_spring" in rs and "MTR_ANIM_MAX_SPRINGS" in rs
    assert api.lib.mtr_abi_version() == 2


def test_record_layouts(tmp_path):
    from mt_renderer_amd import api
    from tests import spring_model as sm
    for dt in (api.SPRING, sm.SPRING):
        assert dt.itemsize == 48 and dt.names == ("joint", "flags", "stiffness", "drag", "tail", "pad0", "gravity", "pad1")
        assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 28, 32, 44]
    for dt in (api.SPRING_STATE, sm.STATE):
        assert dt.itemsize == 32 and dt.names == ("cur", "live", "prev", "pad")
        assert [dt.fields[n][1] for n in dt.names] == [0, 12, 16, 28]
    assert api.ANIM_MAX_SPRINGS == 16 == sm.MAX_SPRINGS
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "mtr.h"\n'
                   '_Static_assert(sizeof(mtr_spring) == 48 && sizeof(mtr_spring_state) == 32, "sizes");\n'
                   '_Static_assert(offsetof(mtr_spring, joint) == 0 && offsetof(mtr_spring, flags) == 4, "joint, flags");\n'
                   '_Static_assert(offsetof(mtr_spring, stiffness) == 8 && offsetof(mtr_spring, drag) == 12, "stiffness, drag");\n'
                   '_Static_assert(offsetof(mtr_spring, tail) == 16 && offsetof(mtr_spring, pad0) == 28, "tail, pad0");\n'
                   '_Static_assert(offsetof(mtr_spring, gravity) == 32 && offsetof(mtr_spring, pad1) == 44, "gravity, pad1");\n'
                   '_Static_assert(offsetof(mtr_spring_state, cur) == 0 && offsetof(mtr_spring_state, live) == 12, "cur, live");\n'
                   '_Static_assert(offsetof(mtr_spring_state, prev) == 16 && offsetof(mtr_spring_state, pad) == 28, "prev, pad");\n'
                   '_Static_assert(MTR_ANIM_MAX_SPRINGS == 16, "constants");\n'
                   '_Static_assert(MTR_ABI_VERSION == 2, "ABI version");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["g++", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    # and the C++ mirror compiles
    cpp = tmp_path / "mirror.cpp"
    cpp.write_text('#include "mtr.hpp"\nint main() { return sizeof(mtr::AnimSpring) != 0 ? 0 : 1; }\n')
    subprocess.check_call(["g++", cpp_build.STD, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(cpp)])


def test_null_arguments_are_rejected_without_a_device():
    from mt_renderer_amd import api
    L = api.lib
    par = np.array([255, 0, 1], dtype=np.uint8)
    sp = np.zeros(1, dtype=api.SPRING)
    sp["joint"], sp["tail"] = 1, (0.0, 1.0, 0.0)
    ly = np.zeros(2, dtype=api.ANIM_LAYER)
    st = np.zeros(1, dtype=api.SPRING_STATE)
    out = np.zeros(48, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    h = ctypes.c_void_p(1)
    assert L.mtr_anim_spring_create(None, 3, p(par), 1, p(sp), ctypes.byref(h)) == api.MTR_E_INVALID
    assert L.mtr_anim_spring_destroy(None) is None
    assert L.mtr_batch_animate_spring_device(None, None, None, p(ly), 2, None, None, None, p(st), None, 1.0 / 60.0, None) == api.MTR_E_INVALID
    assert L.mtr_anim_sample_spring(None, None, None, None, p(ly), 2, None, p(st), None, 1.0 / 60.0, 1, p(out), out.size) == api.MTR_E_INVALID
    assert api.lib.mtr_abi_version() == 2


def test_python_builds_a_strand():
    from mt_renderer_amd import anim_spring, api
    parents = [255, 0, 1, 2, 0]
    bt = np.arange(15, dtype=np.float32).reshape(5, 3)
    sp = anim_spring.chain(parents, bt, [1, 2, 3], 30.0, [0.1, 0.2, 0.3], gravity=(0, -9.8, 0), leaf_tail=(0, 0.5, 0))
    assert sp.dtype == api.SPRING and sp.shape == (3,) and list(sp["joint"]) == [1, 2, 3]
    assert (sp["tail"][0] == bt[2]).all() and (sp["tail"][1] == bt[3]).all() and (sp["tail"][2] == (0, 0.5, 0)).all()
    assert (sp["stiffness"] == 30).all() and np.allclose(sp["drag"], [0.1, 0.2, 0.3]) and (sp["gravity"] == (0, np.float32(-9.8), 0)).all()
    assert (sp["flags"] == 0).all() and (sp["pad0"] == 0).all() and (sp["pad1"] == 0).all()
    assert (anim_spring.chain(parents, bt, [1, 2], 1.0, 0.0)["tail"][1] == bt[3]).all(), "the only child's bind translation"
    for bad in (lambda: anim_spring.chain(parents, bt, [1, 3], 1.0, 0.0, leaf_tail=(1, 0, 0)), lambda: anim_spring.chain(parents, bt, [3], 1.0, 0.0),
                lambda: anim_spring.chain(parents, bt, [0], 1.0, 0.0), lambda: anim_spring.chain(parents, bt[:4], [1], 1.0, 0.0),
                lambda: anim_spring.chain(parents, bt, [5], 1.0, 0.0, leaf_tail=(1, 0, 0))):
        with pytest.raises(api.MtrError):
            bad()
