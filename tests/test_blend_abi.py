"""CPU: the entry points of blend spaces (SPEC.md section 23) are declared in include/mtr.h, which compiles as plain C11,
exported by libmtr.so and bound by api.py with the argument counts of their prototypes; the three records have their stated
size (16 bytes) and field offsets, in C and in the dtypes of api.py and of the model; the rows of the error table that need no
device hold (the rest is held on the host build by tests/test_blend_host_sanitizer.py and on the GPU by
tests/test_gpu_blend.py); the ABI version stays 2."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.abi_header import prototypes as _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mtr_anim_blend_create": 15, "mtr_anim_blend_destroy": 1, "mtr_anim_blend_advance_device": 10, "mtr_anim_blend_advance_host": 9}


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
    for name in ("mtr_anim_blend_advance_device", "mtr_anim_blend_advance_host"):
        assert getattr(api.lib, name).argtypes[4] is ctypes.c_float  # dt travels as a float
    assert api.lib.mtr_anim_blend_create.argtypes[12] is ctypes.c_float  # and so does damp
    for word in ("mtr_blend_sample", "mtr_blend_tri", "mtr_blend_state", "mtr_anim_blend"):
        assert word in rs, f"mtr-sys: {word}"
    assert api.lib.mtr_abi_version() == 2


def test_record_layouts_and_the_header_as_c11(tmp_path):
    from mt_renderer_amd import api
    from tests import blend_model as bm
    u4, f4 = np.dtype("<u4"), np.dtype("<f4")
    for dt in (api.BLEND_SAMPLE, bm.SAMPLE):
        assert dt.itemsize == 16 and dt.names == ("clip", "px", "py", "pad")
        assert [dt.fields[n] for n in dt.names] == [(u4, 0), (f4, 4), (f4, 8), (u4, 12)]
    for dt in (api.BLEND_TRI, bm.TRI):
        assert dt.itemsize == 16 and dt.names == ("v", "pad") and dt.fields["v"][1] == 0 and dt.fields["v"][0].shape == (3,) and dt.fields["pad"] == (u4, 12)
    for dt in (api.BLEND_STATE, bm.STATE):
        assert dt.itemsize == 16 and dt.names == ("phase", "px", "py", "speed") and [dt.fields[n] for n in dt.names] == [(f4, 0), (f4, 4), (f4, 8), (f4, 12)]
    assert api.ROOT_STEP == bm.STEP and api.ANIM_LAYER == bm.LAYER
    if shutil.which("gcc") is None and shutil.which("g++") is None:
        pytest.skip("no host compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "mtr.h"\n'
                   '_Static_assert(sizeof(mtr_blend_sample) == 16 && _Alignof(mtr_blend_sample) == 4, "sample size");\n'
                   '_Static_assert(offsetof(mtr_blend_sample, clip) == 0 && offsetof(mtr_blend_sample, px) == 4, "clip, px");\n'
                   '_Static_assert(offsetof(mtr_blend_sample, py) == 8 && offsetof(mtr_blend_sample, pad) == 12, "py, pad");\n'
                   '_Static_assert(sizeof(mtr_blend_tri) == 16 && offsetof(mtr_blend_tri, v) == 0 && offsetof(mtr_blend_tri, pad) == 12, "triangle");\n'
                   '_Static_assert(sizeof(mtr_blend_state) == 16 && offsetof(mtr_blend_state, phase) == 0 && offsetof(mtr_blend_state, px) == 4, "phase, px");\n'
                   '_Static_assert(offsetof(mtr_blend_state, py) == 8 && offsetof(mtr_blend_state, speed) == 12, "py, speed");\n'
                   '_Static_assert(sizeof(mtr_root_step) == 16 && sizeof(mtr_anim_layer) == 16 && MTR_ABI_VERSION == 2, "the records written");\n'
                   'int main(void) { mtr_anim_blend *b = NULL; mtr_anim_blend_destroy(b); return 0; }\n')
    cc = "gcc" if shutil.which("gcc") else "g++"
    subprocess.check_call([cc, "-x", "c", "-std=c11", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_handles_are_rejected_without_a_device():
    """the rows of the error table that need no device: a NULL device or set is MTR_E_INVALID before anything is touched"""
    from mt_renderer_amd import api
    L = api.lib
    st, pr = np.full(3, 0.25, dtype=np.float32).repeat(4).view(api.BLEND_STATE), np.full((3, 2), 7.0, dtype=np.float32)
    ly, sp, sh = np.full(9, 0x5A, dtype=np.uint8).repeat(16).view(api.ANIM_LAYER), np.full(9, 0x5A, dtype=np.uint8).repeat(16).view(api.ROOT_STEP), np.full(9, 9.0, dtype=np.float32)
    nk, fl, rt = np.array([30], dtype=np.uint32), np.array([1], dtype=np.uint32), np.array([30.0], dtype=np.float32)
    sm = np.zeros(1, dtype=api.BLEND_SAMPLE)
    h = ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.mtr_anim_blend_create(None, 1, p(nk), p(fl), p(rt), p(sm), 1, None, 0, 2, 0, 0, 4.0, 3, ctypes.byref(h)) == api.MTR_E_INVALID and not h
    assert L.mtr_anim_blend_advance_device(None, p(st), p(pr), 3, 0.5, p(ly), 3, p(sp), p(sh), None) == api.MTR_E_INVALID
    assert L.mtr_anim_blend_advance_host(None, p(st), p(pr), 3, 0.5, p(ly), 3, p(sp), p(sh)) == api.MTR_E_INVALID
    L.mtr_anim_blend_destroy(None)
    assert (st.view(np.float32) == 0.25).all() and (pr == 7).all() and (ly.view(np.uint8) == 0x5A).all() and (sp.view(np.uint8) == 0x5A).all() and (sh == 9).all()
