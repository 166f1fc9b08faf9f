"""CPU: the entry points of animation layers (SPEC.md section 16) are declared in include/mtr.h, exported by libmtr.so and
bound by api.py with the argument counts of their prototypes; mtr_anim_layer has its stated size and field offsets; NULL
arguments are rejected without a GPU; the ABI version stays 2."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.abi_header import prototypes as _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mtr_anim_masks_create": 5, "mtr_anim_masks_destroy": 1, "mtr_model_animate_layers": 5, "mtr_batch_animate_layers": 5,
         "mtr_batch_animate_layers_device": 6, "mtr_anim_sample_layers": 7}


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
    assert "mtr_anim_layer" in rs and "mtr_anim_masks" in rs
    assert api.lib.mtr_abi_version() == 2


def test_layer_record_layout(tmp_path):
    from mt_renderer_amd import api
    from tests import anim_layers_model as lm
    for dt in (api.ANIM_LAYER, lm.LAYER):
        assert dt.itemsize == 16 and dt.names == ("clip", "x", "w", "mask", "mode")
        assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 14]
    assert (api.ANIM_MAX_LAYERS, api.LAYER_OVERRIDE, api.LAYER_ADDITIVE) == (8, 0, 1) == (lm.MAX_LAYERS, lm.OVERRIDE, lm.ADDITIVE)
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "mtr.h"\n'
                   '_Static_assert(sizeof(mtr_anim_layer) == 16, "mtr_anim_layer");\n'
                   '_Static_assert(offsetof(mtr_anim_layer, clip) == 0 && offsetof(mtr_anim_layer, x) == 4 && offsetof(mtr_anim_layer, w) == 8, "clip, x, w");\n'
                   '_Static_assert(offsetof(mtr_anim_layer, mask) == 12 && offsetof(mtr_anim_layer, mode) == 14, "mask, mode");\n'
                   '_Static_assert(MTR_ANIM_MAX_LAYERS == 8 && MTR_LAYER_OVERRIDE == 0 && MTR_LAYER_ADDITIVE == 1, "constants");\n'
                   '_Static_assert(MTR_ABI_VERSION == 2, "ABI version");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["g++", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_arguments_are_rejected_without_a_device():
    from mt_renderer_amd import api
    L = api.lib
    w = np.ones(4, dtype=np.float32)
    ly = np.zeros(2, dtype=api.ANIM_LAYER)
    out = np.zeros(16, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    h = ctypes.c_void_p(1)
    assert L.mtr_anim_masks_create(None, 4, 1, p(w), ctypes.byref(h)) == api.MTR_E_INVALID
    assert L.mtr_anim_masks_destroy(None) is None
    assert L.mtr_model_animate_layers(None, None, None, p(ly), 2) == api.MTR_E_INVALID
    assert L.mtr_batch_animate_layers(None, None, None, p(ly), 2) == api.MTR_E_INVALID
    assert L.mtr_batch_animate_layers_device(None, None, None, p(ly), 2, None) == api.MTR_E_INVALID
    assert L.mtr_anim_sample_layers(None, None, p(ly), 2, 1, p(out), out.size) == api.MTR_E_INVALID
    assert api.lib.mtr_abi_version() == 2


def test_python_builds_layer_stacks():
    from mt_renderer_amd import api
    ly = api.anim_layers(dict(clip=[[0, 3]], x=[[1.5, 2.0]], mode=[[0, 1]]), 4)
    assert ly.shape == (4, 2) and ly.dtype == api.ANIM_LAYER and ly.flags.c_contiguous
    assert (ly["w"] == 1).all() and (ly["mask"] == 0).all() and (ly["clip"][:, 1] == 3).all() and (ly["mode"][:, 1] == 1).all()
    flat = np.zeros(12, dtype=api.ANIM_LAYER)
    assert api.anim_layers(flat, 4).shape == (4, 3) and api.anim_layers(flat, None, 2).shape == (6, 2)
    assert api.anim_layers(flat.reshape(3, 4), 3, 4).shape == (3, 4)
    for bad in (lambda: api.anim_layers(flat, 5), lambda: api.anim_layers(dict(clip=0)), lambda: api.anim_layers(dict(clip=0, x=0, y=1)),
                lambda: api.anim_layers(np.zeros(4, dtype=api.ANIM_STATE)), lambda: api.anim_layers(flat.reshape(3, 4), 3, 3)):
        with pytest.raises(api.MtrError):
            bad()
