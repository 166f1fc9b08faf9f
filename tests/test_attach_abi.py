"""CPU: the entry points of attachments (SPEC.md section 18) are declared in include/mtr.h, exported by libmtr.so and bound by
api.py with the argument counts of their prototypes; mtr_attach has its stated size and field offsets, in C and in api.ATTACH;
the error table of include/mtr.h holds where no GPU is needed; the ABI version stays 2."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.abi_header import prototypes as _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mtr_batch_attach": 3, "mtr_batch_attach_device": 4, "mtr_batch_sockets": 5, "mtr_batch_sockets_device": 5,
         "mtr_batch_read_model_mats": 3}


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
        assert len(fn.argtypes) == nargs and fn.restype is ctypes.c_int32
        assert name in hpp, f"mtr.hpp: {name}"
        assert name in rs, f"mtr-sys: {name}"
    assert "mtr_attach" in rs and "MTR_ATTACH_NO_JOINT" in rs
    assert api.lib.mtr_abi_version() == 2


def test_record_layout(tmp_path):
    from mt_renderer_amd import api
    from tests import attach_model as am
    for dt in (api.ATTACH, am.ATTACH):
        assert dt.itemsize == 80 and dt.names == ("src_instance", "joint", "flags", "pad", "offset")
        assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16]
        assert dt.fields["offset"][0].shape == (16,) and dt.fields["offset"][0].base == np.dtype("<f4")
    assert (api.ATTACH_NO_JOINT, api.ATTACH_POSITION_ONLY) == (0xFFFFFFFF, 1) == (am.NO_JOINT, am.POSITION_ONLY)
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "mtr.h"\n'
                   '_Static_assert(sizeof(mtr_attach) == 80 && _Alignof(mtr_attach) == 4, "size");\n'
                   '_Static_assert(offsetof(mtr_attach, src_instance) == 0 && offsetof(mtr_attach, joint) == 4, "src_instance, joint");\n'
                   '_Static_assert(offsetof(mtr_attach, flags) == 8 && offsetof(mtr_attach, pad) == 12, "flags, pad");\n'
                   '_Static_assert(offsetof(mtr_attach, offset) == 16, "offset");\n'
                   '_Static_assert(MTR_ATTACH_NO_JOINT == 0xFFFFFFFFu && MTR_ATTACH_POSITION_ONLY == 1u, "constants");\n'
                   '_Static_assert(MTR_ABI_VERSION == 2, "ABI version");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["g++", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_handles_are_rejected_without_a_device():
    """the rows of the error table that need no device: a NULL batch or source is MTR_E_INVALID before anything is touched
    (the rest of the table -- pointers, alignment, n == 0, count, another device -- is held on the host build by
    tests/test_attach_order.py and on the GPU by tests/test_gpu_attach.py)"""
    from mt_renderer_amd import api
    L = api.lib
    recs = np.zeros(3, dtype=api.ATTACH)
    out = np.zeros(48, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.mtr_batch_attach(None, None, p(recs)) == api.MTR_E_INVALID
    assert L.mtr_batch_attach_device(None, None, p(recs), None) == api.MTR_E_INVALID
    assert L.mtr_batch_sockets(None, p(recs), 3, p(out), out.size) == api.MTR_E_INVALID
    assert L.mtr_batch_sockets_device(None, p(recs), 3, p(out), None) == api.MTR_E_INVALID
    assert L.mtr_batch_read_model_mats(None, p(out), out.size) == api.MTR_E_INVALID
    assert api.lib.mtr_abi_version() == 2


def test_python_builds_records():
    from mt_renderer_amd import api
    r = api.attach_records(dict(src_instance=[0, 1, 2], joint=[5, 6, 7]), 3)
    assert r.dtype == api.ATTACH and r.shape == (3,) and r.flags.c_contiguous
    assert (r["flags"] == 0).all() and (r["offset"] == np.eye(4, dtype=np.float32).reshape(16)).all() and list(r["joint"]) == [5, 6, 7]
    r = api.attach_records(dict(src_instance=[4]), None)
    assert r["joint"][0] == api.ATTACH_NO_JOINT
    flat = np.zeros((2, 3), dtype=api.ATTACH)
    assert api.attach_records(flat, 6).shape == (6,)
    for bad in (lambda: api.attach_records(flat, 5), lambda: api.attach_records(dict(joint=[1]), 1), lambda: api.attach_records(dict(src_instance=[0], x=1), 1),
                lambda: api.attach_records(np.zeros(4, dtype=api.ANIM_LAYER), 4), lambda: api.attach_records(np.zeros(0, dtype=api.ATTACH), None)):
        with pytest.raises(api.MtrError):
            bad()
