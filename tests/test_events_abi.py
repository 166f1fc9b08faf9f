"""CPU: the entry points of animation events (SPEC.md section 22) are declared in include/mtr.h, which compiles as plain C11,
exported by libmtr.so and bound by api.py with the argument counts of their prototypes; the two records have their stated sizes
(8 and 16 bytes) and field offsets, in C and in the dtypes of api.py and of the model; the rows of the error table that need no
device hold (the rest is held on the host build by tests/test_events_host_sanitizer.py and on the GPU by
tests/test_gpu_events.py); anim_events.build sorts stably and decode splits `where`; the ABI version stays 2."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.abi_header import prototypes as _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mtr_anim_events_create": 8, "mtr_anim_events_destroy": 1, "mtr_anim_events_collect_device": 10, "mtr_anim_events_collect_host": 9}


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
    for name in ("mtr_anim_events_collect_device", "mtr_anim_events_collect_host"):
        assert getattr(api.lib, name).argtypes[4] is ctypes.c_float  # min_weight travels as a float
    for word in ("mtr_event_marker", "mtr_anim_event", "mtr_anim_events", "MTR_EVENT_BACKWARD"):
        assert word in rs, f"mtr-sys: {word}"
    assert api.lib.mtr_abi_version() == 2


def test_record_layouts_and_the_header_as_c11(tmp_path):
    from mt_renderer_amd import api
    from tests import events_model as em
    u4, f4 = np.dtype("<u4"), np.dtype("<f4")
    for dt in (api.EVENT_MARKER, em.MARKER):
        assert dt.itemsize == 8 and dt.names == ("x", "id") and dt.fields["x"] == (f4, 0) and dt.fields["id"] == (u4, 4)
    for dt in (api.EVENT, em.EVENT):
        assert dt.itemsize == 16 and dt.names == ("instance", "id", "where", "w")
        assert [dt.fields[n] for n in dt.names] == [(u4, 0), (u4, 4), (u4, 8), (f4, 12)]
    assert api.EVENT_BACKWARD == 0x80000000 == em.BACKWARD and api.ROOT_STEP == em.STEP
    if shutil.which("gcc") is None and shutil.which("g++") is None:
        pytest.skip("no host compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "mtr.h"\n'
                   '_Static_assert(sizeof(mtr_event_marker) == 8 && _Alignof(mtr_event_marker) == 4, "marker size");\n'
                   '_Static_assert(offsetof(mtr_event_marker, x) == 0 && offsetof(mtr_event_marker, id) == 4, "x, id");\n'
                   '_Static_assert(sizeof(mtr_anim_event) == 16 && _Alignof(mtr_anim_event) == 4, "event size");\n'
                   '_Static_assert(offsetof(mtr_anim_event, instance) == 0 && offsetof(mtr_anim_event, id) == 4, "instance, id");\n'
                   '_Static_assert(offsetof(mtr_anim_event, where) == 8 && offsetof(mtr_anim_event, w) == 12, "where, w");\n'
                   '_Static_assert(sizeof(mtr_root_step) == 16 && MTR_ROOT_MAX_STEPS == 8, "the steps are the root steps");\n'
                   '_Static_assert(MTR_EVENT_BACKWARD == 0x80000000u && MTR_ABI_VERSION == 2, "constants");\n'
                   'int main(void) { mtr_anim_events *ev = NULL; mtr_anim_events_destroy(ev); return 0; }\n')
    cc = "gcc" if shutil.which("gcc") else "g++"
    subprocess.check_call([cc, "-x", "c", "-std=c11", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_handles_are_rejected_without_a_device():
    """the rows of the error table that need no device: a NULL device or set is MTR_E_INVALID before anything is touched"""
    from mt_renderer_amd import api
    L = api.lib
    sp, ev = np.zeros((3, 2), dtype=api.ROOT_STEP), np.full(4, 0x5A, dtype=np.uint8).repeat(16).view(api.EVENT)
    ct, bt = np.full(2, 7, dtype=np.uint32), np.full(3, 9, dtype=np.uint32)
    nk, cn, mk = np.array([30], dtype=np.uint32), np.array([1], dtype=np.uint32), np.zeros(1, dtype=api.EVENT_MARKER)
    h = ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.mtr_anim_events_create(None, 1, p(nk), None, p(cn), p(mk), 3, ctypes.byref(h)) == api.MTR_E_INVALID and not h
    assert L.mtr_anim_events_collect_device(None, p(sp), 2, 3, 0.0, p(ev), 4, p(ct), p(bt), None) == api.MTR_E_INVALID
    assert L.mtr_anim_events_collect_host(None, p(sp), 2, 3, 0.0, p(ev), 4, p(ct), p(bt)) == api.MTR_E_INVALID
    L.mtr_anim_events_destroy(None)
    assert (ev.view(np.uint8) == 0x5A).all() and (ct == 7).all() and (bt == 9).all()


def test_python_builds_and_decodes():
    from mt_renderer_amd import anim_events, api
    counts, mk = anim_events.build({2: [(7.0, 1), (3.0, 2), (7.0, 3), (3.0, 4)], 0: [(0.0, 9)]}, 4)
    assert counts.dtype == np.uint32 and list(counts) == [1, 0, 4, 0] and mk.dtype == api.EVENT_MARKER
    assert list(mk["x"]) == [0.0, 3.0, 3.0, 7.0, 7.0] and list(mk["id"]) == [9, 2, 4, 1, 3], "sorted by x, ties in the order given"
    c0, m0 = anim_events.build({}, 2)
    assert list(c0) == [0, 0] and m0.shape == (0,) and m0.dtype == api.EVENT_MARKER
    for bad in (lambda: anim_events.build({4: [(0.0, 1)]}, 4), lambda: anim_events.build({0: [(float("nan"), 1)]}, 1), lambda: anim_events.build({0: [(1.0,)]}, 1)):
        with pytest.raises(api.MtrError):
            bad()
    ev = np.zeros(2, dtype=api.EVENT)
    ev[0] = (5, 77, 3 | (1 << 24) | api.EVENT_BACKWARD, 0.25)
    ev[1] = (6, 78, 0xFFFFFF | (7 << 24), 1.0)
    d = anim_events.decode(ev)
    assert list(d["instance"]) == [5, 6] and list(d["id"]) == [77, 78] and list(d["clip"]) == [3, 0xFFFFFF] and list(d["step"]) == [1, 7]
    assert list(d["backward"]) == [True, False] and list(d["w"]) == [0.25, 1.0]
