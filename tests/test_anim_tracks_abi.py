"""CPU: mtr_anim_create_tracks (SPEC.md section 15) is declared in include/mtr.h, exported by libmtr.so and bound by api.py
with the argument count of its prototype; mtr_anim_track has its stated size and field offsets; NULL arguments are rejected
without a GPU; the ABI version stays 2."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.abi_header import prototypes as _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mtr_anim_create_tracks"


def test_prototype_declared_exported_and_bound():
    from mt_renderer_amd import api
    protos = _prototypes()
    assert protos.get(NAME) == 10, f"include/mtr.h: {NAME} with ten arguments"
    assert hasattr(ctypes.CDLL(api.LIB_PATH), NAME), f"libmtr.so does not export {NAME}"
    assert NAME in api.EXPORTED_SYMBOLS
    fn = getattr(api.lib, NAME)
    assert fn.restype is ctypes.c_int32 and len(fn.argtypes) == protos[NAME]
    for text, where in ((open(os.path.join(ROOT, "include", "mtr.hpp")).read(), "mtr.hpp"),
                        (open(os.path.join(ROOT, "rust", "mtr-sys", "src", "lib.rs")).read(), "mtr-sys")):
        assert NAME in text and "mtr_anim_track" in text, where
    assert api.lib.mtr_abi_version() == 2


def test_track_descriptor_layout(tmp_path):
    from mt_renderer_amd import anim_tracks, api
    from tests import anim_tracks_model as tm
    for dt in (api.ANIM_TRACK, anim_tracks.ANIM_TRACK, tm.TRACK):
        assert dt.itemsize == 32 and dt.names == ("first", "count", "lo", "step")
        assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 20]
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "mtr.h"\n'
                   '_Static_assert(sizeof(mtr_anim_track) == 32, "mtr_anim_track");\n'
                   '_Static_assert(offsetof(mtr_anim_track, first) == 0 && offsetof(mtr_anim_track, count) == 4, "first, count");\n'
                   '_Static_assert(offsetof(mtr_anim_track, lo) == 8 && offsetof(mtr_anim_track, step) == 20, "lo, step");\n'
                   '_Static_assert(MTR_ABI_VERSION == 2, "ABI version");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["g++", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_arguments_are_rejected_without_a_device():
    from mt_renderer_amd import api
    L = api.lib
    one = np.ones(1, dtype=np.uint32)
    tr = np.zeros(3, dtype=api.ANIM_TRACK)
    tr["count"] = 1
    t, v = np.zeros(1, dtype=np.uint16), np.zeros(4, dtype=np.uint16)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = ctypes.c_void_p(1)
    assert L.mtr_anim_create_tracks(None, 1, 1, p(one), None, p(tr), p(t), p(v), 1, ctypes.byref(out)) == api.MTR_E_INVALID
    assert L.mtr_anim_create_tracks(None, 1, 1, None, None, None, None, None, 0, ctypes.byref(out)) == api.MTR_E_INVALID
    assert L.mtr_anim_create_tracks(None, 1, 1, p(one), None, p(tr), p(t), p(v), 1, None) == api.MTR_E_INVALID
    assert api.lib.mtr_abi_version() == 2


def test_python_concatenates_and_rebases():
    from mt_renderer_amd import api
    from tests import anim_tracks_model as tm
    clips = tm.random_track_clips(np.random.default_rng(2), 3)
    nt, fl, tr, t, v = api.anim_track_arrays(3, clips)
    mn, mf, mtr_, mt, mv = tm.concat(clips, 3)
    assert (nt == mn).all() and (fl == mf).all() and (t == mt).all() and (v == mv).all()
    assert tr.dtype == api.ANIM_TRACK and tr.tobytes() == mtr_.reshape(-1).tobytes()
    assert clips[1][2]["first"].min() == 0, "the caller's arrays are left as they were"
    with pytest.raises(api.MtrError):
        api.anim_track_arrays(4, clips)
    with pytest.raises(api.MtrError):
        api.anim_track_arrays(3, [])
