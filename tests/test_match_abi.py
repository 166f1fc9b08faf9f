"""CPU: the entry points of motion matching (SPEC.md section 25) are declared in include/mtr.h, exported by libmtr.so and bound
by api.py with the argument counts of their prototypes, and mirrored in mtr.hpp and mtr-sys; the three records have their
stated sizes and field offsets, in C and in the dtypes of api.py and of the model; the constants agree; the rows of the error
table that need no device hold (the rest is held on the host build by tests/test_match_host_sanitizer.py and on the GPU by
tests/test_gpu_match.py); anim_match.py builds rows, normalised features and trajectory features; the ABI version stays 2."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import cpp_build
from tests.abi_header import prototypes as _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mtr_anim_match_create": 17, "mtr_anim_match_destroy": 1, "mtr_anim_match_search_device": 9, "mtr_anim_match_search_host": 8,
         "mtr_anim_match_scores_host": 5}


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
    create = api.lib.mtr_anim_match_create.argtypes
    assert create[5] is ctypes.c_uint64 and create[6] is ctypes.c_uint32 and all(create[k] is ctypes.c_float for k in (7, 8, 9))  # not pointer-sized integers
    for name in ("mtr_anim_match_search_device", "mtr_anim_match_search_host"):
        assert getattr(api.lib, name).argtypes[5] is ctypes.c_uint32
    for word in ("mtr_match_row", "mtr_match_filter", "mtr_match_result", "mtr_anim_match", "MTR_MATCH_INTERRUPT", "MTR_MATCH_NONE"):
        assert word in rs, f"mtr-sys: {word}"
    assert api.lib.mtr_abi_version() == 2


def test_record_layouts(tmp_path):
    from mt_renderer_amd import api
    from tests import match_model as mm
    u4, f4 = np.dtype("<u4"), np.dtype("<f4")
    for dt in (api.MATCH_ROW, mm.ROW):
        assert dt.itemsize == 16 and dt.names == ("clip", "x", "bias", "tags")
        assert [dt.fields[n] for n in dt.names] == [(u4, 0), (f4, 4), (f4, 8), (u4, 12)]
    for dt in (api.MATCH_FILTER, mm.FILTER):
        assert dt.itemsize == 8 and dt.names == ("require", "exclude") and [dt.fields[n] for n in dt.names] == [(u4, 0), (u4, 4)]
    for dt in (api.MATCH_RESULT, mm.RESULT):
        assert dt.itemsize == 16 and dt.names == ("row", "cur", "score", "cur_score")
        assert [dt.fields[n] for n in dt.names] == [(u4, 0), (u4, 4), (f4, 8), (f4, 12)]
    assert api.MATCH_INTERRUPT == 1 == mm.INTERRUPT and api.MATCH_NONE == 0xFFFFFFFF == mm.NONE and api.MATCH_MAX_DIMS == 64
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "mtr.h"\n'
                   '_Static_assert(sizeof(mtr_match_row) == 16 && _Alignof(mtr_match_row) == 4, "row size");\n'
                   '_Static_assert(offsetof(mtr_match_row, clip) == 0 && offsetof(mtr_match_row, x) == 4, "clip, x");\n'
                   '_Static_assert(offsetof(mtr_match_row, bias) == 8 && offsetof(mtr_match_row, tags) == 12, "bias, tags");\n'
                   '_Static_assert(sizeof(mtr_match_filter) == 8 && _Alignof(mtr_match_filter) == 4, "filter size");\n'
                   '_Static_assert(offsetof(mtr_match_filter, require) == 0 && offsetof(mtr_match_filter, exclude) == 4, "require, exclude");\n'
                   '_Static_assert(sizeof(mtr_match_result) == 16 && _Alignof(mtr_match_result) == 4, "result size");\n'
                   '_Static_assert(offsetof(mtr_match_result, row) == 0 && offsetof(mtr_match_result, cur) == 4, "row, cur");\n'
                   '_Static_assert(offsetof(mtr_match_result, score) == 8 && offsetof(mtr_match_result, cur_score) == 12, "score, cur_score");\n'
                   '_Static_assert(MTR_MATCH_INTERRUPT == 1u && MTR_MATCH_NONE == 0xFFFFFFFFu && MTR_MATCH_MAX_DIMS == 64, "constants");\n'
                   '_Static_assert(MTR_ABI_VERSION == 2, "ABI version");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["g++", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    cpp = tmp_path / "mirror.cpp"
    cpp.write_text('#include "mtr.hpp"\nint main() { return sizeof(mtr::AnimMatch) != 0 ? 0 : 1; }\n')
    subprocess.check_call(["g++", cpp_build.STD, "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(cpp)])


def test_null_handles_are_rejected_without_a_device():
    """the rows of the error table that need no device: a NULL device or set is MTR_E_INVALID before anything is touched"""
    from mt_renderer_amd import api
    L = api.lib
    pl, cm_, rs = np.zeros(3, dtype=api.PLAY_STATE), np.zeros(3, dtype=api.PLAY_CMD), np.zeros(3, dtype=api.MATCH_RESULT)
    nk, rows, ft, q, sc = np.array([30], dtype=np.uint32), np.zeros(1, dtype=api.MATCH_ROW), np.ones((1, 4), dtype=np.float32), np.zeros((3, 4), dtype=np.float32), np.zeros((3, 1), dtype=np.float32)
    h = ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.mtr_anim_match_create(None, 1, p(nk), None, 4, 0, 0, 0.2, 0.0, 0.0, p(rows), 1, p(ft), None, None, 3, ctypes.byref(h)) == api.MTR_E_INVALID and not h
    assert L.mtr_anim_match_search_device(None, p(pl), p(q), None, 3, 0, p(cm_), p(rs), None) == api.MTR_E_INVALID
    assert L.mtr_anim_match_search_host(None, p(pl), p(q), None, 3, 0, p(cm_), p(rs)) == api.MTR_E_INVALID
    assert L.mtr_anim_match_scores_host(None, p(pl), p(q), 3, p(sc)) == api.MTR_E_INVALID
    L.mtr_anim_match_destroy(None)
    assert not cm_.view(np.uint8).any() and not rs.view(np.uint8).any() and not sc.any()


def test_python_builds_the_database():
    from mt_renderer_amd import anim_match, api
    from tests import root_model as rm
    rows = anim_match.rows_of([30, 12, 5], [api.CLIP_LOOP, 0, 0], stride=4, tail=3)
    assert rows.dtype == api.MATCH_ROW and list(rows["clip"]) == [0] * 8 + [1] * 3 + [2] and list(rows["x"]) == [0, 4, 8, 12, 16, 20, 24, 28, 0, 4, 8, 0]
    assert not rows["bias"].any() and not rows["tags"].any()
    raw = np.random.default_rng(3).standard_normal((40, 8)) * [1, 2, 3, 4, 5, 6, 7, 0] + 5.0
    w = [1, 1, 1, 1, 2, 2, 2, 2]
    feats, mean, scale = anim_match.normalise(raw, w)
    assert feats.dtype == mean.dtype == scale.dtype == np.float32 and feats.shape == (40, 8)
    assert np.allclose(feats[:, :7].std(0), w[:7], rtol=1e-5) and np.allclose(feats.mean(0), 0, atol=1e-5) and scale[7] == 2.0 and not feats[:, 7].any()
    # a query equal to a row's raw features is that row's features bit for bit: the set normalises in the same two operations
    q = ((raw.astype(np.float32)[7] - mean).astype(np.float32) * scale).astype(np.float32)
    assert q.tobytes() == feats[7].tobytes()
    # trajectory features: a straight walk along +z at 0.1 per key, no turn; then a cyclic one that runs on into the next cycle
    keys = np.zeros((6, 12)); keys[:, 2] = 0.1 * np.arange(6); keys[:, 7] = 1
    tf = anim_match.trajectory_features(keys, (1, 3), cyclic=False)
    assert tf.shape == (6, 8) and np.allclose(tf[0], [0, 0.1, 0, 1, 0, 0.3, 0, 1]) and np.allclose(tf[4], [0, 0.1, 0, 1, 0, 0.1, 0, 1])
    tf = anim_match.trajectory_features(keys, (1, 3), cyclic=True)
    assert np.allclose(tf[4], [0, 0.1, 0, 1, 0, 0.3, 0, 1])
    walk = rm.walk_clip(31, 1)[0][0]
    tf = anim_match.trajectory_features(walk, (4, 8))
    assert tf.shape == (31, 8) and np.isfinite(tf).all() and np.allclose(tf[:, 2] ** 2 + tf[:, 3] ** 2, 1) and (tf[:, 1] > 0).all()
    assert np.allclose(tf[0], tf[30], atol=1e-6), "the last key is where the next cycle's key 0 stands"
    for bad in (lambda: anim_match.rows_of([30], [0, 0]), lambda: anim_match.rows_of([3], [0], tail=5), lambda: anim_match.normalise(np.zeros((0, 4))),
                lambda: anim_match.normalise(np.zeros((3, 4)), [1, 2]), lambda: anim_match.trajectory_features(np.zeros((4, 7)), (1,))):
        with pytest.raises(api.MtrError):
            bad()
