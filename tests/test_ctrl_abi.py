"""CPU: the entry points of controllers (SPEC.md section 21) are declared in include/mtr.h, exported by libmtr.so and bound by
api.py with the argument counts of their prototypes; the four records have their stated sizes and field offsets, in C and in
the dtypes of api.py and of the model; the constants agree; the rows of the error table that need no device hold (the rest is
held on the host build by tests/test_ctrl_host_sanitizer.py and on the GPU by tests/test_gpu_ctrl.py); anim_ctrl.build makes
the tables of the model's locomotion graph; the ABI version stays 2."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.abi_header import prototypes as _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mtr_anim_ctrl_create": 11, "mtr_anim_ctrl_destroy": 1, "mtr_anim_ctrl_step_device": 9, "mtr_anim_ctrl_step_host": 8}


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
    for name in ("mtr_anim_ctrl_step_device", "mtr_anim_ctrl_step_host"):
        assert getattr(api.lib, name).argtypes[5] is ctypes.c_float  # dt travels as a float, not as a pointer-sized integer
    for word in ("mtr_ctrl_node", "mtr_ctrl_cond", "mtr_ctrl_trans", "mtr_ctrl_state", "mtr_anim_ctrl", "MTR_TR_CONSUME", "MTR_CTRL_FADING", "MTR_OP_NE"):
        assert word in rs, f"mtr-sys: {word}"
    assert api.lib.mtr_abi_version() == 2


def test_record_layouts(tmp_path):
    from mt_renderer_amd import api
    from tests import ctrl_model as cm
    u4, f4, u2 = np.dtype("<u4"), np.dtype("<f4"), np.dtype("<u2")
    for dt in (api.CTRL_NODE, cm.NODE):
        assert dt.itemsize == 16 and dt.names == ("clip", "first", "count", "pad") and all(dt.fields[n] == (u4, 4 * i) for i, n in enumerate(dt.names))
    for dt in (api.CTRL_COND, cm.COND):
        assert dt.itemsize == 8 and dt.names == ("param", "op", "value")
        assert dt.fields["param"] == (u2, 0) and dt.fields["op"] == (u2, 2) and dt.fields["value"] == (f4, 4)
    for dt, cond in ((api.CTRL_TRANS, api.CTRL_COND), (cm.TRANS, cm.COND)):
        assert dt.itemsize == 48 and dt.names == ("target", "flags", "seconds", "x", "ncond", "pad", "cond")
        assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 20, 24]
        assert [dt.fields[n][0] for n in dt.names[:6]] == [u4, u4, f4, f4, u4, u4] and dt.fields["cond"][0] == np.dtype((cond, (3,)))
    for dt in (api.CTRL_STATE, cm.STATE):
        assert dt.itemsize == 16 and dt.names == ("node", "t", "fired", "user")
        assert [dt.fields[n] for n in dt.names] == [(u4, 0), (f4, 4), (u4, 8), (u4, 12)]
    assert (api.OP_LT, api.OP_LE, api.OP_GT, api.OP_GE, api.OP_EQ, api.OP_NE) == (0, 1, 2, 3, 4, 5) == (cm.LT, cm.LE, cm.GT, cm.GE, cm.EQ, cm.NE)
    assert (api.TR_INTERRUPT, api.TR_SELF, api.TR_SYNC, api.TR_CONSUME) == (1, 2, 4, 8) == (cm.INTERRUPT, cm.SELF, cm.SYNC, cm.CONSUME)
    assert (api.CTRL_TIME, api.CTRL_POS, api.CTRL_PHASE, api.CTRL_ENDED, api.CTRL_FADING) == (0xFFFF, 0xFFFE, 0xFFFD, 0xFFFC, 0xFFFB) == cm.BUILTINS
    assert api.CTRL_NONE == 0xFFFFFFFF == cm.NONE and api.CTRL_MAX_COND == 3
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "mtr.h"\n'
                   '_Static_assert(sizeof(mtr_ctrl_node) == 16 && _Alignof(mtr_ctrl_node) == 4, "node size");\n'
                   '_Static_assert(offsetof(mtr_ctrl_node, clip) == 0 && offsetof(mtr_ctrl_node, first) == 4, "clip, first");\n'
                   '_Static_assert(offsetof(mtr_ctrl_node, count) == 8 && offsetof(mtr_ctrl_node, pad) == 12, "count, pad");\n'
                   '_Static_assert(sizeof(mtr_ctrl_cond) == 8 && offsetof(mtr_ctrl_cond, param) == 0, "condition size");\n'
                   '_Static_assert(offsetof(mtr_ctrl_cond, op) == 2 && offsetof(mtr_ctrl_cond, value) == 4, "op, value");\n'
                   '_Static_assert(sizeof(mtr_ctrl_trans) == 48 && _Alignof(mtr_ctrl_trans) == 4, "transition size");\n'
                   '_Static_assert(offsetof(mtr_ctrl_trans, target) == 0 && offsetof(mtr_ctrl_trans, flags) == 4, "target, flags");\n'
                   '_Static_assert(offsetof(mtr_ctrl_trans, seconds) == 8 && offsetof(mtr_ctrl_trans, x) == 12, "seconds, x");\n'
                   '_Static_assert(offsetof(mtr_ctrl_trans, ncond) == 16 && offsetof(mtr_ctrl_trans, pad) == 20, "ncond, pad");\n'
                   '_Static_assert(offsetof(mtr_ctrl_trans, cond) == 24 && MTR_CTRL_MAX_COND == 3, "conditions");\n'
                   '_Static_assert(sizeof(mtr_ctrl_state) == 16 && _Alignof(mtr_ctrl_state) == 4, "state size");\n'
                   '_Static_assert(offsetof(mtr_ctrl_state, node) == 0 && offsetof(mtr_ctrl_state, t) == 4, "node, t");\n'
                   '_Static_assert(offsetof(mtr_ctrl_state, fired) == 8 && offsetof(mtr_ctrl_state, user) == 12, "fired, user");\n'
                   '_Static_assert(MTR_OP_LT == 0 && MTR_OP_LE == 1 && MTR_OP_GT == 2 && MTR_OP_GE == 3 && MTR_OP_EQ == 4 && MTR_OP_NE == 5, "ops");\n'
                   '_Static_assert(MTR_TR_INTERRUPT == 1u && MTR_TR_SELF == 2u && MTR_TR_SYNC == 4u && MTR_TR_CONSUME == 8u, "flags");\n'
                   '_Static_assert(MTR_CTRL_TIME == 0xFFFFu && MTR_CTRL_POS == 0xFFFEu && MTR_CTRL_PHASE == 0xFFFDu, "built-ins");\n'
                   '_Static_assert(MTR_CTRL_ENDED == 0xFFFCu && MTR_CTRL_FADING == 0xFFFBu && MTR_CTRL_NONE == 0xFFFFFFFFu, "built-ins");\n'
                   '_Static_assert(MTR_ABI_VERSION == 2, "ABI version");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["g++", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_handles_are_rejected_without_a_device():
    """the rows of the error table that need no device: a NULL device or controller is MTR_E_INVALID before anything is touched"""
    from mt_renderer_amd import api
    L = api.lib
    st, pl, cm_ = np.zeros(3, dtype=api.CTRL_STATE), np.zeros(3, dtype=api.PLAY_STATE), np.zeros(3, dtype=api.PLAY_CMD)
    nk, nd = np.array([30], dtype=np.uint32), np.zeros(1, dtype=api.CTRL_NODE)
    h = ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.mtr_anim_ctrl_create(None, 1, p(nk), None, p(nd), 1, None, 0, 0, 0, ctypes.byref(h)) == api.MTR_E_INVALID and not h
    assert L.mtr_anim_ctrl_step_device(None, p(st), p(pl), None, 3, 0.0, p(cm_), None, None) == api.MTR_E_INVALID
    assert L.mtr_anim_ctrl_step_host(None, p(st), p(pl), None, 3, 0.0, p(cm_), None) == api.MTR_E_INVALID
    L.mtr_anim_ctrl_destroy(None)
    assert not st.view(np.uint8).any() and not cm_.view(np.uint8).any()


def test_python_builds_the_tables():
    from mt_renderer_amd import anim_ctrl, api
    from tests import ctrl_model as cm
    nodes = [dict(name="idle", clip=0), dict(name="walk", clip=1), dict(name="run", clip=2), dict(name="jump", clip=3)]
    trans = [
        dict(src="walk", dst="idle", when=[("speed", "<", 0.4)], seconds=0.2),
        dict(src="idle", dst="walk", when=[("speed", ">", 0.6)], seconds=0.2),
        dict(src="any", dst="jump", when=[("trigger", ">", 0.5)], flags=("interrupt", "consume")),
        dict(src="walk", dst="run", when=[("speed", ">", 2.2)], seconds=0.2, flags=("sync",)),
        dict(src="run", dst="walk", when=[("speed", "<", 1.8)], seconds=0.2, flags=("sync",)),
        dict(src="jump", dst="idle", when=[("ENDED", ">=", 1.0)], seconds=0.1),
    ]
    g = anim_ctrl.build(nodes, trans, params=["speed", "trigger"])
    want = cm.locomotion()
    assert g["nany"] == want["nany"] == 1 and g["params"] == ["speed", "trigger"] and g["index"]["jump"] == cm.JUMP
    assert g["nodes"].dtype == api.CTRL_NODE and g["trans"].dtype == api.CTRL_TRANS
    assert g["nodes"].tobytes() == want["nodes"].tobytes() and g["trans"].tobytes() == want["trans"].tobytes()
    # names numbered by first appearance, a node without transitions, no transitions at all
    g2 = anim_ctrl.build(nodes[:2], [dict(src="idle", dst="walk", when=[("b", "!=", 1.0), ("TIME", ">", 2.0), ("a", "==", 0.0)])])
    assert g2["params"] == ["b", "a"] and list(g2["nodes"]["count"]) == [1, 0] and list(g2["nodes"]["first"]) == [0, 0]
    assert list(g2["trans"]["cond"]["param"][0]) == [0, api.CTRL_TIME, 1] and list(g2["trans"]["cond"]["op"][0]) == [api.OP_NE, api.OP_GT, api.OP_EQ]
    g3 = anim_ctrl.build(nodes[:1], [])
    assert g3["trans"].shape == (0,) and g3["nany"] == 0 and g3["params"] == []
    for bad in (lambda: anim_ctrl.build([dict(name="any", clip=0)], []), lambda: anim_ctrl.build(nodes + nodes[:1], []),
                lambda: anim_ctrl.build(nodes, [dict(src="idle", dst="nowhere")]), lambda: anim_ctrl.build(nodes, [dict(src="idle", dst="walk", flags=("loop",))]),
                lambda: anim_ctrl.build(nodes, [dict(src="idle", dst="walk", when=[("a", "~", 1.0)])]),
                lambda: anim_ctrl.build(nodes, [dict(src="idle", dst="walk", when=[("a", ">", 1.0)] * 4)]),
                lambda: anim_ctrl.build(nodes, [dict(src="idle", dst="walk", when=[("a", ">", 1.0)])], params=["b"])):
        with pytest.raises(api.MtrError):
            bad()
