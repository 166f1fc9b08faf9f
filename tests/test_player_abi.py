"""CPU: the entry points of players (SPEC.md section 20) are declared in include/mtr.h, exported by libmtr.so and bound by api.py
with the argument counts of their prototypes; mtr_play_state and mtr_play_cmd have their stated sizes and field offsets, in C and
in api.PLAY_STATE / api.PLAY_CMD; the constants agree; the error table of include/mtr.h holds where no GPU is needed (the rest is
held on the host build by tests/test_player_host_sanitizer.py and on the GPU by tests/test_gpu_player.py); the ABI version stays 2."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.abi_header import prototypes as _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"mtr_anim_player_create": 7, "mtr_anim_player_destroy": 1, "mtr_anim_player_advance_device": 11, "mtr_anim_player_advance_device_cmds": 11,
         "mtr_anim_player_advance_host": 10}


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
    for name in ("mtr_anim_player_advance_device", "mtr_anim_player_advance_device_cmds", "mtr_anim_player_advance_host"):
        assert getattr(api.lib, name).argtypes[3] is ctypes.c_float  # dt travels as a float, not as a pointer-sized integer
    assert "mtr_play_state" in rs and "mtr_play_cmd" in rs and "MTR_PLAY_ENDED" in rs and "mtr_anim_player" in rs
    assert api.lib.mtr_abi_version() == 2


def test_record_layouts(tmp_path):
    from mt_renderer_amd import api
    from tests import player_model as pm
    for dt in (api.PLAY_STATE, pm.PLAY):
        assert dt.itemsize == 32 and dt.names == ("clip_a", "clip_b", "x_a", "x_b", "w", "fade", "speed", "flags")
        assert [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12, 16, 20, 24, 28]
        assert all(dt.fields[n][0] == np.dtype("<u4") for n in ("clip_a", "clip_b", "flags"))
        assert all(dt.fields[n][0] == np.dtype("<f4") for n in ("x_a", "x_b", "w", "fade", "speed"))
    for dt in (api.PLAY_CMD, pm.CMD):
        assert dt.itemsize == 16 and dt.names == ("instance", "clip", "x", "seconds") and [dt.fields[n][1] for n in dt.names] == [0, 4, 8, 12]
        assert dt.fields["instance"][0] == np.dtype("<u4") and dt.fields["seconds"][0] == np.dtype("<f4")
    assert (api.PLAY_ENDED, api.CLIP_LOOP) == (1, 1) == (pm.ENDED, pm.LOOP)
    assert (api.ANIM_STATE, api.ANIM_LAYER, api.ROOT_STEP) == (pm.STATE, pm.LAYER, pm.STEP)
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "mtr.h"\n'
                   '_Static_assert(sizeof(mtr_play_state) == 32 && _Alignof(mtr_play_state) == 4, "state size");\n'
                   '_Static_assert(offsetof(mtr_play_state, clip_a) == 0 && offsetof(mtr_play_state, clip_b) == 4, "clips");\n'
                   '_Static_assert(offsetof(mtr_play_state, x_a) == 8 && offsetof(mtr_play_state, x_b) == 12, "positions");\n'
                   '_Static_assert(offsetof(mtr_play_state, w) == 16 && offsetof(mtr_play_state, fade) == 20, "w, fade");\n'
                   '_Static_assert(offsetof(mtr_play_state, speed) == 24 && offsetof(mtr_play_state, flags) == 28, "speed, flags");\n'
                   '_Static_assert(sizeof(mtr_play_cmd) == 16 && _Alignof(mtr_play_cmd) == 4, "command size");\n'
                   '_Static_assert(offsetof(mtr_play_cmd, instance) == 0 && offsetof(mtr_play_cmd, clip) == 4, "instance, clip");\n'
                   '_Static_assert(offsetof(mtr_play_cmd, x) == 8 && offsetof(mtr_play_cmd, seconds) == 12, "x, seconds");\n'
                   '_Static_assert(MTR_PLAY_ENDED == 1u && MTR_CLIP_LOOP == 1u, "constants");\n'
                   '_Static_assert(MTR_ABI_VERSION == 2, "ABI version");\n'
                   'int main(void) { return 0; }\n')
    subprocess.check_call(["g++", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_null_handles_are_rejected_without_a_device():
    """the rows of the error table that need no device: a NULL device or player is MTR_E_INVALID before anything is touched"""
    from mt_renderer_amd import api
    L = api.lib
    st = np.zeros(3, dtype=api.PLAY_STATE)
    nk, rt = np.array([30], dtype=np.uint32), np.array([30.0], dtype=np.float32)
    h = ctypes.c_void_p()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert L.mtr_anim_player_create(None, 1, p(nk), None, p(rt), 8, ctypes.byref(h)) == api.MTR_E_INVALID and not h
    assert L.mtr_anim_player_advance_device(None, p(st), 3, 0.0, None, 0, None, None, 0, None, None) == api.MTR_E_INVALID
    assert L.mtr_anim_player_advance_device_cmds(None, p(st), 3, 0.0, None, 0, None, None, 0, None, None) == api.MTR_E_INVALID
    assert L.mtr_anim_player_advance_host(None, p(st), 3, 0.0, None, 0, None, None, 0, None) == api.MTR_E_INVALID
    L.mtr_anim_player_destroy(None)


def test_python_builds_commands():
    from mt_renderer_amd import api
    c = api.play_cmds(dict(instance=[0, 5, 5], clip=[1, 2, 0], seconds=[0.0, 0.25, 0.5]))
    assert c.dtype == api.PLAY_CMD and c.shape == (3,) and c.flags.c_contiguous and (c["x"] == 0).all() and list(c["instance"]) == [0, 5, 5]
    assert api.play_cmds(None).shape == (0,) and api.play_cmds(np.zeros(4, dtype=api.PLAY_CMD)).shape == (4,)
    for bad in (lambda: api.play_cmds(dict(instance=[1])), lambda: api.play_cmds(dict(instance=[1], clip=[0], y=[1])),
                lambda: api.play_cmds(np.zeros(4, dtype=api.ROOT_STEP)), lambda: api.play_cmds(np.zeros((2, 2), dtype=api.PLAY_CMD))):
        with pytest.raises(api.MtrError):
            bad()
