"""CPU: what the pure-numpy record builders of the binding return (anim_states, anim_layers, ik_targets, attach_records,
root_steps, play_cmds, anim_track_arrays) over a fixed corpus of inputs, held to tests/golden/api_records.txt: per case the
dtype, shape, contiguity and SHA-256 of the result's bytes, or the exact text of the MtrError.  The golden was recorded by
``python -m tests.test_api_records --record`` before the binding was restructured; record again only when a builder is meant
to answer differently."""
import hashlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "api_records.txt")


def _filled(dtype, shape):
    """a structured array whose every 32-bit word differs: word k holds k + 1, floats k + 0.5"""
    a = np.zeros(shape, dtype=dtype)
    words = a.view(np.uint32).reshape(-1)
    words[:] = np.arange(1, words.size + 1, dtype=np.uint32)
    flat = a.reshape(-1)
    for name in dtype.names:
        if dtype[name].base == np.dtype("<f4"):
            col = flat[name]
            col[...] = (np.arange(col.size, dtype=np.float32) + np.float32(0.5)).reshape(col.shape)
    return a


def _cases(api):
    """builder name -> [(case name, thunk)]"""
    f4, u4 = np.float32, np.uint32
    ar = lambda n, k=1.0: np.arange(n, dtype=f4) * f4(k)
    S, Ly, T, A, R, P = api.ANIM_STATE, api.ANIM_LAYER, api.ANIM_IK_TARGET, api.ATTACH, api.ROOT_STEP, api.PLAY_CMD
    wrong = np.zeros((3, 6), dtype=f4)
    c = {}
    c["anim_states"] = [
        ("minimal dict", lambda: api.anim_states(dict(clip_a=1, x_a=0.5))),
        ("full dict", lambda: api.anim_states(dict(clip_a=[0, 1, 2], clip_b=[2, 1, 0], x_a=ar(3, 0.5), x_b=ar(3, 1.5), w=[0.0, 0.25, 1.0]))),
        ("scalars broadcast", lambda: api.anim_states(dict(clip_a=[0, 1, 2], x_a=ar(3, 0.5), w=0.25))),
        ("scalars broadcast to n", lambda: api.anim_states(dict(clip_a=1, x_a=2.0), 4)),
        ("unknown key", lambda: api.anim_states(dict(clip_a=[0], x_a=[0.0], speed=[1.0]))),
        ("missing clip_a", lambda: api.anim_states(dict(x_a=[0.0]))),
        ("missing x_a", lambda: api.anim_states(dict(clip_a=[0]))),
        ("array flat", lambda: api.anim_states(_filled(S, 3), 3)),
        ("array 2-D", lambda: api.anim_states(_filled(S, (2, 3)))),
        ("array non-contiguous", lambda: api.anim_states(_filled(S, 6)[::2], 3)),
        ("array wrong dtype", lambda: api.anim_states(wrong)),
        ("array count mismatch", lambda: api.anim_states(_filled(S, 3), 4)),
        ("dict count mismatch", lambda: api.anim_states(dict(clip_a=[0, 1, 2], x_a=ar(3)), 4)),
    ]
    c["anim_layers"] = [
        ("minimal dict", lambda: api.anim_layers(dict(clip=0, x=0.0))),
        ("full dict", lambda: api.anim_layers(dict(clip=np.arange(6).reshape(2, 3), x=ar(6, 0.5).reshape(2, 3), w=ar(6, 0.125).reshape(2, 3),
                                                  mask=np.arange(6).reshape(2, 3) % 3, mode=np.arange(6).reshape(2, 3) % 2), 2, 3)),
        ("scalars broadcast to n", lambda: api.anim_layers(dict(clip=[[0, 1, 2]], x=0.5), 4)),
        ("scalars broadcast to L", lambda: api.anim_layers(dict(clip=[[0], [1]], x=0.5, mode=1), None, 2)),
        ("scalars broadcast to n and L", lambda: api.anim_layers(dict(clip=3, x=0.5), 2, 3)),
        ("one row of fields", lambda: api.anim_layers(dict(clip=[0, 1, 2], x=ar(3)))),
        ("fields of three dimensions", lambda: api.anim_layers(dict(clip=np.zeros((1, 2, 3)), x=0.0))),
        ("unknown key", lambda: api.anim_layers(dict(clip=0, x=0.0, speed=1.0))),
        ("missing clip", lambda: api.anim_layers(dict(x=0.0))),
        ("missing x", lambda: api.anim_layers(dict(clip=0))),
        ("array 2-D", lambda: api.anim_layers(_filled(Ly, (2, 3)), 2, 3)),
        ("array flat with n", lambda: api.anim_layers(_filled(Ly, 6), 2)),
        ("array flat with L", lambda: api.anim_layers(_filled(Ly, 6), None, 3)),
        ("array flat with n and L", lambda: api.anim_layers(_filled(Ly, 6), 3, 2)),
        ("array flat with neither", lambda: api.anim_layers(_filled(Ly, 6))),
        ("array flat that n does not divide", lambda: api.anim_layers(_filled(Ly, 6), 4)),
        ("array flat that L does not divide", lambda: api.anim_layers(_filled(Ly, 6), None, 4)),
        ("array non-contiguous", lambda: api.anim_layers(_filled(Ly, (2, 6))[:, ::2], 2, 3)),
        ("array wrong dtype", lambda: api.anim_layers(wrong)),
        ("array n mismatch", lambda: api.anim_layers(_filled(Ly, (2, 3)), 3)),
        ("array L mismatch", lambda: api.anim_layers(_filled(Ly, (2, 3)), None, 2)),
        ("array n and L mismatch", lambda: api.anim_layers(_filled(Ly, (2, 3)), 3, 2)),
        ("dict n mismatch", lambda: api.anim_layers(dict(clip=np.zeros((2, 3)), x=0.0), 3)),
        ("dict L mismatch", lambda: api.anim_layers(dict(clip=np.zeros((2, 3)), x=0.0), 2, 4)),
    ]
    pos = lambda n, K: ar(n * K * 3, 0.25).reshape(n, K, 3)
    c["ik_targets"] = [
        ("minimal dict", lambda: api.ik_targets(dict(pos=[1.0, 2.0, 3.0]), None, 1)),
        ("full dict", lambda: api.ik_targets(dict(pos=pos(2, 2), w=ar(4, 0.25).reshape(2, 2), pole=pos(2, 2) + f4(7)), 2, 2)),
        ("scalars broadcast", lambda: api.ik_targets(dict(pos=pos(3, 1), w=0.5), 3, 1)),
        ("unknown key", lambda: api.ik_targets(dict(pos=pos(1, 1), pad=0), 1, 1)),
        ("missing pos", lambda: api.ik_targets(dict(w=1.0), 1, 1)),
        ("array flat", lambda: api.ik_targets(_filled(T, 4), 2, 2)),
        ("array 2-D", lambda: api.ik_targets(_filled(T, (2, 2)), None, 2)),
        ("array non-contiguous", lambda: api.ik_targets(_filled(T, (2, 4))[:, ::2], 2, 2)),
        ("array wrong dtype", lambda: api.ik_targets(wrong, 3, 1)),
        ("array that K does not divide", lambda: api.ik_targets(_filled(T, 3), None, 2)),
        ("array empty", lambda: api.ik_targets(np.zeros(0, dtype=T), None, 2)),
        ("array count mismatch", lambda: api.ik_targets(_filled(T, (2, 2)), 3, 2)),
        ("dict count mismatch", lambda: api.ik_targets(dict(pos=pos(2, 2)), 3, 2)),
    ]
    c["attach_records"] = [
        ("minimal dict", lambda: api.attach_records(dict(src_instance=[0, 1]), 2)),
        ("full dict", lambda: api.attach_records(dict(src_instance=[1, 0], joint=[3, api.ATTACH_NO_JOINT], flags=[0, api.ATTACH_POSITION_ONLY],
                                                      offset=ar(32, 0.5).reshape(2, 16)), 2)),
        ("scalars broadcast", lambda: api.attach_records(dict(src_instance=[0, 1, 2], joint=5, flags=1), None)),
        ("unknown key", lambda: api.attach_records(dict(src_instance=[0], pad=[0]), 1)),
        ("missing src_instance", lambda: api.attach_records(dict(joint=[0]), 1)),
        ("array flat", lambda: api.attach_records(_filled(A, 3), 3)),
        ("array 2-D", lambda: api.attach_records(_filled(A, (2, 2)), 4)),
        ("array non-contiguous", lambda: api.attach_records(_filled(A, 6)[::2], None)),
        ("array wrong dtype", lambda: api.attach_records(wrong, None)),
        ("array empty", lambda: api.attach_records(np.zeros(0, dtype=A), None)),
        ("array count mismatch", lambda: api.attach_records(_filled(A, 2), 3)),
        ("dict count mismatch", lambda: api.attach_records(dict(src_instance=[0, 1]), 3)),
    ]
    c["root_steps"] = [
        ("minimal dict", lambda: api.root_steps(dict(clip=[0, 1], x=ar(2, 0.5), dx=ar(2, 0.25)), 2)),
        ("full dict", lambda: api.root_steps(dict(clip=np.arange(6).reshape(2, 3), x=ar(6, 0.5).reshape(2, 3), dx=ar(6, 0.25).reshape(2, 3),
                                                  w=ar(6, 0.125).reshape(2, 3)), 2)),
        ("scalars", lambda: api.root_steps(dict(clip=0, x=1.5, dx=0.25), None)),
        ("unknown key", lambda: api.root_steps(dict(clip=[0], x=[0.0], dx=[0.0], speed=[1.0]), 1)),
        ("missing dx", lambda: api.root_steps(dict(clip=[0], x=[0.0]), 1)),
        ("array flat", lambda: api.root_steps(_filled(R, 3), 3)),
        ("array 2-D", lambda: api.root_steps(_filled(R, (2, 3)), None)),
        ("array 3-D", lambda: api.root_steps(_filled(R, (2, 3, 1)), None)),
        ("array non-contiguous", lambda: api.root_steps(_filled(R, (2, 6))[:, ::2], 2)),
        ("array wrong dtype", lambda: api.root_steps(wrong, None)),
        ("array count mismatch", lambda: api.root_steps(_filled(R, (2, 3)), 3)),
        ("dict count mismatch", lambda: api.root_steps(dict(clip=[0, 1], x=ar(2), dx=ar(2)), 3)),
    ]
    c["play_cmds"] = [
        ("None", lambda: api.play_cmds(None)),
        ("minimal dict", lambda: api.play_cmds(dict(instance=[0, 1], clip=[2, 3]))),
        ("full dict", lambda: api.play_cmds(dict(instance=[2, 0], clip=[1, 1], x=ar(2, 0.5), seconds=[0.0, 0.25]))),
        ("scalars", lambda: api.play_cmds(dict(instance=3, clip=1, x=0.5))),
        ("unknown key", lambda: api.play_cmds(dict(instance=[0], clip=[0], speed=[1.0]))),
        ("missing clip", lambda: api.play_cmds(dict(instance=[0]))),
        ("missing instance", lambda: api.play_cmds(dict(clip=[0]))),
        ("array flat", lambda: api.play_cmds(_filled(P, 3))),
        ("array empty", lambda: api.play_cmds(np.zeros(0, dtype=P))),
        ("array 2-D", lambda: api.play_cmds(_filled(P, (2, 3)))),
        ("array non-contiguous", lambda: api.play_cmds(_filled(P, 6)[::2])),
        ("array wrong dtype", lambda: api.play_cmds(wrong)),
    ]

    def clip(nj, nkeys, first0=0, nticks=30, flags=0):
        tr = _filled(api.ANIM_TRACK, (nj, 3))
        tr["first"] = (first0 + np.arange(nj * 3, dtype=np.uint64).reshape(nj, 3)).astype(u4)
        tr["count"] = 1
        return nticks, flags, tr, np.arange(nkeys, dtype=np.uint16) * 3, (np.arange(nkeys * 4) * 257 % 65536).astype(np.uint16).reshape(nkeys, 4)
    c["anim_track_arrays"] = [
        ("one clip", lambda: api.anim_track_arrays(2, [clip(2, 6)])),
        ("two clips, first rebased", lambda: api.anim_track_arrays(2, [clip(2, 6), clip(2, 9, nticks=12, flags=api.CLIP_LOOP)])),
        ("a first near 2^32 does not wrap", lambda: api.anim_track_arrays(1, [clip(1, 5), clip(1, 4, first0=0xFFFFFFFD)])),
        ("flat tracks, flat values, lists", lambda: api.anim_track_arrays(1, [(7, 1, clip(1, 3)[2].reshape(-1), [0, 3, 6], list(range(12)))])),
        ("non-contiguous tracks", lambda: api.anim_track_arrays(2, [(30, 0, _filled(api.ANIM_TRACK, (2, 6))[:, ::2], clip(2, 6)[3], clip(2, 6)[4])])),
        ("tracks of another joint count", lambda: api.anim_track_arrays(3, [clip(2, 6)])),
        ("values that do not match the times", lambda: api.anim_track_arrays(2, [clip(2, 6)[:4] + (np.zeros((5, 4), dtype=np.uint16),)])),
        ("no clips", lambda: api.anim_track_arrays(2, [])),
    ]
    return c


BUILDERS = ["anim_states", "anim_layers", "ik_targets", "attach_records", "root_steps", "play_cmds", "anim_track_arrays"]


def _describe(api, value) -> str:
    names = [k for k in dir(api) if isinstance(getattr(api, k), np.dtype)]
    parts = []
    for a in value if isinstance(value, tuple) else (value,):
        assert isinstance(a, np.ndarray), type(a)
        dt = next((k for k in names if getattr(api, k) == a.dtype), str(a.dtype))
        lay = "C" if a.flags.c_contiguous else "not contiguous"
        parts.append(f"{dt} {list(a.shape)} {lay} sha256 {hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()}")
    return " | ".join(parts)


def _lines(api, builder):
    out = []
    for name, thunk in _cases(api)[builder]:
        try:
            res = _describe(api, thunk())
        except api.MtrError as e:
            res = f"MtrError {e.code}: {e}"
        except Exception as e:  # what numpy itself refuses: the type is held, its wording is numpy's own
            res = f"raises {type(e).__name__}"
        out.append(f"{builder} / {name} -> {res}")
    return out


def _golden():
    with open(GOLDEN) as f:
        return [ln.rstrip("\n") for ln in f if ln.strip()]


@pytest.mark.parametrize("builder", BUILDERS)
def test_builder_answers_as_recorded(builder):
    from mt_renderer_amd import api
    want = [ln for ln in _golden() if ln.startswith(builder + " / ")]
    got = _lines(api, builder)
    assert len(want) == len(got) >= 8, "the corpus and the golden hold the same cases"
    for g, w in zip(got, want):
        assert g == w


def test_golden_holds_every_builder_and_every_kind_of_answer():
    from mt_renderer_amd import api
    lines = _golden()
    assert sorted(set(ln.split(" / ")[0] for ln in lines)) == sorted(BUILDERS) == sorted(_cases(api))
    assert sum("sha256" in ln for ln in lines) >= 40 and sum("MtrError 1: mtr error 1: " in ln for ln in lines) >= 30
    assert all("sha256" in ln or "MtrError" in ln or "raises " in ln for ln in lines)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python -m tests.test_api_records --record")
    sys.path.insert(0, ROOT)
    from mt_renderer_amd import api as _api
    with open(GOLDEN, "w") as f:
        for b in BUILDERS:
            f.write("\n".join(_lines(_api, b)) + "\n")
    print(f"recorded {len(_golden())} cases into {GOLDEN}")
