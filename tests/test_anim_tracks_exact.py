"""CPU: csrc/anim_tracks.h, the source k_anim.hip's track source is made of (position -> r, the key search with (k, k1, a),
the two key decodes), compiled by g++ with -ffp-contract=off and compared bit for bit with the numpy model of SPEC.md
section 15 on the inputs the GPU tests use: the GPU bit-exactness test's rehearsal on a machine without a GPU."""
import subprocess

import numpy as np
import pytest

from tests import anim_tracks_model as tm
from tests import cpp_build


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = cpp_build.build("anim_tracks_exact", tmp_path_factory.mktemp("anim_tracks_exact"), cpp_build.EXACT)
    return out


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("kind", list(tm.JOINT_COUNTS))
def test_header_equals_the_model_bit_for_bit(exe, tmp_path, kind):
    J = tm.JOINT_COUNTS[kind]
    rng = np.random.default_rng(15)
    clips = tm.random_track_clips(rng, J)
    st = tm.track_states(rng, clips, J)
    nticks, flags, tracks, times, values = tm.concat(clips, J)
    n, C, nkeys = st.size, len(clips), times.size
    blob = tmp_path / "in.bin"
    with open(blob, "wb") as f:
        f.write(np.array([J, C, nkeys, n], dtype="<u4").tobytes())
        f.write(np.stack([nticks, flags], axis=1).astype("<u4").tobytes())
        f.write(tracks.tobytes())
        f.write(values.astype("<u2").tobytes())
        f.write(times.astype("<u2").tobytes() + (b"\0\0" if nkeys % 2 else b""))
        f.write(st.tobytes())
    res = tmp_path / "out.bin"
    subprocess.check_call([exe, str(blob), str(res)], timeout=120)
    raw = np.fromfile(res, dtype="<u4")
    got = raw[:n * 2 * J * 3 * 12].reshape(n, 2, J, 3, 12)
    for slot, (cf, xf) in enumerate((("clip_a", "x_a"), ("clip_b", "x_b"))):
        r, k0, k1, a, d0, d1 = tm.located(clips, st[cf], st[xf], J)
        g = got[:, slot]
        assert (g[..., 0] == _bits(r)[:, None, None]).all(), f"{kind} slot {slot}: r"
        assert (g[..., 1] == k0).all(), f"{kind} slot {slot}: k differs in {int((g[..., 1] != k0).sum())} tracks"
        assert (g[..., 2] == k1).all(), f"{kind} slot {slot}: k1"
        assert (g[..., 3] == _bits(a)).all(), f"{kind} slot {slot}: a differs in {int((g[..., 3] != _bits(a)).sum())} tracks"
        assert (g[..., 4:8] == _bits(d0)).all(), f"{kind} slot {slot}: the decoded key k"
        assert (g[..., 8:12] == _bits(d1)).all(), f"{kind} slot {slot}: the decoded key k1"
    # the Snorm16 of every code: the header's division sequence is the IEEE division of the section
    codes = np.arange(65536, dtype=np.uint16).view(np.int16).astype(np.float32)
    want = np.maximum(codes / np.float32(32767), np.float32(-1))
    assert (raw[n * 2 * J * 3 * 12:] == _bits(want)).all()
    # the searches went deep: the 65536-key track was located at keys far apart
    deep, _ = tm.special_tracks(J)
    ks = np.unique(got[st["clip_a"] == tm.HUGE][:, 0, deep[0], deep[1], 1])
    assert ks.size >= 10, ks
