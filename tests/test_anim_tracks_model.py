"""CPU: the numpy model of SPEC.md section 15 (tests/anim_tracks_model.py), which the GPU tests pin the kernel to, gives the
answers the section's rules imply and stays within the section's bound of its own float64 version; the inputs shared with
the GPU tests would tell the wrong readings of the section apart; and the reference encoder
(mt_renderer_amd/anim_tracks.py) reproduces its source within the tolerances, on the models alone."""
import numpy as np
import pytest

from mt_renderer_amd import anim_tracks
from tests import anim_model as am
from tests import anim_tracks_model as tm

F = np.float32


def _states(**cols):
    n = max(np.atleast_1d(v).size for v in cols.values())
    st = np.zeros(n, dtype=tm.STATE)
    for k, v in cols.items():
        st[k] = v
    return st


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _clip(nticks, flags, per_channel):
    """one joint: per channel (times, words [n, 4], lo, step)"""
    tr = np.zeros((1, 3), dtype=tm.TRACK)
    times, values, base = [], [], 0
    for ch, (t, w, lo, step) in enumerate(per_channel):
        tr[0, ch] = (base, len(t), lo, step)
        base += len(t)
        times.append(np.asarray(t, dtype=np.uint16))
        values.append(np.asarray(w, dtype=np.uint16).reshape(-1, 4))
    return nticks, flags, tr, np.concatenate(times), np.concatenate(values)


def _q(*q):
    return np.rint(np.array(q) * 32767).astype(np.int16).view(np.uint16)


def _simple(nticks=100, flags=0, t_times=(0, 10, 40), q_times=(0, 50)):
    T = (t_times, [[100 * i, 200 * i, 300 * i, 9999] for i in range(len(t_times))], (1.0, 2.0, 3.0), (0.01, 0.02, 0.03))
    Q = (q_times, [_q(0.3, -0.2, 0.5, 0.7), _q(0.0, 0.6, 0.0, 0.8)][:len(q_times)], (0, 0, 0), (0, 0, 0))
    S = ((0,), [[0, 65535, 30000, 1]], (1.0, 0.5, 0.75), (0.0, 1.0 / 65535, 0.0))
    return _clip(nticks, flags, (T, Q, S))


def _matrix(t, q, s):
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    M = np.eye(4)
    M[:3, :3] = R * np.asarray(s)[None, :]
    M[:3, 3] = t
    return M.T.reshape(16)


# ---- known answers -------------------------------------------------------------------------------------------------
def test_on_a_key_time_a_is_zero_and_the_value_is_the_key():
    clip = _simple()
    r, k0, k1, a, d0, d1 = tm.located([clip], [0, 0, 0], [10.0, 40.0, 50.0], 1)
    assert list(k0[:, 0, 0]) == [1, 2, 2] and list(a[:, 0, 0]) == [0, 0, 0]
    assert list(k0[:, 0, 1]) == [3, 3, 4] and a[2, 0, 1] == 0 and a[0, 0, 1] == F(10) / F(50)
    got = tm.sample([clip], _states(clip_a=0, x_a=10.0), 1)[0, 0]
    q = np.array([0.3, -0.2, 0.5, 0.7])
    qa = np.maximum(np.rint(q * 32767).astype(F) / F(32767), F(-1)).astype(np.float64)
    qb = np.array([0.0, np.rint(0.6 * 32767) / 32767, 0.0, np.rint(0.8 * 32767) / 32767])
    qm = qa + 0.2 * (qb - qa)
    want = _matrix((2.0, 6.0, 12.0), qm / np.linalg.norm(qm), (1.0, 1.5, 0.75))
    assert got[12] == F(1.0) + F(100) * F(0.01) and got[13] == F(2.0) + F(200) * F(0.02) and got[14] == F(3.0) + F(300) * F(0.03)
    assert np.abs(got - want).max() < 2e-6
    # at the rotation's own key the quaternion is that key, renormalised
    got = tm.sample([clip], _states(clip_a=0, x_a=50.0), 1)[0, 0]
    want = _matrix((3.0, 10.0, 21.0), qb / np.linalg.norm(qb), (1.0, 1.5, 0.75))  # the translation holds its last key (clamp)
    assert np.abs(got - want).max() < 2e-6
    assert abs(np.linalg.norm(got[0:3].astype(np.float64)) - 1.0) < 1e-6
    # the binary32 neighbours of a key time fall into the two intervals around it
    _, k0, _, a, _, _ = tm.located([clip], [0, 0], [np.nextafter(F(40), F(0)), np.nextafter(F(40), F(100))], 1)
    assert list(k0[:, 0, 0]) == [1, 2] and a[0, 0, 0] < 1 and a[0, 0, 0] > F(0.9999) and a[1, 0, 0] == 0  # past the last key of a clamp clip


def test_a_one_key_track_is_constant_for_every_x():
    clip = _simple(t_times=(0,), q_times=(0,))
    for fl in (0, tm.CLIP_LOOP):
        c = (clip[0], fl) + clip[2:]
        xs = np.array([0.0, -0.0, -3.5, 0.75, 1e9, -1e9, np.nan, np.inf, -np.inf, 99.0, 99.99, 100.0], dtype=F)
        out = tm.sample([c], _states(clip_a=0, x_a=xs), 1)
        assert (_bits(out) == _bits(out[:1])).all()
        assert np.isfinite(out).all()


@pytest.mark.parametrize("N", [100, 65536])
def test_loop_interpolates_last_to_first_over_the_ticks_up_to_N(N):
    clip = _simple(nticks=N, flags=tm.CLIP_LOOP)
    x = F(40 + (N - 40) * 0.25)
    r, k0, k1, a, d0, d1 = tm.located([clip], [0], [x], 1)
    assert k0[0, 0, 0] == 2 and k1[0, 0, 0] == 0, "the last key interpolates towards the track's first key"
    assert a[0, 0, 0] == (x - F(40)) / F(N - 40) == F(0.25)
    assert k0[0, 0, 1] == 4 and k1[0, 0, 1] == 3 and a[0, 0, 1] == (x - F(50)) / F(N - 50)
    # the same value as a two-key clamp track (last, first) at the same fraction
    got = tm.sample([clip], _states(clip_a=0, x_a=x), 1)[0, 0]
    assert got[12] == F(3.0) + F(0.25) * (F(1.0) - F(3.0))
    # one lap later the position is the same tick
    again = tm.sample([clip], _states(clip_a=0, x_a=[x, x + F(N)]), 1)
    assert (_bits(again[0]) == _bits(again[1])).all()
    # the clamp clip holds the last key instead
    hold = _simple(nticks=N, flags=0)
    _, k0, k1, a, _, _ = tm.located([hold], [0, 0], [x, 1e9], 1)
    assert (k0[:, 0, 0] == 2).all() and (k1[:, 0, 0] == 2).all() and (a[:, 0, 0] == 0).all()
    out = tm.sample([hold], _states(clip_a=0, x_a=[45.0, float(N - 1), 1e9, np.inf]), 1)
    assert (out[:, 0, 12:15] == out[0, 0, 12:15]).all()


def test_the_difference_in_a_never_rounds():
    rng = np.random.default_rng(1)
    clips = tm.random_track_clips(rng, 4)
    arrays = tm.concat(clips, 4)
    times = arrays[3]
    for ci in (tm.LONG, tm.HUGE):
        N = clips[ci][0]
        x = rng.uniform(0, N, 1000).astype(F)
        _, r, K0, _, _, _ = tm._locate_states(arrays, np.full(1000, ci), x, 4)
        tk = times[K0].astype(np.int64)
        num32 = (r[:, None, None] - tk.astype(F))
        assert (num32.astype(np.float64) == r.astype(np.float64)[:, None, None] - tk).all()
        assert (tk <= r[:, None, None]).all()


def test_cross_fade_clip_index_clamp_and_w_zero():
    rng = np.random.default_rng(3)
    clips = tm.random_track_clips(rng, 3)
    a = tm.sample(clips, _states(clip_a=0, x_a=17.25, clip_b=0xFFFFFFFF, x_b=np.nan, w=0.0), 3)
    b = tm.sample(clips, _states(clip_a=0, x_a=17.25, clip_b=1, x_b=3.0, w=[-0.5, np.nan, -0.0]), 3)
    assert np.isfinite(a).all() and (_bits(b) == _bits(a)).all()
    c = tm.sample(clips, _states(clip_a=[3, 4, 0xFFFFFFFF], x_a=5.0), 3)
    assert (_bits(c) == _bits(c[:1])).all()
    one = tm.sample(clips, _states(clip_a=0, x_a=17.25, clip_b=1, x_b=3.0, w=[1.0, 7.0]), 3)
    only_b = tm.sample(clips, _states(clip_a=1, x_a=3.0), 3)
    assert (_bits(one[0]) == _bits(one[1])).all() and np.abs(one[0] - only_b[0]).max() < 1e-4


def test_a_track_clip_of_all_ticks_equals_the_uniform_clip_of_its_decoded_keys():
    """positions mean the same in both kinds: a track set with a key on every tick is section 14 on the decoded keys"""
    rng = np.random.default_rng(8)
    J, N = 3, 31
    for fl in (0, tm.CLIP_LOOP):
        tr = np.zeros((J, 3), dtype=tm.TRACK)
        times, values = [], []
        keys = np.zeros((N, J, 12), dtype=F)
        for j in range(J):
            for ch in range(3):
                w = rng.integers(0, 65536, (N, 4)).astype(np.uint16)
                lo, step = rng.uniform(-1, 1, 3).astype(F), rng.uniform(0, 1e-4, 3).astype(F)
                tr[j, ch] = ((j * 3 + ch) * N, N, lo, step)
                times.append(np.arange(N))
                values.append(w)
                if ch == 1:
                    keys[:, j, 4:8] = tm.decode_rot(w)
                else:
                    keys[:, j, ch * 4:ch * 4 + 3] = tm.decode_lin(w, lo[None, :], step[None, :])
        clip = (N, fl, tr, np.concatenate(times).astype(np.uint16), np.concatenate(values))
        st = _states(clip_a=0, x_a=rng.uniform(-40, 80, 200).astype(F), clip_b=0, x_b=rng.uniform(-40, 80, 200).astype(F),
                     w=np.where(rng.random(200) < 0.5, 0, rng.uniform(0, 1, 200)))
        assert (_bits(tm.sample([clip], st, J)) == _bits(am.sample([(keys, fl)], st, J))).all()


# ---- the shared inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(tm.JOINT_COUNTS))
def test_inputs_show_the_wrong_readings_and_the_model_holds_its_bound(kind):
    J = tm.JOINT_COUNTS[kind]
    rng = np.random.default_rng(15)
    clips = tm.random_track_clips(rng, J)
    st = tm.track_states(rng, clips, J)
    assert tm.validate(clips, J) is None
    # the special tracks of the 65536-tick clip
    deep, wide = tm.special_tracks(J)
    tr = clips[tm.HUGE][2]
    assert clips[tm.HUGE][0] == 65536 and tr[deep]["count"] == 65536 and tr[wide]["count"] == 2
    assert set(int(c) for c in np.concatenate([c[2]["count"].reshape(-1) for c in clips[:2]])) <= set(tm.KEY_COUNTS)
    assert (st["clip_a"] > 3).any() and (st["clip_b"] > 3).any(), "clip indices beyond C - 1"
    ref = tm.sample(clips, st, J)
    assert np.isfinite(ref).all()
    for v in tm.WRONG_VARIANTS:
        inst = float((_bits(tm.sample(clips, st, J, variant=v)) != _bits(ref)).any(axis=(1, 2)).mean())
        print(f"{kind}: {v} differs in {inst:.3f} of the instances")
        assert inst >= 0.10, f"{v} must be visible"
    fused = float((_bits(tm.sample(clips, st, J, lerp=am.lerp_fused)) != _bits(ref)).any(axis=(1, 2)).mean())
    assert fused >= 0.10, "a contracted lerp must be visible"
    # the model against its float64 self
    trc = am.Trace()
    val, mag = tm.sample_exact(clips, st, J, trace=trc)
    keep = ~trc.near
    assert (~keep).sum() < 0.01 * keep.size and (np.abs(trc.all_d()) < 8 * tm.U).mean() < 0.01
    frac = np.abs(ref.astype(np.float64) - val)[keep] / (tm.K_LOCALS * tm.U * mag[keep] + 1e-300)
    print(f"{kind}: largest fraction of the bound {frac.max():.4f}, left out {int((~keep).sum())}, min |d| {np.abs(trc.all_d()).min():.3e}")
    assert frac.max() <= 1.0


def test_validator_names_every_violation():
    valid = tm.random_track_clips(np.random.default_rng(4), 40)
    assert tm.validate(valid, 40) is None
    seen = set()
    for what, bad, c, j, ch in tm.invalid_sets(valid, 40):
        got = tm.validate(bad, 40)
        assert got is not None and got[:3] == (c, j, ch), (what, got)
        seen.add(got[3])
    assert seen == {"ticks", "count", "range", "first time", "increase", "last time"}


# ---- the reference encoder, on the models alone ---------------------------------------------------------------------
TOL_T, TOL_Q, TOL_S = 2e-3, 1e-3, 1e-3


def _smooth_clip(rng, N, J, loop):
    """a few harmonics per component (periodic over the clip when it loops), some channels constant"""
    t = np.arange(N) / N
    k = np.zeros((N, J, 12), dtype=F)
    for j in range(J):
        ph = rng.uniform(0, 2 * np.pi, (11, 2))
        amp = rng.uniform(0.2, 1.0, (11, 2))
        wave = lambda i: amp[i, 0] * np.sin(2 * np.pi * t + ph[i, 0]) + 0.3 * amp[i, 1] * np.sin(4 * np.pi * t + ph[i, 1])
        if not loop:
            wave = lambda i: amp[i, 0] * np.sin(2.3 * t + ph[i, 0]) + 0.3 * amp[i, 1] * np.sin(5.1 * t + ph[i, 1])
        k[:, j, 0:3] = np.stack([2.0 * wave(i) for i in range(3)], axis=1) if j % 3 else 0.5
        q = np.array([0.2, -0.4, 0.1, 0.85])[None, :] + 0.25 * np.stack([wave(3 + i) for i in range(4)], axis=1)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        k[:, j, 4:8] = q * (-1.0 if j % 4 == 1 else 1.0)
        k[:, j, 8:11] = 1.0 + (0.1 * np.stack([wave(7 + i) for i in range(3)], axis=1) if j % 2 else 0.0)
    return k


@pytest.fixture(scope="module")
def smooth():
    rng = np.random.default_rng(21)
    J = 6
    src = [(_smooth_clip(rng, 120, J, True), tm.CLIP_LOOP), (_smooth_clip(rng, 120, J, False), 0)]
    enc = [anim_tracks.compress(k, fl, TOL_T, TOL_Q, TOL_S) for k, fl in src]
    assert tm.validate(enc, J) is None
    return J, src, enc


def _channels(tclips, clip, x, J):
    """(T, Q, S) of one clip at positions x by the section's rule: [n, J, 3], [n, J, 4], [n, J, 3] float32"""
    r, K0, K1, A, d0, d1 = tm.located(tclips, np.full(len(x), clip), x, J)
    T = am.lerp_rule(d0[:, :, 0, :3], d1[:, :, 0, :3], A[:, :, 0, None])
    S = am.lerp_rule(d0[:, :, 2, :3], d1[:, :, 2, :3], A[:, :, 2, None])
    Q = np.stack(am.nlerp(tuple(d0[:, :, 1, i] for i in range(4)), tuple(d1[:, :, 1, i] for i in range(4)), A[:, :, 1], am.lerp_rule, True, None, None), axis=-1)
    return T, Q, S


def _aligned(q, ref):
    return np.where((np.sum(q * ref, axis=-1) < 0)[..., None], -q, q)


def test_encoder_reproduces_every_source_key_within_the_tolerances(smooth):
    J, src, enc = smooth
    total_u = total_e = 0
    for ci, (k, fl) in enumerate(src):
        N = k.shape[0]
        T, Q, S = _channels(enc, ci, np.arange(N, dtype=F), J)
        assert np.abs(T.astype(np.float64) - k[:, :, 0:3]).max() <= TOL_T
        assert np.abs(S.astype(np.float64) - k[:, :, 8:11]).max() <= TOL_S
        assert np.abs(_aligned(Q, k[:, :, 4:8]).astype(np.float64) - k[:, :, 4:8]).max() <= TOL_Q
        total_u += anim_tracks.uniform_bytes(N, J)
        total_e += anim_tracks.encoded_bytes(enc[ci])
        assert enc[ci][3].size < 3 * J * N / 2, "smooth clips lose keys"
    print(f"smooth clips: {total_e} bytes of tracks for {total_u} bytes of uniform keys, ratio {total_u / total_e:.2f}")


def test_encoder_holds_translation_and_scale_between_the_ticks_too(smooth):
    """At a fractional position the uniform clip interpolates its two neighbouring source keys and the track clip its two
    kept keys: both are linear inside a source interval, so their difference peaks at the interval's ends, where it is at
    most tol.  The slack beyond tol: the kept keys' quantisation, step / 2 per component, and the roundings -- section 14's
    lerp (3) on the uniform side, section 15's decode (2), a (1) and lerp (3) on the track side: 9 u of the largest
    magnitude involved, the sum of |terms| being at most 3 times the largest component."""
    J, src, enc = smooth
    rng = np.random.default_rng(22)
    for ci, (k, fl) in enumerate(src):
        N = k.shape[0]
        x = rng.uniform(0, N if fl else N - 1, 1000).astype(F)
        T, _, S = _channels(enc, ci, x, J)
        i0, i1, a = am.position(x, np.full(1000, N), np.full(1000, bool(fl)))
        for got, sl, tol, ch in ((T, slice(0, 3), TOL_T, 0), (S, slice(8, 11), TOL_S, 2)):
            want = am.lerp_rule(k[i0][:, :, sl], k[i1][:, :, sl], a[:, None, None])
            step = enc[ci][2]["step"][:, ch, :].astype(np.float64)  # [J, 3]
            big = np.abs(k[:, :, sl]).max(axis=0).astype(np.float64)
            slack = step / 2 + 9 * tm.U * 3 * big
            assert (np.abs(got.astype(np.float64) - want) <= tol + slack[None, :, :]).all()


def test_encoder_sizes():
    rng = np.random.default_rng(5)
    J, N = 5, 64
    const = np.zeros((N, J, 12), dtype=F)
    const[:, :, 0:3] = rng.uniform(-1, 1, (1, J, 3))
    const[:, :, 4:8] = [0.0, 0.6, 0.0, 0.8]
    const[:, :, 8:11] = 1.0
    for fl in (0, tm.CLIP_LOOP):
        c = anim_tracks.compress(const, fl, 0.0, 0.0, 0.0)
        assert c[0] == N and c[3].size == 3 * J and (c[2]["count"] == 1).all(), "a constant clip is one key per track"
        T, _, _ = _channels([c], 0, np.array([0.0, 17.5], dtype=F), J)
        assert (T[0] == const[0, :, 0:3]).all(), "a constant component is stored exactly (step 0, word 0)"
    noise = am.random_clips(rng, J, shape=[(N, tm.CLIP_LOOP)])[0][0]
    c = anim_tracks.compress(noise, tm.CLIP_LOOP, 0.0, 0.0, 0.0)
    assert (c[2]["count"] == N).all() and c[3].size == 3 * J * N
    per_joint_tick = (anim_tracks.encoded_bytes(c) - 32 * 3 * J) / (J * N)
    assert per_joint_tick == 3 * (2 + 8) == 30, "30 bytes per joint and tick against 48"
    with pytest.raises(ValueError):
        anim_tracks.compress(np.zeros((65537, 1, 12), dtype=F))
    one = anim_tracks.compress(noise[:1], 0)
    assert one[0] == 1 and one[3].size == 3 * J
