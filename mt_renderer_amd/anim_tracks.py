"""Reference encoder for animation tracks (SPEC.md section 15): from a clip of uniformly spaced keys, as
``mtr_anim_create`` takes it, to a track clip for ``api.AnimTracks`` at the same positions.  numpy on the host; an
asset-build step, not a hot path.

Every joint's translation, rotation and scale become one track each.  Values are quantised to 16 bits (translation and
scale: ``lo`` = the component's minimum, ``step = (max - min) / 65535``, ``step = 0`` and word 0 for a constant component;
rotation: ``rint(q * 32767)``).  Keys are then dropped greedily: a segment is extended while every source key it skips is
reproduced within the tolerance by section 15's rule on the segment's quantised end keys.  Kept keys carry the
quantisation error alone (at most ``step / 2`` per component; about 2e-5 for a rotation component).  In a LOOP clip the
last segment runs to the first key at tick N; in any other clip the last kept key is held.

The search is the plain one: a segment of m keys costs O(m^2) key evaluations, so a clip of tens of thousands of keys
that compresses well takes minutes.  Tracks that are constant after quantisation are recognised at once."""
import numpy as np

F = np.float32
CLIP_LOOP = 1
ANIM_TRACK = np.dtype([("first", "<u4"), ("count", "<u4"), ("lo", "<f4", 3), ("step", "<f4", 3)])
MAX_KEYS = 65536


def _lerp(v0, v1, a):
    return v0 + a * (v1 - v0)


def _dot(p, q):
    return ((p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1]) + p[..., 2] * q[..., 2]) + p[..., 3] * q[..., 3]


def _nlerp(q0, q1, a):
    """section 14's nlerp in binary32: q0, q1 [..., 4], a [...]"""
    with np.errstate(all="ignore"):
        q1 = np.where((_dot(q0, q1) < 0)[..., None], -q1, q1)
        q = _lerp(q0, q1, a[..., None])
        n2 = _dot(q, q)
        rn = F(1) / np.sqrt(n2)
        out = q * rn[..., None]
    bad = (n2 == 0) | ~np.isfinite(rn)
    return np.where(bad[..., None], np.array([0, 0, 0, 1], dtype=F), out).astype(F)


def quantise_lin(v):
    """v [n, 3] float32 -> lo [3], step [3] (float32), words [n, 4] u16 (the fourth is 0), and the decoded values [n, 3]"""
    v = np.asarray(v, dtype=F)
    lo = v.min(axis=0)
    step = ((v.max(axis=0) - lo) / F(65535)).astype(F)
    words = np.zeros((v.shape[0], 4), dtype=np.uint16)
    with np.errstate(all="ignore"):
        q = np.where(step > 0, np.rint((v - lo) / np.where(step > 0, step, F(1))), 0)
    words[:, :3] = np.clip(np.nan_to_num(q), 0, 65535).astype(np.uint16)
    return lo, step, words, (lo + words[:, :3].astype(F) * step).astype(F)


def quantise_rot(q):
    """q [n, 4] float32 -> words [n, 4] (s16 stored as u16) and the decoded values [n, 4]"""
    w = np.clip(np.rint(np.asarray(q, dtype=np.float64) * 32767), -32767, 32767).astype(np.int16)
    return w.view(np.uint16), np.maximum(w.astype(F) / F(32767), F(-1)).astype(F)


def _reduce(n, loop, fits):
    """the kept keys of one track: fits(s, e) says whether every source key strictly between s and e is reproduced by
    the segment from key s to key e; e == n stands for what follows the last kept key (the wrap, or the hold)"""
    kept, s = [0], 0
    while s + 1 < n:
        e = s + 1
        while e < n and fits(s, e + 1):
            e += 1
        if e == n:
            break
        kept.append(e)
        s = e
    return kept


def _track(src, dec, loop, tol, rot):
    """kept key indices of one track; src: the source keys [n, 3 or 4], dec: their quantised, decoded values"""
    n = src.shape[0]

    def fits(s, e):
        i = np.arange(s + 1, min(e, n))
        if i.size == 0:
            return True
        if e == n and not loop:
            got = np.broadcast_to(dec[s], (i.size, dec.shape[1]))  # the last key is held: a = 0
            a = np.zeros(i.size, dtype=F)
        else:
            a = (i.astype(F) - F(s)) / F(e - s)
            got = None
        end = dec[0] if e == n else dec[e]
        if rot:
            got = _nlerp(np.broadcast_to(dec[s], (i.size, 4)), np.broadcast_to(end, (i.size, 4)), a)
            want = src[i]
            want = np.where((_dot(want, got) < 0)[:, None], -want, want)
        else:
            if got is None:
                got = _lerp(dec[s][None, :], end[None, :], a[:, None])
            want = src[i]
        return bool((np.abs(got.astype(np.float64) - want.astype(np.float64)) <= tol).all())

    return _reduce(n, loop, fits)


def compress(keys, flags=0, tol_t=1e-3, tol_q=1e-3, tol_s=1e-3):
    """One clip of uniformly spaced keys [nkeys, njoints, 12] float32 (t.xyz 0 | q.xyzw | s.xyz 0) -> the track clip
    (nticks, flags, tracks, times, values) of nkeys ticks that ``api.AnimTracks`` takes: tracks an ANIM_TRACK array
    [njoints, 3] with ``first`` counted inside this clip's times (u16) and values (u16 [n, 4])."""
    keys = np.asarray(keys, dtype=F)
    if keys.ndim != 3 or keys.shape[2] != 12 or keys.shape[0] < 1:
        raise ValueError("compress: keys are [nkeys, njoints, 12] float32")
    n, J = keys.shape[0], keys.shape[1]
    if n > MAX_KEYS:
        raise ValueError(f"compress: a track clip has at most {MAX_KEYS} ticks, the clip has {n} keys")
    loop = bool(int(flags) & CLIP_LOOP)
    tracks = np.zeros((J, 3), dtype=ANIM_TRACK)
    times, values, base = [], [], 0
    for j in range(J):
        for ch, (sl, tol) in enumerate(((slice(0, 3), tol_t), (slice(4, 8), tol_q), (slice(8, 11), tol_s))):
            src = keys[:, j, sl]
            if ch == 1:
                words, dec = quantise_rot(src)
            else:
                lo, step, words, dec = quantise_lin(src)
                tracks[j, ch]["lo"], tracks[j, ch]["step"] = lo, step
            kept = [0] if (words == words[0]).all() else _track(src, dec, loop, tol, ch == 1)
            tracks[j, ch]["first"], tracks[j, ch]["count"] = base, len(kept)
            base += len(kept)
            times.append(np.asarray(kept, dtype=np.uint16))
            values.append(words[kept])
    return n, int(flags), tracks, np.concatenate(times), np.concatenate(values)


def encoded_bytes(clip):
    """device bytes of a track clip: 32 per descriptor, 2 + 8 per key"""
    _, _, tracks, times, _ = clip
    return int(tracks.size) * 32 + int(times.size) * 10


def uniform_bytes(nkeys, njoints):
    return int(nkeys) * int(njoints) * 48
