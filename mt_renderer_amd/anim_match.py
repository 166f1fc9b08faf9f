"""Helpers that build the database of a match set (SPEC.md section 25) from clips.  Not part of the rule: the rule is what the
rows and features say.

    rows = rows_of(nkeys, clip_flags, stride=2, tail=4)                   # which keys of which clips are rows
    raw = np.concatenate([pose_part, trajectory_part], axis=1)             # one line of raw features per row
    feats, mean, scale = normalise(raw, weights)                           # what AnimMatch takes
    match = api.AnimMatch(dev, nkeys, clip_flags, rows, feats, pose_dims=0xF, mean=mean, scale=scale, ...)

The query of a search is raw: the set normalises it with the same mean and scale, in the same two binary32 operations
(a difference, then a product) that `normalise` uses, so a query equal to a row's raw features has distance zero to it."""
import numpy as np

from . import api

F = np.float32


def _bad(msg):
    return api.MtrError(api.MTR_E_INVALID, "anim match build: " + msg)


def normalise(raw, weights=None):
    """raw features [R, D] -> (features float32 [R, D], mean float32 [D], scale float32 [D]): per dimension the mean is taken
    off and the rest multiplied by weight / standard deviation (a constant dimension keeps scale = weight)"""
    raw = np.asarray(raw, dtype=np.float64)
    if raw.ndim != 2 or raw.shape[0] == 0 or not np.isfinite(raw).all():
        raise _bad("raw features are a finite array [R, D]")
    D = raw.shape[1]
    w = np.ones(D) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.size != D or not np.isfinite(w).all():
        raise _bad("one finite weight per dimension")
    std = raw.std(axis=0)
    mean, scale = raw.mean(axis=0).astype(F), (w / np.where(std > 0, std, 1.0)).astype(F)
    feats = ((raw.astype(F) - mean[None, :]).astype(F) * scale[None, :]).astype(F)
    return feats, mean, scale


def rows_of(nkeys, flags=None, stride=1, tail=0):
    """the row table: every ``stride``-th key of every clip as a MATCH_ROW (x = the key's index, bias 0, tags 0), sorted by clip;
    the last ``tail`` keys of a one-shot clip are left out (a jump there would have nothing left to play)"""
    nkeys = np.asarray(nkeys, dtype=np.int64).reshape(-1)
    fl = np.zeros(nkeys.size, dtype=np.int64) if flags is None else np.asarray(flags, dtype=np.int64).reshape(-1)
    if fl.size != nkeys.size or stride < 1 or tail < 0:
        raise _bad("one flag word per clip, stride >= 1, tail >= 0")
    out = []
    for c, (n, f) in enumerate(zip(nkeys, fl)):
        last = n - 1 if f & api.CLIP_LOOP else n - 1 - tail
        out += [(c, float(k), 0.0, 0) for k in range(0, last + 1, stride)]
    if not out:
        raise _bad("no rows")
    return np.array(out, dtype=api.MATCH_ROW)


def _planar(keys):
    """root keys [N, 12] (translation, pad, quaternion xyzw, ...) -> x, z and the yaw about y"""
    keys = np.asarray(keys, dtype=np.float64)
    if keys.ndim == 3:
        keys = keys[:, 0, :]
    if keys.ndim != 2 or keys.shape[1] != 12:
        raise _bad("trajectory keys are [N, 12] or [N, J, 12] ANIM_KEY floats")
    return keys[:, 0], keys[:, 2], 2.0 * np.arctan2(keys[:, 5], keys[:, 7])


def trajectory_features(traj_keys, offsets, cyclic=True):
    """future root positions and facings at key offsets, in the space of the current root: float64 [N, 4 * len(offsets)] with
    (dx, dz, sin(dyaw), cos(dyaw)) per offset for every key k of one clip's root trajectory.  cyclic: the last key is where the
    next cycle's key 0 stands, and offsets run on into the next cycles; otherwise they stop at the last key."""
    x, z, yaw = _planar(traj_keys)
    N = x.size
    out = np.zeros((N, 4 * len(offsets)))
    span = N - 1

    def pose(k):
        if not cyclic or span == 0:
            k = min(k, N - 1)
            return x[k], z[k], yaw[k]
        m, r = divmod(k, span)
        px, pz, pa = x[r] - x[0], z[r] - z[0], yaw[r] - yaw[0]  # within the cycle, from key 0
        cx, cz, ca = x[span] - x[0], z[span] - z[0], yaw[span] - yaw[0]  # one whole cycle
        ox, oz, oa = x[0], z[0], yaw[0]
        for _ in range(m):  # the cycles before it, each turned by what came before
            ox, oz, oa = ox + np.cos(oa - yaw[0]) * cx + np.sin(oa - yaw[0]) * cz, oz - np.sin(oa - yaw[0]) * cx + np.cos(oa - yaw[0]) * cz, oa + ca
        t = oa - yaw[0]
        return ox + np.cos(t) * px + np.sin(t) * pz, oz - np.sin(t) * px + np.cos(t) * pz, oa + pa

    for k in range(N):
        x0, z0, a0 = pose(k)
        for j, o in enumerate(offsets):
            x1, z1, a1 = pose(k + int(o))
            dx, dz = x1 - x0, z1 - z0
            out[k, 4 * j:4 * j + 4] = (np.cos(a0) * dx - np.sin(a0) * dz, np.sin(a0) * dx + np.cos(a0) * dz, np.sin(a1 - a0), np.cos(a1 - a0))
    return out
