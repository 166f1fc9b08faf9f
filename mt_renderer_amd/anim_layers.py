"""Additive clips for animation layers (SPEC.md section 16): from a clip of uniformly spaced keys and a reference pose to
the clip of deltas an ``MTR_LAYER_ADDITIVE`` layer plays.  numpy on the host; an asset-build step, not a hot path.

An additive layer at effective weight ``e`` adds ``e`` times the clip's translation, multiplies the rotation on the
right by the clip's rotation (nlerp'ed from the identity by ``e``) and multiplies the scale by ``1 + e (s - 1)``.  So the
delta of a key from the reference pose is, per joint, ``T - T_ref``, ``conj(Q_ref) Q`` and ``S / S_ref``: at ``e = 1``
over the reference pose the layer reproduces the source clip to binary32 rounding.

``delta_clip`` returns keys in the layout of ``api.Anim`` ([nkeys, njoints, 12] float32: t.xyz 0 | q.xyzw | s.xyz 0), which
feed ``api.Anim`` directly or ``anim_tracks.compress`` for a track set."""
import numpy as np

F = np.float32


def _qmul(p, q):
    """the Hamilton product p q of quaternions (x, y, z, w) in the last axis, float64"""
    px, py, pz, pw = (p[..., i] for i in range(4))
    qx, qy, qz, qw = (q[..., i] for i in range(4))
    return np.stack([pw * qx + px * qw + py * qz - pz * qy,
                     pw * qy - px * qz + py * qw + pz * qx,
                     pw * qz + px * qy - py * qx + pz * qw,
                     pw * qw - px * qx - py * qy - pz * qz], axis=-1)


def _keys(a):
    a = np.asarray(a, dtype=np.float64)
    if a.shape[-1] != 12:
        raise ValueError("keys are [..., njoints, 12]: t.xyz 0 | q.xyzw | s.xyz 0")
    return a


def delta_clip(keys, ref):
    """keys [nkeys, njoints, 12], ref [njoints, 12] (a reference pose: one key) -> the delta keys [nkeys, njoints, 12]
    float32.  The reference rotations must not be zero and the reference scales must not have a zero component."""
    k, r = _keys(keys), _keys(ref)
    if k.ndim != 3 or r.shape != k.shape[1:]:
        raise ValueError("delta_clip: keys [nkeys, njoints, 12] and a reference pose [njoints, 12]")
    qr = r[:, 4:8]
    n2 = (qr * qr).sum(axis=-1, keepdims=True)
    if (n2 == 0).any() or (r[:, 8:11] == 0).any():
        raise ValueError("delta_clip: the reference pose has a zero rotation or scale")
    conj = qr * np.array([-1.0, -1.0, -1.0, 1.0]) / n2  # the inverse: the reference need not be normalised
    out = np.zeros(k.shape, dtype=np.float64)
    out[..., 0:3] = k[..., 0:3] - r[None, :, 0:3]
    dq = _qmul(np.broadcast_to(conj[None], k[..., 4:8].shape), k[..., 4:8])
    out[..., 4:8] = dq / np.linalg.norm(dq, axis=-1, keepdims=True)
    out[..., 8:11] = k[..., 8:11] / r[None, :, 8:11]
    return out.astype(F)


def apply(ref, delta):
    """the inverse of delta_clip in float64: ref [njoints, 12] with the deltas [nkeys, njoints, 12] applied in full
    (T_ref + dT, Q_ref dQ normalised, S_ref dS) -> [nkeys, njoints, 12] float64"""
    r, d = _keys(ref), _keys(delta)
    out = np.zeros(d.shape, dtype=np.float64)
    out[..., 0:3] = r[None, :, 0:3] + d[..., 0:3]
    q = _qmul(np.broadcast_to(r[None, :, 4:8], d[..., 4:8].shape), d[..., 4:8])
    out[..., 4:8] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    out[..., 8:11] = r[None, :, 8:11] * d[..., 8:11]
    return out
