"""Host helper for root motion (SPEC.md section 19): splits a clip that carries its root's movement into the in-place clip
the pose calls play and the one-joint trajectory ``Batch.root_motion`` plays.  numpy on the host; an asset-build step, not a
hot path, and not part of the rule: the rule takes whatever trajectory keys the set holds.

Per key the root joint's local transform ``L = (T, Q, S)`` is split into a rigid part ``R = (T_r, Q_r)`` -- the selected
components of the translation, and the twist of the rotation about ``up`` -- and the rest ``R^-1 o L``, which stays on the
root joint of the in-place clip, so that ``R(k) o in-place(k) = L(k)`` at every key."""
import numpy as np

F = np.float32


def _qmul(p, q):
    px, py, pz, pw = (p[..., i] for i in range(4))
    qx, qy, qz, qw = (q[..., i] for i in range(4))
    return np.stack([pw * qx + px * qw + py * qz - pz * qy,
                     pw * qy - px * qz + py * qw + pz * qx,
                     pw * qz + px * qy - py * qx + pz * qw,
                     pw * qw - px * qx - py * qy - pz * qz], axis=-1)


def _qrot(q, v):
    a = q[..., :3]
    t = 2.0 * np.cross(a, v)
    return v + q[..., 3:4] * t + np.cross(a, t)


def _norm4(q):
    n = np.linalg.norm(q, axis=-1, keepdims=True)
    ident = np.zeros_like(q)
    ident[..., 3] = 1.0
    with np.errstate(all="ignore"):
        return np.where((n == 0) | ~np.isfinite(1.0 / n), ident, q / n)


def split_root(keys, joint, translate=(1, 0, 1), up=(0, 1, 0), rotate="twist", loop=False):
    """keys [nkeys, njoints, 12] (t.xyz 0 | q.xyzw | s.xyz 0) -> (in-place keys [nkeys, njoints, 12], trajectory keys
    [nkeys, 1, 12]), float32, formed in float64 and rounded once.

    joint: the root joint that carries the movement.  translate: which translation components go to the trajectory (the
    ground plane by default; the height stays in the pose).  rotate: "twist" sends the rotation about ``up`` to the
    trajectory -- ``norm4((q . up) up, q.w)``, no trigonometry -- "all" the whole rotation, "none" none of it.
    loop: the source loops and holds the duplicated end key (its last key is the first one a cycle later): the in-place
    clip drops that key and is played with ``CLIP_LOOP``; the trajectory keeps it and is marked ``ROOT_CYCLIC``, so a
    position means the same in both."""
    k = np.asarray(keys, dtype=np.float64)
    if k.ndim != 3 or k.shape[-1] != 12 or not 0 <= joint < k.shape[1]:
        raise ValueError("split_root: keys [nkeys, njoints, 12] and a joint of theirs")
    if rotate not in ("twist", "none", "all"):
        raise ValueError('split_root: rotate is "twist", "none" or "all"')
    if loop and k.shape[0] < 2:
        raise ValueError("split_root: a looping source holds at least its first key and the duplicated end key")
    sel = np.asarray(translate, dtype=np.float64).reshape(3) != 0
    u = np.asarray(up, dtype=np.float64).reshape(3)
    if not np.linalg.norm(u) > 0:
        raise ValueError("split_root: up is not a direction")
    u = u / np.linalg.norm(u)
    T, Q = k[:, joint, 0:3], _norm4(k[:, joint, 4:8])
    Tr = np.where(sel[None, :], T, 0.0)
    if rotate == "twist":
        Qr = _norm4(np.concatenate([(Q[:, :3] @ u)[:, None] * u[None, :], Q[:, 3:4]], axis=-1))
    elif rotate == "all":
        Qr = Q
    else:
        Qr = np.zeros_like(Q)
        Qr[:, 3] = 1.0
    inv = Qr * np.array([-1.0, -1.0, -1.0, 1.0])
    inplace = k.copy()
    inplace[:, joint, 0:3] = _qrot(inv, T - Tr)
    inplace[:, joint, 4:8] = _norm4(_qmul(inv, Q))
    traj = np.zeros((k.shape[0], 1, 12))
    traj[:, 0, 0:3], traj[:, 0, 4:8], traj[:, 0, 8:11] = Tr, Qr, 1.0
    if loop:
        inplace = inplace[:-1]
    return np.ascontiguousarray(inplace.astype(F)), np.ascontiguousarray(traj.astype(F))
