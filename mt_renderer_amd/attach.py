"""Host helpers for attachments (SPEC.md section 18).

An attachment record's ``offset`` places the object in the SOURCE MODEL'S BIND SPACE, because the batch holds
``palette_j = world_j * imat_j`` and not ``world_j``.  What a user thinks in is a placement relative to the joint (the grip
of a sword in the hand's frame).  ``bind_offsets`` converts one into the other.  It is a helper, not part of the rule: the
rule takes whatever offset the record holds."""
import numpy as np


def bind_offsets(imats, joints, local_offsets) -> np.ndarray:
    """offsets for ATTACH records, [n, 16] float32 column-major: ``inverse(imat_j) * local`` per record, formed in float64
    and rounded once.

    imats: the skeleton's inverse bind matrices [njoints, 16] (column-major, as given to Model.set_skeleton);
    joints: [n] joint index per record; local_offsets: [n, 16] (or [16], shared) placements relative to the joint.
    With it, ``M_src * palette_j * offset = M_src * world_j * local`` up to rounding."""
    im = np.asarray(imats, dtype=np.float64).reshape(-1, 4, 4)  # [j][column][row]
    j = np.asarray(joints, dtype=np.int64).reshape(-1)
    if j.size and (j.min() < 0 or j.max() >= im.shape[0]):
        raise ValueError("bind_offsets: a joint outside the skeleton")
    loc = np.asarray(local_offsets, dtype=np.float64).reshape(-1, 4, 4)
    if loc.shape[0] == 1:
        loc = np.broadcast_to(loc, (j.size, 4, 4))
    if loc.shape[0] != j.size:
        raise ValueError("bind_offsets: one local offset per joint index (or one for all)")
    # column-major storage [c][r] is the transpose of the mathematical matrix
    inv = np.linalg.inv(im[j].transpose(0, 2, 1))
    out = inv @ loc.transpose(0, 2, 1)
    return np.ascontiguousarray(out.transpose(0, 2, 1).reshape(-1, 16).astype(np.float32))
