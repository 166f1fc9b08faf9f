"""Spring records for api.AnimSpring (include/mtr.h, SPEC.md section 24) from what an asset holds: a chain of joints and their
bind translations."""
import numpy as np

from .api import MTR_E_INVALID, SPRING, MtrError


def chain(parents, bind_translations, joints, stiffness, drag, gravity=(0.0, 0.0, 0.0), leaf_tail=None) -> np.ndarray:
    """The SPRING records of the joints of one strand, root end first: each joint's ``tail`` is the bind translation of the next
    joint of the list, which must be its child.  The last joint takes ``leaf_tail`` -- or, where that is None, the bind
    translation of its only child; a leaf needs ``leaf_tail``.  parents: one byte per joint (a root: 255 or itself);
    bind_translations: [njoints, 3], each joint's translation in its parent's space; stiffness, drag: one value, or one per
    joint of the list; gravity: one vector for all of them.  Records of several strands are concatenated by the caller."""
    par = np.asarray(parents, dtype=np.uint8).reshape(-1)
    bt = np.asarray(bind_translations, dtype=np.float32).reshape(-1, 3)
    js = [int(j) for j in joints]
    if bt.shape[0] != par.size or not js or any(not 0 <= j < par.size for j in js):
        raise MtrError(MTR_E_INVALID, "spring chain: one bind translation per joint, and joints of the skeleton")
    out = np.zeros(len(js), dtype=SPRING)
    out["joint"] = js
    out["stiffness"] = np.broadcast_to(np.asarray(stiffness, dtype=np.float32), (len(js),))
    out["drag"] = np.broadcast_to(np.asarray(drag, dtype=np.float32), (len(js),))
    out["gravity"] = np.asarray(gravity, dtype=np.float32).reshape(3)
    for k, j in enumerate(js):
        if k + 1 < len(js):
            if int(par[js[k + 1]]) != j or js[k + 1] == j:
                raise MtrError(MTR_E_INVALID, f"spring chain: joint {js[k + 1]} is not the child of joint {j}")
            out["tail"][k] = bt[js[k + 1]]
        elif leaf_tail is not None:
            out["tail"][k] = np.asarray(leaf_tail, dtype=np.float32).reshape(3)
        else:
            kids = [c for c in range(par.size) if int(par[c]) == j and c != j]
            if len(kids) != 1:
                raise MtrError(MTR_E_INVALID, f"spring chain: joint {j} has {len(kids)} children, give leaf_tail")
            out["tail"][k] = bt[kids[0]]
    return out
