"""CPU: the skeletal-pose entry points (SPEC.md section 12) are declared in include/mtr.h, exported by libmtr.so and bound
by api.py with the argument count of their prototype."""
import ctypes
import os

from tests.abi_header import prototypes as _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mtr_model_set_skeleton", "mtr_model_set_pose", "mtr_batch_update", "mtr_batch_set_poses", "mtr_batch_set_poses_device",
       "mtr_batch_read_palettes"]


def test_pose_prototypes_declared_exported_and_bound():
    from mt_renderer_amd import api
    protos = _prototypes()
    lib = ctypes.CDLL(api.LIB_PATH)
    for name in NEW:
        assert name in protos, f"include/mtr.h does not declare {name}"
        assert hasattr(lib, name), f"libmtr.so does not export {name}"
        assert name in api.EXPORTED_SYMBOLS, name
        fn = getattr(api.lib, name)
        assert fn.restype is ctypes.c_int32, name
        assert len(fn.argtypes) == protos[name], (name, len(fn.argtypes), protos[name])
    assert api.lib.mtr_abi_version() == 2


def test_null_handles_are_rejected_without_a_device():
    from mt_renderer_amd import api
    L = api.lib
    assert L.mtr_model_set_skeleton(None, None, None, 0) == api.MTR_E_INVALID
    assert L.mtr_model_set_pose(None, None, 0) == api.MTR_E_INVALID
    assert L.mtr_batch_update(None, None, None, 0) == api.MTR_E_INVALID
    assert L.mtr_batch_set_poses(None, None, 0) == api.MTR_E_INVALID
    assert L.mtr_batch_set_poses_device(None, None, 0, None) == api.MTR_E_INVALID
    assert L.mtr_batch_read_palettes(None, None, 0) == api.MTR_E_INVALID


def test_model_file_skeleton_is_the_joint_parents_and_imats():
    import numpy as np
    from mt_renderer_amd import files, scene
    from tests import mt_files
    md = scene.skinned_capsule_model([((0.0, 0.0, 0.0), 0.35, 1.6)], rows=2, cols=3)
    parents = [255, 0, 0, 2, 3]
    joints = [(j, p, (0.0, 0.1 * j, 0.0)) for j, p in enumerate(parents)]
    rng = np.random.default_rng(3)
    lm = rng.standard_normal((5, 16)).astype(np.float32)
    im = rng.standard_normal((5, 16)).astype(np.float32)
    mf = files.ModelFile(mt_files.write_rmodel(md, [0] * md.nprims, ["m"], [0] * md.nprims, joints=joints, lmats=lm, imats=im))
    p, i = mf.skeleton()
    assert p.dtype == np.uint8 and list(p) == parents
    assert (i.view(np.uint32) == im.view(np.uint32)).all()
