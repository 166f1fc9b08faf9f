"""Root motion (SPEC.md section 19): mtr_batch_root_motion_device for 1 024 and 65 535 instances at S = 2, uniform keys and
tracks, next to a device copy of the same bytes (steps in, matrices in and out): hipEvents around the call on a side stream,
median of 20 after 5 warm-ups, and a check that the batch still holds the model's matrices.  A target for prof_probe.sh.
    usage: root_motion.py [out.json]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mt_renderer_amd import api, scene  # noqa: E402
from tests import attach_model as am  # noqa: E402
from tests import root_model as rm  # noqa: E402

dev = api.Device(0)
cube = api.Model.new(dev, scene.cube_model())
out = {}
side = torch.cuda.Stream()
for kind in ("uniform", "tracks"):
    tr = rm.make_set(kind, 1, 77)
    traj = api.Anim(dev, 1, tr) if kind == "uniform" else api.AnimTracks(dev, 1, tr)
    root = api.AnimRoot(dev, 1, len(rm.LENGTHS), 0, rm.ROOT_FLAGS)
    for n in (1024, 65535):
        rng = np.random.default_rng(n)
        st = np.zeros((n, 2), dtype=api.ROOT_STEP)
        st["clip"] = rng.choice([5, 6], size=(n, 2))
        st["x"] = rng.uniform(0, 30, size=(n, 2))
        st["dx"] = 0.37
        st["w"] = 0.5
        M = am.trs(rng, n)
        b = api.Batch(dev, cube, M)
        t = torch.from_numpy(st.view(np.uint8).reshape(n, 2, 16).copy()).to("cuda:0")
        src = torch.empty(n * 96, dtype=torch.uint8, device="cuda:0")
        dst = torch.empty_like(src)
        torch.cuda.synchronize()
        calls, copies = [], []
        for it in range(25):
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            with torch.cuda.stream(side):
                e0.record()
                b.root_motion_device(traj, root, t)
                e1.record()
                dst.copy_(src)
                e2.record()
            torch.cuda.synchronize()
            if it >= 5:
                calls.append(e0.elapsed_time(e1) * 1e3)
                copies.append(e1.elapsed_time(e2) * 1e3)
        # the result is still the model's
        b.update(model_mats=M)
        b.root_motion_device(traj, root, t)
        assert rm.same_bits(b.read_model_mats(), rm.root_motion(M, tr, (0, np.array(rm.ROOT_FLAGS, dtype=np.uint32)), st)).all()
        out[f"{kind}_{n}"] = dict(call_us=[float(np.median(calls)), min(calls), max(calls)], copy_us=[float(np.median(copies)), min(copies), max(copies)])
        print(kind, n, out[f"{kind}_{n}"], flush=True)
        b.close()
    root.close()
    traj.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
