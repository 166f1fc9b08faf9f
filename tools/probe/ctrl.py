"""Controllers (SPEC.md section 21): mtr_anim_ctrl_step_device on the locomotion graph of tests/ctrl_model.py for 1 024 and
65 535 instances -- a step alone; a step plus the player's advance that consumes its n-slot command list, next to an advance
with no commands; and the host recipe the controller replaces: the play states read back, the numpy model of the rule on
them, the command list uploaded (wall clock, with the waits).  hipEvents around the calls on a side stream, median of 20 after
5 warm-ups, three runs of each; the controller states are checked against the numpy model at the end.
    usage: ctrl.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mt_renderer_amd import api  # noqa: E402
from tests import ctrl_model as cm  # noqa: E402
from tests import player_model as pm  # noqa: E402

dev = api.Device(0)
tab, g = cm.LOCO_TAB, cm.locomotion()
out = {}
side = torch.cuda.Stream()
DT = pm.DT


def dev_u8(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1, a.dtype.itemsize).copy()).to("cuda:0")


def timed(fn, reps=25, warm=5):
    t = []
    for it in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        if it >= warm:
            t.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(t))


for n in (1024, 65535):
    rng = np.random.default_rng(n)
    play = np.zeros(n, dtype=api.PLAY_STATE)
    play["x_a"] = rng.uniform(0, 30, n)
    play["speed"] = rng.uniform(0.5, 1.5, n)
    st = np.zeros(n, dtype=api.CTRL_STATE)
    params = np.zeros((n, 2), dtype=np.float32)
    params[:, cm.SPEED] = rng.uniform(0, 3, n)
    params[::50, cm.TRIGGER] = 1.0
    ct = api.AnimCtrl(dev, tab[0], tab[1], g["nodes"], g["trans"], g["nany"], g["nparams"])
    pl = api.AnimPlayer(dev, tab[0], tab[2], tab[1], max_instances=n)
    t_st, t_pl, t_pr = dev_u8(st), dev_u8(play), torch.from_numpy(params.copy()).to("cuda:0")
    t_cm = torch.empty((n, 16), dtype=torch.uint8, device="cuda:0")
    t_ct = torch.zeros(len(g["trans"]), dtype=torch.int32, device="cuda:0")
    t_ol = torch.zeros((n, 2, 16), dtype=torch.uint8, device="cuda:0")
    t_os = torch.empty((n, 2, 16), dtype=torch.uint8, device="cuda:0")
    t_pl2 = t_pl.clone()  # the advance without commands moves a crowd of its own
    torch.cuda.synchronize()
    calls = []  # what moved the deciding crowd, replayed through the models after the timing

    def step():
        ct.step(t_st, t_pl, t_pr, DT, t_cm, counts=t_ct, stream=side)
        calls.append("step")

    def step_advance():
        step()
        pl.advance(t_pl, DT, t_cm, out_layers=t_ol, out_steps=t_os, stream=side)
        calls.append("advance")

    runs = {k: [] for k in ("step_us", "step_advance_us", "advance_us", "host_recipe_us")}
    for run in range(3):
        runs["step_us"].append(timed(step))
        runs["step_advance_us"].append(timed(step_advance))
        runs["advance_us"].append(timed(lambda: pl.advance(t_pl2, DT, None, out_layers=t_ol, out_steps=t_os, stream=side)))
        # the host recipe: read the play states back, decide in numpy, upload the command list (wall clock, with the waits)
        hst, hpr = st.copy(), params.copy()
        t = []
        for it in range(25):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hpl = t_pl2.cpu().numpy().reshape(-1).view(api.PLAY_STATE)
            hst, hpr, hcm, _ = cm.step(g, tab, hst, hpl, hpr, DT)
            up = torch.from_numpy(hcm.view(np.uint8).reshape(n, 16)).to("cuda:0", non_blocking=False)
            torch.cuda.synchronize()
            if it >= 5:
                t.append((time.perf_counter() - t0) * 1e6)
        runs["host_recipe_us"].append(float(np.median(t)))
    if n == 1024:  # the states are still the models' after every timed call
        rs, rp, rpl, cmds, cnt = st, params, play, None, np.zeros(len(g["trans"]), dtype=np.uint32)
        for what in calls:
            if what == "step":
                rs, rp, cmds, cnt = cm.step(g, tab, rs, rpl, rp, DT, cnt)
            else:
                rpl = pm.advance(rpl, DT, tab, cmds)[0]
        assert pm.same_bits(t_st.cpu().numpy().reshape(-1).view(api.CTRL_STATE), rs).all()
        assert pm.same_bits(t_pl.cpu().numpy().reshape(-1).view(api.PLAY_STATE), rpl).all()
        assert (t_ct.cpu().numpy().view(np.uint32) == cnt).all()
    out[str(n)] = runs
    print(n, runs, flush=True)
    ct.close()
    pl.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
