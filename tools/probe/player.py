"""Players (SPEC.md section 20): mtr_anim_player_advance_device with all three outputs for 1 024 and 65 535 instances, with no
commands, with 1 % of the instances commanded from a host list and from a device list, next to a device copy that moves the
same bytes (152 per instance: 32 in, 32 + 24 + 32 + 32 out), and the host recipe the player replaces: a vectorised numpy
advance of every instance plus the upload of its animation states and root steps.  hipEvents around the call on a side
stream, median of 20 after 5 warm-ups, three runs of each; the states are checked against the numpy model at the end.
    usage: player.py [out.json]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mt_renderer_amd import api  # noqa: E402
from tests import player_model as pm  # noqa: E402

dev = api.Device(0)
tab = pm.table([30, 20, 40], [pm.LOOP, pm.LOOP, 0], [30.0, 24.0, 30.0])
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
    st = np.zeros(n, dtype=api.PLAY_STATE)
    st["clip_a"] = rng.integers(0, 2, n)
    st["x_a"] = rng.uniform(0, 20, n)
    st["speed"] = rng.uniform(0.5, 1.5, n)
    pl = api.AnimPlayer(dev, tab[0], tab[2], tab[1], max_instances=n)
    t_st = dev_u8(st)
    t_oa = torch.empty((n, 24), dtype=torch.uint8, device="cuda:0")
    t_ol = torch.zeros((n, 2, 16), dtype=torch.uint8, device="cuda:0")
    t_os = torch.empty((n, 2, 16), dtype=torch.uint8, device="cuda:0")
    src = torch.empty(n * 76, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)
    cm = np.zeros(max(1, n // 100), dtype=api.PLAY_CMD)
    cm["instance"] = rng.choice(n, cm.size, replace=False)
    cm["clip"], cm["x"], cm["seconds"] = 1, 0.5, 0.3
    t_cm = dev_u8(cm)
    torch.cuda.synchronize()
    applied = []  # what every call carried, replayed through the model after the timing

    def advance(cmds):
        pl.advance(t_st, DT, cmds, out_states=t_oa, out_layers=t_ol, out_steps=t_os, stream=side)
        applied.append(cmds is not None)

    runs = {k: [] for k in ("call_us", "copy_us", "call_cmds_host_us", "call_cmds_device_us", "host_recipe_us")}
    for run in range(3):
        runs["call_us"].append(timed(lambda: advance(None)))
        runs["copy_us"].append(timed(lambda: dst.copy_(src)))
        runs["call_cmds_host_us"].append(timed(lambda: advance(cm)))
        runs["call_cmds_device_us"].append(timed(lambda: advance(t_cm)))
        # the host recipe: advance and wrap every instance in numpy, rebuild the records, upload them (wall clock, with the wait)
        x, clip, speed = st["x_a"].copy(), st["clip_a"].astype(np.int64), st["speed"].copy()
        N, rate = tab[0][clip].astype(np.float32), tab[2][clip]
        hs, hp = np.zeros(n, dtype=api.ANIM_STATE), np.zeros((n, 2), dtype=api.ROOT_STEP)
        hs["clip_a"], hp["clip"][:, 0] = clip, clip
        t = []
        for it in range(25):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dx = np.float32(DT) * speed * rate
            hp["x"][:, 0], hp["dx"][:, 0] = x, dx
            x = np.mod(x + dx, N)
            hs["x_a"] = x
            a = torch.from_numpy(hs.view(np.uint8).reshape(n, 24)).to("cuda:0", non_blocking=False)
            b = torch.from_numpy(hp.view(np.uint8).reshape(n, 32)).to("cuda:0", non_blocking=False)
            torch.cuda.synchronize()
            if it >= 5:
                t.append((time.perf_counter() - t0) * 1e6)
        runs["host_recipe_us"].append(float(np.median(t)))
    if n == 1024:  # the states are still the model's after every timed call
        ref = st
        for with_cmds in applied:
            ref = pm.advance(ref, DT, tab, cm if with_cmds else None)[0]
        got = t_st.cpu().numpy().reshape(-1).view(api.PLAY_STATE)
        assert pm.same_bits(got, ref).all()
    out[str(n)] = runs
    print(n, runs, flush=True)
    pl.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
