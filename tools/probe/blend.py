"""Blend spaces (SPEC.md section 23): mtr_anim_blend_advance_device with the layers, the steps and the shares out, for 4 096
and 262 144 instances, on a 1-D space of three samples and on the 3 x 3 grid (8 triangles), the parameters spread over the
space and a little beyond its hull -- next to a player's advance with layers and steps out for the same instances.  hipEvents
around the call on a side stream, median of 20 after 5 warm-ups, three runs of each; the states and records of the last call
are checked against the numpy model at the end.
    usage: blend.py [out.json]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mt_renderer_amd import api  # noqa: E402
from tests import blend_model as bm  # noqa: E402
from tests import player_model as pm  # noqa: E402

dev = api.Device(0)
tab = pm.table([30, 32, 16], [pm.LOOP] * 3, [30.0, 32.0, 24.0])
SPACES = {
    "line3": bm.blend_set(tab, [(0, 0.0), (1, 1.4), (2, 4.0)], None, nparams=2, param_x=0, damp=8.0),
    "grid9": bm.blend_set(tab, [(k % 3, x, y) for k, (x, y) in enumerate(bm.GRID)], bm.GRID_TRIS, nparams=2, param_x=0, param_y=1, damp=8.0),
}
out = {}
side = torch.cuda.Stream()
DT = pm.DT
NL = 3


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


for n in (4096, 262144):
    rng = np.random.default_rng(n)
    runs = {}
    for name, bs in SPACES.items():
        s = bs["samples"]
        lo, hi = np.array([s["px"].min(), s["py"].min()]), np.array([s["px"].max(), s["py"].max()])
        params = (lo + rng.uniform(-0.15, 1.15, (n, 2)) * np.maximum(hi - lo, 1.0)).astype(np.float32)
        st = np.zeros(n, dtype=api.BLEND_STATE)
        st["phase"], st["speed"] = rng.uniform(0, 1, n), rng.uniform(0.5, 1.5, n) * np.where(rng.random(n) < 0.1, -1, 1)
        st["px"], st["py"] = params[:, 0] * 0.5, params[:, 1] * 0.5
        bl = api.AnimBlend(dev, tab[0], tab[2], tab[1], bs["samples"], bs["tris"] if bs["tris"].size else None, nparams=2, param_x=bs["param_x"],
                           param_y=bs["param_y"], damp=float(bs["damp"]), max_instances=n)
        t_st, t_pr = dev_u8(st), torch.from_numpy(params.copy()).to("cuda:0")
        t_ly = torch.zeros((n, NL, 16), dtype=torch.uint8, device="cuda:0")
        t_sp = torch.zeros((n, 3, 16), dtype=torch.uint8, device="cuda:0")
        t_sh = torch.zeros((n, 3), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        call = lambda: bl.advance(t_st, t_pr, DT, out_layers=t_ly, out_steps=t_sp, out_shares=t_sh, stream=side)
        runs[name + "_us"] = [timed(call) for _ in range(3)]
        # the last call against the model, from the states it read
        before = t_st.cpu().numpy().reshape(-1).view(api.BLEND_STATE).copy()
        with torch.cuda.stream(side):
            call()
        torch.cuda.synchronize()
        tr = {}
        want = bm.advance(bs, before, params, DT, NL, trace=tr)
        assert pm.same_bits(t_st.cpu().numpy().reshape(-1).view(api.BLEND_STATE), want[0]).all()
        assert pm.same_bits(t_ly.cpu().numpy().reshape(-1).view(api.ANIM_LAYER).reshape(n, NL), want[1]).all()
        assert pm.same_bits(t_sp.cpu().numpy().reshape(-1).view(api.ROOT_STEP).reshape(n, 3), want[2]).all()
        assert pm.same_bits(t_sh.cpu().numpy(), want[3]).all()
        runs[name + "_fallback_lanes"] = tr.get("fb_outside", 0) + tr.get("fb_crack", 0)
        bl.close()
    # a player's advance with the same outputs, for scale
    play = np.zeros(n, dtype=api.PLAY_STATE)
    play["x_a"], play["speed"] = rng.uniform(0, 16, n), rng.uniform(0.5, 1.5, n)
    pl = api.AnimPlayer(dev, tab[0], tab[2], tab[1], max_instances=n)
    t_pl = dev_u8(play)
    t_l2 = torch.zeros((n, 2, 16), dtype=torch.uint8, device="cuda:0")
    t_s2 = torch.zeros((n, 2, 16), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    runs["player_advance_us"] = [timed(lambda: pl.advance(t_pl, DT, None, out_layers=t_l2, out_steps=t_s2, stream=side)) for _ in range(3)]
    pl.close()
    out[str(n)] = runs
    print(n, runs, flush=True)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
