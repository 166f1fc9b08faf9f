"""Animation events (SPEC.md section 22): mtr_anim_events_collect_device on the steps a player wrote for a crowd on the
locomotion clips of tests/ctrl_model.py, 4 096 and 262 144 instances with S = 2 (half the crowd in a cross-fade, so both steps
are live) -- a collect alone, with and without the per-instance masks; an advance alone; and an advance plus the collect of
its steps.  hipEvents around the calls on a side stream, median of 20 after 5 warm-ups, three runs of each; the list of the
last collect is checked against the numpy model at the end.
    usage: events.py [out.json]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from mt_renderer_amd import anim_events, api  # noqa: E402
from tests import ctrl_model as cm  # noqa: E402
from tests import events_model as em  # noqa: E402
from tests import player_model as pm  # noqa: E402

dev = api.Device(0)
tab = cm.LOCO_TAB
MARKS = {cm.IDLE: [(15.0, 7)], cm.WALK: [(8.0, 1), (24.0, 2)], cm.RUN: [(4.0, 1), (12.0, 2)], cm.JUMP: [(0.5, 40), (11.0, 99)]}
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


for n in (4096, 262144):
    rng = np.random.default_rng(n)
    play = np.zeros(n, dtype=api.PLAY_STATE)
    play["clip_a"], play["clip_b"] = rng.integers(0, 4, n), rng.integers(0, 3, n)
    play["x_a"], play["x_b"] = rng.uniform(0, 11, n), rng.uniform(0, 16, n)
    play["speed"] = rng.uniform(0.5, 1.5, n) * np.where(rng.random(n) < 0.1, -1, 1)
    fading = rng.random(n) < 0.5
    play["fade"] = np.where(fading, 0.5, 0.0)  # slow fades: they run through every timed call
    play["w"] = np.where(fading, rng.uniform(0.0, 0.2, n), 0.0)
    counts, markers = anim_events.build(MARKS, 4)
    ev = api.AnimEvents(dev, tab[0], tab[1], counts, markers, max_instances=n)
    pl = api.AnimPlayer(dev, tab[0], tab[2], tab[1], max_instances=n)
    t_pl = dev_u8(play)
    t_sp = torch.zeros((n, 2, 16), dtype=torch.uint8, device="cuda:0")
    cap = n
    t_out = torch.zeros((cap, 16), dtype=torch.uint8, device="cuda:0")
    t_ct = torch.zeros(2, dtype=torch.int32, device="cuda:0")
    t_bits = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    pl.advance(t_pl, DT, None, out_steps=t_sp, stream=side)  # the steps of one real frame
    torch.cuda.synchronize()

    def advance_collect():
        pl.advance(t_pl, DT, None, out_steps=t_sp, stream=side)
        ev.collect(t_sp, 0.0, t_out, t_ct, bits=t_bits, stream=side)

    runs = {k: [] for k in ("collect_us", "collect_bits_us", "advance_us", "advance_collect_us")}
    for run in range(3):
        runs["collect_us"].append(timed(lambda: ev.collect(t_sp, 0.0, t_out, t_ct, stream=side)))
        runs["collect_bits_us"].append(timed(lambda: ev.collect(t_sp, 0.0, t_out, t_ct, bits=t_bits, stream=side)))
        runs["advance_us"].append(timed(lambda: pl.advance(t_pl, DT, None, out_steps=t_sp, stream=side)))
        runs["advance_collect_us"].append(timed(advance_collect))
    # the last collect against the model, on the steps it read
    sp = t_sp.cpu().numpy().reshape(-1).view(api.ROOT_STEP).reshape(n, 2)
    want = em.collect(em.event_set(tab, MARKS), sp, 0.0, cap)
    got_ct = t_ct.cpu().numpy().view(np.uint32)
    assert (got_ct == want[1]).all() and (t_bits.cpu().numpy().view(np.uint32) == want[2]).all()
    assert pm.same_bits(t_out.cpu().numpy().reshape(-1).view(api.EVENT)[:int(got_ct[1])], want[0][:int(want[1][1])]).all()
    runs["events_last_frame"] = int(got_ct[0])
    out[str(n)] = runs
    print(n, runs, flush=True)
    ev.close()
    pl.close()
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
