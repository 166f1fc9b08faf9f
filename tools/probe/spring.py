"""Spring bones (SPEC.md section 24): microseconds per call of mtr_batch_animate_spring_device for 4 096 and 262 140
instances of 64 joints (a batch holds at most 65 535: the larger count is four batches of 65 535, animated by four calls in
a row, and the figure is the four together), two layers per instance, on two spring sets of 16 springs each over one skeleton:
  rounds4   four strands of four joints hung onto joint 12 of a spine (paths of 14 to 17 joints): 4 rounds, 4 threads a round
  rounds16  one strand of sixteen joints hung onto the root (paths of 2 to 17 joints): 16 rounds, 1 thread a round
next to mtr_batch_animate_ik_device (one AIM chain on joint 12) and mtr_batch_animate_layers_device on the same layers in the
same run; the spring calls carry the same IK set and targets, so what they add to the IK call is the springs.  Every call
gets a motion matrix per instance and steps the states in place.  A timed region is --calls stream-ordered calls between two
events on one stream, repeated --reps times per mode with the modes alternating; the median per call is reported.
    python tools/probe/spring.py [--calls N] [--reps R] [--counts 4096,262140] [--json OUT]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
from mt_renderer_amd import anim_spring, api, scene

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--counts", default="4096,262140")
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--json", default=None)
args = ap.parse_args()

J = 64
# a spine 0..12, four strands of four on joint 12, a strand of sixteen on the root, the rest on the root
PARENTS = [255] + list(range(12)) + [12, 13, 14, 15, 12, 17, 18, 19, 12, 21, 22, 23, 12, 25, 26, 27] + [0] + list(range(29, 44)) + [0] * 19
STRANDS4 = [list(range(13 + 4 * s, 17 + 4 * s)) for s in range(4)]
STRAND16 = list(range(29, 45))
assert len(PARENTS) == J


def clips(rng):
    """(keys [nkeys, 64, 12], flags): small bends, bones of length 0.1 along y, unit scale"""
    out = []
    for nk, fl in ((60, api.CLIP_LOOP), (31, api.CLIP_LOOP)):
        a = rng.uniform(-0.2, 0.2, size=(nk, J))
        k = np.zeros((nk, J, 12), dtype=np.float32)
        k[..., 1] = 0.1
        k[..., 6], k[..., 7] = np.sin(a / 2), np.cos(a / 2)
        k[..., 8:11] = 1.0
        out.append((k, fl))
    return out


dev = api.Device(0)
rng = np.random.default_rng(args.seed)
model = api.Model.new(dev, scene.skinned_capsule_model([((0.0, 0.0, 0.0), 0.35, 1.6)], rows=2, cols=3))
model.set_skeleton(PARENTS, np.tile(np.eye(4, dtype=np.float32).reshape(16), (J, 1)))
anim = api.Anim(dev, J, clips(rng))
bind = np.tile(np.array([0.0, 0.1, 0.0], dtype=np.float32), (J, 1))
rec4 = np.concatenate([anim_spring.chain(PARENTS, bind, s, 40.0, 0.2, gravity=(0.0, -1.0, 0.0), leaf_tail=(0.0, 0.1, 0.0)) for s in STRANDS4])
rec16 = anim_spring.chain(PARENTS, bind, STRAND16, 40.0, 0.2, gravity=(0.0, -1.0, 0.0), leaf_tail=(0.0, 0.1, 0.0))
sets = {"spring_rounds4": api.AnimSpring(dev, PARENTS, rec4), "spring_rounds16": api.AnimSpring(dev, PARENTS, rec16)}
chain = np.zeros(1, dtype=api.ANIM_IK_CHAIN)
chain["kind"], chain["joint"], chain["axis"] = api.IK_AIM, [(12, 0, 0)], [(0.0, 1.0, 0.0)]
iks = api.AnimIK(dev, PARENTS, chain)
stream = torch.cuda.Stream()
results = []
MAX_BATCH = 65535
for total in [int(c) for c in args.counts.split(",")]:
    nb = -(-total // MAX_BATCH)
    n = total // nb  # per batch; the batches share their records
    batches = [api.Batch(dev, model, np.tile(np.eye(4, dtype=np.float32).reshape(16), (n, 1))) for _ in range(nb)]
    ly = np.zeros((n, 2), dtype=api.ANIM_LAYER)
    ly["clip"][:, 1] = 1
    ly["x"], ly["w"][:, 1] = rng.uniform(0, 60, (n, 2)), rng.uniform(0, 1, n)
    tg = np.zeros((n, 1), dtype=api.ANIM_IK_TARGET)
    tg["pos"], tg["w"] = rng.uniform(-1, 1, (n, 1, 3)), 1.0
    motion = np.tile(np.eye(4, dtype=np.float32).reshape(16), (n, 1))
    motion[:, 12:15] = rng.uniform(-0.01, 0.01, (n, 3))
    t_ly = torch.from_numpy(ly.view(np.uint8).reshape(n, 32).copy()).to("cuda:0")
    t_tg = torch.from_numpy(tg.view(np.uint8).reshape(n, 32).copy()).to("cuda:0")
    t_mo = torch.from_numpy(motion).to("cuda:0")
    t_st = {k: [torch.zeros((n * 16, 32), dtype=torch.uint8, device="cuda:0") for _ in range(nb)] for k in sets}

    def call(mode):
        for b, batch in enumerate(batches):
            if mode == "layers":
                batch.animate_layers(anim, t_ly)
            elif mode == "ik":
                batch.animate_ik(anim, t_ly, iks, t_tg)
            else:
                batch.animate_spring(anim, t_ly, sets[mode], t_st[mode][b], 1.0 / 60.0, iks, t_tg, t_mo)

    def timed(mode):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            for _ in range(args.calls):
                call(mode)
            e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.calls * 1e3

    modes = ["layers", "ik", "spring_rounds4", "spring_rounds16"]
    for mode in modes:  # warm-up: code objects, the batch's version ring
        with torch.cuda.stream(stream):
            for _ in range(3):
                call(mode)
    torch.cuda.synchronize()
    us = {m: [] for m in modes}
    for _ in range(args.reps):
        for mode in modes:
            us[mode].append(timed(mode))
    for mode in modes:
        r = dict(instances=n * nb, batches=nb, joints=J, layers=2, mode=mode, calls=args.calls, us_per_call=round(float(np.median(us[mode])), 2),
                 us_all=[round(v, 2) for v in us[mode]])
        if mode in t_st:
            st = t_st[mode][-1].cpu().numpy().reshape(-1).view(api.SPRING_STATE)
            r["states_finite"] = bool(np.isfinite(st["cur"]).all() and (st["live"] == 1).all())
        results.append(r)
        print(json.dumps(r), flush=True)
    for batch in batches:
        batch.close()
for s in sets.values():
    s.close()
iks.close()
anim.close()
model.close()
dev.close()
if args.json:
    json.dump(results, open(args.json, "w"), indent=1)
