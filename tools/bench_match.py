#!/usr/bin/env python3
"""Motion matching (SPEC.md section 25) against the unfused path a user would otherwise write: the three launches of
mtr_anim_match_search_device next to torch.addmm(c, Q, F.T).argmax(1) in float32, alternated in one process on one side stream and
timed with device events around windows of many calls.

    python tools/bench_match.py [--shapes 4096x65536x32,256x65536x32] [--rounds 7] [--window 0.4] [--out file.json]

Per shape it prints one JSON line: the median, least and greatest time per call of both paths over the rounds, the achieved
FLOP/s of the search (2 n R D operations over its time; the f32 matrix peak of an MI355X is 157.3 TF) and the bytes of features
a call streams at least once.  The yardstick is used for time only: its sums are ordered differently, so the winners of both
paths are compared by cost, in float64, within the bound of section 25.  Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_F32 = 157.3e12


def timed(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters  # ms per call


def bench_shape(dev, n, R, D, rounds, window, python_api=False):
    import torch
    from mt_renderer_amd import api
    rng = np.random.default_rng(25)
    feats = rng.standard_normal((R, D)).astype(np.float32)
    rows = np.zeros(R, dtype=api.MATCH_ROW)
    rows["x"] = np.arange(R, dtype=np.float32) * np.float32(16000.0 / R)  # one long clip, x strictly increasing
    rows["bias"] = (rng.random(R) * 0.01).astype(np.float32)
    q = (feats[rng.integers(0, R, n)] + 0.3 * rng.standard_normal((n, D))).astype(np.float32)
    m = api.AnimMatch(dev, [16384], [0], rows, feats, pose_dims=0, max_instances=n)
    t_play = torch.zeros((n, 32), dtype=torch.uint8, device="cuda:0")
    t_q, t_f = torch.from_numpy(q).to("cuda:0"), torch.from_numpy(feats).to("cuda:0")
    t_cm, t_rs = torch.zeros((n, 16), dtype=torch.uint8, device="cuda:0"), torch.zeros((n, 16), dtype=torch.uint8, device="cuda:0")
    t_c = -(0.5 * (t_f * t_f).sum(1) + torch.from_numpy(rows["bias"]).to("cuda:0"))
    t_ft = t_f.t().contiguous()
    box = {}

    side = torch.cuda.Stream()  # not torch's legacy default stream, which the binding would leave for a helper stream
    ptr = lambda t: C.c_void_p(t.data_ptr())
    c_args = (m._h, ptr(t_play), ptr(t_q), None, n, 0, ptr(t_cm), ptr(t_rs), C.c_void_p(side.cuda_stream))

    def ours():
        if python_api:
            m.search(t_play, t_q, t_cm, results=t_rs, stream=side)
        elif api.lib.mtr_anim_match_search_device(*c_args):  # the C call a host makes: the binding's checks are not the kernels'
            raise RuntimeError(api.lib.mtr_last_error(dev._h).decode())

    def yard():
        box["win"] = torch.addmm(t_c, t_q, t_ft).argmax(1)

    torch.cuda.synchronize()
    ctx = torch.cuda.stream(side)
    ctx.__enter__()
    try:
        for fn in (ours, yard):  # warm-up: code objects, the GEMM's algorithm choice, the allocator's n x R block
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        iters = {}
        for name, fn in (("ours", ours), ("yard", yard)):
            one = timed(fn, 3)
            iters[name] = max(3, int(window * 1000.0 / max(one, 1e-3)))
        ms = {"ours": [], "yard": []}
        for _ in range(rounds):  # the two paths alternate, so that what else the machine does falls on both
            ms["ours"].append(timed(ours, iters["ours"]))
            ms["yard"].append(timed(yard, iters["yard"]))
        # the winners, by cost: float64 scores of every row, a block of instances at a time
        res = t_rs.cpu().numpy().reshape(-1).view(api.MATCH_RESULT)
        w_ours = torch.from_numpy(res["row"].astype(np.int64)).to("cuda:0")
        w_yard = box["win"]
        f64, c64 = t_f.double(), t_c.double()
        u, k = 2.0 ** -24, D + 2
        gamma = k * u / (1 - k * u)
        worst = {"ours": 0.0, "yard": 0.0}
        differ = 0
        for i0 in range(0, n, 512):
            q64 = t_q[i0:i0 + 512].double()
            S = q64 @ f64.t() + c64[None, :]
            bound = gamma * (q64.abs() @ f64.abs().t() + c64.abs()[None, :])
            best, w = S.max(1)
            ar = torch.arange(S.shape[0], device="cuda:0")
            for name, win in (("ours", w_ours[i0:i0 + 512]), ("yard", w_yard[i0:i0 + 512])):
                room = bound[ar, win] + bound[ar, w]
                worst[name] = max(worst[name], float(((best - S[ar, win]) / room).max().item()))
            differ += int((w_ours[i0:i0 + 512] != w_yard[i0:i0 + 512]).sum().item())
    finally:
        ctx.__exit__(None, None, None)
        torch.cuda.synchronize()
        m.close()
    med = {k_: float(np.median(v)) for k_, v in ms.items()}
    flops = 2.0 * n * R * D
    return dict(shape=f"{n}x{R}x{D}", api="python" if python_api else "c", rounds=rounds, iters=iters,
                ours_ms=dict(median=med["ours"], min=min(ms["ours"]), max=max(ms["ours"])),
                torch_addmm_argmax_ms=dict(median=med["yard"], min=min(ms["yard"]), max=max(ms["yard"])),
                speedup=med["yard"] / med["ours"], no_slower=med["ours"] <= med["yard"],
                ours_tflops=flops / (med["ours"] * 1e-3) / 1e12, share_of_f32_matrix_peak=flops / (med["ours"] * 1e-3) / PEAK_F32,
                feature_bytes=R * ((D + 7) // 8 * 8) * 4, yardstick_score_bytes=n * R * 4,
                winners_differ=differ, worst_cost_gap_over_bound=worst, winners_within_bound=worst["ours"] <= 1.0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="4096x65536x32,256x65536x32")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.4, help="seconds of work per path and round")
    ap.add_argument("--python-api", action="store_true", help="time AnimMatch.search with its argument checks instead of the C call")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_match: no GPU (there is no CPU fallback)")
    from mt_renderer_amd import api
    dev = api.Device(0)
    out = []
    try:
        for n, R, D in shapes:
            r = bench_shape(dev, n, R, D, args.rounds, args.window, args.python_api)
            print(json.dumps(r), flush=True)
            out.append(r)
    finally:
        dev.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    if not all(r["no_slower"] and r["winners_within_bound"] for r in out):
        sys.exit(1)


if __name__ == "__main__":
    main()
