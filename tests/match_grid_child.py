"""The child of tests/test_gpu_match_grid.py: `python -m tests.match_grid_child <tune> <out.npz>`, started as a fresh process
with MTR_MATCH_TUNE=<tune> in its environment (the library reads the variable once per process).  It rebuilds the grid cases of
that tuning from their seeds, opens one device, runs the scores call and the search with and without filters for every case
through the host hooks (numpy in, numpy out, each call waits: no torch) and writes the raw outputs.  It compares nothing: the
model and the message that names the case stay in the pytest process."""
import os
import sys
import time

import numpy as np


def open_set(dev, c):
    from mt_renderer_amd import api
    s = c["set"]
    return api.AnimMatch(dev, s["nkeys"], s["clip_flags"], s["rows"], s["feats"], pose_dims=s["pose_dims"], flags=s["flags"], seconds=float(s["seconds"]),
                         near=float(s["near"]), margin=float(s["margin"]), mean=s["mean"] if s["has_norm"] else None, scale=s["scale"] if s["has_norm"] else None,
                         max_instances=c["n"])


def run_case(dev, c):
    """(scores [n, R], (commands, results) with the case's filters, (commands, results) without)"""
    m = open_set(dev, c)
    try:
        return m.scores_host(c["play"], c["raw"]), m.search_host(c["play"], c["raw"], c["filt"], c["base"]), m.search_host(c["play"], c["raw"], None, c["base"])
    finally:
        m.close()


def main(tune, out):
    from mt_renderer_amd import api
    from tests import match_grid_cases as gc
    if os.environ.get("MTR_MATCH_TUNE") != tune:
        raise SystemExit(f"MTR_MATCH_TUNE is {os.environ.get('MTR_MATCH_TUNE')!r}, not {tune!r}")
    cases = gc.forced_cases(tune)
    arrays = {}
    t0 = time.perf_counter()
    dev = api.Device(0)
    try:
        for k, c in enumerate(cases):
            S, (cf, rf), (cn, rn) = run_case(dev, c)
            arrays.update({f"scores{k}": S, f"cmds_f{k}": cf.view(np.uint32), f"res_f{k}": rf.view(np.uint32), f"cmds_n{k}": cn.view(np.uint32), f"res_n{k}": rn.view(np.uint32)})
    finally:
        dev.close()
    arrays["gpu_seconds"] = np.float64(time.perf_counter() - t0)
    np.savez(out, **arrays)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
