"""bench.py on one GPU: a plain run prints the headline line and nothing it has to leave to --full, and --dump-outputs
writes the framebuffer of the last timed frame, which is the CPU oracle's frame of the same scene bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_frame(tmp_path):
    from mt_renderer_amd import scene
    from tests.helpers import render_oracle
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 7 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "Mtris/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert not {"roofline", "latency", "cpu_baseline", "configs", "repetitions"} & set(out)
    assert sorted(os.listdir(tmp_path)) == ["color.npy", "depth.npy"]
    color, depth = np.load(tmp_path / "color.npy"), np.load(tmp_path / "depth.npy")
    assert color.dtype == np.float32 and color.shape == (1080, 1920, 4)
    assert depth.dtype == np.float32 and depth.shape == (1080, 1920)
    w, h = 1920, 1080
    draws = [dict(md=scene.headline_model(), M=scene.to_f32_colmajor(scene.headline_transform(w, h)), palette=scene.bone_palette())]
    rc, rd, _ = render_oracle(w, h, draws, nthreads=max(1, min(len(os.sched_getaffinity(0)), 16)))
    assert (color == rc.astype(np.float32)).all()
    assert (depth.view(np.uint32) == rd.view(np.uint32)).all()
