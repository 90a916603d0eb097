"""A plain `bench.py` run end to end on the GPU: the headline line alone, the dumped outputs, and a set-up cost that
stays small beside the steps (the --full legs are what take minutes)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_line_and_dumps_the_last_step(tmp_path):
    steps, warmup = 5, 2
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                          "--warmup", str(warmup), "--dump-outputs", str(tmp_path)],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [s for s in out.stdout.splitlines() if s.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == "hypotheses scored/sec" and d["unit"] == "hyp/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["n_gpus"] == 1 and d["steps"] == steps and d["warmup"] == warmup
    assert d["value"] > 0 and abs(d["value"] - 1000.0 * 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    for key in ("roofline", "stage_ms", "featurize", "cpu_baseline", "dtoid"):
        assert key not in d, key
    scores, top1 = np.load(tmp_path / "scores.npy"), np.load(tmp_path / "top1.npy")
    assert scores.shape == (1000,) and scores.dtype == np.float32 and np.isfinite(scores).all()
    assert top1.tolist() == [float(d["config"]["top1"])] and scores[d["config"]["top1"]] == scores.max()
    # everything but the warm-up and timed steps: start-up, set-up, teardown
    outside = wall - (steps + warmup) * d["ms_per_step"] / 1e3
    assert outside < 30.0, "a plain run spent %.1f s outside its steps" % outside
