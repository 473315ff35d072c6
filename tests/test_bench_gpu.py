"""bench.py as the per-change measurement runs it: a plain line (headline keys only, the side measurements left to --full) and
--dump-outputs, whose arrays are the same from run to run for the same arguments.  Small workload (32x32, batch 2)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--size", "32", "--batch", "2",
           "--T", "20", "--dump-outputs", str(out_dir)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_bench_line_and_dumped_outputs_repeat(tmp_path):
    lines = [_plain_run(tmp_path / d) for d in ("a", "b")]
    for line in lines:
        assert line["metric"] == "denoising steps/sec (32x32 bs2)" and line["unit"] == "steps/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f32" and line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0
        assert abs(line["ms_per_step"] - 1e3 / line["value"]) < 0.01 * line["ms_per_step"] + 1e-3
        assert line["full"] is False and line["roofline"] is None and line["cpu_baseline"] is None and line["train"].startswith("skipped")
    xa, xb = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    assert xa.dtype == np.float32 and xa.shape == (2, 1, 32, 32) and np.isfinite(xa).all()
    assert np.allclose(xa, xb, rtol=0, atol=1e-6)
