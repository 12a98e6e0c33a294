"""bench.py's plain run on one GPU: exactly the timed steps and the result line (no roofline, head-only, trained-offsets or
CPU-baseline legs; those need --full), and --dump-outputs writing what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(900)
def test_plain_run_prints_the_headline_and_dumps_outputs(tmp_path):
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--size", "512",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=800)
    assert r.returncode == 0, f"bench.py failed:\n{r.stdout[-2000:]}\n{r.stderr[-6000:]}"
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "images/sec" and out["higher_is_better"] is True and out["dtype"]
    assert out["ms_per_step"] > 0 and abs(out["value"] - 2 * 1e3 / out["ms_per_step"]) <= 0.01 * out["value"]
    assert out["roofline"] is None and out["cpu_baseline"] is None and out["config"]["full"] is False
    assert not {"head_only", "trained_like_offsets", "roofline_steps"} & set(out["config"])
    files = sorted(os.listdir(out_dir))
    assert files == ["grad_sums.npy", "grads_sample.npy", "loss.npy", "param_sums.npy", "params_sample.npy"]
    total = 0
    for f in files:
        a = np.load(out_dir / f)
        assert a.dtype in (np.float32, np.float64), f
        assert np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 << 20
    loss = np.load(out_dir / "loss.npy")
    assert loss.shape == (1,) and abs(float(loss[0]) - out["config"]["final_loss"]) <= 1e-3 * abs(float(loss[0])) + 1e-3
    assert np.load(out_dir / "params_sample.npy").shape == (1 << 21,)
    assert np.abs(np.load(out_dir / "grads_sample.npy")).max() > 0
