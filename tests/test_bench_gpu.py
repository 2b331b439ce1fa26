"""
bench.py end to end at a small batch, in fresh processes as it is run: a plain run prints the headline line alone and
writes --dump-outputs; --full adds the second timed region and the dominant kernel's roofline.  Needs a real MI355X.
"""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("value_no_overlap", "ms_per_step_no_overlap", "roofline", "rooflines", "extra", "cpu_baseline")


def _bench(*argv, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "TOCVP_BENCH_STUB"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [json.loads(l) for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout[-3000:]
    return lines[0]


@pytest.mark.gpu
def test_bench_plain_run_is_the_headline_alone(tmp_path):
    import numpy as np
    B, K = 2, 2
    line = _bench("--gpus", "1", "--batch", str(B), "--steps", str(K), "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert all(k in line for k in HEADLINE), sorted(line)
    assert not [k for k in FULL_ONLY if k in line], sorted(line)
    assert line["steps"] == K and line["warmup"] == 1 and line["gathered_rows"] == K * B
    assert line["value"] > 0 and line["higher_is_better"] is True
    assert abs(line["value"] * line["ms_per_step"] / 1e3 - B * 19) < 0.01 * B * 19
    psnr = np.load(tmp_path / "psnr.npy")
    assert psnr.shape == (B, 19) and np.isfinite(psnr).all()
    assert np.load(tmp_path / "pred_imgs.npy").shape == (B, 19, 3, 64, 64)


@pytest.mark.gpu
def test_bench_full_run_adds_the_second_region_and_roofline():
    line = _bench("--gpus", "1", "--batch", "2", "--steps", "2", "--warmup", "1", "--full", "--no-extra",
                  "--no-cpu-baseline")
    assert all(k in line for k in HEADLINE), sorted(line)
    assert line["value_no_overlap"] > 0 and line["ms_per_step_no_overlap"] > 0
    assert line["roofline"]["launches"] > 0 and line["roofline"]["achieved"] > 0
    assert line["rooflines"][0] == line["roofline"]
    assert "extra" not in line and "cpu_baseline" not in line
