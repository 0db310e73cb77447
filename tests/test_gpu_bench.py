"""bench.py's own contract on the MI355X: a plain run prints the lean headline line, --full adds the per-kernel / roofline /
CPU-baseline figures, --dump-outputs writes what the last timed step computed, the same files from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--batch", "2", "--seconds", "4", "--steps", "3", "--warmup", "1"]
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"}
FULL_ONLY = {"roofline", "layer_roofline", "step_roofline", "kernel_breakdown_ms", "gpu_time_ms_per_step_sum_of_kernels", "cpu_baseline"}
DUMPED = ("loss", "logits", "params", "grads", "bn_running_stats", "features")


def _bench(*args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "SED_DDP_FORCE"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    lines = [ln for ln in p.stdout.decode().splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _load(d):
    return {n: np.load(os.path.join(d, n + ".npy")) for n in DUMPED}


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    r = _bench(*SMALL, "--dump-outputs", a)
    assert HEADLINE <= set(r) and not (FULL_ONLY & set(r)) and r["config"]["comm"] is None
    assert r["steps"] == 3 and r["warmup"] == 1 and r["dtype"] == "bf16" and r["unit"] == "clips/s" and r["higher_is_better"] is True
    assert r["ms_per_step"] > 0 and abs(r["value"] - 2 / (r["ms_per_step"] / 1e3)) < 1e-6 * r["value"]
    oa = _load(a)
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in oa.values())
    assert sum(os.path.getsize(os.path.join(a, n + ".npy")) for n in DUMPED) <= 64 << 20
    assert abs(float(oa["loss"][0]) - r["loss"]) <= 1e-6 * max(1.0, abs(r["loss"]))
    assert oa["logits"].shape[0] == 2 and oa["params"].shape == oa["grads"].shape and oa["features"].shape[:2] == (2, 1)
    assert np.abs(oa["grads"]).max() > 0
    # same arguments, same inputs: a second run computes the same step
    _bench(*SMALL, "--dump-outputs", b)
    ob = _load(b)
    for n in DUMPED:
        np.testing.assert_allclose(ob[n], oa[n], rtol=1e-3, atol=1e-5, err_msg=n)


def test_full_run_keeps_the_per_kernel_and_cpu_figures():
    r = _bench(*SMALL, "--full", "--cpu-seconds", "1")
    assert HEADLINE <= set(r) and FULL_ONLY <= set(r)
    assert r["steps"] == 3 and r["roofline"]["kernel"] in r["kernel_breakdown_ms"] and r["roofline"]["avg_ms"] > 0
    assert r["cpu_baseline"]["value"] > 0 and "peaks_measured" in r["roofline"]
