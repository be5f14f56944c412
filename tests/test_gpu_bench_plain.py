"""A plain `bench.py` run (no --full): it times exactly the K steps it is given, prints the headline fields and nothing that needs
runs of its own, and with --dump-outputs writes the state the last timed step ended in."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_times_k_steps_and_dumps_the_last_state(tmp_path):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GINGR_BENCH_SHARED_DEVICE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--points", "6000",
                        "--rank", "40", "--dump-outputs", str(tmp_path)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])
    assert out["valid"] is True, out["reason"]
    assert out["steps"] == 5 and out["warmup"] == 2 and out["timing"]["blocks"] == 1
    assert out["ms_per_step"] > 0.0 and out["value"] == pytest.approx(1e3 / out["ms_per_step"])
    assert out["unit"] == "iterations/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    for k in ("sustained", "roofline", "parity_check", "cpu_baseline", "exchange"):
        assert out[k] is None, k
    assert out["kernels"] == []
    got = {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}
    assert {"alpha", "fit", "sigma2", "translation", "euler", "iteration", "status"} <= set(got)
    assert all(v.dtype == np.float64 for v in got.values())
    assert got["alpha"].shape == (40,) and got["fit"].shape == (6000, 3) and np.all(np.isfinite(got["fit"]))
    assert got["iteration"] == 2 + 5 and got["status"] == 0
    assert got["sigma2"] == out["sigma2_after_timed_steps"]
