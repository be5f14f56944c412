"""Timing of a resident model localized (gingr_model_localize): the whole call to the finalized model, and the pivot step alone
(device timer 21, HIP events on the context's stream around every step launch) with the factor's column count and residual.  Beside
the step goes its bound: step k reads the k factor columns and the r basis columns over the 3M entries, sum_k (r + k) * 3M * 8
bytes, at the bandwidth a streaming copy reaches on an MI355X.  No host route is timed: a dense 3M x 3M covariance does not exist at
this size.  The source is the leading r components of a Gaussian kernel model on a closed hull (points on an ellipsoid of
400 x 80 x 60 units), given a per-vertex mean displacement so that the model's row order is not the caller's.
Writes profiles/localize_model_<M>_<r>.json and prints the same document.  Not the benchmark metric.
Usage: python tools/bench_localize_model.py [M] [r] [sigma] [tol]      (defaults 50000, 8, 60, 0.01)"""
import datetime
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import gingr_amd as ga  # noqa: E402

HBM_BYTES_PER_S = 6.29e12      # a streaming copy on an MI355X (tools/bench_augment_model.py)


def hull(rng, M):
    """M points on the surface of an ellipsoid with semi-axes 200, 40, 30"""
    v = rng.standard_normal((M, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    return v * np.array([200.0, 40.0, 30.0])[None, :]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    r = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    sigma = float(sys.argv[3]) if len(sys.argv) > 3 else 60.0
    tol = float(sys.argv[4]) if len(sys.argv) > 4 else 0.01
    rng = np.random.default_rng(5)
    ref = hull(rng, M)
    ctx = ga.Context(0)
    # the source: the leading r components of a smooth kernel model (as many as the kernel model has, if fewer)
    kernel_model = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=1e-4).Gaussian(sigma=80.0, scaling=30.0)
    host = kernel_model.to_host()
    kernel_model.device().close()
    r = min(r, host.rank)
    src_host = host.truncate(r)
    src_host.mean = rng.normal(0.0, 3.0, (M, 3))
    src = ga.DeviceModel(ctx, src_host)

    # the whole call, to the finalized model: median of three after a warm-up, timers off
    whole = []
    for rep in range(4):
        t0 = time.perf_counter()
        dm = src.localize(sigma, relativeTolerance=tol)
        ctx.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        if rep:
            whole.append(dt)
        info = dm.host.localizeInfo
        dm.close()

    # the pivot step alone: HIP events around every step launch (timer 21), median of three calls each read on its own
    ctx.timing_enable(True)
    step_ms, launches = [], []
    for rep in range(3):
        ctx.timing_reset()
        src.localize(sigma, relativeTolerance=tol).close()
        ms, n = ctx.timing_read(21)
        step_ms.append(ms)
        launches.append(int(n))
    ctx.timing_enable(False)

    cols = info.columns
    bound_bytes = sum((r + k) * 3.0 * M * 8.0 for k in range(cols))
    bound_ms = 1e3 * bound_bytes / HBM_BYTES_PER_S
    out = {"command": "python tools/bench_localize_model.py " + " ".join(sys.argv[1:]), "machines": "1 x MI355X",
           "date": datetime.date.today().isoformat(), "M": M, "source_rank": r, "sigma": sigma, "relative_tolerance": tol,
           "columns": cols, "rank": info.rank, "tolerance_reached": info.tolerance_reached, "residual_fraction": info.residual_fraction,
           "total_variance": info.total_variance, "kept_variance": info.kept_variance,
           "whole_call_ms": {"median": median(whole), "min": min(whole), "max": max(whole)},
           # (the launches include the up to fifteen behind the stop that return at once: the driver looks at the flag every sixteen steps)
           "pivot_step_all_launches_ms": {"median": median(step_ms), "all": step_ms, "launches": median(launches)},
           "pivot_step_us_per_column": 1e3 * median(step_ms) / cols,
           "pivot_step_bound": {"gigabytes": bound_bytes / 1e9, "hbm_bytes_per_s": HBM_BYTES_PER_S, "ms": bound_ms,
                                "measured_over_bound": median(step_ms) / bound_ms}}
    path = os.path.join(ROOT, "profiles", f"localize_model_{M}_{r}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    src.close()


if __name__ == "__main__":
    main()
