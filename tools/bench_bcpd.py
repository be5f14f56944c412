#!/usr/bin/env python3
"""Iteration time of the Bayesian coherent point drift (classic.BCPD, csrc/bcpd.hip) next to the non-rigid classic CPD at the same
size: host clock around synchronised iterations after a warm-up, and -- with --kernel-stats, in a run of its own -- the split by kernel
from `rocprofv3 --kernel-trace --stats`.  M = 1622 is the femur pair of tests/golden, any other size a jittered grid with a warped,
rotated, scaled target.  Writes profiles/bcpd_<M>.json.
    PYTHONPATH=. python tools/bench_bcpd.py [M] [N] [iterations] [--kernel-stats]"""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clouds(M, N):
    if M == 1622:
        d = np.load(os.path.join(ROOT, "tests", "golden", "inputs.npz"))
        Y, X = d["femur"].astype(np.float64), d["femur_target"].astype(np.float64)
        return "femur", Y, X[:N] if N else X, 30.0
    rng = np.random.default_rng(M)
    g = int(np.ceil(M ** (1.0 / 3.0)))
    ax = np.arange(g, dtype=float)
    Y = (np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3) + rng.normal(0, 0.25, (g ** 3, 3)))[rng.permutation(g ** 3)[:M]]
    c, s = np.cos(0.2), np.sin(0.2)
    X = 1.1 * (Y + 0.3 * np.sin(0.7 * Y[:, (1, 2, 0)])) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]).T + np.array([0.5, -0.3, 0.2])
    X = X[rng.permutation(M)[:N or M]] + rng.normal(0, 0.02, (N or M, 3))
    return f"grid {M}", Y, X, 1.5


def measure(M, N, iterations):
    import torch  # noqa: F401  (first: one HIP runtime per process)
    import gingr_amd as ga
    from gingr_amd import classic as cl
    name, Y, X, beta = clouds(M, N)
    ctx = ga.Context(0)
    row = {"case": name, "M": int(Y.shape[0]), "N": int(X.shape[0]), "iterations": iterations, "beta": beta}
    reg = cl.BCPD(ctx, Y, X, w=0.1, lambda_=10.0, gamma=0.3, k=1.0, beta=beta)
    reg._lib.gingr_bcpd_iterate(reg._h, 2)                      # warm-up: code objects
    reg.reset()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(iterations):
        reg._lib.gingr_bcpd_iterate(reg._h, 1)                   # synchronises
    row["bcpd_ms_per_iteration"] = (time.perf_counter() - t0) / iterations * 1e3
    row["bcpd_sigma2"], row["bcpd_s"] = reg.sigma2(), reg.transform()[0]
    reg.close()
    cpd = cl.CPDFactory(ctx, Y, lambda_=2.0, beta=beta, w=0.1).registerNonRigidly(X)
    cpd._lib.gingr_classic_cpd_iterate(cpd._h, 2)
    cpd.set_state(Y, cpd._sigma2_init)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(iterations):
        cpd._lib.gingr_classic_cpd_iterate(cpd._h, 1)
    row["nonrigid_cpd_ms_per_iteration"] = (time.perf_counter() - t0) / iterations * 1e3
    cpd.close()
    ctx.close()
    return row


def kernel_stats(M, N, iterations):
    """a fresh child under rocprofv3 (kernel trace alone), then the stats table: the kernels of the BCPD iteration by total time"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "bcpd", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), str(M), str(N), str(iterations), "--bcpd-only"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, cwd=tmp, timeout=900)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None
        rows = list(csv.DictReader(open(files[0])))
    return [{"kernel": r["Name"][:96], "calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3,
             "total_ms": float(r["TotalDurationNs"]) / 1e6, "percent": float(r["Percentage"])} for r in rows[:16]]


def bcpd_only(M, N, iterations):
    import torch  # noqa: F401
    import gingr_amd as ga
    from gingr_amd import classic as cl
    _, Y, X, beta = clouds(M, N)
    ctx = ga.Context(0)
    reg = cl.BCPD(ctx, Y, X, w=0.1, lambda_=10.0, gamma=0.3, k=1.0, beta=beta)
    reg._lib.gingr_bcpd_iterate(reg._h, iterations)
    reg.close()
    ctx.close()


if __name__ == "__main__":
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    nums = [int(a) for a in sys.argv[1:] if not a.startswith("--")]
    M = nums[0] if len(nums) > 0 else 1622
    N = nums[1] if len(nums) > 1 else 0
    iterations = nums[2] if len(nums) > 2 else 10
    if "--bcpd-only" in flags:
        bcpd_only(M, N, iterations)
        sys.exit(0)
    out = measure(M, N, iterations)
    out["kernel_stats"] = kernel_stats(M, N, iterations) if "--kernel-stats" in flags else "not measured"
    path = os.path.join(ROOT, "profiles", f"bcpd_{M}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
