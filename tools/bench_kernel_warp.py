#!/usr/bin/env python3
"""The kernel warp (csrc/kernel_warp.hip; RigidCPD.transformPoints / BCPD.transformPoints): P query points through the fitted map of a
task over M template points.  One run: the call (host clock around one synchronising call after a warm-up call: upload, pass,
download), the pass alone (`rocprofv3 --kernel-trace --stats` around a child of its own), pairs/s against the bound of 17 float64
VALU instructions per pair, and the host route it replaces: exp(-cdist^2 / 2 beta^2) @ W in numpy, blocked, on 16 threads (timed on
--host-queries of the queries and scaled to P).  Writes profiles/kernel_warp_<P>x<M>.json.
    PYTHONPATH=. python tools/bench_kernel_warp.py [P] [M] [--lowrank] [--host-queries Q] [--no-kernel-stats]
Defaults: 1 000 000 x 5 000 (a dense non-rigid CPD task); with --lowrank the task is the low-rank one (100 000 x 50 000 is the size
past the dense routes)."""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BOUND_PAIRS_PER_S = 2.7e12 * 15 / 17        # 2.7e12 pairs/s at 15 f64 VALU instructions per pair and 2.4 GHz
HOST_THREADS, HOST_BLOCK = 16, 512


def clouds(P, M):
    """template: a jittered grid; target: a quarter of it (at most 5 000 points) warped, rotated, scaled; queries: uniform in its box"""
    rng = np.random.default_rng(M)
    g = int(np.ceil(M ** (1.0 / 3.0)))
    ax = np.arange(g, dtype=float)
    Y = (np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3) + rng.normal(0, 0.25, (g ** 3, 3)))[rng.permutation(g ** 3)[:M]]
    c, s = np.cos(0.2), np.sin(0.2)
    N = min(5000, max(1, M // 4))
    X = 1.1 * (Y + 0.3 * np.sin(0.7 * Y[:, (1, 2, 0)])) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]).T + np.array([0.5, -0.3, 0.2])
    X = X[rng.permutation(M)[:N]] + rng.normal(0, 0.02, (N, 3))
    Z = rng.uniform(Y.min(0), Y.max(0), (P, 3))
    return Y, X, Z, 1.5


def task(ctx, Y, X, beta, lowrank):
    from gingr_amd import classic as cl
    reg = cl.CPDFactory(ctx, Y, lambda_=2.0, beta=beta, w=0.1).registerNonRigidly(X, cl.LowRankG(1e-4) if lowrank else None)
    reg.Iteration()
    return reg


def host_route(Z, Y, W, beta):
    def block(p0):
        z = Z[p0:p0 + HOST_BLOCK]
        d2 = (z * z).sum(1)[:, None] - 2.0 * (z @ Y.T) + (Y * Y).sum(1)[None, :]
        return z + np.exp(np.maximum(d2, 0.0) / (-2.0 * beta * beta)) @ W
    with ThreadPoolExecutor(HOST_THREADS) as ex:
        return np.concatenate(list(ex.map(block, range(0, Z.shape[0], HOST_BLOCK))))


def measure(P, M, lowrank, host_queries):
    import torch  # noqa: F401  (first: one HIP runtime per process)
    import gingr_amd as ga
    Y, X, Z, beta = clouds(P, M)
    ctx = ga.Context(0)
    reg = task(ctx, Y, X, beta, lowrank)
    row = {"P": P, "M": M, "task": "non-rigid CPD, " + (f"low-rank ({reg.lowRankInfo['columns']} columns)" if lowrank else "dense"), "beta": beta}
    reg.transformPoints(Z[:1024])                                # warm-up: code objects, the centres' extent
    reg.transformPoints(Z)                                       # ... and the buffers of the full size
    ctx.synchronize()
    t0 = time.perf_counter()
    out = reg.transformPoints(Z)                                 # synchronises
    row["call_ms"] = (time.perf_counter() - t0) * 1e3
    W = reg.W()
    q = min(P, host_queries)
    t0 = time.perf_counter()
    ref = host_route(Z[:q], Y, W, beta)
    host = time.perf_counter() - t0
    row["host_numpy_ms"] = host * 1e3 * P / q
    row["host_numpy_note"] = f"{HOST_THREADS} threads, blocks of {HOST_BLOCK} queries, timed on {q} queries and scaled to P"
    row["max_abs_difference_from_host"] = float(np.abs(out[:q] - ref).max())
    reg.close()
    ctx.close()
    return row


def warp_only(P, M, lowrank):
    import torch  # noqa: F401
    import gingr_amd as ga
    Y, X, Z, beta = clouds(P, M)
    ctx = ga.Context(0)
    reg = task(ctx, Y, X, beta, lowrank)
    reg.transformPoints(Z)
    reg.close()
    ctx.close()


def kernel_stats(P, M, lowrank):
    """a fresh child under rocprofv3 (kernel trace alone): one call of the full size; the two kernels of the pass"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "warp", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), str(P), str(M), "--warp-only"] + (["--lowrank"] if lowrank else [])
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, cwd=tmp, timeout=900)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None
        rows = [r for r in csv.DictReader(open(files[0])) if "kernel_warp" in r["Name"]]
    return [{"kernel": r["Name"][:96], "calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6} for r in rows]


if __name__ == "__main__":
    argv = sys.argv[1:]
    host_queries = 20000
    if "--host-queries" in argv:
        i = argv.index("--host-queries")
        host_queries = int(argv[i + 1])
        del argv[i:i + 2]
    nums = [int(a) for a in argv if not a.startswith("--")]
    P = nums[0] if len(nums) > 0 else 1000000
    M = nums[1] if len(nums) > 1 else 5000
    lowrank = "--lowrank" in argv
    if "--warp-only" in argv:
        warp_only(P, M, lowrank)
        sys.exit(0)
    out = measure(P, M, lowrank, host_queries)
    out["bound_pairs_per_s"] = BOUND_PAIRS_PER_S
    stats = None if "--no-kernel-stats" in argv else kernel_stats(P, M, lowrank)
    if stats:
        pair = sum(r["total_ms"] for r in stats if "finish" not in r["kernel"])
        out["kernel_stats"] = stats
        out["pass_ms"], out["finish_ms"] = pair, sum(r["total_ms"] for r in stats if "finish" in r["kernel"])
        out["pairs_per_s"] = P * M / (pair * 1e-3)
        out["fraction_of_bound"] = out["pairs_per_s"] / BOUND_PAIRS_PER_S
    else:
        out["kernel_stats"] = out["pairs_per_s"] = "not measured"
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", f"kernel_warp_{P}x{M}.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
