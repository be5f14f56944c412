#!/usr/bin/env python3
"""Iteration time of the Bayesian coherent point drift (classic.BCPD, csrc/bcpd.hip) next to the non-rigid classic CPD at the same
size: host clock around synchronised iterations after a warm-up, and -- with --kernel-stats, in a run of its own -- the split by kernel
from `rocprofv3 --kernel-trace --stats`.  M = 1622 is the femur pair of tests/golden, any other size a jittered grid with a warped,
rotated, scaled target.  Writes profiles/bcpd_<M>.json.
    PYTHONPATH=. python tools/bench_bcpd.py [M] [N] [iterations] [--kernel-stats]

--lowrank TOL [--max-columns K] [--beta B] measures the low-rank route (csrc/bcpd_lowrank.hip) instead: the create time (the pivoted
Cholesky of the kernel matrix), then every timed iteration from the same state (the one two iterations leave, injected again before
each), with the dense route beside it from that state where it can run (M <= 32768); --kernel-stats adds the kernels of the low-rank
iteration and their sums by step (E: soft assignment, deformation, rest).  Writes profiles/bcpd_lowrank_<M>[_k<K>].json."""
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

PARAMS = dict(w=0.1, lambda_=10.0, gamma=0.3, k=1.0)
DENSE_LIMIT = 32768
E_KERNELS = ("absmax", "bcpd_weights", "bcpd_colsum", "bcpd_den_finalize", "bcpd_rowstats", "bcpd_rows_finish")
DEFORMATION_KERNELS = ("lowrank_gram", "lowrank_reduce", "spd_system", "chol_", "bcpd_forward", "bcpd_lowrank_deform")
REST_KERNELS = ("bcpd_sums_", "bcpd_means_finish", "bcpd_alpha", "bcpd_similarity", "bcpd_shape", "bcpd_variance")


def clouds(M, N, beta=None):
    if M == 1622:
        d = np.load(os.path.join(ROOT, "tests", "golden", "inputs.npz"))
        Y, X = d["femur"].astype(np.float64), d["femur_target"].astype(np.float64)
        return "femur", Y, X[:N] if N else X, beta or 30.0
    rng = np.random.default_rng(M)
    g = int(np.ceil(M ** (1.0 / 3.0)))
    ax = np.arange(g, dtype=float)
    Y = (np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3) + rng.normal(0, 0.25, (g ** 3, 3)))[rng.permutation(g ** 3)[:M]]
    c, s = np.cos(0.2), np.sin(0.2)
    X = 1.1 * (Y + 0.3 * np.sin(0.7 * Y[:, (1, 2, 0)])) @ np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]).T + np.array([0.5, -0.3, 0.2])
    X = X[rng.permutation(M)[:N or M]] + rng.normal(0, 0.02, (N or M, 3))
    return f"grid {M}", Y, X, beta or 1.5


def measure(M, N, iterations):
    import torch  # noqa: F401  (first: one HIP runtime per process)
    import gingr_amd as ga
    from gingr_amd import classic as cl
    name, Y, X, beta = clouds(M, N)
    ctx = ga.Context(0)
    row = {"case": name, "M": int(Y.shape[0]), "N": int(X.shape[0]), "iterations": iterations, "beta": beta}
    reg = cl.BCPD(ctx, Y, X, beta=beta, **PARAMS)
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


def timed_from(ctx, reg, st, iterations):
    """ms of one iteration, each from the state `st` (median and minimum over `iterations`)"""
    t = []
    for _ in range(iterations):
        reg.set_state(st["yhat"], st["sigma_diag"], st["alpha"], st["s"], st["R"], st["t"], st["sigma2"])
        ctx.synchronize()
        t0 = time.perf_counter()
        reg._lib.gingr_bcpd_iterate(reg._h, 1)                   # synchronises
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(min(t))


def measure_lowrank(M, N, iterations, tol, max_columns, beta):
    import torch  # noqa: F401
    import gingr_amd as ga
    from gingr_amd import classic as cl
    name, Y, X, beta = clouds(M, N, beta)
    ctx = ga.Context(0)
    row = {"case": name, "M": int(Y.shape[0]), "N": int(X.shape[0]), "iterations": iterations, "beta": beta, "tolerance": tol,
           "max_columns": max_columns}
    cl.BCPD(ctx, Y[:64], X[:64], beta=beta, lowRank=cl.LowRankG(tol, max_columns), **PARAMS).close()   # code objects of the factor build
    ctx.synchronize()
    t0 = time.perf_counter()
    reg = cl.BCPD(ctx, Y, X, beta=beta, lowRank=cl.LowRankG(tol, max_columns), **PARAMS)
    row["create_ms"] = (time.perf_counter() - t0) * 1e3
    row.update(reg.lowRankInfo)
    reg._lib.gingr_bcpd_iterate(reg._h, 2)                      # warm-up; the state every timed iteration starts from
    st = reg.state()
    row["lowrank_ms_per_iteration"], row["lowrank_ms_per_iteration_min"] = timed_from(ctx, reg, st, iterations)
    low = reg.state()
    reg.close()
    if Y.shape[0] <= DENSE_LIMIT:
        dense = cl.BCPD(ctx, Y, X, beta=beta, **PARAMS)
        dense._lib.gingr_bcpd_iterate(dense._h, 1)
        row["dense_ms_per_iteration"], row["dense_ms_per_iteration_min"] = timed_from(ctx, dense, st, max(2, min(iterations, 5)))
        den = dense.state()
        dense.close()
        row["distance_from_dense"] = {"yhat": float(np.linalg.norm(low["yhat"] - den["yhat"]) / np.linalg.norm(den["yhat"])),
                                      "sigma2": abs(low["sigma2"] - den["sigma2"]) / den["sigma2"]}
    else:
        row["dense_ms_per_iteration"] = "refused: M > 32768"
    ctx.close()
    return row


def kernel_stats(M, N, iterations, extra=()):
    """a fresh child under rocprofv3 (kernel trace alone), then the stats table: the kernels of the BCPD iteration by total time"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "bcpd", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), str(M), str(N), str(iterations), "--bcpd-only", *extra]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, cwd=tmp, timeout=900)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None
        rows = list(csv.DictReader(open(files[0])))
    return [{"kernel": r["Name"][:96], "calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3,
             "total_ms": float(r["TotalDurationNs"]) / 1e6, "percent": float(r["Percentage"])} for r in rows[:16 if not extra else 64]]


def steps_of(stats, iterations):
    """ms per iteration of the three parts of the low-rank iteration, from the kernel table (kernels of the create are left out)"""
    out = {"E": 0.0, "deformation": 0.0, "rest": 0.0}
    for r in stats or []:
        for step, names in (("E", E_KERNELS), ("deformation", DEFORMATION_KERNELS), ("rest", REST_KERNELS)):
            if any(n in r["kernel"] for n in names):
                out[step] += r["total_ms"] / iterations
                break
    return out


def bcpd_only(M, N, iterations, lowrank=None, beta=None):
    import torch  # noqa: F401
    import gingr_amd as ga
    from gingr_amd import classic as cl
    _, Y, X, beta = clouds(M, N, beta)
    ctx = ga.Context(0)
    reg = cl.BCPD(ctx, Y, X, beta=beta, lowRank=None if lowrank is None else cl.LowRankG(*lowrank), **PARAMS)
    reg._lib.gingr_bcpd_iterate(reg._h, iterations)
    reg.close()
    ctx.close()


def arguments(argv):
    """(numbers, flags, {option: value}) -- --lowrank, --max-columns and --beta take a value"""
    valued, nums, flags, opts = ("--lowrank", "--max-columns", "--beta"), [], [], {}
    it = iter(argv)
    for a in it:
        if a in valued:
            opts[a] = next(it)
        elif a.startswith("--"):
            flags.append(a)
        else:
            nums.append(int(a))
    return nums, flags, opts


if __name__ == "__main__":
    nums, flags, opts = arguments(sys.argv[1:])
    M = nums[0] if len(nums) > 0 else 1622
    N = nums[1] if len(nums) > 1 else 0
    iterations = nums[2] if len(nums) > 2 else 10
    beta = float(opts["--beta"]) if "--beta" in opts else None
    lowrank = (float(opts["--lowrank"]), int(opts.get("--max-columns", 0))) if "--lowrank" in opts else None
    if "--bcpd-only" in flags:
        bcpd_only(M, N, iterations, lowrank, beta)
        sys.exit(0)
    if lowrank is None:
        out = measure(M, N, iterations)
        out["kernel_stats"] = kernel_stats(M, N, iterations) if "--kernel-stats" in flags else "not measured"
        path = os.path.join(ROOT, "profiles", f"bcpd_{M}.json")
    else:
        out = measure_lowrank(M, N, iterations, lowrank[0], lowrank[1], beta)
        if "--kernel-stats" in flags:
            extra = [a for kv in opts.items() for a in kv]
            out["kernel_stats"] = kernel_stats(M, N, iterations, extra)
            out["ms_per_iteration_by_step"] = steps_of(out["kernel_stats"], iterations)
        else:
            out["kernel_stats"] = "not measured"
        path = os.path.join(ROOT, "profiles", f"bcpd_lowrank_{M}" + (f"_k{lowrank[1]}" if lowrank[1] > 0 else "") + ".json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
