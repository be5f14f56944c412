#!/usr/bin/env python3
"""Global rigid pre-alignment (Context.rigid_search: S start poses x K iterations of trimmed ICP in one call), timed on an asymmetric
closed shape of M template points against N target points of the same shape under a random rigid motion; one run, same process,
same device:
  batched_us        the call, from call to return (uploads, k-d order and grid of the target, S x (K + 1) passes, one read-back)
  sequential_us     the route it replaces: S rigid-ICP tasks (gingr_rigid_icp_create, K iterations, destroy) one after another, each from
                    its start pose; sequential_iterate_us is the share of gingr_rigid_icp_iterate alone (one read-back per iteration)
  host_us           the numpy / scipy.spatial.cKDTree restatement (tests/rigid_search_restatement.py) on the host
  split             HIP-event time of one more call by stage (gingr_ctx_timing_*): search (grid kernel and masked tile scan), selection,
                    sums, the rest (pose, step and argmin kernels); what is left of the call is host work, transfers and launch gaps
Each figure is the median over 5 timed blocks after a warm-up (the minimum beside it; the host restatement: 3 blocks).  Writes
profiles/rigid_search_<M>_<N>_<S>_<K>.json and prints it as a JSON line; no pass / fail threshold.
    usage: bench_rigid_search.py [M] [N] [S] [K] [overlap]"""
import json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shape(n, seed):
    """n points of a bumpy ellipsoid without a symmetry (jittered Fibonacci directions)"""
    rng = np.random.default_rng(seed)
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * np.pi * (3.0 - np.sqrt(5.0)) + rng.uniform(0, 0.3, n)
    u = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], axis=1)
    r = 1.0 + 0.35 * u[:, 0] + 0.25 * u[:, 1] * u[:, 2] + 0.2 * np.sin(3.0 * u[:, 2] + u[:, 0])
    return u * r[:, None] * [120.0, 45.0, 30.0]


def wall(fn, repeats=5):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out), min(out)


def measure(M, N, S, K, rho):
    import torch  # noqa: F401
    import gingr_amd as ga
    from gingr_amd import classic
    from gingr_amd.api import _check
    from tests import rigid_search_restatement as rs
    X = shape(M, 1)
    rng = np.random.default_rng(2)
    R_true = rs.random_rotation(rng)
    Y = np.ascontiguousarray(shape(N, 3) @ R_true.T + rng.normal(size=3) * 100.0)
    ctx = ga.Context(0)
    R0 = ctx.rotation_samples(S)
    res = {"what": "batched multi-start trimmed ICP against S sequential rigid-ICP tasks and the host restatement; one run",
           "moving_points": M, "target_points": N, "starts": S, "iterations": K, "overlap": rho}
    out = ctx.rigid_search(X, Y, R0, K, rho)                                   # warm-up
    res["batched_us"], res["batched_us_min"] = wall(lambda: ctx.rigid_search(X, Y, R0, K, rho))
    res["best"], res["score"] = out.best, out.score
    res["degrees_from_truth"] = rs.angle_deg(out.R, R_true)

    starts = [X @ R.T + t for R, t in rs.start_poses(X, Y, R0)]
    lib = ctx._lib
    spent = {"iterate": 0.0}

    def sequential():
        spent["iterate"] = 0.0
        for p in starts:
            task = classic.ICPFactory(ctx, p).registerRigidly(Y)
            t0 = time.perf_counter()
            _check(ctx.handle, lib.gingr_rigid_icp_iterate(task._h, K, None), "gingr_rigid_icp_iterate")
            spent["iterate"] += (time.perf_counter() - t0) * 1e6
            task.close()

    sequential()                                                               # warm-up
    shares = []

    def sequential_timed():
        sequential()
        shares.append(spent["iterate"])

    res["sequential_us"], res["sequential_us_min"] = wall(sequential_timed)
    res["sequential_iterate_us"] = statistics.median(shares)
    res["sequential_over_batched"] = res["sequential_us"] / res["batched_us"]
    res["sequential_iterate_over_batched"] = res["sequential_iterate_us"] / res["batched_us"]
    if rho < 1.0:
        res["note"] = "the sequential tasks do not trim: their time stands for the untrimmed route"

    host = {}

    def restatement():
        host["res"] = rs.search(X, Y, R0, K, rho)

    res["host_us"], res["host_us_min"] = wall(restatement, 3)
    res["host_over_batched"] = res["host_us"] / res["batched_us"]
    res["host_best"] = host["res"]["best"]
    res["score_relative_to_host"] = float(np.abs(out.scores / host["res"]["scores"] - 1.0).max())

    ctx.timing_enable(True)
    ctx.timing_reset()
    ctx.rigid_search(X, Y, R0, K, rho)
    ctx.synchronize()
    split = {}
    for name, which in (("search", 8), ("selection", 24), ("sums", 25), ("rest", 26)):
        ms, n = ctx.timing_read(which)
        split[name + "_us"], split[name + "_launches"] = ms * 1e3, n
    ctx.timing_enable(False)
    split["device_total_us"] = sum(v for k, v in split.items() if k.endswith("_us"))
    res["split"] = split
    ctx.close()
    return res


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if not x.startswith("--")]
    M = int(args[0]) if len(args) > 0 else 2000
    N = int(args[1]) if len(args) > 1 else 50000
    S = int(args[2]) if len(args) > 2 else 64
    K = int(args[3]) if len(args) > 3 else 10
    rho = float(args[4]) if len(args) > 4 else 1.0
    res = measure(M, N, S, K, rho)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", f"rigid_search_{M}_{N}_{S}_{K}.json"), "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
