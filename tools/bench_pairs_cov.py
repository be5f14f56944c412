#!/usr/bin/env python3
"""Time per `update` of the fitter's "pairs given" flavour (gingr_fitter_update_pairs_async) with ONE PAIR PER VERTEX on a hull of M
points (an ellipsoid; the target is the hull displaced, the covariances are normal / tangent: variance 0.25 along the hull's normal,
25 across it -- point-to-plane ICP), for the three routes a pair list can take:
  isotropic_us          (a) gingr_fitter_set_pairs, var = 1: the weighted Gram pass
  cov_landmark_us       (b) gingr_fitter_set_pairs_cov: the covariances through the landmark pass, O(K r^2)
  cov_gram_us           (c) gingr_fitter_set_pairs_cov_dense: the covariances through the 3 x 3-weighted Gram pass
  set_dense_alone_us    the consolidation call of (c) by itself
  landmark_over_gram    (b) / (c)
and, with --kernel-stats (a fresh child under rocprofv3, kernel trace alone), the kernel time of the new pass beside the isotropic Gram
pass of the same model, with one read of the basis at 6.29 TB/s and the MFMA floor of the symmetric product at 78.6 TFLOP/s.
Writes profiles/pairs_cov_gram_<M>_<rank>.json and prints it as one JSON line; no pass / fail threshold.
    usage: bench_pairs_cov.py [M] [rank] [--kernel-stats]"""
import csv, glob, json, os, statistics, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STREAM_BYTES_PER_S, MFMA_FLOPS = 6.29e12, 78.6e12


def hull(M, seed=5):
    """(points on the ellipsoid 50 (1, 0.7, 0.5), unit normals there, the target: the hull grown by 2 along its normals and moved)"""
    rng = np.random.default_rng(seed)
    axes = 50.0 * np.array([1.0, 0.7, 0.5])
    d = rng.normal(0, 1, (M, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    pts = d * axes
    n = pts / (axes * axes)
    n /= np.linalg.norm(n, axis=1)[:, None]
    return pts, n, pts + 2.0 * n + np.array([0.5, -0.3, 0.2]) + rng.normal(0, 0.1, (M, 3))


def setup(M, rank):
    import torch  # noqa: F401
    import gingr_amd as ga
    from gingr_amd.sharded import ShardedFitter
    from bench import synth_gpmm
    y, normals, x = hull(M)
    basis, lam = synth_gpmm(y, rank)
    ctx = ga.Context(0)
    f = ShardedFitter(ctx, ga.PointDistributionModel(y, np.zeros_like(y), basis, lam), x)
    covs = np.ascontiguousarray(ga.normalTangentCovariances(normals, 0.25, 25.0))
    return ctx, f, np.arange(M, dtype=np.int32), np.ascontiguousarray(x), covs


def calls(ctx, f):
    from gingr_amd._native import dptr, iptr
    from gingr_amd.api import _check
    lib, h = f._lib, f.handle

    def setter(name):
        def go(pids, pts, third):
            k = pids.shape[0]
            _check(ctx.handle, getattr(lib, name)(h, k, iptr(pids) if k else None, dptr(pts) if k else None, dptr(third) if k else None), name)
        return go

    def update(n):
        _check(ctx.handle, lib.gingr_fitter_update_pairs_async(h, n), "gingr_fitter_update_pairs_async")
    return setter("gingr_fitter_set_pairs"), setter("gingr_fitter_set_pairs_cov"), setter("gingr_fitter_set_pairs_cov_dense"), update


def measure(M, rank):
    ctx, f, pids, pts, covs = setup(M, rank)
    set_iso, set_cov, set_dense, update = calls(ctx, f)
    none = (np.zeros(0, dtype=np.int32), np.zeros((0, 3)), np.zeros(0))

    def timed(step, n, repeats):
        """median and minimum over `repeats` of the time per iteration of n back-to-back iterations, from the same state"""
        out = []
        for _ in range(repeats):
            f.set_state(np.zeros(rank), 1.0)
            ctx.synchronize()
            t0 = time.perf_counter()
            step(n)
            ctx.synchronize()
            out.append((time.perf_counter() - t0) / n * 1e6)
        return statistics.median(out), min(out)

    res = {"what": "time per update of the pairs flavour, one pair per vertex on a hull, normal / tangent covariances", "points": M, "rank": rank}
    fits = {}
    for key, setter, third, n, repeats in (("isotropic", set_iso, np.ones(M), 20, 5), ("cov_gram", set_dense, covs, 20, 5),
                                           ("cov_landmark", set_cov, covs, 2, 3)):
        setter(pids, pts, third)
        f.set_state(np.zeros(rank), 1.0)
        update(1)                                                   # warm-up
        res[key + "_us"], res[key + "_us_min"] = timed(update, n, repeats)
        f.set_state(np.zeros(rank), 1.0)
        update(1)
        _, sc, fit = f.get_state()
        res[key + "_status"] = int(sc.status)
        fits[key] = fit
        if key == "cov_gram":
            res["set_dense_alone_us"], res["set_dense_alone_us_min"] = timed(lambda k: [setter(pids, pts, third) for _ in range(k)], 5, 5)
        setter(*none)
    res["landmark_over_gram"] = res["cov_landmark_us"] / res["cov_gram_us"]
    res["gram_against_landmark_rel_fit"] = float(np.linalg.norm(fits["cov_gram"] - fits["cov_landmark"]) / np.linalg.norm(fits["cov_landmark"]))
    rp = -(-rank // 16) * 16
    res["basis_read_floor_us"] = 3 * M * rp * 8 / STREAM_BYTES_PER_S * 1e6
    res["mfma_floor_us"] = 3 * M * rp * (rp + 1) / MFMA_FLOPS * 1e6    # the upper triangle of a symmetric product: rp (rp + 1) / 2 entries, 2 flops per row
    f.close()
    ctx.close()
    return res


def passes_only(M, rank, iterations=10):
    """the child of --kernel-stats: `iterations` updates on the isotropic list, then as many on the dense covariance list"""
    ctx, f, pids, pts, covs = setup(M, rank)
    set_iso, _, set_dense, update = calls(ctx, f)
    set_iso(pids, pts, np.ones(M))
    f.set_state(np.zeros(rank), 1.0)
    update(iterations)
    set_iso(np.zeros(0, dtype=np.int32), np.zeros((0, 3)), np.zeros(0))
    set_dense(pids, pts, covs)
    f.set_state(np.zeros(rank), 1.0)
    update(iterations)
    ctx.synchronize()
    f.close()
    ctx.close()


def kernel_stats(M, rank):
    """a fresh child under rocprofv3 (kernel trace alone), then the stats table: the Gram and observation kernels of the two passes"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "pairs_cov", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), str(M), str(rank), "--passes-only"]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, cwd=tmp, timeout=900)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None
        rows = list(csv.DictReader(open(files[0])))
    keep = ("gram", "cov_obs", "obs_points", "phase1_finalize")
    return [{"kernel": r["Name"][:96], "calls": int(r["Calls"]), "average_us": float(r["AverageNs"]) / 1e3,
             "total_ms": float(r["TotalDurationNs"]) / 1e6} for r in rows if any(k in r["Name"] for k in keep)]


if __name__ == "__main__":
    nums = [int(a) for a in sys.argv[1:] if not a.startswith("--")]
    flags = [a for a in sys.argv[1:] if a.startswith("--")]
    M = nums[0] if len(nums) > 0 else 50000
    rank = nums[1] if len(nums) > 1 else 100
    if "--passes-only" in flags:
        passes_only(M, rank)
        sys.exit(0)
    out = measure(M, rank)
    out["kernel_stats"] = kernel_stats(M, rank) if "--kernel-stats" in flags else "not measured"
    path = os.path.join(ROOT, "profiles", f"pairs_cov_gram_{M}_{rank}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
