"""Timing of the model metrics on one MI355X (gingr_model_instances, gingr_model_generalization, gingr_model_specificity) and of the host
route they replace: DeviceModel.coefficients and .instance shape by shape with numpy distances, and -- for the specificity -- a blocked
numpy distance matrix on 16 threads.  Beside the whole calls: the three passes alone (device timers 18, 19, 20: HIP events on the
context's stream) against their own bounds -- the reconstruct-and-measure pass against one read of the basis at the bandwidth a
streaming copy reaches and against its MFMA work at the float64 MFMA peak, the pair pass against its instruction count per pair.
Writes profiles/model_metrics_<M>_<r>_<n>_<S>.json and prints the same document.  Not the benchmark metric.
Usage: python tools/bench_model_metrics.py [M] [r] [n] [S]      (defaults 50000, 100, 100, 1000; n shapes, S samples)"""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import gingr_amd as ga  # noqa: E402

HBM_BYTES_PER_S = 6.29e12      # a streaming copy on an MI355X
F64_MFMA_FLOPS = 78.6e12       # v_mfma_f64_16x16x4_f64 peak
F64_VALU_LANE_OPS = 256 * 4 * 16 * 2.4e9   # one float64 VALU instruction per lane and clock: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz
PAIR_OPS = 8                   # per pair and vertex: 3 subtractions, a multiply, 2 FMAs, a square root (counted once), an add
HOST_THREADS = 16


def pad(r):
    return (r + 15) // 16 * 16


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def timed(call, repeats=3):
    call()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        out.append(1e3 * (time.perf_counter() - t0))
    return {"median": median(out), "min": min(out), "max": max(out)}


def host_generalization(dm, X):
    """the route of today: one coefficients and one instance call per shape, numpy distances"""
    avg = np.empty(X.shape[0])
    for i, x in enumerate(X):
        avg[i] = np.linalg.norm(dm.instance(dm.coefficients(x)) - x, axis=1).mean()
    return avg


def host_specificity(dm, train, A, block=64):
    """one instance call per sample, then the distance matrix in blocks of training shapes on HOST_THREADS threads"""
    samples = np.stack([dm.instance(a) for a in A])

    def one(s):
        best = np.inf
        for j0 in range(0, train.shape[0], block):
            best = min(best, float(np.linalg.norm(train[j0:j0 + block] - s[None], axis=2).mean(axis=1).min()))
        return best
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        return np.array(list(pool.map(one, samples)))


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    r = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 100
    S = int(sys.argv[4]) if len(sys.argv) > 4 else 1000
    rng = np.random.default_rng(5)
    ref = rng.normal(0, 100, (M, 3))
    basis = np.asfortranarray(rng.standard_normal((3 * M, r)) / np.sqrt(3.0 * M))
    model = ga.PointDistributionModel(ref, rng.normal(0, 1, (M, 3)), basis, 64.0 * (0.25 / 64.0) ** (np.arange(r) / max(r - 1, 1)))
    ctx = ga.Context(0)
    dm = ga.DeviceModel(ctx, model)
    A = rng.standard_normal((S, r))
    X = dm.instances(rng.standard_normal((n, r))) + rng.normal(0, 0.5, (n, M, 3))
    ranks = sorted({1, max(1, r // 2), r})
    rp, np_ = pad(r), pad(n)

    whole = {"instances": timed(lambda: dm.instances(A)),
             "generalization_full_rank": timed(lambda: dm.project(X)),
             f"generalization_{len(ranks)}_ranks": timed(lambda: dm.project(X, ranks)),
             "specificity_full_rank": timed(lambda: ga.ModelMetrics.specificity(ctx, dm, X, S, alphas=A))}

    ctx.timing_enable(True)
    kernels = {}
    for name, call, which in (("project_measure_kernel", lambda: dm.project(X, ranks), 18),
                              ("pair_distance_kernel", lambda: ga.ModelMetrics.specificity(ctx, dm, X, S, alphas=A), 19),
                              ("instances_kernel", lambda: dm.instances(A), 20)):
        us, launches = [], 0
        for _ in range(3):
            ctx.timing_reset()
            call()
            ms, launches = ctx.timing_read(which)
            us.append(1e3 * ms)
        kernels[name] = {"us_per_call": median(us), "launches_per_call": int(launches), "all_samples_us": us}
    ctx.timing_enable(False)

    a = kernels["project_measure_kernel"]
    cols = len(ranks) * np_
    a.update(columns=cols, basis_megabytes=24.0 * M * rp / 1e6, gflop=6.0 * M * rp * cols / 1e9,
             us_of_one_basis_read=24.0 * M * rp / HBM_BYTES_PER_S * 1e6, us_of_the_mfma_work=6.0 * M * rp * cols / F64_MFMA_FLOPS * 1e6,
             basis_reads_by_column_chunks=(cols + 63) // 64)
    b = kernels["pair_distance_kernel"]
    pairs = float(S) * n * M
    b.update(pair_vertices=pairs, ns_per_thousand_pair_vertices=1e6 * b["us_per_call"] / pairs,
             us_of_the_instruction_count=PAIR_OPS * pairs / F64_VALU_LANE_OPS * 1e6,
             lane_instruction_slots_per_pair_vertex=b["us_per_call"] * 1e-6 * F64_VALU_LANE_OPS / pairs)
    c = kernels["instances_kernel"]
    sp = sum(pad(min(512, S - c0)) for c0 in range(0, S, 512))
    c.update(gflop=6.0 * M * rp * sp / 1e9, megabytes_written=24.0 * M * sp / 1e6,
             us_of_the_store=24.0 * M * sp / HBM_BYTES_PER_S * 1e6, us_of_the_mfma_work=6.0 * M * rp * sp / F64_MFMA_FLOPS * 1e6)

    # the host route, once each (it is slow); a subset of the samples where the whole set would take minutes, scaled
    t0 = time.perf_counter()
    host_avg = host_generalization(dm, X)
    host_gen_ms = 1e3 * (time.perf_counter() - t0)
    sub = min(S, 64)
    t0 = time.perf_counter()
    host_min = host_specificity(dm, X, A[:sub])
    host_spec_ms = 1e3 * (time.perf_counter() - t0) * S / sub
    dev = dm.project(X)[1][0]
    spec = ga.ModelMetrics.specificity(ctx, dm, X, sub, alphas=A[:sub]).min_avg[0]

    out = {"M": M, "r": r, "n_shapes": n, "n_samples": S, "ranks": ranks, "threads": HOST_THREADS,
           "whole_call_ms": whole, "kernels": kernels,
           "host_route_ms": {"generalization_full_rank": host_gen_ms, "specificity_full_rank_scaled_from_samples": host_spec_ms,
                             "samples_timed": sub},
           "host_route_over_device": {"generalization_full_rank": host_gen_ms / whole["generalization_full_rank"]["median"],
                                      "specificity_full_rank": host_spec_ms / whole["specificity_full_rank"]["median"]},
           "largest_difference_device_against_host_route": {"generalization_avg": float(np.abs(dev - host_avg).max()),
                                                            "specificity_min_avg": float(np.abs(spec - host_min).max())}}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", f"model_metrics_{M}_{r}_{n}_{S}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    dm.close()
    ctx.close()


if __name__ == "__main__":
    main()
