"""Timing of the leave-one-out generalization on one MI355X (gingr_pca_leave_one_out) and of the loop it replaces: one createUsingPCA and
one generalization call per fold.  Beside the whole call: the batched eigen-decomposition of the folds alone (device timer 22) and the
measure pass alone (device timer 18), HIP events on the context's stream, next to the floors they stand against -- one read of the
centred shapes D at the bandwidth a streaming copy reaches (the Gram pass and the measure pass each need at least that), the MFMA work
of D W at the float64 MFMA peak, and the time of a single decomposition of the fold size (profiles/r06_ubench_sym_eig.txt: 1.3 ms at
n = 100).  Writes profiles/pca_leave_one_out_<M>_<n>.json and prints the same document.  Not the benchmark metric.
Usage: python tools/bench_leave_one_out.py [M] [n] [n_ranks]      (defaults 50000, 100, 3)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import gingr_amd as ga  # noqa: E402

HBM_BYTES_PER_S = 6.29e12      # a streaming copy on an MI355X
F64_MFMA_FLOPS = 78.6e12       # v_mfma_f64_16x16x4_f64 peak


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


def shapes(M, n, seed=5, modes=12):
    """n shapes: a few strong modes and a little noise in every coordinate (tests/pca_restatement.dataset at scale)"""
    rng = np.random.default_rng(seed)
    ref = rng.normal(0, 100, (M, 3))
    B = rng.standard_normal((3 * M, modes)) * (8.0 * 0.7 ** np.arange(modes))[None]
    return ref, ref[None] + (rng.standard_normal((n, modes)) @ B.T).reshape(n, M, 3) + rng.normal(0, 0.05, (n, M, 3))


def loop_of_existing_calls(ctx, ref, X, ranks):
    """what a user writes today: per fold a model of the others and the left-out shape projected onto it"""
    avg = np.empty((len(ranks), X.shape[0]))
    for i in range(X.shape[0]):
        model = ga.PointDistributionModel.createUsingPCA(ctx, ref, np.delete(X, i, axis=0))
        try:
            avg[:, i] = ga.ModelMetrics.generalization(ctx, model, X[i][None], ranks).avg[:, 0]
        finally:
            model.device().close()
    return avg


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    n_ranks = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    ref, X = shapes(M, n)
    ranks = sorted({int(round(k)) for k in np.linspace(1, n - 2, n_ranks)})
    ctx = ga.Context(0)
    call = lambda: ga.ModelMetrics.generalizationLeaveOneOut(ctx, X, ranks)  # noqa: E731
    whole = timed(call)

    ctx.timing_enable(True)
    kernels = {}
    for name, which in (("batched_decomposition", 22), ("project_measure_kernel", 18), ("gram", 2)):
        us, launches = [], 0
        for _ in range(3):
            ctx.timing_reset()
            call()
            ms, launches = ctx.timing_read(which)
            us.append(1e3 * ms)
        kernels[name] = {"us_per_call": median(us), "launches_per_call": int(launches), "all_samples_us": us}
    ctx.timing_enable(False)

    np_ = pad(n)
    cols = len(ranks) * np_
    d_bytes = 24.0 * M * np_
    kernels["project_measure_kernel"].update(columns=cols, gflop=6.0 * M * np_ * cols / 1e9, us_of_the_mfma_work=6.0 * M * np_ * cols / F64_MFMA_FLOPS * 1e6,
                                             reads_of_D_by_column_chunks=(cols + 63) // 64)
    kernels["batched_decomposition"].update(folds=n, fold_size=n - 1, workgroups=n)
    floors = {"megabytes_of_D": d_bytes / 1e6, "us_of_one_read_of_D": d_bytes / HBM_BYTES_PER_S * 1e6,
              "us_of_one_decomposition_n100_profiles_r06_ubench_sym_eig": 1300.0}

    t0 = time.perf_counter()
    loop_avg = loop_of_existing_calls(ctx, ref, X, ranks)
    loop_ms = 1e3 * (time.perf_counter() - t0)
    res = call()

    out = {"M": M, "n_shapes": n, "ranks": ranks, "whole_call_ms": whole, "kernels": kernels, "floors": floors,
           "loop_of_existing_calls_ms": loop_ms, "loop_over_call": loop_ms / whole["median"],
           "fold_ranks": [int(res.foldRanks.min()), int(res.foldRanks.max())], "curve": res.curve().tolist(),
           "largest_difference_call_against_loop": float(np.abs(res.avg - loop_avg).max())}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", f"pca_leave_one_out_{M}_{n}.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
