"""Timing of the exact per-vertex posterior covariance map (GingrAlgorithm.posteriorCovariance) at 50k points, rank 100 and 256:
the whole fitter query -- correspondences and Gram matrix of a new state, factorisation, pass over the basis, 6 M doubles to the
host -- the same query when the memo already holds the state's Gram matrix, and the pass over the basis alone (device timer 9)
beside the weighted Gram pass of the same shape from the same run (device timer 2).  Not the benchmark metric."""
import json
import sys
import time

import numpy as np
import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
import torch  # noqa: F401  (first: one HIP runtime per process)

import gingr_amd as ga

M = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
ctx = ga.Context(0)
out = []
for rank in (100, 256):
    rng = np.random.default_rng(1234)
    ref = rng.normal(0, 100, (M, 3))
    model = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.0, maxRank=rank).Gaussian(70.0, 50.0)
    target = ref[rng.permutation(M)[: M - M // 10]] + rng.normal(0, 1.0, (M - M // 10, 3))
    algo = ga.CpdRegistration(ctx)
    s0 = algo.createInitialState(model, target, ga.CpdConfiguration(maxIterations=100, w=0.1))
    # three states in turn: the posterior memo keeps two, so every query below computes correspondences and Gram matrix afresh
    states = [s0.updateGeneral(s0.general.updateSigma2(s0.general.sigma2 * f)) for f in (1.0, 0.9, 0.8)]
    for s in states:
        algo.posteriorCovariance(s)                      # warm-up: allocations, code objects
    ctx.timing_enable(True)
    ctx.timing_reset()
    reps = 9
    t0 = time.perf_counter()
    for k in range(reps):
        cov6 = algo.posteriorCovariance(states[k % 3])
    fresh = (time.perf_counter() - t0) / reps
    kern_ms, kern_n = ctx.timing_read(9)
    gram_ms, gram_n = ctx.timing_read(2)
    ctx.timing_enable(False)
    t0 = time.perf_counter()
    for k in range(reps):
        cov6 = algo.posteriorCovariance(states[(reps - 1) % 3])   # the state the memo holds
    memo = (time.perf_counter() - t0) / reps
    rp = (model.rank + 15) // 16 * 16
    out.append({"points": M, "rank": model.rank, "query_fresh_state_ms": 1e3 * fresh, "query_memo_hit_ms": 1e3 * memo,
                "covariance_pass_us": 1e3 * kern_ms / max(kern_n, 1), "covariance_pass_launches": kern_n,
                "weighted_gram_pass_us": 1e3 * gram_ms / max(gram_n, 1), "weighted_gram_launches": gram_n,
                "basis_megabytes": 3 * M * rp * 8 / 1e6, "covariance_pass_gflop": 3 * M * rp * rp / 1e9,   # upper-triangular factor
                "mean_total_variance": float((cov6[:, 0] + cov6[:, 3] + cov6[:, 5]).mean())})
    print(out[-1], file=sys.stderr)
    algo.close()
    model.device().close()
print(json.dumps(out))
