"""Timing of the posterior as a resident model (GingrAlgorithm.posteriorModel) at 50k points, rank 100 and 256: the pass over the
basis alone (basis_rotate_kernel, device timer 10) beside its byte floor -- 48 M rp bytes read and written once, at the 6.29 TB/s a
streaming copy reaches on an MI355X --, the whole query for a state whose Gram matrix the memo holds and for one it does not, and
the host route the query replaces: download of the basis, numpy GEMM with the same r x r factor, upload.  Not the benchmark metric."""
import json
import sys
import time

import numpy as np
import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
import torch  # noqa: F401  (first: one HIP runtime per process)

import gingr_amd as ga

HBM_BYTES_PER_S = 6.29e12
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
    # three states in turn: the posterior memo keeps two, so every query of the first loop computes correspondences and Gram matrix afresh
    states = [s0.updateGeneral(s0.general.updateSigma2(s0.general.sigma2 * f)) for f in (1.0, 0.9, 0.8)]
    for s in states:
        algo.posteriorModel(s).close()                   # warm-up: allocations, code objects
    ctx.timing_enable(True)
    ctx.timing_reset()
    reps = 6
    t0 = time.perf_counter()
    for k in range(reps):
        algo.posteriorModel(states[k % 3]).close()
    fresh = (time.perf_counter() - t0) / reps
    kern_ms, kern_n = ctx.timing_read(10)
    ctx.timing_enable(False)
    t0 = time.perf_counter()
    for k in range(reps):
        post = algo.posteriorModel(states[(reps - 1) % 3])   # the state the memo holds
        if k < reps - 1:
            post.close()
    memo = (time.perf_counter() - t0) / reps
    # the host route: basis to the host, one GEMM with an r x r factor (its cost does not depend on the factor), back to the device
    dm = model.device()
    t0 = time.perf_counter()
    host = dm.download()
    t_down = time.perf_counter() - t0
    Tm = np.linalg.qr(rng.normal(0, 1, (model.rank, model.rank)))[0]
    t0 = time.perf_counter()
    Qn = (np.asarray(host.basis) * np.sqrt(host.variance)[None, :]) @ Tm
    lam = np.maximum((Qn * Qn).sum(0), 1e-300)
    rotated = ga.PointDistributionModel(host.reference, host.mean, np.asfortranarray(Qn / np.sqrt(lam)[None, :]), lam)
    t_gemm = time.perf_counter() - t0
    t0 = time.perf_counter()
    up = ga.DeviceModel(ctx, rotated)
    t_up = time.perf_counter() - t0
    up.close()
    rp = (model.rank + 15) // 16 * 16
    pass_us = 1e3 * kern_ms / max(kern_n, 1)
    floor_us = 1e6 * 48.0 * M * rp / HBM_BYTES_PER_S
    out.append({"points": M, "rank": model.rank, "rotate_pass_us": pass_us, "rotate_pass_launches": kern_n,
                "byte_floor_us": floor_us, "fraction_of_byte_floor": floor_us / pass_us if pass_us > 0 else None,
                "rotate_pass_gflop": 6.0 * M * rp * rp / 1e9, "basis_megabytes_read_and_written": 48.0 * M * rp / 1e6,
                "query_fresh_state_ms": 1e3 * fresh, "query_memo_hit_ms": 1e3 * memo,
                "host_route_ms": {"download": 1e3 * t_down, "numpy_gemm": 1e3 * t_gemm, "upload": 1e3 * t_up,
                                  "total": 1e3 * (t_down + t_gemm + t_up)},
                "largest_posterior_variance": float(post.download(basis=False).variance[0])})
    print(out[-1], file=sys.stderr)
    post.close()
    algo.close()
    model.device().close()
print(json.dumps(out))
