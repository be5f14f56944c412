#!/usr/bin/env python3
"""Iteration time of the classic CPD family on the device (G/other/algorithms/cpd): femur pair (1 622 vertices) and synthetic
clouds, rigid / affine / non-rigid.  For the non-rigid kind the host-LAPACK time of the same M x M solve (numpy.linalg.solve on
this box's cores -- the reference's `A \\ B` is the same LAPACK call through Breeze) is printed beside it.
    PYTHONPATH=. python tools/bench_classic_cpd.py [M ...]
With --lowrank TOL [--max-columns K] the non-rigid kind alone: the low-rank route (G ~ L L^T, classic.LowRankG) beside the dense one
where the dense one can run (M <= 46 000): create time (the factorisation / the M x M kernel matrix), the factor's columns and
residual, and the time of one iteration split into E-step and M-step.  Every timed iteration starts from the same state (template,
initial variance); the E-step is the iteration of the rigid kind from that state (the same two pair passes; its own M-step is five
launches over O(M + N) numbers, some 20 us), the M-step the difference."""
import json
import os
import sys
import time

import numpy as np
import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
import torch  # noqa: F401  (first: one HIP runtime per process)

import gingr_amd as ga
from gingr_amd import classic as cl

ctx = ga.Context(0)
root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")
d = np.load(os.path.join(root, "inputs.npz"))
cases = [("femur", d["femur"].astype(np.float64), d["femur_target"].astype(np.float64), 30.0)]
argv, lowrank_tol, max_columns = sys.argv[1:], None, 0
if "--lowrank" in argv:
    at = argv.index("--lowrank")
    lowrank_tol = float(argv[at + 1])
    del argv[at:at + 2]
if "--max-columns" in argv:
    at = argv.index("--max-columns")
    max_columns = int(argv[at + 1])
    del argv[at:at + 2]


def same_state_ms(reg, template, s0, n=5):
    """median time of one iteration from (template, s0)"""
    t = []
    for _ in range(n + 1):
        reg.set_state(template, s0)
        ctx.synchronize()
        t0 = time.perf_counter()
        reg.cpd.ctx._lib.gingr_classic_cpd_iterate(reg._h, 1)   # synchronises
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t[1:]))                              # the first one warms up


def created(make):
    ctx.synchronize()
    t0 = time.perf_counter()
    reg = make()
    ctx.synchronize()
    return reg, (time.perf_counter() - t0) * 1e3


for M in [int(a) for a in argv] or [5000]:
    rng = np.random.default_rng(M)
    Y = rng.normal(0, 50, (M, 3))
    X = Y[rng.permutation(M)] @ np.array([[0.995, -0.0998, 0], [0.0998, 0.995, 0], [0, 0, 1.0]]) + rng.normal(0, 2, (M, 3)) + 1.0
    cases.append((f"synthetic {M}", Y, X, 15.0))
out = []
for name, Y, X, beta in cases:
    f = cl.CPDFactory(ctx, Y, lambda_=2.0, beta=beta, w=0.0)
    row = {"case": name, "M": int(Y.shape[0]), "N": int(X.shape[0])}
    if lowrank_tol is not None:
        created(lambda: f.registerRigidly(X))[0].close()       # code objects, allocator
        reg, row["lowrank_create_ms"] = created(lambda: f.registerNonRigidly(X, lowRank=cl.LowRankG(lowrank_tol, max_columns)))
        s0 = reg.sigma2()
        row.update({"lowrank_tolerance": lowrank_tol, "lowrank_max_columns": max_columns, **{"lowrank_" + k: v for k, v in reg.lowRankInfo.items()}})
        row["lowrank_ms_per_iteration"] = same_state_ms(reg, Y, s0)
        row["lowrank_sigma2"] = reg.sigma2()
        reg.close()
        rigid = f.registerRigidly(X)
        row["e_step_ms"] = same_state_ms(rigid, Y, s0)
        rigid.close()
        row["lowrank_m_step_ms"] = row["lowrank_ms_per_iteration"] - row["e_step_ms"]
        if Y.shape[0] <= 46000:
            reg, row["dense_create_ms"] = created(lambda: f.registerNonRigidly(X))
            row["dense_ms_per_iteration"] = same_state_ms(reg, Y, s0)
            row["dense_sigma2"] = reg.sigma2()
            reg.close()
        out.append(row)
        continue
    for kind, mk in (("rigid", f.registerRigidly), ("affine", f.registerAffine), ("nonrigid", f.registerNonRigidly)):
        reg = mk(X)
        reg.Iteration()
        ctx.synchronize()
        n = 5
        t0 = time.perf_counter()
        for _ in range(n):
            reg.cpd.ctx._lib.gingr_classic_cpd_iterate(reg._h, 1)
        ctx.synchronize()
        row[f"{kind}_ms_per_iteration"] = (time.perf_counter() - t0) / n * 1e3
        row[f"{kind}_sigma2"] = reg.sigma2()
        reg.close()
    M = Y.shape[0]
    A = np.exp(-((Y[:, None, :] - Y[None, :, :]) ** 2).sum(-1) / (2 * beta * beta)) + np.eye(M) if M <= 6000 else None
    if A is not None:
        B = np.random.default_rng(0).normal(0, 1, (M, 3))
        t0 = time.perf_counter()
        np.linalg.solve(A, B)
        row["host_lapack_solve_ms"] = (time.perf_counter() - t0) * 1e3
        row["host_cores"] = os.cpu_count()
    out.append(row)
print(json.dumps(out))
