#!/usr/bin/env python3
"""The two least-squares solvers of the optimal-step non-rigid ICP side by side: "dense" (normal equations as a dense matrix, blocked
Cholesky) and "sparse" (matrix-free block-Jacobi preconditioned CG over the edge graph).

    python tools/bench_nicp_sparse.py [n=50000] [steps=3]

On the femur pair (1 622 vertices) both solvers run, both kinds.  On a pair of sphere hulls with n vertices the sparse solver runs
for both kinds and the dense one where its matrix fits (DENSE_LIMIT unknowns).  Per (pair, kind, solver): wall time of one whole
Iteration (correspondence + solve, host clock around synchronising calls), of the solve alone (the C entry point on a fixed
correspondence), and the CG iterations of every step.  One JSON line on stdout, the same into profiles/nicp_sparse_<n>.json."""
import ctypes
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
import gingr_amd as ga  # noqa: E402
from gingr_amd import classic  # noqa: E402
from gingr_amd import _native as nat  # noqa: E402

DENSE_LIMIT = 16000       # unknowns the dense solver is asked for here: a 2 GB matrix, a little past the 12 000 its tests reach
ALPHAS = [10.0, 5.0, 1.0]


def sphere_mesh(n, seed, radius=30.0, noise=0.0):
    """closed triangle mesh: convex hull of n points on a sphere, outward orientation"""
    from scipy.spatial import ConvexHull
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    tris = ConvexHull(p).simplices.astype(np.int32).copy()
    a, b, c = p[tris[:, 0]], p[tris[:, 1]], p[tris[:, 2]]
    flip = np.einsum("ij,ij->i", np.cross(b - a, c - a), a) < 0
    tris[flip] = tris[flip][:, [0, 2, 1]]
    v = p * radius
    if noise:
        v = v * (1.0 + noise * rng.normal(size=(n, 1)))
    return v, tris


def sphere_pair(n):
    tv, tt = sphere_mesh(n, 0)
    gv, gt = sphere_mesh(n + 37, 1, radius=31.5, noise=0.01)
    gv = gv * np.array([1.05, 0.97, 1.02]) + np.array([0.8, -0.5, 0.3])
    lm_t = {"a": tv[3] + 0.1, "b": tv[n // 4] - 0.1, "c": tv[n // 2]}
    lm_g = {"a": gv[10], "b": gv[n // 3] + 0.05, "c": gv[n - 5]}
    return (tv, tt), (gv, gt), lm_t, lm_g


def femur_pair():
    d = np.load(os.path.join(ROOT, "tests", "golden", "inputs.npz"))
    m = np.load(os.path.join(ROOT, "tests", "golden", "femur_mesh.npz"))
    tv, gv = d["femur"].astype(np.float64), d["femur_target"].astype(np.float64)
    lm_t = {f"L{i}": p for i, p in enumerate(d["femur_lm"].astype(np.float64))}
    lm_g = {f"L{i}": p for i, p in enumerate(d["femur_target_lm"].astype(np.float64))}
    return (tv, m["femur_cells"]), (gv, m["femur_target_cells"]), lm_t, lm_g


def run(ctx, pair, kind, solver, steps):
    (tv, tt), (gv, gt), lm_t, lm_g = pair
    n = tv.shape[0]
    task = classic.NonRigidOptimalStepICP(ctx, (tv, tt), (gv, gt), lm_t, lm_g, kind=kind, solver=solver)
    task.Iteration(tv, 10.0, 10.0)            # warm-up: allocations, code load
    ctx.synchronize()
    fit, cg, whole = tv, [], []
    for s in range(steps):
        alpha = ALPHAS[min(s, len(ALPHAS) - 1)]
        t0 = time.perf_counter()
        fit = task.Iteration(fit, alpha, alpha)[0]          # (returns host arrays: the call has synchronised)
        whole.append(1e3 * (time.perf_counter() - t0))
        if solver == "sparse":
            cg.append(task.solveInfo["iterations"])
    # the solve alone, on the correspondence of the template, alpha = 10
    cp, w, _ = task.getClosestPoints(tv)
    L = task.lmIdsOnTemplate.shape[0]
    out, lm = np.empty((n, 3)), np.empty((max(L, 1), 3))
    lib, solve = ctx._lib, []
    for _ in range(steps + 1):
        t0 = time.perf_counter()
        if solver == "sparse":
            info = nat.NicpInfo()
            rc = lib.gingr_nicp_step(task._nicp, nat.dptr(tv), nat.dptr(w), nat.dptr(cp), nat.dptr(task.UL) if L else None, 10.0, 10.0,
                                     task.gamma, 0.0, 0, nat.dptr(out), nat.dptr(lm) if L else None, ctypes.byref(info))
        else:
            rc = lib.gingr_nicp_solve(ctx.handle, 0 if kind == "T" else 1, n, nat.dptr(tv), task.edges.shape[0], nat.iptr(task.edges),
                                      nat.dptr(w), nat.dptr(cp), L, nat.iptr(task.lmIdsOnTemplate) if L else None,
                                      nat.dptr(task.UL) if L else None, 10.0, 10.0, task.gamma, nat.dptr(out), nat.dptr(lm) if L else None)
        solve.append(1e3 * (time.perf_counter() - t0))
        if rc != 0:
            raise RuntimeError(f"solve failed: {rc} {lib.gingr_last_error(ctx.handle)}")
    res = {"unknowns": n * (1 if kind == "T" else 4), "alphas": [ALPHAS[min(s, len(ALPHAS) - 1)] for s in range(steps)],
           "iteration_ms": [round(v, 3) for v in whole], "solve_ms_alpha10": [round(v, 3) for v in solve[1:]]}
    if solver == "sparse":
        res["cg_iterations_per_step"] = cg
        res["cg_iterations_alpha10"] = int(info.iterations)
        res["solve_us_per_cg_iteration_alpha10"] = round(1e3 * min(solve[1:]) / max(int(info.iterations), 1), 3)
    task.close()
    return res, out.copy()


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    ctx = ga.Context(0)
    result = {"what": "optimal-step non-rigid ICP, dense against sparse least-squares step; one run on one machine", "steps": steps,
              "build": ctx._lib.gingr_build_info().decode()}
    for name, pair in (("femur_1622", femur_pair()), (f"sphere_{n}", sphere_pair(n))):
        block = {"vertices": int(pair[0][0].shape[0])}
        for kind in ("T", "A"):
            unknowns = pair[0][0].shape[0] * (1 if kind == "T" else 4)
            got = {}
            for solver in ("sparse", "dense"):
                if solver == "dense" and unknowns > DENSE_LIMIT:
                    block[f"{kind}_dense"] = (f"not run: {unknowns} unknowns (a dense matrix of {unknowns * unknowns * 8 / 1e9:.0f} GB), "
                                             f"above this tool's limit of {DENSE_LIMIT}")
                    continue
                block[f"{kind}_{solver}"], got[solver] = run(ctx, pair, kind, solver, steps)
            if len(got) == 2:
                block[f"{kind}_max_difference_alpha10"] = float(np.abs(got["sparse"] - got["dense"]).max())
        result[name] = block
    ctx.close()
    line = json.dumps(result)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", f"nicp_sparse_{n}.json"), "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
