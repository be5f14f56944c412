#!/usr/bin/env python3
"""The reference's classic CPD baselines (src/main/scala/gingr/other/algorithms/CPDRegistration.scala) on the femur pair through the
Python host layer (needs an MI355X):    PYTHONPATH=. python examples/demo_classic_cpd.py"""
import os
import time

import numpy as np
import os as _os, sys as _sys
_sys.path.insert(0, _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__))))
import torch  # noqa: F401  (first: one HIP runtime per process)

import gingr_amd as ga
from gingr_amd import classic as cl

here = os.path.dirname(os.path.abspath(__file__))
d = np.load(os.path.join(here, "..", "tests", "golden", "inputs.npz"))
m = np.load(os.path.join(here, "..", "tests", "golden", "femur_mesh.npz"))
ref, target = d["femur"].astype(np.float64), d["femur_target"].astype(np.float64)
cells, tcells = m["femur_cells"], m["femur_target_cells"]
ctx = ga.Context(0)
rc = ga.RegistrationComparison(ctx, verbose=False)
gt = ga.TriangleMesh3D(target, tcells)
print(f"start: average distance to the target surface {rc.avgDistance(ga.TriangleMesh3D(ref, cells), gt):.3f} mm")
for name, Reg, kw in (("rigid", cl.RigidCPDRegistration, {}), ("affine", cl.AffineCPDRegistration, {}),
                      ("non-rigid", cl.NonRigidCPDRegistration, dict(lambda_=2.0, beta=30.0)),
                      ("low-rank", cl.NonRigidCPDRegistration, dict(lambda_=2.0, beta=30.0, lowRank=cl.LowRankG(1e-8)))):
    t0 = time.perf_counter()
    fit = Reg(ctx, ref, w=0.0, max_iterations=100, **kw).register(target)
    dt = time.perf_counter() - t0
    avg, hd = rc.evaluateReconstruction2GroundTruthDouble(name, ga.TriangleMesh3D(fit, cells), gt)
    print(f"{name:9s} CPD: {dt:6.3f} s, average surface distance (both ways) {avg:.3f} mm, Hausdorff {hd:.3f} mm")

# Past the dense limit (46 000 template points): non-rigid CPD over a low-rank factor of the kernel matrix, G ~ L L^T, on an ellipsoid
# hull of 50 000 points against a rotated, scaled, noisy three-quarter subset.  The dense route cannot run here.
M = 50000
rng = np.random.default_rng(5)
u = rng.normal(size=(M, 3))
hull = u / np.linalg.norm(u, axis=1)[:, None] * (50.0 * np.array([1.0, 0.7, 0.5]))
a = 0.15
R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
moved = 1.05 * hull[rng.permutation(M)[:3 * M // 4]] @ R.T + rng.normal(0, 0.3, (3 * M // 4, 3))
t0 = time.perf_counter()
task = cl.CPDFactory(ctx, hull, lambda_=2.0, beta=25.0).registerNonRigidly(moved, lowRank=cl.LowRankG(1e-8))
t1 = time.perf_counter()
fit = task.Registration(30)
t2 = time.perf_counter()
info = task.lowRankInfo
task.close()
print(f"hull {M} -> {moved.shape[0]}: factor of {info['columns']} columns (residual fraction {info['residual_fraction']:.1e}, "
      f"{info['factor_bytes'] / 2**20:.0f} MiB) in {t1 - t0:.3f} s; {task.iterations} iterations in {t2 - t1:.3f} s; "
      f"mean distance to the closest target point {ctx.nn(fit, moved)[2]:.3f} (start {ctx.nn(hull, moved)[2]:.3f})")

# Register the femur decimated to about 400 vertices, then carry the fit to all 1 622 vertices (csrc/kernel_warp.hip).
# transformPoints is the map of ONE Iteration, z + sum_m g(z, y_m) W_m, and the reference feeds TY back into the next Iteration with G
# fixed over the template, TY' = TY + G W: the whole registration is TY = Y + G sum_i W_i, so the displacements of the iterations
# add up at any other point as they do at the template.
kept, _, _ = ctx.mesh_decimate(ref, cells, 400)
task = cl.CPDFactory(ctx, ref[kept], lambda_=2.0, beta=30.0, w=0.0).registerNonRigidly(target)
t0 = time.perf_counter()
fit, s2 = ref.copy(), task.sigma2()
for _ in range(100):
    new = task.Iteration()[1]
    fit += task.transformPoints(ref) - ref
    if abs(new - s2) < 0.001:
        break
    s2 = new
dt = time.perf_counter() - t0
task.close()
avg, hd = rc.evaluateReconstruction2GroundTruthDouble("decimated", ga.TriangleMesh3D(fit, cells), gt)
print(f"non-rigid CPD on {kept.shape[0]} of {ref.shape[0]} vertices, all vertices warped: {dt:6.3f} s, "
      f"average surface distance (both ways) {avg:.3f} mm, Hausdorff {hd:.3f} mm (the full-resolution run: the non-rigid line above)")
