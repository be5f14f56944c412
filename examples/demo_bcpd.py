#!/usr/bin/env python3
"""Bayesian coherent point drift (classic.BCPDRegistration; the method of the reference's draft other/algorithms/cpd/BCPD.scala) on the
femur pair next to the non-rigid classic CPD, through the Python host layer (needs an MI355X):
    PYTHONPATH=. python examples/demo_bcpd.py"""
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
for name, reg in (("non-rigid CPD", cl.NonRigidCPDRegistration(ctx, ref, lambda_=2.0, beta=30.0, w=0.0, max_iterations=100)),
                  ("Bayesian CPD", cl.BCPDRegistration(ctx, ref, w=0.0, lambda_=2.0, gamma=1.0, k=1.0, beta=30.0, max_iterations=100))):
    t0 = time.perf_counter()
    fit = reg.register(target)
    dt = time.perf_counter() - t0
    avg, hd = rc.evaluateReconstruction2GroundTruthDouble(name, ga.TriangleMesh3D(fit, cells), gt)
    print(f"{name:13s}: {dt:6.3f} s, average surface distance (both ways) {avg:.3f} mm, Hausdorff {hd:.3f} mm")

# the same registration over a low-rank factor of the kernel matrix (G ~ L L^T, csrc/bcpd_lowrank.hip)
low = cl.BCPD(ctx, ref, target, w=0.0, lambda_=2.0, gamma=1.0, k=1.0, beta=30.0, lowRank=cl.LowRankG(1e-8))
t0 = time.perf_counter()
fit = low.Registration(100)
dt = time.perf_counter() - t0
avg, hd = rc.evaluateReconstruction2GroundTruthDouble("low rank", ga.TriangleMesh3D(fit, cells), gt)
info = low.lowRankInfo
low.close()
print(f"Bayesian CPD, low rank ({info['columns']} columns, residual fraction {info['residual_fraction']:.1e}): {dt:6.3f} s, "
      f"average surface distance (both ways) {avg:.3f} mm, Hausdorff {hd:.3f} mm")

# past the dense limit of 32 768 template points: 50 000 points on an ellipsoid hull, 10 000 of them moved as the target
rng = np.random.default_rng(5)
u = rng.normal(size=(50000, 3))
hull = u / np.linalg.norm(u, axis=1)[:, None] * (50.0 * np.array([1.0, 0.7, 0.5]))
c, s = np.cos(0.15), np.sin(0.15)
moved = 1.05 * hull[rng.permutation(50000)[:10000]] @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]).T + rng.normal(0, 0.3, (10000, 3))
t0 = time.perf_counter()
big = cl.BCPD(ctx, hull, moved, w=0.1, lambda_=10.0, gamma=0.3, k=1.0, beta=25.0, lowRank=cl.LowRankG(1e-8))
t1 = time.perf_counter()
big.Registration(30, tolerance=0.0)
t2 = time.perf_counter()
info, start, end = big.lowRankInfo, big._sigma2_init, big.sigma2()
big.close()
print(f"hull of 50 000 points: {info['columns']} columns, {info['factor_bytes'] / 2**20:.0f} MiB, built in {(t1 - t0) * 1e3:.0f} ms; "
      f"30 iterations in {(t2 - t1) * 1e3:.0f} ms, sigma2 {start:.1f} -> {end:.4f} (target noise 0.3^2 = 0.09)")

# BCPD++ (Hirose 2021): register the femur decimated to about 400 vertices, then carry the fit to all 1 622 vertices -- the
# Gaussian-process posterior mean of the displacement field at each of them, then the similarity (csrc/kernel_warp.hip)
kept, _, _ = ctx.mesh_decimate(ref, cells, 400)
t0 = time.perf_counter()
_, fit = cl.BCPDRegistration(ctx, ref[kept], w=0.0, lambda_=2.0, gamma=1.0, k=1.0, beta=30.0, max_iterations=100).register(target, ref)
dt = time.perf_counter() - t0
avg, hd = rc.evaluateReconstruction2GroundTruthDouble("decimated", ga.TriangleMesh3D(fit, cells), gt)
print(f"Bayesian CPD on {kept.shape[0]} of {ref.shape[0]} vertices, all vertices warped: {dt:6.3f} s, "
      f"average surface distance (both ways) {avg:.3f} mm, Hausdorff {hd:.3f} mm (the full-resolution run: second line above)")
ctx.close()
