#!/usr/bin/env python3
"""The kernel extension on the femur pair (needs an MI355X):

    PYTHONPATH=. python examples/demo_kernel_extension.py

(a) Register the femur with ICP, then carry the fit to points that are no vertices of the model: the six landmarks, and an inner
    offset surface (the reference shrunk about its centroid) -- GingrAlgorithm.transformPoints.
(b) Build the Gaussian model on a decimated reference (about 400 vertices), put it on all 1 622 vertices once by the kernel extension
    (model.extend) and once by the nearest-neighbour route, register with both and with the model built directly on the 1 622
    vertices, and print average surface distance and Hausdorff distance of the three fits.

Far from every pivot of the build the extended model has no variance (the deformation goes to zero): that is the nature of the
Nystroem extension, not a defect.  Data: tests/golden (the reference's demo meshes)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import gingr_amd as ga  # noqa: E402
from gingr_amd import simple  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
d = np.load(os.path.join(HERE, "..", "tests", "golden", "inputs.npz"))
m = np.load(os.path.join(HERE, "..", "tests", "golden", "femur_mesh.npz"))
ref, target = d["femur"].astype(np.float64), d["femur_target"].astype(np.float64)
cells, tcells = m["femur_cells"], m["femur_target_cells"]
SIGMA, SCALING, TOL = 70.0, 50.0, 0.01

ctx = ga.Context(0)
cmp_ = ga.RegistrationComparison(ctx, verbose=False)
tmesh = ga.TriangleMesh3D(target, tcells)


def register(model):
    icp = ga.IcpRegistration(ctx)
    cfg = ga.IcpConfiguration(maxIterations=100, initialSigma=10.0, endSigma=1.0, correspondenceMethod="TriangularClosestPoint")
    state = icp.createInitialState(model, target, cfg, targetCells=tcells)
    return icp, icp.run(state)


def report(name, fit, fit_cells):
    mesh = ga.TriangleMesh3D(fit, fit_cells)
    avg = (cmp_.avgDistance(mesh, tmesh) + cmp_.avgDistance(tmesh, mesh)) / 2.0
    print(f"  {name:46s} average surface distance {avg:.3f} mm, Hausdorff {cmp_.hausdorffDistance(mesh, tmesh):.3f} mm")


# ---- (a) the fit at points off the model
model = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=TOL, cells=cells).Gaussian(SIGMA, SCALING)
icp, best = register(model)
print(f"(a) ICP on the full model: rank {model.rank}, pivots per coordinate {model.device().kernelExtension.counts}, "
      f"{best.general.iteration} iterations")
lm = icp.transformPoints(best, d["femur_lm"])
dist = np.linalg.norm(lm - d["femur_target_lm"], axis=1)
print("  the six landmarks carried by the fit: distance to the target's landmarks (mm)", np.round(dist, 2),
      "| before:", np.round(np.linalg.norm(d["femur_lm"] - d["femur_target_lm"], axis=1), 2))
inner = ref.mean(axis=0) + 0.8 * (ref - ref.mean(axis=0))
t0 = time.perf_counter()
inner_fit = icp.transformPoints(best, inner)
print(f"  inner offset surface (reference shrunk to 0.8 about its centroid, {inner.shape[0]} points) carried in "
      f"{(time.perf_counter() - t0) * 1e3:.2f} ms; mean displacement {np.linalg.norm(inner_fit - inner, axis=1).mean():.2f} mm "
      f"(surface: {np.linalg.norm(best.general.fit - ref, axis=1).mean():.2f} mm)")
report("fit of the model built on 1 622 vertices", best.general.fit, cells)
icp.close()

# ---- (b) a model built small, used on the full mesh
kept, small_cells, _ = ctx.mesh_decimate(ref, cells, 400)
small = ga.GPMMTriangleMesh3D(ctx, ref[kept], relativeTolerance=TOL, cells=small_cells).Gaussian(SIGMA, SCALING)
print(f"(b) model built on {kept.shape[0]} vertices: rank {small.rank}")
t0 = time.perf_counter()
by_kernel = simple.kernel_new_reference(ctx, small, ref, cells)
by_kernel.device()
t_kernel = time.perf_counter() - t0
t0 = time.perf_counter()
by_nn = simple.new_reference_nearest_neighbor(ctx, small, ref, cells)
by_nn.device()
t_nn = time.perf_counter() - t0
print(f"  on all {ref.shape[0]} vertices: kernel extension {t_kernel * 1e3:.1f} ms, nearest neighbour {t_nn * 1e3:.1f} ms (whole calls)")
for name, mdl in (("kernel extension of the decimated model", by_kernel), ("nearest-neighbour copy of the decimated model", by_nn)):
    algo, st = register(mdl)
    report(name, st.general.fit, cells)
    algo.close()
ctx.close()
