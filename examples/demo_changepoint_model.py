#!/usr/bin/env python3
"""Spatially varying kernels on the femur pair (needs an MI355X):    PYTHONPATH=. python examples/demo_changepoint_model.py

Three models of equal rank over the same reference, each registered to the same target by the same surface ICP:
  plain         DiagonalKernel(Gaussian(70) * 50): one amplitude and one scale for the whole bone
  scaled        the same Gaussian with its amplitude a function of position -- a sigmoid across the neck lets the head move 2.5 times
                as far as the shaft (GPMMTriangleMesh3D.ScaledGaussian)
  change point  the same Gaussian on the shaft, a small-scale Gaussian(25) * 20 on the head, blended by the same sigmoid
                (GPMMTriangleMesh3D.ChangePoint: scalismo's ChangePointKernel)
The head end is found from the mesh: of the two ends of the long axis, the one whose centroid lies further off the shaft's axis.
Nothing is promised about which model fits best: the lines below are what came out, with the date of the run."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import gingr_amd as ga  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
d = np.load(os.path.join(HERE, "..", "tests", "golden", "inputs.npz"))
m = np.load(os.path.join(HERE, "..", "tests", "golden", "femur_mesh.npz"))
ref, tgt = d["femur"].astype(np.float64), d["femur_target"].astype(np.float64)
cells, tgt_cells = m["femur_cells"], m["femur_target_cells"]
RANK, ITERATIONS = 100, 50

# the neck: a plane across the long axis, 18 % of the bone's length from the head end
axis = int(np.argmax(ref.max(0) - ref.min(0)))
lo, hi = ref[:, axis].min(), ref[:, axis].max()
length = hi - lo
shaft = ref[(ref[:, axis] > lo + 0.3 * length) & (ref[:, axis] < hi - 0.3 * length)].mean(0)


def off_axis(end):
    c = end.mean(0) - shaft
    c[axis] = 0.0
    return float(np.linalg.norm(c))


head_high = off_axis(ref[ref[:, axis] > hi - 0.15 * length]) > off_axis(ref[ref[:, axis] < lo + 0.15 * length])
normal = np.zeros(3)
normal[axis] = 1.0 if head_high else -1.0
point = ref.mean(0)
point[axis] = hi - 0.18 * length if head_high else lo + 0.18 * length
ctx = ga.Context(0)
g = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.0, maxRank=RANK, cells=cells)
s = ga.sigmoidField(ref, point, normal, width=0.03 * length)
shaft_pars, head_pars = [ga.GaussianKernelParameters(70.0, 50.0)], [ga.GaussianKernelParameters(25.0, 20.0)]
models = [("plain Gaussian", g.Gaussian(70.0, 50.0)),
          ("scaled Gaussian", g.ScaledGaussian(shaft_pars, 1.0 + 1.5 * s)),
          ("change point", g.ChangePoint(head_pars, shaft_pars, s))]
print(f"femur pair, {ref.shape[0]} vertices, {int((s > 0.5).sum())} of them on the head side of the neck plane; rank {RANK}, "
      f"{ITERATIONS} surface-ICP iterations; run of {time.strftime('%Y-%m-%d')}")
compare = ga.RegistrationComparison(ctx, verbose=False)
target = ga.TriangleMesh3D(tgt, tgt_cells)
for name, dm in models:
    host = dm.to_host()
    model = ga.PointDistributionModel(host.reference, host.mean, host.basis, host.variance, cells=cells)
    algo = ga.IcpRegistration(ctx)
    cfg = ga.IcpConfiguration(maxIterations=ITERATIONS, initialSigma=100.0, endSigma=1.0)
    t0 = time.perf_counter()
    out = algo.run(algo.createInitialState(model, tgt, cfg, targetCells=tgt_cells))
    dt = time.perf_counter() - t0
    fit = ga.TriangleMesh3D(np.asarray(out.general.fit), cells)
    avg, hd = compare.evaluateReconstruction2GroundTruthDouble(name, fit, target)
    print(f"{name:16s}: rank {dm.rank}, average surface distance {avg:.4f} mm, Hausdorff {hd:.4f} mm "
          f"({out.general.iteration} iterations, {dt * 1e3:.0f} ms)")
    algo.close()
ctx.close()
