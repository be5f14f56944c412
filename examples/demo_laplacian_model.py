#!/usr/bin/env python3
"""The inverse-Laplacian model at a size the dense route cannot reach (needs an MI355X):
    PYTHONPATH=. python examples/demo_laplacian_model.py [vertices=50000]

On the femur (1 622 vertices) both routes build the model -- InverseLaplacian (dense pseudo-inverse on the host, pivoted Cholesky on the
device) and InverseLaplacianSpectral (the sparse Laplacian's own smallest eigenpairs, found on the device) -- and twenty CPD updates
of the femur pair run from the spectral one.  Then the spectral route alone on a closed hull of `vertices` points, where the dense
route would need a vertices x vertices matrix."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import gingr_amd as ga  # noqa: E402
from bench_nicp_sparse import sphere_mesh  # noqa: E402

d = np.load(os.path.join(ROOT, "tests", "golden", "inputs.npz"))
m = np.load(os.path.join(ROOT, "tests", "golden", "femur_mesh.npz"))
ref, target = d["femur"].astype(np.float64), d["femur_target"].astype(np.float64)
cells = m["femur_cells"].astype(np.int32)
n_big = int(sys.argv[1]) if len(sys.argv) > 1 else 50000

ctx = ga.Context(0)
t0 = time.perf_counter()
dense = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.0, maxRank=102, cells=cells).InverseLaplacian(scaling=30.0)
print(f"femur, InverseLaplacian(maxRank=102):       rank {dense.rank} in {1e3 * (time.perf_counter() - t0):.0f} ms (host SVD included)")
t0 = time.perf_counter()
model = ga.GPMMTriangleMesh3D(ctx, ref, cells=cells).InverseLaplacianSpectral(scaling=30.0, rank=102)
print(f"femur, InverseLaplacianSpectral(rank=102):  rank {model.rank} in {1e3 * (time.perf_counter() - t0):.0f} ms; {model.laplacianInfo}")
print(f"leading variances: spectral {np.round(model.variance[:6], 1)}, 100-column pivoted Cholesky {np.round(dense.variance[:6], 1)}")


def mean_distance(fit):
    return float(np.sqrt(ctx.nn(fit, target)[1]).mean())


cpd = ga.CpdRegistration(ctx)
state = cpd.createInitialState(model, target, ga.CpdConfiguration(maxIterations=40, w=0.1))
print(f"CPD on the femur pair: mean vertex distance {mean_distance(ref):.3f} mm before", end="")
for _ in range(20):
    state = cpd.update(state)
print(f", {mean_distance(state.general.fit):.3f} mm after 20 updates")
cpd.close()

v, c = sphere_mesh(n_big, 0)
t0 = time.perf_counter()
big = ga.GPMMTriangleMesh3D(ctx, v, cells=c).InverseLaplacianSpectral(scaling=30.0, rank=102)
print(f"hull of {n_big} vertices, rank {big.rank} in {1e3 * (time.perf_counter() - t0):.0f} ms; {big.laplacianInfo}")
print(f"(the dense route would start from a {n_big * n_big * 8 / 1e9:.0f} GB pseudo-inverse)")
