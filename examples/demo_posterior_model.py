#!/usr/bin/env python3
"""Landmarks first, surface second (needs an MI355X):    PYTHONPATH=. python examples/demo_posterior_model.py

The femur GPMM is conditioned on its six landmark pairs (model.posterior(landmark observations) of scalismo), the posterior comes
back as a model of its own that stays in HBM (DeviceModel.posterior: the basis is rotated on the device), is saved as a statismo
.h5.json file, and is then the prior of a CPD registration of the femur pair."""
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import gingr_amd as ga  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
d = np.load(os.path.join(HERE, "..", "tests", "golden", "inputs.npz"))
m = np.load(os.path.join(HERE, "..", "tests", "golden", "femur_mesh.npz"))
ref, target = d["femur"].astype(np.float64), d["femur_target"].astype(np.float64)
cells = m["femur_cells"]
M = ref.shape[0]

ctx = ga.Context(0)
model = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.01, cells=cells).Gaussian(sigma=70.0, scaling=50.0)
lms = ga.io.landmark_correspondences(ref, [ga.io.Landmark(f"L{k}", p) for k, p in enumerate(d["femur_lm"])],
                                     [ga.io.Landmark(f"L{k}", p) for k, p in enumerate(d["femur_target_lm"])])


def mean_distance(fit):
    return float(np.sqrt(ctx.nn(fit, target)[1]).mean())


t0 = time.perf_counter()
post = model.device().posterior(np.zeros((M, 3)), np.zeros(M), landmarks=lms)          # no dense observation: weight 0 everywhere
print(f"posterior model of the six landmarks: rank {post.rank}, built in {1e3 * (time.perf_counter() - t0):.1f} ms")
prior_var = model.device().marginalCovariance()[:, [0, 3, 5]].sum(1)
post_var = post.marginalCovariance()[:, [0, 3, 5]].sum(1)
print(f"total variance per vertex: prior {prior_var.mean():.2f} mm^2 on average, posterior {post_var.mean():.2f} "
      f"({post_var[lms.pids].mean():.3f} at the landmark vertices)")
print(f"mean vertex distance to the target: prior mean {mean_distance(ref):.3f} mm, posterior mean {mean_distance(post.instance(np.zeros(post.rank))):.3f} mm")

host = post.host.to_host()
host.cells = cells
path = os.path.join(tempfile.gettempdir(), "femur_landmark_posterior.h5.json")
ga.io.write_statistical_mesh_model(host, path, dtype="float64")
print(f"wrote {path} (statismo model, {os.path.getsize(path) / 1e6:.1f} MB)")

cfg = ga.CpdConfiguration(maxIterations=100, w=0.0, threshold=1e-10)
for name, prior in (("prior model    ", model), ("posterior model", post.host)):
    cpd = ga.CpdRegistration(ctx)
    best = cpd.run(cpd.createInitialState(prior, target, cfg, transform=ga.GlobalTranformationType.RigidTransforms))
    print(f"CPD from the {name}: {best.general.iteration} iterations, mean vertex distance {mean_distance(best.general.fit):.3f} mm")
    cpd.close()
post.close()
