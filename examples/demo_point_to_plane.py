#!/usr/bin/env python3
"""Point-to-plane ICP as an observation uncertainty (needs an MI355X):    PYTHONPATH=. python examples/demo_point_to_plane.py

GiNGR's point is that an algorithm is a kernel, a correspondence function and an observation uncertainty -- and the uncertainty may be
a full 3 x 3 covariance per vertex.  Here every template vertex is paired with its closest point on the target SURFACE and believed
with a small variance along the target's normal there and a large one in the tangent plane, so a vertex may slide on the surface:
`normalTangentCovariances` builds the covariances, `covariancePass="gram"` sends one per vertex through the 3 x 3-weighted Gram pass.
Printed next to plain IcpRegistration (closest target vertex, isotropic variance) from the same start.  It closes with the target as a
scanner would deliver it -- its vertices only, no triangles: the normals are estimated from each point's 12 nearest neighbours on the
device and the registration is point-to-plane against the cloud, judged against the true target mesh like the others."""
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
ctx = ga.Context(0)
model = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.01).Gaussian(sigma=70.0, scaling=50.0).to_host()
TANGENT_OVER_NORMAL, DECAY, FLOOR, ITERATIONS = 100.0, 0.9, 1.0, 50
a, b, c = (tgt[tgt_cells[:, k]] for k in range(3))
cell_normals = np.cross(b - a, c - a)                    # (normalTangentCovariances normalises them)


def closest(state):
    cp, _, tid, _ = ctx.mesh_closest_points(state.general.fit, tgt, tgt_cells)   # closest point on the target surface, on the device
    return cp, tid


def correspondence(state):
    return ga.CorrespondencePairs(np.arange(ref.shape[0]), closest(state)[0])


def uncertainty(pids, state):                            # tight along the target's normal at the closest point, loose across it
    s2 = state.general.sigma2
    return ga.normalTangentCovariances(cell_normals[closest(state)[1][pids]], s2, TANGENT_OVER_NORMAL * s2)


def report(name, state):
    fit = np.asarray(state.general.fit)
    s, mx, n, _ = ctx.mesh_distance_stats(fit, tgt, tgt_cells)
    _, back, _, _ = ctx.mesh_distance_stats(tgt, fit, cells)
    print(f"{name:24s}: average distance to the target surface {s / n:.3f} mm, Hausdorff distance {max(mx, back):.3f} mm "
          f"after {state.general.iteration} iterations")


def timed(name, run):
    t0 = time.perf_counter()
    out = run()
    dt = time.perf_counter() - t0
    report(name, out)
    print(f"{'':24s}  wall time {dt * 1e3:.1f} ms")


plane = ga.TemplateRegistration(ctx, correspondence, uncertainty, updateSigma2=lambda s: max(s.general.sigma2 * DECAY, FLOOR),
                                covariancePass="gram")
state = plane.createInitialState(model, tgt, ga.TemplateConfiguration(maxIterations=ITERATIONS), sigma2=100.0)
timed("point-to-plane", lambda: plane.run(state))
# The same algorithm resident on the device: PointToPlaneIcpRegistration makes correspondence and covariances there and enqueues the
# whole run in one call.  It steps sigma2 by ICP's linear schedule, so the Template route is run once more with that schedule: those
# two are the same algorithm by two routes.
STEP = (100.0 - FLOOR) / ITERATIONS
linear = ga.TemplateRegistration(ctx, correspondence, uncertainty, updateSigma2=lambda s: max(s.general.sigma2 - STEP, FLOOR),
                                 covariancePass="gram")
timed("Template, ICP schedule", lambda: linear.run(linear.createInitialState(model, tgt, ga.TemplateConfiguration(maxIterations=ITERATIONS),
                                                                             sigma2=100.0)))
native = ga.PointToPlaneIcpRegistration(ctx)
pcfg = ga.PointToPlaneConfiguration(maxIterations=ITERATIONS, initialSigma=100.0, endSigma=FLOOR, tangentOverNormal=TANGENT_OVER_NORMAL)
meshed = ga.PointDistributionModel(model.reference, model.mean, model.basis, model.variance, cells=cells)   # (it scans the surfaces)
native.run(native.createInitialState(meshed, tgt, pcfg, targetCells=tgt_cells))         # (first run: uploads, code objects)
timed("PointToPlaneIcp (native)", lambda: native.run(native.createInitialState(meshed, tgt, pcfg, targetCells=tgt_cells)))
icp = ga.IcpRegistration(ctx)
cfg = ga.IcpConfiguration(maxIterations=ITERATIONS, initialSigma=100.0, endSigma=1.0, correspondenceMethod="PointcloudClosestPoint")
timed("IcpRegistration", lambda: icp.run(icp.createInitialState(model, tgt, cfg)))
# The target's vertices only: no targetCells and no model.cells, a normal per target point estimated on the device (k = 12).  Beside
# it above: the surface route (PointToPlaneIcp, native) and plain point-cloud ICP (IcpRegistration), from the same start.
cloud = ga.PointToPlaneIcpRegistration(ctx)
cloud.run(cloud.createInitialState(model, tgt, pcfg, targetNormals="estimate", targetNeighbours=12))   # (first run: uploads, code objects)
timed("PointToPlaneIcp (cloud)", lambda: cloud.run(cloud.createInitialState(model, tgt, pcfg, targetNormals="estimate", targetNeighbours=12)))
for a in (plane, linear, native, icp, cloud):
    a.close()
ctx.close()
