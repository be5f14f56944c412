#!/usr/bin/env python3
"""Global alignment of a PARTIAL scan in front of a registration, on the femur pair (needs an MI355X):
    PYTHONPATH=. python examples/demo_partial_alignment.py

The target's lower third is cut away -- a scan that did not see the whole bone -- and what is left is turned by a random rotation and
shifted, as a raw scan arrives in its scanner's frame.  Two starts are found on the device:
  classic.GlobalRigidAlignment(overlap=0.6)   64 spiral rotations about the centroids, trimmed ICP from each
  classic.FeatureRigidAlignment               FPFH descriptors on both clouds, their mutual matches, 2 000 triples, the pose with the
                                              most inliers, 30 iterations of trimmed ICP from it
and from each the robust point-to-plane ICP of examples/demo_robust_icp.py (Cauchy weights, the scan as a cloud with estimated
normals) is run, with the scan brought into the model's frame by the inverse of the found pose.  Judged by the angle to the scan's true
rotation and by the distance of the template vertices that DO have a counterpart to the full target.  The script prints what the run
gives, whichever way it comes out."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import gingr_amd as ga  # noqa: E402
from gingr_amd import classic  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
d = np.load(os.path.join(HERE, "..", "tests", "golden", "inputs.npz"))
m = np.load(os.path.join(HERE, "..", "tests", "golden", "femur_mesh.npz"))
ref, tgt = d["femur"].astype(np.float64), d["femur_target"].astype(np.float64)
tgt_cells = m["femur_target_cells"]
axis = int(np.argmax(tgt.max(0) - tgt.min(0)))                               # the bone's long axis
cut = tgt[:, axis].min() + (tgt[:, axis].max() - tgt[:, axis].min()) / 3.0
part = np.ascontiguousarray(tgt[tgt[:, axis] >= cut])
judged = ref[:, axis] >= cut + 10.0                                          # template vertices well inside the part that was scanned

rng = np.random.default_rng(11)
q = rng.normal(size=4)
x, y, z, w = q / np.linalg.norm(q)
R_scan = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                   [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                   [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
t_scan = rng.normal(size=3) * 100.0
scan = part @ R_scan.T + t_scan                                              # what arrives
full = tgt @ R_scan.T + t_scan                                               # (the whole bone in the scanner's frame: for judging only)

ctx = ga.Context(0)
model = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.01).Gaussian(sigma=70.0, scaling=50.0).to_host()
icp = ga.PointToPlaneIcpRegistration(ctx)
cfg = ga.PointToPlaneConfiguration(maxIterations=50, initialSigma=100.0, endSigma=1.0, tangentOverNormal=100.0, robust=ga.RobustLoss("cauchy"))


def angle(R):
    return float(np.degrees(np.arccos(np.clip((np.trace(R_scan.T @ R) - 1.0) / 2.0, -1.0, 1.0))))


def follow(name, R, t, seconds):
    """robust point-to-plane ICP from the start (R, t): the scan is taken into the model's frame by the inverse pose"""
    back, full_back = (scan - t) @ R, (full - t) @ R
    state = icp.run(icp.createInitialState(model, back, cfg, targetNormals="estimate"))
    fit = np.asarray(state.general.fit)
    s0, mx0, n0, _ = ctx.mesh_distance_stats(ref[judged], full_back, tgt_cells)
    s1, mx1, n1, _ = ctx.mesh_distance_stats(fit[judged], full_back, tgt_cells)
    print(f"{name:24s}: {angle(R):6.2f} degrees from the scan's rotation ({seconds * 1e3:.1f} ms); scanned part to the full target "
          f"{s0 / n0:.3f} mm at the start (max {mx0:.3f}), {s1 / n1:.3f} mm after robust point-to-plane ICP (max {mx1:.3f})")


centroid = classic.GlobalRigidAlignment(ctx, ref, overlap=0.6)
centroid.register(scan)                                                      # (first run: uploads, code objects)
t0 = time.perf_counter()
centroid.register(scan)
follow("centroid starts", *centroid.transform, time.perf_counter() - t0)

feature = classic.FeatureRigidAlignment(ctx, ref, radius=25.0, inlierDistance=3.0)
feature.register(scan)
t0 = time.perf_counter()
feature.register(scan)
dt = time.perf_counter() - t0
print(f"{'':24s}  {feature.info}")
follow("feature matches", *feature.transform, dt)
ctx.close()
