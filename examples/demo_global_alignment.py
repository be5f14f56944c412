#!/usr/bin/env python3
"""Global rigid pre-alignment in front of a registration, on the femur pair (needs an MI355X):
    PYTHONPATH=. python examples/demo_global_alignment.py

The target is turned by a fixed arbitrary rotation and shifted, as a raw scan arrives in its scanner's frame.  Deterministic CPD
through `GingrInterface(...).CPD(cfg).runDecimated(100, 100)` from that raw start, then the same with the pose that
`classic.GlobalRigidAlignment` finds (64 spiral start rotations, 10 iterations of ICP each, all on the device in one call, the best
refined by the RigidICP task) passed as the state's initial pose (`initialModelParameterTransform`, GeneralRegistrationState.apply).
There is no reference counterpart: the reference's demos ship pre-aligned data."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import gingr_amd as ga  # noqa: E402
from gingr_amd import classic  # noqa: E402
from gingr_amd.simple import euler_to_rotation_matrix  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
d = np.load(os.path.join(HERE, "..", "tests", "golden", "inputs.npz"))
m = np.load(os.path.join(HERE, "..", "tests", "golden", "femur_mesh.npz"))
ref = d["femur"].astype(np.float64)
R_scan, t_scan = euler_to_rotation_matrix(2.2, 0.9, -1.4), np.array([130.0, -220.0, 95.0])
tgt = d["femur_target"].astype(np.float64) @ R_scan.T + t_scan

ctx = ga.Context(0)
model = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.01).Gaussian(sigma=70.0, scaling=50.0).to_host()
model.cells = m["femur_cells"]
target = ga.TriangleMesh3D(tgt, m["femur_target_cells"])
cfg = ga.CpdConfiguration(maxIterations=30)


def report(name, state):
    fit = np.asarray(state.general.fit)
    s, mx, n, _ = ctx.mesh_distance_stats(fit, tgt, m["femur_target_cells"])
    print(f"{name:18s}: average distance to the target surface {s / n:.3f} mm, max {mx:.3f} mm")


raw = ga.GingrInterface(ctx, model, target, evaluatorUncertainty=2.0, verbose=False).CPD(cfg).runDecimated(100, 100)
report("raw start", raw)

align = classic.GlobalRigidAlignment(ctx, ref)                      # 64 starts, 10 iterations, overlap 1, refined on all points
align.register(tgt)
R, t = align.transform
res = align.searchResult
order = np.argsort(res.scores)
angle = np.degrees(np.arccos(np.clip((np.trace(R_scan.T @ R) - 1.0) / 2.0, -1.0, 1.0)))
print(f"global alignment  : start {res.best} of {res.scores.shape[0]} wins with score {res.score:.3f} mm (runner-up: start {order[1]}, "
      f"{res.scores[order[1]]:.3f} mm); {align.refineIterationsDone} refining iterations; {angle:.2f} degrees from the scan's rotation")
pose = ga.TranslationAfterRotation(tuple(float(v) for v in t), R)
aligned = ga.GingrInterface(ctx, model, target, initialModelParameterTransform=pose, evaluatorUncertainty=2.0,
                            verbose=False).CPD(cfg).runDecimated(100, 100)
report("after alignment", aligned)
ctx.close()
