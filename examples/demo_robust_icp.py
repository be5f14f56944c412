#!/usr/bin/env python3
"""Robust point-to-plane ICP on a partial target (needs an MI355X):    PYTHONPATH=. python examples/demo_robust_icp.py

The femur pair with the target's lower third cut away -- a scan that did not see the whole bone.  Plain point-to-plane ICP pairs every
template vertex with its closest point on what is left of the target, so the vertices over the missing part are dragged to the cut;
with PointToPlaneConfiguration(robust=RobustLoss(...)) every observed vertex's variance is inflated by its residual against a scale that
follows the fit (1.4826 x the median residual, found on the device every iteration), and those vertices stop pulling.  Both run through
the resident route: correspondence, residuals, median, weights, update and schedule on the device, the whole run enqueued in one call.
TemplateRegistration with callbacks that apply the same Cauchy formula on the host runs beside it: the same algorithm, one transfer and
one synchronisation per iteration.  Judged by the distance of the template vertices that DO have a counterpart to the full target."""
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
axis = int(np.argmax(tgt.max(0) - tgt.min(0)))                               # the bone's long axis
cut = tgt[:, axis].min() + (tgt[:, axis].max() - tgt[:, axis].min()) / 3.0
kept = tgt[:, axis] >= cut
index = np.cumsum(kept) - 1
part_cells = index[tgt_cells[kept[tgt_cells].all(1)]].astype(np.int32)       # the triangles whose corners all remain
part = np.ascontiguousarray(tgt[kept])
ctx = ga.Context(0)
model = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.01).Gaussian(sigma=70.0, scaling=50.0).to_host()
meshed = ga.PointDistributionModel(model.reference, model.mean, model.basis, model.variance, cells=cells)
RATIO, FLOOR, ITERATIONS, TUNING = 100.0, 1.0, 50, 2.385
STEP = (100.0 - FLOOR) / ITERATIONS
judged = ref[:, axis] >= cut + 10.0                                          # template vertices well inside the part that was scanned


def report(name, state, dt):
    fit = np.asarray(state.general.fit)
    s, mx, n, _ = ctx.mesh_distance_stats(fit[judged], tgt, tgt_cells)
    print(f"{name:28s}: average distance of the scanned part to the full target {s / n:.3f} mm (max {mx:.3f}) after "
          f"{state.general.iteration} iterations, {dt * 1e3:.1f} ms")


def run(name, algo, make_state):
    algo.run(make_state())                                                   # (first run: uploads, code objects)
    t0 = time.perf_counter()
    out = algo.run(make_state())
    report(name, out, time.perf_counter() - t0)
    return out


def config(robust=None):
    return ga.PointToPlaneConfiguration(maxIterations=ITERATIONS, initialSigma=100.0, endSigma=FLOOR, tangentOverNormal=RATIO, robust=robust)


plain, robust = ga.PointToPlaneIcpRegistration(ctx), ga.PointToPlaneIcpRegistration(ctx)
run("plain (resident)", plain, lambda: plain.createInitialState(meshed, part, config(), targetCells=part_cells))
for kind in ("cauchy", "huber", "tukey"):
    cfg = config(ga.RobustLoss(kind))
    out = run(f"{kind} (resident)", robust, lambda: robust.createInitialState(meshed, part, cfg, targetCells=part_cells))
    w, c, n = robust.robustWeights(out)
    print(f"{'':28s}  scale c {c:.3f}, {n} vertices observed, {(w < 0.5).sum()} of them at less than half weight, {(w == 0).sum()} not observed")

# the same Cauchy formula through callbacks: closest points on the device, residuals, median and covariances on the host
a, b, cc = (part[part_cells[:, k]] for k in range(3))
unit = np.cross(b - a, cc - a)
unit /= np.linalg.norm(unit, axis=1)[:, None]
memo = {}


def look(state):
    if memo.get("state") is not state:
        cp, _, tid, _ = ctx.mesh_closest_points(state.general.fit, part, part_cells)
        dd, nrm = state.general.fit - cp, unit[tid]
        en = (dd * nrm).sum(1)
        s = en * en + np.maximum((dd * dd).sum(1) - en * en, 0.0) / RATIO      # the squared distance in the metric of the observation
        k = (s.shape[0] - 1) // 2
        c = TUNING * 1.4826 * np.sqrt(np.partition(s, k)[k])                 # the lower median, an element of the data
        memo.update(state=state, cp=cp, nrm=nrm, u=1.0 + s / c ** 2 if c > 0 else np.ones_like(s))
    return memo


def correspondence(state):
    return ga.CorrespondencePairs(np.arange(ref.shape[0]), look(state)["cp"])


def uncertainty(pids, state):
    q = look(state)
    vn = state.general.sigma2 * q["u"][pids]
    return ga.normalTangentCovariances(q["nrm"][pids], vn, RATIO * vn)


tmpl = ga.TemplateRegistration(ctx, correspondence, uncertainty, updateSigma2=lambda s: max(s.general.sigma2 - STEP, FLOOR), covariancePass="gram")
run("cauchy (Template callbacks)", tmpl, lambda: tmpl.createInitialState(model, part, ga.TemplateConfiguration(maxIterations=ITERATIONS), sigma2=100.0))
for algo in (plain, robust, tmpl):
    algo.close()
ctx.close()
