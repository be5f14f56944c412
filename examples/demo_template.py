#!/usr/bin/env python3
"""A registration algorithm of one's own in thirty lines (needs an MI355X):    PYTHONPATH=. python examples/demo_template.py

GiNGR's point (the reference's README) is that an algorithm is three inputs -- a kernel, a correspondence function and an observation
uncertainty.  `TemplateRegistration` takes the last two as Python callables and leaves everything else of `update` to the device.
Here: robust closest point -- every template vertex is paired with its closest target VERTEX, and a pair is trusted less the further
it reaches, variance sigma2 (1 + d^2 / tau^2); sigma2 decays exponentially.  Neither CpdConfiguration nor IcpConfiguration can say
that (ICP gives every pair the same variance).  Printed next to plain IcpRegistration on the same model and target."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import gingr_amd as ga  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
d = np.load(os.path.join(HERE, "..", "tests", "golden", "inputs.npz"))
m = np.load(os.path.join(HERE, "..", "tests", "golden", "femur_mesh.npz"))
ref, tgt = d["femur"].astype(np.float64), d["femur_target"].astype(np.float64)
ctx = ga.Context(0)
model = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.01).Gaussian(sigma=70.0, scaling=50.0).to_host()
TAU2, DECAY, FLOOR, ITERATIONS = 5.0 ** 2, 0.9, 1.0, 50


def closest(state):
    idx, d2, _ = ctx.nn(state.general.fit, tgt)          # closest target vertex of every template vertex, on the device
    return idx, d2


def correspondence(state):
    return ga.CorrespondencePairs(np.arange(ref.shape[0]), tgt[closest(state)[0]])


def uncertainty(pids, state):                            # one variance per pair: far pairs are believed less
    return state.general.sigma2 * (1.0 + closest(state)[1][pids] / TAU2)


def report(name, state):
    s, mx, n, _ = ctx.mesh_distance_stats(np.asarray(state.general.fit), tgt, m["femur_target_cells"])
    print(f"{name:24s}: average distance to the target surface {s / n:.3f} mm, max {mx:.3f} mm, sigma2 {state.general.sigma2:.3f}")


mine = ga.TemplateRegistration(ctx, correspondence, uncertainty, updateSigma2=lambda s: max(s.general.sigma2 * DECAY, FLOOR))
state = mine.createInitialState(model, tgt, ga.TemplateConfiguration(maxIterations=ITERATIONS), sigma2=100.0)
report("robust closest point", mine.run(state))
icp = ga.IcpRegistration(ctx)
cfg = ga.IcpConfiguration(maxIterations=ITERATIONS, initialSigma=100.0, endSigma=1.0, correspondenceMethod="PointcloudClosestPoint")
report("IcpRegistration", icp.run(icp.createInitialState(model, tgt, cfg)))
mine.close()
icp.close()
ctx.close()
