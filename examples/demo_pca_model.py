#!/usr/bin/env python3
"""From registrations to the next prior (needs an MI355X):    PYTHONPATH=. python examples/demo_pca_model.py

The femur GPMM is registered (CPD) to a handful of perturbed femurs -- samples of the model itself, moved rigidly, with noise.  The
fits are point for point on the reference's vertices, so they go straight into PointDistributionModel.createUsingPCA with
generalised Procrustes alignment (DataCollection.gpa + createUsingPCA of scalismo, on the device).  The PCA model is saved as a
statismo .h5.json file and is then the prior of one more CPD registration.  A model of eight fits has rank 7 at most and is far too
stiff to reach a new femur, so a third prior is the PCA model augmented with a Gaussian kernel model on its own reference
(PointDistributionModel.augmentModel: the covariances are added and re-diagonalised on the device), and a fourth is the PCA model
localized (PointDistributionModel.localizeModel: the sample covariance under a Gaussian taper of the distance on the reference --
every vertex keeps its variance, the long-range correlations eight fits cannot support are removed, nothing generic is added)."""
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

ctx = ga.Context(0)
gpmm = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.01, cells=cells).Gaussian(sigma=70.0, scaling=50.0)
rng = np.random.default_rng(1)
cfg = ga.CpdConfiguration(maxIterations=60, w=0.0, threshold=1e-10)


def mean_distance(fit, to):
    return float(np.sqrt(ctx.nn(fit, to)[1]).mean())


fits = []
for i in range(8):
    angle = rng.normal(0, 0.05, 3)
    sample = gpmm.device().instance(rng.normal(0, 0.7, gpmm.rank), euler=angle, center=ref.mean(axis=0), translation=rng.normal(0, 3, 3))
    sample = sample + rng.normal(0, 0.2, sample.shape)
    cpd = ga.CpdRegistration(ctx)
    best = cpd.run(cpd.createInitialState(gpmm, sample, cfg, transform=ga.GlobalTranformationType.RigidTransforms))
    cpd.close()
    fits.append(best.general.fit)
    print(f"registration {i}: {best.general.iteration} iterations, mean vertex distance {mean_distance(best.general.fit, sample):.3f} mm")

t0 = time.perf_counter()
pca = ga.PointDistributionModel.createUsingPCA(ctx, ref, np.stack(fits), alignment="gpa", cells=cells)
info = pca.pcaInfo
print(f"PCA model of {len(fits)} registrations: rank {info.rank}, {info.gpa_sweeps} Procrustes sweeps (last change {info.gpa_last_change:.2e} mm), "
      f"variance kept {info.kept_variance:.1f} of {info.total_variance:.1f} mm^2, built in {1e3 * (time.perf_counter() - t0):.1f} ms")

host = pca.to_host()
host.cells = cells
path = os.path.join(tempfile.gettempdir(), "femur_pca.h5.json")
ga.io.write_statistical_mesh_model(host, path, dtype="float64")
print(f"wrote {path} (statismo model, {os.path.getsize(path) / 1e6:.1f} MB)")

t0 = time.perf_counter()
augmented = ga.PointDistributionModel.augmentModel(ctx, pca, [ga.GaussianKernelParameters(sigma=70.0, scaling=20.0)], biasTolerance=0.01)
ainfo = augmented.augmentInfo
print(f"PCA model + Gaussian kernel (sigma 70, scaling 20): {ainfo.columns} columns, rank {ainfo.rank}, variance kept {ainfo.kept_variance:.1f} of "
      f"{ainfo.total_variance:.1f} mm^2, built in {1e3 * (time.perf_counter() - t0):.1f} ms")

t0 = time.perf_counter()
localized = ga.PointDistributionModel.localizeModel(ctx, pca, sigma=70.0, relativeTolerance=0.01)
linfo = localized.localizeInfo
print(f"PCA model localized (sigma 70): {linfo.columns} factor columns, rank {linfo.rank}, residual {linfo.residual_fraction:.2e} of the trace, variance "
      f"kept {linfo.kept_variance:.1f} of {linfo.total_variance:.1f} mm^2, built in {1e3 * (time.perf_counter() - t0):.1f} ms")

PRIORS = (("kernel GPMM     ", gpmm), ("PCA model       ", pca), ("PCA + kernel    ", augmented), ("PCA localized   ", localized))
for name, prior in PRIORS:
    cpd = ga.CpdRegistration(ctx)
    best = cpd.run(cpd.createInitialState(prior, target, cfg, transform=ga.GlobalTranformationType.RigidTransforms))
    print(f"CPD of the femur pair from the {name} (rank {prior.rank}): {best.general.iteration} iterations, "
          f"mean vertex distance {mean_distance(best.general.fit, target):.3f} mm")
    cpd.close()

# ---- how good are the four models?  ModelMetrics: generalization on fits the PCA model was not built from, specificity against
# the fits it was built from.  Distances are vertex to corresponding vertex here (the default; the closest-surface-point measure of
# scalismo's ModelMetrics follows at the end); there is no pose in either measure, so every shape is first moved rigidly onto the model's own mean shape.


def onto_mean(model, shapes):
    """Kabsch, vertex for vertex: every shape rotated and translated onto model.reference + model.mean"""
    h = model.device().download(basis=False)
    tgt = np.asarray(h.reference) + np.asarray(h.mean)
    out = []
    for x in shapes:
        cx, ct = x.mean(axis=0), tgt.mean(axis=0)
        u, _, vt = np.linalg.svd((tgt - ct).T @ (x - cx))
        R = u @ np.diag([1.0, 1.0, np.sign(np.linalg.det(u @ vt))]) @ vt
        out.append((x - cx) @ R.T + ct)
    return np.stack(out)


held_out = []
for i in range(3):
    sample = gpmm.device().instance(rng.normal(0, 0.7, gpmm.rank), euler=rng.normal(0, 0.05, 3), center=ref.mean(axis=0),
                                    translation=rng.normal(0, 3, 3))
    cpd = ga.CpdRegistration(ctx)
    best = cpd.run(cpd.createInitialState(gpmm, sample + rng.normal(0, 0.2, sample.shape), cfg, transform=ga.GlobalTranformationType.RigidTransforms))
    cpd.close()
    held_out.append(best.general.fit)
for name, prior in PRIORS:
    t0 = time.perf_counter()
    ranks = sorted({1, max(1, prior.rank // 2), prior.rank})
    gen = ga.ModelMetrics.generalization(ctx, prior, onto_mean(prior, held_out), ranks=ranks)
    spec = ga.ModelMetrics.specificity(ctx, prior, onto_mean(prior, fits), 200, seed=2)
    compact = ga.ModelMetrics.compactness(prior.device().download(basis=False), ranks=ranks)
    print(f"{name} (rank {prior.rank}): generalization on {len(held_out)} held-out fits at ranks {ranks}: "
          + ", ".join(f"{v:.3f}" for v in gen.curve()) + " mm (compactness " +", ".join(f"{v:.2f}" for v in compact)
          + f"); specificity of 200 samples against the {len(fits)} fits: {spec.curve()[0]:.3f} mm; {1e3 * (time.perf_counter() - t0):.0f} ms")

# ---- and without shapes to spare: leave-one-out over the eight fits themselves (Crossvalidation.leaveOneOutCrossvalidation of scalismo).
# Every fold's model is the PCA of the other seven, the left-out fit is projected onto its k leading components -- one call, no model
# built per fold.  The folds take the fits as aligned, so they are first moved onto the PCA model's mean shape, as above.
t0 = time.perf_counter()
loo = ga.ModelMetrics.generalizationLeaveOneOut(ctx, onto_mean(pca, fits), ranks=[1, 3, len(fits) - 2])
print(f"leave-one-out generalization of the {len(fits)} fits at ranks {loo.ranks.tolist()}: " + ", ".join(f"{v:.3f}" for v in loo.curve())
      + f" mm (largest vertex distance {loo.max[-1].max():.3f} mm, fold ranks {loo.foldRanks.tolist()}); {1e3 * (time.perf_counter() - t0):.0f} ms")

# ---- the same two measures against the closest SURFACE point (distance="surface": what scalismo's ModelMetrics and the literature
# report, MeshMetrics.avgDistance from the projection or sample to the shape's surface), beside the vertex-to-vertex ones: a vertex that
# slides along the surface costs nothing here, and sliding is what the kernel, augmented and localized models allow.
for name, prior in PRIORS:
    t0 = time.perf_counter()
    shapes_g, shapes_s = onto_mean(prior, held_out), onto_mean(prior, fits)
    gen_v = ga.ModelMetrics.generalization(ctx, prior, shapes_g)
    gen_s = ga.ModelMetrics.generalization(ctx, prior, shapes_g, distance="surface", cells=cells)
    spec_v = ga.ModelMetrics.specificity(ctx, prior, shapes_s, 200, seed=2)
    spec_s = ga.ModelMetrics.specificity(ctx, prior, shapes_s, 200, seed=2, distance="surface", cells=cells)
    print(f"{name} (rank {prior.rank}), surface | vertex distance: generalization at full rank {gen_s.curve()[0]:.3f} | {gen_v.curve()[0]:.3f} mm, "
          f"specificity {spec_s.curve()[0]:.3f} | {spec_v.curve()[0]:.3f} mm; {1e3 * (time.perf_counter() - t0):.0f} ms")
localized.device().close()
augmented.device().close()
pca.device().close()
