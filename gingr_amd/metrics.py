"""Model metrics: how good is a shape model?  The three measures of the shape-model literature (and of scalismo's ModelMetrics), with the
two expensive ones batched on the device:

  generalization   how closely the model, cut to its k leading components, reproduces shapes it has not seen
  specificity      how far random samples of the model lie from the nearest real shape
  compactness      the share of the variance the k leading components keep (host only)

and generalization the way the literature defines it when there are no shapes to spare, leave-one-out over the training shapes
themselves (generalizationLeaveOneOut: every fold's model, projection and distance in one call).

What is not scalismo's is this package's definition -- scalismo's own source is not in reach.  Two distances exist.  distance="vertex"
(the default) is vertex to corresponding vertex.  distance="surface" is the measure scalismo and the literature use,
MeshMetrics.avgDistance: the mean (and the largest) distance from every vertex of the model-side mesh -- the projection or the sample --
to the closest point on the surface of the data shape; the direction, model side -> data surface, is this package's definition, and it
is what Context.mesh_distance_stats(projection, shape, cells) computes pair by pair.  The two differ whenever vertices slide along the
surface, which is what a localized or augmented model lets them do.  Either way the shapes must be in correspondence with the model's
reference, as the shapes of PointDistributionModel.createUsingPCA are: the projection needs it.  The projection of a shape onto k components is the existing rule,
model.truncate(k).coefficients(shape) followed by .instance: the regression with noise 1e-5 at the identity pose.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import numpy as np

from ._native import f64, dptr, iptr
from .context import Context, _check
from .models import _resident


@dataclasses.dataclass
class GeneralizationResult:
    ranks: np.ndarray          # [n_ranks]
    avg: np.ndarray            # [n_ranks, n] mean vertex distance between shape and projection
    max: np.ndarray            # [n_ranks, n] largest vertex distance
    coefficients: np.ndarray   # [n_ranks, n, rank], zero from entry k on
    distance: str = "vertex"   # "vertex": to the corresponding vertex; "surface": to the closest point on the shape's surface

    def curve(self) -> np.ndarray:
        """the mean over the shapes of the mean distance, per rank"""
        return self.avg.mean(axis=1)


@dataclasses.dataclass
class SpecificityResult:
    ranks: np.ndarray          # [n_ranks]
    min_avg: np.ndarray        # [n_ranks, nSamples] mean vertex distance to the nearest training shape
    argmin: np.ndarray         # [n_ranks, nSamples] that shape's index (the lowest on an exact tie)
    alphas: np.ndarray         # [nSamples, rank] the coefficient vectors of the samples
    distance: str = "vertex"   # "vertex": to the corresponding vertex; "surface": to the closest point on the shape's surface

    def curve(self) -> np.ndarray:
        """the mean over the samples, per rank"""
        return self.min_avg.mean(axis=1)


@dataclasses.dataclass
class LeaveOneOutResult:
    ranks: np.ndarray          # [n_ranks]
    avg: np.ndarray            # [n_ranks, n] mean vertex distance between shape i and its projection onto the model of the others
    max: np.ndarray            # [n_ranks, n] largest vertex distance
    foldRanks: np.ndarray      # [n] rank of the model built without shape i (a rank k above it counts as that rank)

    def curve(self) -> np.ndarray:
        """the mean over the folds of the mean distance, per rank"""
        return self.avg.mean(axis=1)


class ModelMetrics:
    """model: a device-built model, a DeviceModel, or a host PointDistributionModel (uploaded for the call)."""

    @staticmethod
    def generalizationLeaveOneOut(ctx: Context, shapes, ranks=None, relativeTolerance: float = 1e-10) -> LeaveOneOutResult:
        """Crossvalidation.leaveOneOutCrossvalidation with the generalization measure (gingr_pca_leave_one_out): for every one of the
        3 <= n <= 512 shapes (n x M x 3, in correspondence, taken as aligned) the PCA model of the others -- createUsingPCA(alignment
        "none", relativeTolerance) -- and that shape's distance to its projection onto the k leading components, for every k in ranks
        (1 <= k <= n - 2, at most 16; None: n - 2 only).  One call: no model is built, nothing of mesh size is repeated per fold.
        Vertex to corresponding vertex only: this route never forms the projections, so there is nothing to measure against a surface."""
        X = f64(shapes)
        if X.ndim != 3 or X.shape[2] != 3:
            raise ValueError(f"shapes: expected (n, M, 3), got {X.shape}")
        n, M = X.shape[0], X.shape[1]
        k = np.ascontiguousarray([n - 2] if ranks is None else np.atleast_1d(ranks), dtype=np.int32)
        avg, mx, fr = np.empty((k.size, n)), np.empty((k.size, n)), np.empty(n, dtype=np.int32)
        _check(ctx.handle, ctx._lib.gingr_pca_leave_one_out(ctx.handle, M, n, dptr(X), float(relativeTolerance), k.size, iptr(k), dptr(avg), dptr(mx),
                                                            iptr(fr)), "gingr_pca_leave_one_out")
        return LeaveOneOutResult(k.astype(np.int64), avg, mx, fr.astype(np.int64))

    @staticmethod
    def generalization(ctx: Context, model, shapes, ranks=None, distance: str = "vertex", cells=None) -> GeneralizationResult:
        """shapes: n x M x 3 in correspondence with the model's reference, n <= 512 per call.  ranks=None: the full rank only.
        distance="surface": every vertex of the projection to the closest point on the shape's surface (triangles: cells, else the
        model's); the default "vertex": to the corresponding vertex."""
        dm, own = _resident(ctx, model)
        try:
            coef, avg, mx = dm.project(shapes, ranks, distance=distance, cells=cells)
            return GeneralizationResult(dm._ranks(ranks).astype(np.int64), avg, mx, coef, distance)
        finally:
            if own:
                dm.close()

    @staticmethod
    def specificity(ctx: Context, model, shapes, nSamples: int, ranks=None, seed: int = 0, alphas=None, distance: str = "vertex",
                    cells=None) -> SpecificityResult:
        """shapes: the n <= 512 training shapes.  The samples are the instances of `alphas` (nSamples x rank), drawn here with
        numpy.random.default_rng(seed).standard_normal unless given -- the library draws nothing; for rank k the entries from k on
        count as zero.  distance="surface": every vertex of the sample to the closest point on the training shape's surface (triangles:
        cells, else the model's); the default "vertex": to the corresponding vertex."""
        dm, own = _resident(ctx, model)
        try:
            X, k = dm._shapes(shapes), dm._ranks(ranks)
            c = dm._surface_cells(distance, cells)
            A = np.random.default_rng(seed).standard_normal((int(nSamples), dm.rank)) if alphas is None else f64(alphas)
            if A.ndim != 2 or A.shape != (int(nSamples), dm.rank):
                raise ValueError(f"alphas: expected ({int(nSamples)}, {dm.rank}), got {A.shape}")
            A = f64(A)
            S = A.shape[0]
            mn, am = np.empty((k.size, S)), np.empty((k.size, S), dtype=np.int32)
            if c is None:
                _check(ctx.handle, ctx._lib.gingr_model_specificity(ctx.handle, dm.handle, X.shape[0], dptr(X), S, dptr(A), k.size, iptr(k),
                                                                    dptr(mn), iptr(am)), "gingr_model_specificity")
            else:
                _check(ctx.handle, ctx._lib.gingr_model_specificity_surface(ctx.handle, dm.handle, X.shape[0], dptr(X), c.shape[0], iptr(c), S, dptr(A),
                                                                            k.size, iptr(k), dptr(mn), iptr(am)), "gingr_model_specificity_surface")
            return SpecificityResult(k.astype(np.int64), mn, am.astype(np.int64), A, distance)
        finally:
            if own:
                dm.close()

    @staticmethod
    def compactness(model, ranks: Optional[np.ndarray] = None) -> np.ndarray:
        """Host only: the cumulative fraction of the model's variance that the k leading components keep -- for every k = 1 .. rank,
        or for the k in ranks."""
        host = getattr(model, "host", model)
        var = np.asarray(host.variance, dtype=np.float64)
        frac = np.cumsum(var) / var.sum()
        return frac if ranks is None else frac[np.atleast_1d(np.asarray(ranks, dtype=np.int64)) - 1]
