"""The model layer: the host `PointDistributionModel`, the models built or adopted in HBM (`DevicePointDistributionModel` and its
kinds), `DeviceModel` (gingr_model: the handle a fitter reads) and the GPMM construction helpers of
G/api/gpmm/GPMMHelper.scala and registration/utils/GPMMHelper.scala."""
from __future__ import annotations

import ctypes
import dataclasses
from ctypes import c_int64, c_void_p
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _native as nat
from ._native import f64, dptr, iptr
from .context import Context, _check


# ----------------------------------------------------------------------------- model
@dataclasses.dataclass
class PointDistributionModel:
    """Numeric content of scalismo's PointDistributionModel: reference points, mean displacement, basisMatrix
    (3M x r, element (row, k) = U[row, k]) and variance."""
    reference: np.ndarray      # (M,3)
    mean: np.ndarray           # (M,3) displacement
    basis: np.ndarray          # (3M, r)
    variance: np.ndarray       # (r,)
    cells: Optional[np.ndarray] = None   # (T,3) int: triangulation of the reference mesh (TriangleMesh.triangulation)

    @property
    def rank(self) -> int:
        return int(self.variance.shape[0])

    @property
    def numberOfPoints(self) -> int:
        return int(self.reference.shape[0])

    def truncate(self, k: int) -> "PointDistributionModel":
        """PointDistributionModel.truncate(k): the first k basis functions, as an independent model (copies)."""
        k = int(k)
        if k < 1 or k > self.rank:
            raise ValueError(f"truncate: k = {k} outside 1..{self.rank} (the model's rank)")
        return PointDistributionModel(reference=np.array(self.reference, dtype=np.float64), mean=np.array(self.mean, dtype=np.float64),
                                      basis=np.array(np.asarray(self.basis)[:, :k], dtype=np.float64, order="F"),
                                      variance=np.array(np.asarray(self.variance)[:k], dtype=np.float64),
                                      cells=None if self.cells is None else np.array(self.cells))

    @staticmethod
    def createUsingPCA(ctx: "Context", reference, shapes, alignment: str = "none", relativeTolerance: float = 1e-10, maxRank: int = 0,
                       cells=None, gpaMaxIterations: int = 3, gpaTolerance: float = 1e-5) -> "PcaDevicePointDistributionModel":
        """DataCollection.gpa(...) + PointDistributionModel.createUsingPCA(...) on the device (gingr_model_from_shapes): the PCA model
        of `shapes` (n x M x 3, point for point on `reference`'s vertices, 2 <= n <= 512), resident in HBM.  alignment: "none",
        "rigid" (every shape onto the reference, Kabsch) or "gpa" (generalised Procrustes; the model's reference is then the final
        Procrustes target).  The leading components with variance > relativeTolerance * the largest are kept, at most maxRank
        (0: no limit besides n - 1 and 512).  relativeTolerance = 1e-10 is this package's default; scalismo's own cutoff constant
        is not pinned by anything in reach."""
        return PcaDevicePointDistributionModel(ctx, reference, shapes, alignment, relativeTolerance, maxRank, cells, gpaMaxIterations,
                                               gpaTolerance)

    @staticmethod
    def augmentModel(ctx: "Context", model, bias, relativeTolerance: float = 1e-10, maxRank: int = 0, biasTolerance: float = 0.01,
                     cells=None) -> "AugmentedDevicePointDistributionModel":
        """PointDistributionModel.augmentModel(pcaModel, biasModel) on the device (gingr_model_augment): the model on `model`'s
        reference with mean model.mean + bias.mean and covariance cov(model) + cov(bias), re-diagonalised, resident in HBM.  model /
        bias: device-built models, DeviceModels or host PointDistributionModels (those are uploaded), on the same reference and of at
        most 512 columns together.  bias may also be a sequence of GaussianKernelParameters: the bias is then the Gaussian-mixture
        kernel model GPMMTriangleMesh3D(ctx, model.reference, biasTolerance, cells).GaussianMixture(...) built on the model's own
        reference (for a GPA-aligned PCA model: the Procrustes target).  The leading components with variance > relativeTolerance *
        the largest are kept, at most maxRank (0: no limit besides 512).  The sum of the means and relativeTolerance = 1e-10 are this
        package's definition; scalismo's own are not pinned by anything in reach."""
        return AugmentedDevicePointDistributionModel(ctx, model, bias, relativeTolerance, maxRank, biasTolerance, cells)

    @staticmethod
    def localizeModel(ctx: "Context", model, sigma: float, relativeTolerance: float = 0.01, maxRank: int = 0,
                      cells=None) -> "LocalizedDevicePointDistributionModel":
        """The localized model of Luethi et al. (Gaussian Process Morphable Models) on the device (gingr_model_localize): `model`'s
        covariance multiplied element-wise by the Gaussian taper exp(-|x - y|^2 / sigma^2) over its reference, factored to
        relativeTolerance by the pivoted Cholesky of the GPMM builder (at most 512 columns; `localizeInfo` says whether the tolerance was
        reached) and re-diagonalised, resident in HBM.  Every vertex keeps its variance, nearby correlations survive, far ones go; the
        mean is the model's.  model: a device-built model, a DeviceModel or a host PointDistributionModel (uploaded for the call).  At
        most maxRank components are kept (0: no limit besides 512)."""
        return LocalizedDevicePointDistributionModel(ctx, model, sigma, relativeTolerance, maxRank, cells)


@dataclasses.dataclass(frozen=True)
class AugmentInfo:
    """gingr_augment_info: what the build behind PointDistributionModel.augmentModel / DeviceModel.augment did."""
    columns: int             # columns of the two bases together (ra + rb)
    rank: int                # rank of the model
    total_variance: float    # sum of all eigenvalues of the summed covariance (= the two models' total variances)
    kept_variance: float     # sum of the kept ones


@dataclasses.dataclass(frozen=True)
class LocalizeInfo:
    """gingr_localize_info: what the build behind PointDistributionModel.localizeModel / DeviceModel.localize did."""
    columns: int               # factor columns of the pivoted Cholesky
    rank: int                  # rank of the model
    tolerance_reached: bool    # False: stopped at the ceiling of 512 columns above the tolerance
    residual_fraction: float   # residual trace / trace of the tapered covariance after the last column
    total_variance: float      # trace of the tapered covariance (= the source's total variance)
    kept_variance: float       # sum of the kept eigenvalues


@dataclasses.dataclass(frozen=True)
class PcaInfo:
    """gingr_pca_info: what the build behind PointDistributionModel.createUsingPCA did."""
    rank: int                # rank of the model
    gpa_sweeps: int          # Procrustes sweeps run (0 unless alignment = "gpa")
    gpa_last_change: float   # RMS distance per point between the last two Procrustes targets
    total_variance: float    # sum of all eigenvalues of the sample covariance
    kept_variance: float     # sum of the kept ones


@dataclasses.dataclass(frozen=True)
class LaplacianInfo:
    """gingr_laplacian_info: what the eigensolver behind GPMMTriangleMesh3D.InverseLaplacianSpectral did."""
    n_components: int        # connected components of the edge graph (an isolated vertex is one)
    n_dropped: int           # eigenvalues <= 1e-5 (the components' null vectors and whatever else lies below the cut-off)
    block_columns: int       # columns of the iteration block
    outer_iterations: int    # filter + orthonormalisation + Rayleigh-Ritz steps
    total_degree: int        # products of the Laplacian with the block
    converged: bool          # every wanted residual within the tolerance
    max_residual: float      # largest |L v - mu v| / (2 max degree) of the wanted pairs
    cut_gap: float           # (mu_{k+1} - mu_k) / mu_k at the cut; inf when no eigenvalue is left beyond it


@dataclasses.dataclass(frozen=True)
class KernelExtensionInfo:
    """gingr_model_kernel_extension: `counts` pivots per coordinate; `shared`: the coordinates share one kernel, and their pivot
    lists are prefixes of one sequence."""
    counts: Tuple[int, int, int]
    shared: bool


@dataclasses.dataclass(frozen=True)
class GpmmBuildInfo:
    """gingr_gpmm_info: what the factorisation behind a device-built model did."""
    columns: int                   # factor columns of the pivoted Cholesky (= the model's rank before truncation)
    rank: int                      # rank of the model
    tolerance_reached: bool        # the residual trace fell below relativeTolerance * trace
    residual_fraction: float       # residual trace / trace at the stop
    kept_variance_fraction: float  # kept eigenvalues / all eigenvalues (1 without truncation)


@dataclasses.dataclass(frozen=True)
class ScalarKernelSpec:
    """One scalar kernel of a DiagonalKernel (gingr_scalar_kernel): `kind` "gauss" (mixture of scaling_i exp(-|x-y|^2/sigma_i^2),
    optionally + mirror * the x-mirrored mixture), "dot" (scaling * x.y) or "lookup" (scaling * lookup[i, j])."""
    kind: str
    sigmas: Tuple[float, ...] = ()
    scalings: Tuple[float, ...] = ()
    mirror: float = 0.0
    scaling: float = 1.0
    lookup: Optional[np.ndarray] = None

    def _native(self, keep: list) -> "nat.ScalarKernel":
        k = nat.ScalarKernel()
        k.kind = {"gauss": nat.KERNEL_GAUSSIAN_MIXTURE, "dot": nat.KERNEL_DOT, "lookup": nat.KERNEL_LOOKUP}[self.kind]
        if self.kind == "gauss":
            sg, sc = f64(self.sigmas), f64(self.scalings)
            keep += [sg, sc]
            k.n_kernels, k.sigmas, k.scalings, k.mirror = len(self.sigmas), dptr(sg), dptr(sc), float(self.mirror)
        else:
            k.scaling = float(self.scaling)
            if self.kind == "lookup":
                m = f64(self.lookup)
                keep.append(m)
                k.lookup = dptr(m)
        return k


def _native_kernels(kernels: Sequence[ScalarKernelSpec]) -> Tuple[list, list]:
    """(the native structs of (k_x, k_y, k_z), the arrays they point into -- hold on to them over the call).  Equal specs -> the
    SAME native struct (one factorisation)."""
    keep: list = []
    uniq = {}
    for spec in kernels:
        if id(spec) not in uniq:
            uniq[id(spec)] = spec._native(keep)
    return [uniq[id(spec)] for spec in kernels], keep


RADIAL_FAMILIES = {"gaussian": nat.RADIAL_GAUSSIAN, "rationalQuadratic": nat.RADIAL_RATIONAL_QUADRATIC,
                   "inverseMultiquadric": nat.RADIAL_INVERSE_MULTIQUADRIC}


@dataclasses.dataclass(frozen=True, eq=False)
class RadialKernelTerm:
    """One term w[i] w[j] scaling f(|x_i - x_j|^2) of a scalar kernel (gingr_radial_term).  `family`: "gaussian" (parameter = sigma:
    exp(-nn / sigma^2)), "rationalQuadratic" (parameter = beta: 1 - nn / (nn + beta^2), KernelHelper.scala:64-73) or
    "inverseMultiquadric" (1 / sqrt(nn + beta^2), :53-61).  `weight`: a field over the reference's vertices (any real values), or
    None.  Terms that are given the same array share one upload."""
    family: str
    parameter: float
    scaling: float
    weight: Optional[np.ndarray] = None

    def __post_init__(self):
        if not isinstance(self.family, int) and self.family not in RADIAL_FAMILIES:
            raise ValueError(f"unknown radial family {self.family!r}: one of {sorted(RADIAL_FAMILIES)}")
        if self.weight is not None:
            w = f64(self.weight)
            if w.ndim != 1:
                raise ValueError(f"a weight field is one value per vertex, got an array of shape {w.shape}")
            object.__setattr__(self, "weight", w)

    @property
    def family_code(self) -> int:
        return int(self.family) if isinstance(self.family, int) else RADIAL_FAMILIES[self.family]


def _native_radial(kernels: Sequence[Sequence[RadialKernelTerm]]) -> Tuple[list, list]:
    """(the gingr_radial_kernel structs of (k_x, k_y, k_z), what they point into -- hold on to it over the call).  The same list of
    terms -> the SAME native struct; the same weight array -> the same pointer."""
    keep: list = []
    uniq = {}
    for terms in kernels:
        if id(terms) in uniq:
            continue
        arr = (nat.RadialTerm * max(len(terms), 1))()
        for i, t in enumerate(terms):
            arr[i].family, arr[i].parameter, arr[i].scaling = t.family_code, float(t.parameter), float(t.scaling)
            if t.weight is not None:
                keep.append(t.weight)
                arr[i].weight = dptr(t.weight)
        k = nat.RadialKernel()
        k.n_terms, k.terms = len(terms), arr
        keep.append(arr)
        uniq[id(terms)] = k
    return [uniq[id(terms)] for terms in kernels], keep


def sigmoidField(reference, point, normal, width: float) -> np.ndarray:
    """1 / (1 + exp(-((x - point) . n) / width)) over the vertices x of `reference`, n = normal / |normal|: 0 far behind the plane
    through `point`, 1 far in front of it, `width` the length over which it changes -- the indicator of a ChangePoint kernel or
    (scaled and shifted) the amplitude of a ScaledGaussian."""
    n = f64(normal).reshape(3)
    length = float(np.sqrt((n * n).sum()))
    if not length > 0.0 or not np.isfinite(length):
        raise ValueError("sigmoidField: the normal must be a finite, non-zero vector")
    if not float(width) > 0.0:
        raise ValueError(f"sigmoidField: width = {width} must be positive")
    s = ((f64(reference).reshape(-1, 3) - f64(point).reshape(1, 3)) @ (n / length)) / float(width)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-s))


def _landmarks_native(landmarks) -> tuple:
    """(n, pids int32, points, covs) of a LandmarkCorrespondences as the landmark arguments of the library take them; none or
    empty -> (0, None, None, None)"""
    if landmarks is None or len(landmarks.pids) == 0:
        return 0, None, None, None
    lp = np.ascontiguousarray(landmarks.pids, dtype=np.int32)
    return lp.shape[0], lp, f64(landmarks.points), f64(landmarks.covs)


class DevicePointDistributionModel:
    """A PointDistributionModel whose basis lives in HBM: the result of the on-device GPMM construction
    (gingr_gpmm_build_gaussian / gingr_gpmm_build_diagonal).  Quacks like PointDistributionModel (reference / mean / basis /
    variance / rank / numberOfPoints); basis and variance are downloaded lazily, only if somebody asks for them."""

    _kernel_built = True                    # built from kernels by _build; False for the kinds made from other models or from data
    _kernels, _to_tolerance, _keep, _info = None, False, 0, None   # the kernel build's own; the other kinds leave them alone
    _radial = None                                   # (terms_x, terms_y, terms_z) of a model of radial terms (gingr_gpmm_build_radial)
    _full: Optional["DeviceModel"] = None            # the complete model on self.ctx, once built or adopted
    _host: Optional[PointDistributionModel] = None   # what has been downloaded of it

    def __init__(self, ctx: Context, reference, sigmas: Sequence[float], scalings: Sequence[float],
                 relativeTolerance: float, maxRank: int = 0, kernels: Optional[Sequence[ScalarKernelSpec]] = None,
                 cells: Optional[np.ndarray] = None, toTolerance: bool = False, keepRank: int = 0,
                 radial: Optional[Sequence[Sequence["RadialKernelTerm"]]] = None):
        """toTolerance / keepRank: the build goes through gingr_gpmm_build_diagonal_ex -- maxRank is then the largest number of FACTOR
        columns (0: run to relativeTolerance, an error if the library's ceiling comes first; nothing is shortened silently) and the
        model keeps the keepRank leading eigenpairs (0: all).  Without them: today's call, maxRank silently clamped to 512.
        radial: three lists of RadialKernelTerm instead of sigmas / scalings / kernels (gingr_gpmm_build_radial: the stops of
        gingr_gpmm_build_diagonal_ex, so buildInfo is always there)."""
        self.ctx = ctx
        self.reference = f64(reference)
        self._sig, self._sc = f64(sigmas), f64(scalings)
        self._tol, self._maxrank = float(relativeTolerance), int(maxRank)
        self._kernels = None if kernels is None else tuple(kernels)          # (k_x, k_y, k_z) of a DiagonalKernel
        self.cells = cells
        self._to_tolerance, self._keep = bool(toTolerance), int(keepRank)
        self._radial = None if radial is None else tuple(radial)

    def _build_ex(self, ctx: Context, row_begin: int, row_end: int):
        kernels = self._kernels
        if self._radial is not None:
            entry, (nk, keep) = "gingr_gpmm_build_radial", _native_radial(self._radial)
        else:
            if kernels is None:
                k = ScalarKernelSpec("gauss", tuple(float(v) for v in self._sig), tuple(float(v) for v in self._sc))
                kernels = (k, k, k)
            entry, (nk, keep) = "gingr_gpmm_build_diagonal_ex", _native_kernels(kernels)
        if self._to_tolerance:
            max_columns = self._maxrank
        else:            # today's stop (maxRank clamped to the rank limit), with a truncation folded in
            max_columns = self._maxrank if 0 < self._maxrank <= 512 else 512
        h, info = c_void_p(), nat.GpmmInfo()
        rc = getattr(ctx._lib, entry)(ctx.handle, self.numberOfPoints, dptr(self.reference), ctypes.byref(nk[0]), ctypes.byref(nk[1]),
                                      ctypes.byref(nk[2]), self._tol, int(max_columns), self._keep, row_begin, row_end,
                                      ctypes.byref(info), ctypes.byref(h))
        del keep
        self._info = GpmmBuildInfo(int(info.columns), int(info.rank), bool(info.tolerance_reached), float(info.residual_fraction),
                                   float(info.kept_variance_fraction))
        _check(ctx.handle, rc, entry)
        return h

    @property
    def buildInfo(self) -> Optional[GpmmBuildInfo]:
        """gingr_gpmm_info of the build (builds the model if that has not happened); None for a model that was not built through
        gingr_gpmm_build_diagonal_ex or gingr_gpmm_build_radial (toTolerance / truncate / radial terms)."""
        if self._to_tolerance or self._keep > 0 or self._radial is not None:
            self.device()
        return self._info

    def truncate(self, k: int) -> "DevicePointDistributionModel":
        """PointDistributionModel.truncate(k) on the device.  A kernel model that has not been built yet folds the truncation into its
        build (keep_rank = k: the only way a factor of more than 512 columns becomes a model); a resident one is truncated in HBM
        (gingr_model_truncate)."""
        k = int(k)
        if k < 1:
            raise ValueError(f"truncate: k = {k} < 1")
        if self._full is None and self._kernel_built:
            keep = k if self._keep <= 0 else min(k, self._keep)
            return DevicePointDistributionModel(self.ctx, self.reference, self._sig, self._sc, self._tol, self._maxrank, self._kernels,
                                                self.cells, toTolerance=self._to_tolerance, keepRank=keep, radial=self._radial)
        return TruncatedDevicePointDistributionModel(self.device(), k, cells=self.cells)

    def extend(self, newReference, cells=None) -> "ExtendedDevicePointDistributionModel":
        """This model on the points newReference (anywhere in space) by the kernel extension: see ExtendedDevicePointDistributionModel.
        Kernel models without lookup kernels or weight fields, and what truncate / extend make of them; others raise
        GingrNativeError (GINGR_ERR_STATE) when the extended model is first used."""
        return ExtendedDevicePointDistributionModel(self.device(), newReference, cells=cells)

    def _build(self, ctx: Context, row_begin: int, row_end: int):
        if self._to_tolerance or self._keep > 0 or self._radial is not None:
            return self._build_ex(ctx, row_begin, row_end)
        h = c_void_p()
        if self._kernels is not None:
            nk, keep = _native_kernels(self._kernels)
            _check(ctx.handle, ctx._lib.gingr_gpmm_build_diagonal(ctx.handle, self.numberOfPoints, dptr(self.reference),
                                                                  ctypes.byref(nk[0]), ctypes.byref(nk[1]), ctypes.byref(nk[2]),
                                                                  self._tol, self._maxrank, row_begin, row_end, ctypes.byref(h)),
                   "gingr_gpmm_build_diagonal")
            return h
        _check(ctx.handle, ctx._lib.gingr_gpmm_build_gaussian(ctx.handle, self.numberOfPoints, dptr(self.reference),
                                                              len(self._sig), dptr(self._sig), dptr(self._sc), self._tol,
                                                              self._maxrank, row_begin, row_end, ctypes.byref(h)),
               "gingr_gpmm_build_gaussian")
        return h

    def device(self) -> "DeviceModel":
        if self._full is None:
            M = self.numberOfPoints
            self._full = DeviceModel._adopt(self.ctx, self._build(self.ctx, 0, M), self, M)
        return self._full

    @property
    def numberOfPoints(self) -> int:
        return int(self.reference.shape[0])

    @property
    def rank(self) -> int:
        return self.device().rank

    @property
    def mean(self) -> np.ndarray:
        return np.zeros_like(self.reference)       # GaussianProcess(kernel): zero mean (GPMMHelper.scala:45)

    def to_host(self, basis: bool = True) -> PointDistributionModel:
        if self._host is None or (basis and self._host.basis is None):
            self._host = self.device().download(basis=basis)
        return self._host

    @property
    def variance(self) -> np.ndarray:
        return self.to_host(basis=False).variance

    @property
    def basis(self) -> np.ndarray:
        return self.to_host(basis=True).basis


class _DerivedDevicePointDistributionModel(DevicePointDistributionModel):
    """What the kinds made from other models or from data share: the mean is the device's own, and a kind that wraps a finished native
    model adopts it in one place.  An adopted model lives whole on its context: `_build`, which would make it again for another
    context or a row shard, raises the kind's `_ELSEWHERE`."""

    _kernel_built = False
    _ELSEWHERE = ""

    def _adopt(self, ctx: Context, handle, cells, M: Optional[int] = None):
        """Take over the finished native model `handle` (M points; None: ask the library): reference and mean are read back once,
        without the basis; a failure there gives the handle back."""
        self.ctx, self.cells = ctx, cells
        self._full = DeviceModel._adopt(ctx, handle, self, int(ctx._lib.gingr_model_num_points(handle)) if M is None else M)
        try:
            self._host = self._full.download(basis=False)
        except Exception:
            self._full.close()
            raise
        self.reference = self._host.reference

    def _build(self, ctx: Context, row_begin: int, row_end: int):
        raise ValueError(self._ELSEWHERE)

    @property
    def mean(self) -> np.ndarray:
        return self.to_host(basis=False).mean


class InterpolatedDevicePointDistributionModel(_DerivedDevicePointDistributionModel):
    """model.newReference(newReference, interpolator) with the basis gathered in HBM (gingr_model_new_reference): every new point
    takes the fixed combination sum_k weights[i, k] * (value at source point vertex_ids[i, k]) of mean and basis functions;
    eigenvalues and rank are the source's."""

    def __init__(self, ctx: Context, source, new_reference, vertex_ids, weights, cells=None):
        self.ctx = ctx
        self.reference = f64(new_reference).reshape(-1, 3)
        self._ids = np.ascontiguousarray(vertex_ids, dtype=np.int32).reshape(-1, 3)
        self._w = f64(weights).reshape(-1, 3)
        if self._ids.shape[0] != self.reference.shape[0] or self._w.shape[0] != self.reference.shape[0]:
            raise ValueError("one (vertex_ids, weights) triple per new reference point")
        self._source = source
        # the source model resident on this context (a device-built model shares its handle; a host model is uploaded once)
        self._src_dev = DeviceModel(ctx, source)
        self.cells = None if cells is None else np.ascontiguousarray(cells, dtype=np.int32)

    def _build(self, ctx: Context, row_begin: int, row_end: int):
        if ctx is not self.ctx:
            raise ValueError("an interpolated model lives on the context of its source; download it (to_host) for another device")
        h = c_void_p()
        _check(ctx.handle, ctx._lib.gingr_model_new_reference(ctx.handle, self._src_dev.handle, self.numberOfPoints, dptr(self.reference),
                                                              iptr(self._ids), dptr(self._w), row_begin, row_end, ctypes.byref(h)),
               "gingr_model_new_reference")
        return h


class TruncatedDevicePointDistributionModel(_DerivedDevicePointDistributionModel):
    """model.truncate(k) of a model resident in HBM (gingr_model_truncate): the k leading basis functions, an independent model."""

    def __init__(self, source: "DeviceModel", k: int, cells=None):
        if source.row_begin != 0 or source.M_local != source.host.numberOfPoints:
            raise ValueError("truncate: the source is a row shard")
        self.ctx = source.ctx
        self.reference = f64(source.host.reference)
        self._src_dev, self._k = source, int(k)
        self.cells = cells
        if self._k < 1 or self._k > source.rank:
            raise ValueError(f"truncate: k = {self._k} outside 1..{source.rank} (the model's rank)")

    def _build(self, ctx: Context, row_begin: int, row_end: int):
        if ctx is not self.ctx or int(row_begin) != 0 or int(row_end) != self.numberOfPoints:
            raise ValueError("a truncated resident model lives whole on the context of its source; download it (to_host) for anything else")
        h = c_void_p()
        _check(ctx.handle, ctx._lib.gingr_model_truncate(ctx.handle, self._src_dev.handle, self._k, ctypes.byref(h)), "gingr_model_truncate")
        return h


class ExtendedDevicePointDistributionModel(_DerivedDevicePointDistributionModel):
    """A kernel-built model on other points (gingr_model_extend): every basis function evaluated at the new points from the kernel
    and the build's pivots (the Nystroem extension) -- exact on the source's own vertices, defined anywhere in space; zero mean, the
    source's variances.  Far from every pivot the extended model has no variance.  Carries `cells` of the new points."""

    def __init__(self, source: "DeviceModel", new_reference, cells=None):
        if not isinstance(source, DeviceModel):
            source = source.device()
        self.ctx = source.ctx
        self.reference = f64(new_reference).reshape(-1, 3)
        self._src_dev = source
        self.cells = None if cells is None else np.ascontiguousarray(cells, dtype=np.int32)

    def _build(self, ctx: Context, row_begin: int, row_end: int):
        if ctx is not self.ctx or int(row_begin) != 0 or int(row_end) != self.numberOfPoints:
            raise ValueError("an extended model lives whole on the context of its source; download it (to_host) for anything else")
        h = c_void_p()
        _check(ctx.handle, ctx._lib.gingr_model_extend(ctx.handle, self._src_dev.handle, self.numberOfPoints, dptr(self.reference),
                                                       ctypes.byref(h)), "gingr_model_extend")
        return h


class PosteriorDevicePointDistributionModel(_DerivedDevicePointDistributionModel):
    """model.transform(rigid).posterior(observations) as a model resident in HBM (gingr_model_posterior,
    gingr_fitter_posterior_model_*; computePosterior, GingrAlgorithm.scala:281-302): wraps the finished native model.  Reference and
    mean are the posterior's own (read back once, without the basis); basis and variance are downloaded only if somebody asks."""

    _ELSEWHERE = "a posterior model lives whole on the context of its source; download it (to_host) for anything else"

    def __init__(self, ctx: Context, handle, cells=None):
        self._adopt(ctx, handle, cells)


class PcaDevicePointDistributionModel(_DerivedDevicePointDistributionModel):
    """PointDistributionModel.createUsingPCA: the PCA model of shapes in correspondence, built in HBM (gingr_model_from_shapes) and
    adopted like a posterior model.  `pcaInfo` carries gingr_pca_info; reference (the Procrustes target for alignment = "gpa") and
    mean are read back once, basis and variance only if somebody asks."""

    ALIGNMENTS = {"none": 0, "rigid": 1, "gpa": 2}
    _ELSEWHERE = "a PCA model lives whole on the context it was built on; download it (to_host) for anything else"

    def __init__(self, ctx: Context, reference, shapes, alignment="none", relativeTolerance: float = 1e-10, maxRank: int = 0, cells=None,
                 gpaMaxIterations: int = 3, gpaTolerance: float = 1e-5):
        if alignment not in self.ALIGNMENTS:
            raise ValueError(f"alignment must be one of {sorted(self.ALIGNMENTS)}, not {alignment!r}")
        ref = f64(reference).reshape(-1, 3)
        X = f64(shapes)
        M = ref.shape[0]
        if X.ndim == 2 and X.shape[1] == 3 * M:
            X = X.reshape(X.shape[0], M, 3)
        if X.ndim != 3 or X.shape[1:] != (M, 3):
            raise ValueError(f"shapes must be (n, {M}, 3): every shape point for point on the reference")
        h, info = c_void_p(), nat.PcaInfo()
        _check(ctx.handle, ctx._lib.gingr_model_from_shapes(ctx.handle, M, int(X.shape[0]), dptr(ref), dptr(X), self.ALIGNMENTS[alignment],
                                                            int(gpaMaxIterations), float(gpaTolerance), float(relativeTolerance), int(maxRank),
                                                            ctypes.byref(h), ctypes.byref(info)), "gingr_model_from_shapes")
        self.pcaInfo = PcaInfo(int(info.rank), int(info.gpa_sweeps), float(info.gpa_last_change), float(info.total_variance),
                               float(info.kept_variance))
        self._adopt(ctx, h, cells, M)


class LaplacianDevicePointDistributionModel(_DerivedDevicePointDistributionModel):
    """The inverse-Laplacian model from the sparse graph Laplacian's own smallest eigenpairs (gingr_model_from_laplacian), built in
    HBM and adopted like a PCA model.  `laplacianInfo` carries gingr_laplacian_info -- also on the exception of a solve that did not
    converge (`.laplacianInfo` of the GingrNativeError); reference and mean are read back once, basis and variance only if somebody asks."""

    _ELSEWHERE = "a spectral inverse-Laplacian model lives whole on the context it was built on; download it (to_host) for anything else"

    def __init__(self, ctx: Context, reference, cells, scaling: float, pairs: int, tolerance: Optional[float] = None,
                 maxDegree: Optional[int] = None):
        ref = f64(reference).reshape(-1, 3)
        tri = np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 3)
        M = ref.shape[0]
        h, info = c_void_p(), nat.LaplacianInfo()
        rc = ctx._lib.gingr_model_from_laplacian(ctx.handle, M, dptr(ref), tri.shape[0], iptr(tri), float(scaling), int(pairs),
                                                 0.0 if tolerance is None else float(tolerance), 0 if maxDegree is None else int(maxDegree),
                                                 ctypes.byref(info), ctypes.byref(h))
        self.laplacianInfo = LaplacianInfo(int(info.n_components), int(info.n_dropped), int(info.block_columns), int(info.outer_iterations),
                                           int(info.total_degree), bool(info.converged), float(info.max_residual), float(info.cut_gap))
        try:
            _check(ctx.handle, rc, "gingr_model_from_laplacian")
        except nat.GingrNativeError as e:
            e.laplacianInfo = self.laplacianInfo
            raise
        self._adopt(ctx, h, tri, M)


class AugmentedDevicePointDistributionModel(_DerivedDevicePointDistributionModel):
    """PointDistributionModel.augmentModel: covariance and mean of two resident models added (gingr_model_augment), built in HBM and
    adopted like a PCA model.  `augmentInfo` carries gingr_augment_info; reference and mean are read back once, basis and variance only
    if somebody asks.  cells: the argument's, else the model's, else the bias's."""

    _ELSEWHERE = "an augmented model lives whole on the context it was built on; download it (to_host) for anything else"

    def __init__(self, ctx: Context, model, bias, relativeTolerance: float = 1e-10, maxRank: int = 0, biasTolerance: float = 0.01, cells=None,
                 _handle=None, _info=None):
        if _handle is None:
            if cells is None:
                cells = _cells_of(model)
            if not isinstance(bias, (DeviceModel, DevicePointDistributionModel, PointDistributionModel)):
                pars = list(bias)
                if not pars or not all(isinstance(p, GaussianKernelParameters) for p in pars):
                    raise ValueError("bias must be a model or a non-empty sequence of GaussianKernelParameters")
                ref = f64((model.host if isinstance(model, DeviceModel) else model).reference)
                bias = GPMMTriangleMesh3D(ctx, ref, biasTolerance, cells=cells).GaussianMixture(pars)
            if cells is None:
                cells = _cells_of(bias)
            (da, own_a), (db, own_b) = _resident(ctx, model), _resident(ctx, bias)
            try:
                _handle, _info = da._augment_native(db, relativeTolerance, maxRank)
            finally:
                for d, own in ((da, own_a), (db, own_b)):
                    if own:
                        d.close()
        self.augmentInfo = _info
        self._adopt(ctx, _handle, cells)


class LocalizedDevicePointDistributionModel(_DerivedDevicePointDistributionModel):
    """PointDistributionModel.localizeModel: a resident model's covariance under a Gaussian taper (gingr_model_localize), built in HBM
    and adopted like a PCA model.  `localizeInfo` carries gingr_localize_info; reference and mean are read back once, basis and
    variance only if somebody asks.  cells: the argument's, else the model's."""

    _ELSEWHERE = "a localized model lives whole on the context it was built on; download it (to_host) for anything else"

    def __init__(self, ctx: Context, model, sigma: float, relativeTolerance: float = 0.01, maxRank: int = 0, cells=None, _handle=None,
                 _info=None):
        if _handle is None:
            if cells is None:
                cells = _cells_of(model)
            d, own = _resident(ctx, model)
            try:
                _handle, _info = d._localize_native(sigma, relativeTolerance, maxRank)
            finally:
                if own:
                    d.close()
        self.localizeInfo = _info
        self._adopt(ctx, _handle, cells)


def _cells_of(model):
    return getattr(model.host if isinstance(model, DeviceModel) else model, "cells", None)


def _resident(ctx: Context, model) -> Tuple["DeviceModel", bool]:
    """(the complete model resident on ctx, whether the caller must close it): a DeviceModel as it is, a device-built model through its
    own handle, a host model uploaded"""
    if isinstance(model, DeviceModel):
        return model, False
    if isinstance(model, DevicePointDistributionModel):
        if model.ctx is not ctx:
            raise ValueError("the model lives on another context; download it (to_host) first")
        return model.device(), False
    return DeviceModel(ctx, model), True


@dataclasses.dataclass
class GaussianKernelParameters:
    """GPMMHelper.scala:94"""
    sigma: float
    scaling: float


class PointSetHelper:
    """GPMMHelper.scala:73-91: the O(n^2) scans behind the automatic kernel parameters, on the device."""

    def __init__(self, ctx: Context, reference):
        self.ctx, self.reference = ctx, f64(reference)
        self._ext: Optional[Tuple[float, float]] = None

    def _extrema(self) -> Tuple[float, float]:
        if self._ext is None:
            mx, mn = ctypes.c_double(), ctypes.c_double()
            _check(self.ctx.handle, self.ctx._lib.gingr_pointset_distance_extrema(
                self.ctx.handle, dptr(self.reference), self.reference.shape[0], ctypes.byref(mx), ctypes.byref(mn)),
                "gingr_pointset_distance_extrema")
            self._ext = (mx.value, mn.value)
        return self._ext

    def maximumPointDistance(self) -> float:
        return self._extrema()[0]

    def minimumPointDistance(self) -> float:
        return self._extrema()[1]


class GPMMTriangleMesh3D:
    """GPMMTriangleMesh3D(reference, relativeTolerance) (GPMMHelper.scala:96-153): every kernel of the reference, the low-rank
    factorisation built in HBM.  `cells` (the triangulation) is only needed by the Laplacian kernels; it is handed on to the model."""

    def __init__(self, ctx: Context, reference, relativeTolerance: float = 0.01, maxRank: int = 0, cells=None, toTolerance: bool = False):
        """toTolerance=False: maxRank columns at most, silently clamped to 512 (the rank limit of a model).  toTolerance=True: the
        reference's behaviour -- the factorisation runs until relativeTolerance is met (maxRank = 0) or to maxRank factor columns,
        and a model above rank 512 is an error that asks for .truncate(k) (see DevicePointDistributionModel)."""
        self.ctx, self.reference, self.relativeTolerance, self.maxRank = ctx, f64(reference), relativeTolerance, maxRank
        self.toTolerance = bool(toTolerance)
        self.cells = None if cells is None else np.ascontiguousarray(cells, dtype=np.int32)

    def Gaussian(self, sigma: float, scaling: float) -> DevicePointDistributionModel:
        return self.GaussianMixture([GaussianKernelParameters(sigma, scaling)])

    def GaussianMixture(self, pars: Sequence[GaussianKernelParameters]) -> DevicePointDistributionModel:
        return DevicePointDistributionModel(self.ctx, self.reference, [p.sigma for p in pars], [p.scaling for p in pars],
                                            self.relativeTolerance, self.maxRank, cells=self.cells, toTolerance=self.toTolerance)

    def AutomaticGaussian(self) -> DevicePointDistributionModel:
        mx = PointSetHelper(self.ctx, self.reference).maximumPointDistance()
        return self.GaussianMixture([GaussianKernelParameters(mx / 4.0, mx / 8.0), GaussianKernelParameters(mx / 8.0, mx / 16.0)])

    def _diagonal(self, kx: ScalarKernelSpec, ky: ScalarKernelSpec, kz: ScalarKernelSpec) -> DevicePointDistributionModel:
        return DevicePointDistributionModel(self.ctx, self.reference, [], [], self.relativeTolerance, self.maxRank,
                                            kernels=(kx, ky, kz), cells=self.cells, toTolerance=self.toTolerance)

    def GaussianDot(self, sigma: float, scaling: float) -> DevicePointDistributionModel:
        """GPMMHelper.scala:103-106: DotProductKernel(GaussianKernel(sigma), 1.0) * scaling.  DotProductKernel.k returns
        x.dot(y) and ignores both the wrapped kernel and gamma (KernelHelper.scala:43-51), so sigma has no effect -- mirrored."""
        k = ScalarKernelSpec("dot", scaling=scaling)
        return self._diagonal(k, k, k)

    def GaussianSymmetry(self, sigma: float, scaling: float) -> DevicePointDistributionModel:
        """GPMMHelper.scala:107-111 + KernelHelper.symmetrizeKernel (:25-31): DiagonalKernel(k, 3) + DiagonalKernel(-km, km, km)
        with km(x, y) = k((-x0, x1, x2), y): the x coordinate gets k - km, y and z get k + km."""
        kx = ScalarKernelSpec("gauss", (float(sigma),), (float(scaling),), mirror=-1.0)
        kyz = ScalarKernelSpec("gauss", (float(sigma),), (float(scaling),), mirror=1.0)
        return self._diagonal(kx, kyz, kyz)

    # -- radial terms with weight fields (gingr_gpmm_build_radial)
    def RadialMixture(self, terms) -> DevicePointDistributionModel:
        """k(x_i, x_j) = sum_t w_t[i] w_t[j] scaling_t f_t(|x_i - x_j|^2) on every coordinate: `terms` a list of at most eight
        RadialKernelTerm, or (termsX, termsY, termsZ) for coordinates that differ (the generic factorisation over the 3M entries)."""
        terms = list(terms)
        if len(terms) == 3 and not isinstance(terms[0], RadialKernelTerm):
            lists: dict = {}
            kernels = [lists.setdefault(id(t), list(t)) for t in terms]     # the same list twice stays one kernel
        else:
            kernels = [terms] * 3
        M = self.reference.shape[0]
        for k in kernels:
            for i, t in enumerate(k):
                if not isinstance(t, RadialKernelTerm):
                    raise TypeError(f"term {i} is {type(t).__name__}, not a RadialKernelTerm")
                if t.weight is not None and t.weight.shape[0] != M:
                    raise ValueError(f"term {i}: a weight field of {t.weight.shape[0]} values on a reference of {M} vertices")
        return DevicePointDistributionModel(self.ctx, self.reference, [], [], self.relativeTolerance, self.maxRank, cells=self.cells,
                                            toTolerance=self.toTolerance, radial=kernels)

    def RationalQuadratic(self, beta: float, scaling: float) -> DevicePointDistributionModel:
        """DiagonalKernel(RationalQuadratic(beta) * scaling, 3) (KernelHelper.scala:64-73)"""
        return self.RadialMixture([RadialKernelTerm("rationalQuadratic", beta, scaling)])

    def InverseMultiquadric(self, beta: float, scaling: float) -> DevicePointDistributionModel:
        """DiagonalKernel(InverseMultiquadric(beta) * scaling, 3) (KernelHelper.scala:53-61)"""
        return self.RadialMixture([RadialKernelTerm("inverseMultiquadric", beta, scaling)])

    @staticmethod
    def _terms(pars, weight) -> list:
        """`pars` (GaussianKernelParameters, or RadialKernelTerm without a field of their own) as terms weighted by `weight`"""
        out = []
        for p in pars:
            if isinstance(p, RadialKernelTerm):
                if p.weight is not None:
                    raise ValueError("a term that is given a field here must not bring one of its own")
                out.append(RadialKernelTerm(p.family, p.parameter, p.scaling, weight))
            else:
                out.append(RadialKernelTerm("gaussian", p.sigma, p.scaling, weight))
        return out

    def ScaledGaussian(self, pars: Sequence[GaussianKernelParameters], amplitude) -> DevicePointDistributionModel:
        """a(x) a(y) sum_i scaling_i exp(-|x-y|^2 / sigma_i^2): the Gaussian mixture with its amplitude a function of position --
        every term weighted by the one field `amplitude` (one value per vertex)."""
        a = f64(amplitude).reshape(-1)
        return self.RadialMixture(self._terms(pars, a))

    def ChangePoint(self, parsA, parsB, indicator) -> DevicePointDistributionModel:
        """scalismo's ChangePointKernel(kA, kB, s): s(x) s(y) kA(x, y) + (1 - s(x)) (1 - s(y)) kB(x, y) -- the terms of A weighted by
        `indicator`, then those of B by 1 - indicator.  The indicator (one value per vertex, e.g. sigmoidField) lies in [0, 1]."""
        s = f64(indicator).reshape(-1)
        if not np.all(np.isfinite(s)) or s.min(initial=0.0) < 0.0 or s.max(initial=0.0) > 1.0:
            raise ValueError("ChangePoint: the indicator must lie in [0, 1]")
        return self.RadialMixture(self._terms(parsA, s) + self._terms(parsB, 1.0 - s))

    def InverseLaplacian(self, scaling: float) -> DevicePointDistributionModel:
        """GPMMHelper.scala:132-136: LookupKernel(reference, pinv(graph Laplacian)) * scaling.  The dense pseudo-inverse is one-off
        host work exactly as in the reference (LaplacianHelper, MatrixHelper.pinv); the low-rank factorisation runs on the device."""
        k = ScalarKernelSpec("lookup", scaling=scaling, lookup=LaplacianHelper(self.reference.shape[0], self._need_cells()).inverseLaplacianMatrix())
        return self._diagonal(k, k, k)

    def InverseLaplacianSpectral(self, scaling: float, rank: int, tolerance: Optional[float] = None,
                                 maxDegree: Optional[int] = None) -> "LaplacianDevicePointDistributionModel":
        """The model of InverseLaplacian(scaling) built to a tight tolerance and truncated to `rank`, without the n x n pseudo-inverse
        (gingr_model_from_laplacian): its leading components are the rank / 3 smallest non-zero eigenpairs of the sparse graph
        Laplacian, each on x, y and z, found by a block eigensolver on the device.  `rank` is the model's rank, a multiple of 3, at most
        510.  tolerance: the residual bound relative to 2 * (largest vertex degree), default 1e-10; maxDegree: the budget of
        products of the Laplacian with the block (default: the library's).  A solve that does not converge within the budget raises;
        `.laplacianInfo` of the model (or of the exception) says what the solver did.
        There is no tolerance-driven rank: the trace of pinv(L) is not available without the whole spectrum, and the spectrum decays
        so slowly (1 % of the trace needs 629 of 660 components at 221 vertices) that a trace rule would mean nothing."""
        cells = self._need_cells()
        rank = int(rank)
        if rank < 3 or rank % 3 != 0:
            raise ValueError(f"rank = {rank}: the spectral inverse-Laplacian model holds every eigenvector on x, y and z, so its rank is a "
                             "positive multiple of 3")
        return LaplacianDevicePointDistributionModel(self.ctx, self.reference, cells, scaling, rank // 3, tolerance, maxDegree)

    def InverseLaplacianDot(self, scaling: float, gamma: float) -> DevicePointDistributionModel:
        """GPMMHelper.scala:138-142: DotProductKernel(LookupKernel(..), gamma) * scaling = scaling * x.y (see GaussianDot); the
        reference still computes the pseudo-inverse it never uses -- skipped."""
        return self.GaussianDot(0.0, scaling)

    def _need_cells(self) -> np.ndarray:
        if self.cells is None:
            raise ValueError("the Laplacian kernels need the triangulation: GPMMTriangleMesh3D(ctx, reference, tol, cells=...)")
        return self.cells

    def computeDistanceAbsMesh(self, model, lmId: int) -> np.ndarray:
        """GPMMHelper.scala:144-153: sum_i |cov(lmId, pid)_ii| per vertex, cov = U diag(variance) U^T (3 x 3 blocks).
        A device-resident model (DevicePointDistributionModel, DeviceModel) is read where it is: one cross-covariance pass
        instead of a download of the basis."""
        dm = model.device() if isinstance(model, DevicePointDistributionModel) else model
        if isinstance(dm, DeviceModel):
            c = dm.crossCovariance(int(lmId))
            return np.abs(c[:, 0, 0]) + np.abs(c[:, 1, 1]) + np.abs(c[:, 2, 2])
        U = f64(model.basis).reshape(model.numberOfPoints, 3, -1)
        w = U[int(lmId)] * f64(model.variance)[None, :]                   # (3, r)
        return np.abs(np.einsum("pdr,dr->pd", U, w)).sum(axis=1)


class LaplacianHelper:
    """G/api/gpmm/LaplacianHelper.scala:25-55 and MatrixHelper.pinv (MatrixHelper.scala:21-26): combinatorial graph Laplacian of
    the triangulation (degree on the diagonal, -1 for adjacent vertices) and its SVD pseudo-inverse with the 1e-5 cut-off."""

    def __init__(self, n: int, cells):
        self.n = int(n)
        c = np.asarray(cells, dtype=np.int64).reshape(-1, 3)
        a = np.zeros((self.n, self.n), dtype=bool)
        for i, j in ((0, 1), (1, 2), (0, 2)):
            a[c[:, i], c[:, j]] = True
            a[c[:, j], c[:, i]] = True
        np.fill_diagonal(a, False)
        self.adjacency = a

    def laplacianMatrix(self, inverse: bool = False) -> np.ndarray:
        m = np.where(self.adjacency, -1.0, 0.0)
        m[np.arange(self.n), np.arange(self.n)] = self.adjacency.sum(axis=1).astype(np.float64)
        return self.pinv(m) if inverse else m

    def inverseLaplacianMatrix(self) -> np.ndarray:
        return self.pinv(self.laplacianMatrix())

    def laplacianNormalizedMatrix(self, inverse: bool = False) -> np.ndarray:
        deg = self.adjacency.sum(axis=1).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.where(self.adjacency, -1.0 / np.sqrt(deg[:, None] * deg[None, :]), 0.0)
        m[np.arange(self.n), np.arange(self.n)] = (deg != 0).astype(np.float64)
        return self.pinv(m) if inverse else m

    @staticmethod
    def pinv(m: np.ndarray, precision: float = 0.00001) -> np.ndarray:
        u, s, vt = np.linalg.svd(m)
        return (u * np.where(s > precision, 1.0 / np.where(s > precision, s, 1.0), 0.0)[None, :]) @ vt


def automaticGPMMfromTemplate(ctx: Context, template, relativeTolerance: float = 0.1, toTolerance: bool = False) -> DevicePointDistributionModel:
    """registration/utils/GPMMHelper.scala:39-69 (on the model's own points the TriangleMeshInterpolator is the identity).
    toTolerance: see GPMMTriangleMesh3D."""
    h = PointSetHelper(ctx, template)
    mx, mn = h.maximumPointDistance(), h.minimumPointDistance()
    sig = [mx / 4, mx / 8, mn * 5]
    return DevicePointDistributionModel(ctx, template, sig, [v / 2 for v in sig], relativeTolerance, toTolerance=toTolerance)


class DeviceModel:
    """gingr_model: the (row shard of the) model resident in HBM.  `model` is either a host PointDistributionModel
    (uploaded) or a DevicePointDistributionModel (built on the device; full-row handles are shared with it)."""

    def __init__(self, ctx: Context, model, row_begin: int = 0, row_end: Optional[int] = None):
        self.ctx = ctx
        self._lib = ctx._lib
        self.host = model
        M = model.numberOfPoints
        row_end = M if row_end is None else row_end
        self._owner = True
        if isinstance(model, DevicePointDistributionModel):
            if int(row_begin) == 0 and int(row_end) == M and model.ctx is ctx:
                self.handle = model.device().handle     # shared, owned by the model
                self._owner = False
            else:
                self.handle = model._build(ctx, int(row_begin), int(row_end))
        else:
            ref, mean = f64(model.reference), f64(model.mean)
            basis = np.asfortranarray(model.basis, dtype=np.float64)   # column-major, as Breeze stores basisMatrix
            var = f64(model.variance)
            h = c_void_p()
            _check(ctx.handle, self._lib.gingr_model_upload(ctx.handle, M, model.rank, dptr(ref), dptr(mean),
                                                            basis.ctypes.data_as(nat._dp), dptr(var), int(row_begin),
                                                            int(row_end), ctypes.byref(h)), "gingr_model_upload")
            self.handle = h
        self.row_begin, self.row_end = int(row_begin), int(row_end)
        self.M_local = self.row_end - self.row_begin
        self.rank = int(self._lib.gingr_model_rank(self.handle))

    @classmethod
    def _adopt(cls, ctx: Context, handle, model, M: int) -> "DeviceModel":
        self = cls.__new__(cls)
        self.ctx, self._lib, self.host, self.handle, self._owner = ctx, ctx._lib, model, handle, True
        self.row_begin, self.row_end, self.M_local = 0, M, M
        self.rank = int(self._lib.gingr_model_rank(handle))
        return self

    def truncate(self, k: int) -> "DeviceModel":
        """The k leading basis functions as a new, independent resident model (gingr_model_truncate); complete models only."""
        if isinstance(self.host, PointDistributionModel):
            host = self.host.truncate(k)
            h = c_void_p()
            _check(self.ctx.handle, self._lib.gingr_model_truncate(self.ctx.handle, self.handle, int(k), ctypes.byref(h)), "gingr_model_truncate")
            return DeviceModel._adopt(self.ctx, h, host, host.numberOfPoints)
        return TruncatedDevicePointDistributionModel(self, k, cells=getattr(self.host, "cells", None)).device()

    def _augment_native(self, other: "DeviceModel", relativeTolerance: float, maxRank: int):
        if not isinstance(other, DeviceModel):
            raise TypeError("augment: the other model must be a DeviceModel")
        h, info = c_void_p(), nat.AugmentInfo()
        _check(self.ctx.handle, self._lib.gingr_model_augment(self.ctx.handle, self.handle, other.handle, float(relativeTolerance), int(maxRank),
                                                              ctypes.byref(h), ctypes.byref(info)), "gingr_model_augment")
        return h, AugmentInfo(int(info.columns), int(info.rank), float(info.total_variance), float(info.kept_variance))

    def augment(self, other: "DeviceModel", relativeTolerance: float = 1e-10, maxRank: int = 0) -> "DeviceModel":
        """This model augmented with `other` as a new resident model (gingr_model_augment): mean = the sum of the two means, covariance =
        the sum of the two covariances, re-diagonalised; both complete models of this context on the same reference, at most 512
        columns together.  The result is an ordinary DeviceModel, independent of both; its host (an
        AugmentedDevicePointDistributionModel) carries `augmentInfo`; cells are carried over from this model, else from the other."""
        h, info = self._augment_native(other, relativeTolerance, maxRank)
        cells = _cells_of(self)
        return AugmentedDevicePointDistributionModel(self.ctx, None, None, cells=cells if cells is not None else _cells_of(other), _handle=h,
                                                     _info=info).device()

    def _localize_native(self, sigma: float, relativeTolerance: float, maxRank: int):
        h, info = c_void_p(), nat.LocalizeInfo()
        _check(self.ctx.handle, self._lib.gingr_model_localize(self.ctx.handle, self.handle, float(sigma), float(relativeTolerance), int(maxRank),
                                                               ctypes.byref(h), ctypes.byref(info)), "gingr_model_localize")
        return h, LocalizeInfo(int(info.columns), int(info.rank), bool(info.tolerance_reached), float(info.residual_fraction),
                               float(info.total_variance), float(info.kept_variance))

    def localize(self, sigma: float, relativeTolerance: float = 0.01, maxRank: int = 0) -> "DeviceModel":
        """This model localized as a new resident model (gingr_model_localize): the covariance multiplied element-wise by the Gaussian
        taper exp(-|x - y|^2 / sigma^2) over the reference, factored to relativeTolerance (at most 512 columns) and re-diagonalised; the
        same reference and mean.  A complete model of this context.  The result is an ordinary DeviceModel, independent of this one;
        its host (a LocalizedDevicePointDistributionModel) carries `localizeInfo`; cells are carried over."""
        h, info = self._localize_native(sigma, relativeTolerance, maxRank)
        return LocalizedDevicePointDistributionModel(self.ctx, None, 0.0, cells=_cells_of(self), _handle=h, _info=info).device()

    def download(self, basis: bool = True) -> "PointDistributionModel":
        """Local rows back on the host in gingr_model_upload's layout (gingr_model_download)."""
        M, r = self.M_local, self.rank
        ref, mean, var = np.empty((M, 3)), np.empty((M, 3)), np.empty(r)
        U = np.empty((3 * M, r), order="F") if basis else None
        _check(self.ctx.handle, self._lib.gingr_model_download(self.ctx.handle, self.handle, dptr(ref), dptr(mean),
                                                               U.ctypes.data_as(nat._dp) if basis else None, dptr(var)),
               "gingr_model_download")
        return PointDistributionModel(reference=ref, mean=mean, basis=U, variance=var)

    def gram_exchange(self) -> Tuple[int, int]:
        p, n = c_void_p(), c_int64()
        _check(self.ctx.handle, self._lib.gingr_model_gram_exchange(self.handle, ctypes.byref(p), ctypes.byref(n)), "gram_exchange")
        return p.value, n.value

    def finalize(self):
        _check(self.ctx.handle, self._lib.gingr_model_finalize(self.ctx.handle, self.handle), "gingr_model_finalize")

    def separable(self) -> Tuple[bool, Tuple[int, int, int], bool]:
        """gingr_model_separable: (every basis column lives on one coordinate, columns per coordinate, the compact basis is kept)"""
        sep, compact, counts = ctypes.c_int32(), ctypes.c_int32(), (ctypes.c_int32 * 3)()
        _check(self.ctx.handle, self._lib.gingr_model_separable(self.handle, ctypes.byref(sep), counts, ctypes.byref(compact)),
               "gingr_model_separable")
        return bool(sep.value), tuple(counts), bool(compact.value)

    # ---- kernel extension: the model at points off its reference -------------------------------
    @property
    def kernelExtension(self) -> Optional["KernelExtensionInfo"]:
        """gingr_model_kernel_extension: the pivots per coordinate and whether the coordinates share one kernel, for a model that
        carries the extension (built from a kernel without lookup tables or weight fields; truncated or extended from one); else None.
        A query, except for a model of coordinate-wise different kernels before its first use: its pivots are counted by forming C."""
        avail, shared, counts = ctypes.c_int32(), ctypes.c_int32(), (ctypes.c_int32 * 3)()
        _check(self.ctx.handle, self._lib.gingr_model_kernel_extension(self.handle, ctypes.byref(avail), counts, ctypes.byref(shared)),
               "gingr_model_kernel_extension")
        return KernelExtensionInfo(tuple(int(c) for c in counts), bool(shared.value)) if avail.value else None

    def kernelExtensionCoefficients(self, d: int) -> Tuple[np.ndarray, np.ndarray]:
        """gingr_model_get_kernel_extension: (ids of coordinate d's pivots, C_d [pivots, rank]) -- basis row 3 x + d of a point x is
        sum_j k_d(x, p_j) C_d[j].  The ids index the reference of the model the extension was BUILT on: this model's own reference,
        unless it was made by extend(), which shares its source's extension and has other points -- read the ids of such a model
        against its source's reference."""
        info = self.kernelExtension
        n = info.counts[int(d)] if info is not None else 0          # (no extension: the native call names the reason)
        ids, C = np.empty(n, dtype=np.int32), np.empty((n, self.rank))
        _check(self.ctx.handle, self._lib.gingr_model_get_kernel_extension(self.ctx.handle, self.handle, int(d), iptr(ids), dptr(C)),
               "gingr_model_get_kernel_extension")
        return ids, C

    def _points(self, points) -> np.ndarray:
        P = f64(points)
        if P.ndim != 2 or P.shape[1] != 3:
            raise ValueError(f"points: expected (n, 3), got {P.shape}")
        return P

    def extend(self, points, cells=None) -> "DeviceModel":
        """This model on other points as a new resident model (gingr_model_extend): zero mean, the same variances, basis rows
        evaluated from the kernel at the points (the Nystroem extension) -- anywhere in space, not only on the surface.  The result
        is an ordinary DeviceModel, independent of this one; its host is an ExtendedDevicePointDistributionModel carrying `cells`."""
        return ExtendedDevicePointDistributionModel(self, points, cells=cells).device()

    def warpPoints(self, points, alpha, euler=(0, 0, 0), center=(0, 0, 0), translation=(0, 0, 0), scale: float = 1.0) -> np.ndarray:
        """s (R (x + u(x) - c) + c + t) for every point x (n x 3), u the model's deformation field for the coefficients alpha
        (gingr_model_warp_points): what extend(points).instance(alpha, ...) returns, without forming a basis of the points."""
        P, a, e, c, t = self._points(points), f64(alpha), f64(euler), f64(center), f64(translation)
        if a.shape != (self.rank,):
            raise ValueError(f"alpha: expected ({self.rank},), got {a.shape}")
        out = np.empty_like(P)
        _check(self.ctx.handle, self._lib.gingr_model_warp_points(self.ctx.handle, self.handle, dptr(a), dptr(e), dptr(c), dptr(t), float(scale),
                                                                  P.shape[0], dptr(P), dptr(out)), "gingr_model_warp_points")
        return out

    def close(self):
        if getattr(self, "handle", None):
            # (a model that outlives its context -- e.g. collected after Context.close() -- must not call into the freed context: its
            # device memory went with the context's process state; dropping the handle is all that is left to do)
            if self._owner and getattr(self.ctx, "handle", None):
                self._lib.gingr_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- stateless model operators ---------------------------------------------------------
    def instance(self, alpha, euler=(0, 0, 0), center=(0, 0, 0), translation=(0, 0, 0), scale: float = 1.0) -> np.ndarray:
        a, e, c, t = f64(alpha), f64(euler), f64(center), f64(translation)
        out = np.empty((self.M_local, 3))
        _check(self.ctx.handle, self._lib.gingr_model_instance(self.ctx.handle, self.handle, dptr(a), dptr(e), dptr(c), dptr(t),
                                                               float(scale), dptr(out)), "gingr_model_instance")
        return out

    def coefficients(self, mesh, euler=(0, 0, 0), center=(0, 0, 0), translation=(0, 0, 0)) -> np.ndarray:
        m, e, c, t = f64(mesh), f64(euler), f64(center), f64(translation)
        out = np.empty(self.rank)
        _check(self.ctx.handle, self._lib.gingr_model_coefficients(self.ctx.handle, self.handle, dptr(e), dptr(c), dptr(t),
                                                                   dptr(m), dptr(out)), "gingr_model_coefficients")
        return out

    def _ranks(self, ranks) -> np.ndarray:
        """ranks=None: the full rank only"""
        return np.ascontiguousarray([self.rank] if ranks is None else np.atleast_1d(ranks), dtype=np.int32)

    def _shapes(self, shapes) -> np.ndarray:
        X = f64(shapes)
        if X.ndim == 2:
            X = X[None]
        if X.ndim != 3 or X.shape[1:] != (self.M_local, 3):
            raise ValueError(f"shapes: expected (n, {self.M_local}, 3), got {X.shape}")
        return X

    def instances(self, alphas) -> np.ndarray:
        """ref + mean + Q0 alpha_i for every row of alphas (n x rank), n x M x 3, no pose (gingr_model_instances): one pass over the
        basis per 512 coefficient vectors instead of a fitter and a pass per vector."""
        A = f64(alphas)
        if A.ndim == 1:
            A = A[None]
        if A.ndim != 2 or A.shape[1] != self.rank:
            raise ValueError(f"alphas: expected (n, {self.rank}), got {A.shape}")
        out = np.empty((A.shape[0], self.M_local, 3))
        _check(self.ctx.handle, self._lib.gingr_model_instances(self.ctx.handle, self.handle, A.shape[0], dptr(A), dptr(out)),
               "gingr_model_instances")
        return out

    def _surface_cells(self, distance: str, cells) -> Optional[np.ndarray]:
        """None for distance="vertex"; for "surface" the triangles (t x 3 int32): `cells`, else the model's"""
        if distance == "vertex":
            return None
        if distance != "surface":
            raise ValueError(f"distance: 'vertex' or 'surface', got {distance!r}")
        cells = _cells_of(self) if cells is None else cells
        if cells is None:
            raise ValueError("distance='surface' needs the triangles: pass cells=, or use a model that carries them")
        return np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 3)

    def project(self, shapes, ranks=None, distance: str = "vertex", cells=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The shapes (n x M x 3, n <= 512) projected onto the k leading components for every k in ranks (gingr_model_generalization):
        (coefficients [n_ranks, n, rank], zero from entry k on; mean distance [n_ranks, n]; largest distance [n_ranks, n]) between each
        shape and its projection -- what truncate(k).coefficients(shape) and .instance give, shape by shape.  distance="vertex" (the
        default): vertex to corresponding vertex.  distance="surface" (gingr_model_generalization_surface): every vertex of the
        projection to the closest point on the surface of the shape, whose triangles are `cells`, else the model's; the same
        coefficients bit for bit."""
        X, k = self._shapes(shapes), self._ranks(ranks)
        c = self._surface_cells(distance, cells)
        n = X.shape[0]
        coef, avg, mx = np.empty((k.size, n, self.rank)), np.empty((k.size, n)), np.empty((k.size, n))
        if c is None:
            _check(self.ctx.handle, self._lib.gingr_model_generalization(self.ctx.handle, self.handle, n, dptr(X), k.size, iptr(k), dptr(coef),
                                                                         dptr(avg), dptr(mx)), "gingr_model_generalization")
        else:
            _check(self.ctx.handle, self._lib.gingr_model_generalization_surface(self.ctx.handle, self.handle, n, dptr(X), c.shape[0], iptr(c), k.size,
                                                                                 iptr(k), dptr(coef), dptr(avg), dptr(mx)),
                   "gingr_model_generalization_surface")
        return coef, avg, mx

    def posterior_mean(self, obs_points, weights, euler=(0, 0, 0), center=(0, 0, 0), translation=(0, 0, 0),
                       landmarks: Optional["LandmarkCorrespondences"] = None) -> Tuple[np.ndarray, np.ndarray]:
        o, w, e, c, t = f64(obs_points), f64(weights), f64(euler), f64(center), f64(translation)
        mean = np.empty((self.M_local, 3))
        coeffs = np.empty(self.rank)
        n, lp, lx, lc = _landmarks_native(landmarks)
        _check(self.ctx.handle, self._lib.gingr_model_posterior_mean(
            self.ctx.handle, self.handle, dptr(e), dptr(c), dptr(t), dptr(o), dptr(w), n, iptr(lp), dptr(lx), dptr(lc),
            dptr(mean), dptr(coeffs)), "gingr_model_posterior_mean")
        return mean, coeffs

    def posterior(self, obs_points, weights, euler=(0, 0, 0), center=(0, 0, 0), translation=(0, 0, 0),
                  landmarks: Optional["LandmarkCorrespondences"] = None) -> "DeviceModel":
        """model.transform(rigid).posterior(observations) as a new resident model (gingr_model_posterior): same arguments as
        posterior_mean.  The basis is rotated in HBM; the result is an ordinary DeviceModel (download, truncate, instance,
        coefficients, marginalCovariance, posterior again, a registration's prior), independent of this one; cells are carried over."""
        o, w, e, c, t = f64(obs_points), f64(weights), f64(euler), f64(center), f64(translation)
        n, lp, lx, lc = _landmarks_native(landmarks)
        h = c_void_p()
        _check(self.ctx.handle, self._lib.gingr_model_posterior(
            self.ctx.handle, self.handle, dptr(e), dptr(c), dptr(t), dptr(o), dptr(w), n, iptr(lp), dptr(lx), dptr(lc),
            ctypes.byref(h)), "gingr_model_posterior")
        return PosteriorDevicePointDistributionModel(self.ctx, h, cells=getattr(self.host, "cells", None)).device()

    def _factor(self, factor):
        if factor is None:
            return None
        W = f64(factor)
        if W.shape != (self.rank, self.rank):
            raise ValueError(f"factor must be ({self.rank}, {self.rank}), row-major")
        return W

    def marginalCovariance(self, factor=None, euler=(0, 0, 0)) -> np.ndarray:
        """(M_local, 6): {xx, xy, xz, yy, yz, zz} of R (Q0_i W)(Q0_i W)^T R^T per local point, Q0 = U sqrt(variance)
        (gingr_model_marginal_covariance).  factor None = identity: the prior marginal U_i diag(variance) U_i^T."""
        W, e = self._factor(factor), f64(euler)
        out = np.empty((self.M_local, 6))
        _check(self.ctx.handle, self._lib.gingr_model_marginal_covariance(self.ctx.handle, self.handle, dptr(W), dptr(e), dptr(out)),
               "gingr_model_marginal_covariance")
        return out

    def crossCovariance(self, pid: int, factor=None, euler=(0, 0, 0)) -> np.ndarray:
        """(M_local, 3, 3): R (Q0_i W)(Q0_pid W)^T R^T per local point for one GLOBAL point id (gingr_model_cross_covariance)."""
        W, e = self._factor(factor), f64(euler)
        out = np.empty((self.M_local, 3, 3))
        _check(self.ctx.handle, self._lib.gingr_model_cross_covariance(self.ctx.handle, self.handle, dptr(W), dptr(e), int(pid), dptr(out)),
               "gingr_model_cross_covariance")
        return out

