"""The records a registration is described by -- the enums, the fitting parameters, the correspondence lists, the general state and the
configuration / state pair of each algorithm -- with the reference's names and field order.  Plain data: nothing here calls into the
library, and the model and algorithm modules are only named in annotations.

  GeneralRegistrationState, ModelFittingParameters              G/api/GeneralRegistrationState.scala:28-41,
                                                                G/api/ModelFittingParameters.scala:31-57
  CpdConfiguration / CpdRegistrationState                       G/api/registration/config/CPD.scala:52-155
  IcpConfiguration / IcpRegistrationState                       G/api/registration/config/ICP.scala:54-107
  TemplateConfiguration / TemplateRegistrationState             G/api/registration/config/Template.scala:24-60
  GlobalTranformationType, FittingStatuses                      G/api/GlobalTranformationType.scala:20-24,
                                                                G/api/FittingStatuses.scala:22
"""
from __future__ import annotations

import dataclasses
from typing import TYPE_CHECKING, Callable, Optional, Tuple

import numpy as np

if TYPE_CHECKING:
    from .models import PointDistributionModel


# ----------------------------------------------------------------------------- enums
class GlobalTranformationType:  # sic: the reference spells it this way
    NoTransforms = 0
    RigidTransforms = 1
    SimilarityTransforms = 2


class FittingStatuses:
    None_ = 0
    Converged = 1
    MaxIteration = 2
    ModelFlexibilityError = 3


# ----------------------------------------------------------------------------- state records
@dataclasses.dataclass(frozen=True)
class EulerAngles:
    phi: float = 0.0
    theta: float = 0.0
    psi: float = 0.0


@dataclasses.dataclass(frozen=True)
class ModelFittingParameters:
    """scale, pose = (translation, Euler rotation about a centre), shape  (ModelFittingParameters.scala:31-57)."""
    scale: float
    translation: Tuple[float, float, float]
    rotation: EulerAngles
    center: Tuple[float, float, float]
    shape: np.ndarray

    @staticmethod
    def zero(rank: int) -> "ModelFittingParameters":
        return ModelFittingParameters(1.0, (0.0, 0.0, 0.0), EulerAngles(), (0.0, 0.0, 0.0), np.zeros(rank))


@dataclasses.dataclass
class LandmarkCorrespondences:
    """(pid, target point, 3x3 covariance) triples (GeneralRegistrationState.scala:43-62)."""
    pids: np.ndarray
    points: np.ndarray
    covs: np.ndarray


@dataclasses.dataclass(frozen=True)
class CorrespondencePairs:
    """(PointId, Point) pairs (G/api/CorrespondencePairs.scala:23)."""
    pids: np.ndarray
    points: np.ndarray


@dataclasses.dataclass(frozen=True)
class GeneralRegistrationState:
    model: PointDistributionModel
    modelParameters: ModelFittingParameters
    target: np.ndarray
    fit: np.ndarray
    sigma2: float = 1.0
    globalTransformation: int = GlobalTranformationType.RigidTransforms
    stepLength: float = 1.0
    generatedBy: str = ""
    iteration: int = 0
    status: int = FittingStatuses.None_
    landmarkCorrespondences: Optional[LandmarkCorrespondences] = None
    targetCells: Optional[np.ndarray] = None   # (T,3) int: triangulation of the target mesh (surface ICP only)

    def updateStatus(self, status: int) -> "GeneralRegistrationState":
        return dataclasses.replace(self, status=status)

    def updateSigma2(self, s2: float) -> "GeneralRegistrationState":
        return dataclasses.replace(self, sigma2=s2)

    def statusText(self) -> str:
        """GeneralRegistrationState.printStatus (GeneralRegistrationState.scala:103-114)"""
        n = self.iteration + 1
        return {FittingStatuses.None_: "Initial state - no iterations performed!",
                FittingStatuses.Converged: f"Fitting converged after {n} accepted iterations!",
                FittingStatuses.MaxIteration: f"Fitting finished the MaxIterations with ({n}) accepted iterations!",
                FittingStatuses.ModelFlexibilityError:
                    f"Model not flexible enough to compute posterior model - finished after {n} accepted iterations!"}[self.status]

    def printStatus(self) -> None:
        print(self.statusText())


# ----------------------------------------------------------------------------- configs
def _cpd_converged(last: GeneralRegistrationState, current: GeneralRegistrationState, threshold: float) -> bool:
    return abs(last.sigma2 - current.sigma2) < threshold          # CPD.scala:108-110


def _never_converged(last, current, threshold) -> bool:
    return False                                                   # ICP.scala:57-58


@dataclasses.dataclass(frozen=True)
class CpdConfiguration:
    maxIterations: int = 100
    threshold: float = 1e-10
    converged: Callable = _cpd_converged
    useLandmarkCorrespondence: bool = True
    initialSigma: Optional[float] = None
    w: float = 0.0
    lambda_: float = 1.0


@dataclasses.dataclass(frozen=True)
class IcpConfiguration:
    maxIterations: int = 100
    threshold: float = 1e-10
    converged: Callable = _never_converged
    useLandmarkCorrespondence: bool = True
    initialSigma: float = 100.0
    endSigma: float = 1.0
    reverseCorrespondenceDirection: bool = False
    correspondenceMethod: str = "TriangularClosestPoint"    # the reference's default (ICP.scala:63); needs both triangulations

    @property
    def sigmaStep(self) -> float:
        return (self.initialSigma - self.endSigma) / float(self.maxIterations)


@dataclasses.dataclass(frozen=True)
class CpdRegistrationState:
    general: GeneralRegistrationState
    config: CpdConfiguration

    def updateGeneral(self, update: GeneralRegistrationState) -> "CpdRegistrationState":
        return dataclasses.replace(self, general=update)


@dataclasses.dataclass(frozen=True)
class IcpRegistrationState:
    general: GeneralRegistrationState
    config: IcpConfiguration

    def updateGeneral(self, update: GeneralRegistrationState) -> "IcpRegistrationState":
        return dataclasses.replace(self, general=update)


def _with_fields(obj, **changes):
    """dataclasses.replace for the plain frozen dataclasses above (no __post_init__, no slots), without its per-field machinery: 1 us
    instead of 7 for a GeneralRegistrationState -- the fused Metropolis-Hastings step builds two objects per step."""
    new = object.__new__(type(obj))
    d = new.__dict__
    d.update(obj.__dict__)
    d.update(changes)
    return new


# ----------------------------------------------------------------------------- Template: correspondence and uncertainty from the host
@dataclasses.dataclass(frozen=True)
class TemplateConfiguration:
    """TemplateConfiguration (G/api/registration/config/Template.scala:24-29)."""
    maxIterations: int = 1
    threshold: float = 1e-5
    converged: Callable = _never_converged
    useLandmarkCorrespondence: bool = True


@dataclasses.dataclass(frozen=True)
class TemplateRegistrationState:
    general: GeneralRegistrationState
    config: TemplateConfiguration

    def updateGeneral(self, update: GeneralRegistrationState) -> "TemplateRegistrationState":
        return dataclasses.replace(self, general=update)


# ----------------------------------------------------------------------------- point-to-plane ICP, correspondence on the device
ROBUST_LOSSES = {"cauchy": 1, "huber": 2, "tukey": 3}
ROBUST_TUNINGS = {"cauchy": 2.385, "huber": 1.345, "tukey": 4.685}     # 95 % efficiency at the normal distribution


@dataclasses.dataclass(frozen=True)
class RobustLoss:
    """M-estimator weighting of point-to-plane ICP (gingr_robust_params): every observed vertex's variance is sigma2 * u, u >= 1 from
    its residual s (the squared distance in the metric of its observation) and a scale c --
    cauchy u = 1 + s / c^2, huber u = max(1, sqrt(s) / c), tukey u = 1 / (1 - s / c^2)^2 and no observation from s >= c^2 on.
    scale="median": c = tuning * 1.4826 * sqrt(lower median of s over the observed vertices), found on the device every iteration
    (tuning None: the loss's 95 % constant -- 2.385, 1.345, 4.685); scale=a float: c itself, fixed.  minScale: a floor under c."""
    kind: str
    scale: object = "median"
    tuning: Optional[float] = None
    minScale: float = 0.0

    def __post_init__(self):
        if self.kind not in ROBUST_LOSSES:
            raise ValueError(f"RobustLoss: kind {self.kind!r}; need one of {sorted(ROBUST_LOSSES)}")
        if isinstance(self.scale, str):
            if self.scale != "median":
                raise ValueError(f"RobustLoss: scale {self.scale!r}; need \"median\" or a positive number")
            value = ROBUST_TUNINGS[self.kind] if self.tuning is None else float(self.tuning)
        else:
            if self.tuning is not None:
                raise ValueError("RobustLoss: a tuning constant goes with scale=\"median\"")
            value = float(self.scale)
        if not (np.isfinite(value) and value > 0.0):
            raise ValueError(f"RobustLoss: scale / tuning {value!r}; need a finite number > 0")
        if not (np.isfinite(self.minScale) and self.minScale >= 0.0):
            raise ValueError(f"RobustLoss: minScale {self.minScale!r}; need a finite number >= 0")

    @property
    def native(self) -> Tuple[int, int, float, float]:
        """(loss, scale_mode, scale, min_scale) of gingr_robust_params"""
        if isinstance(self.scale, str):
            return ROBUST_LOSSES[self.kind], 1, ROBUST_TUNINGS[self.kind] if self.tuning is None else float(self.tuning), float(self.minScale)
        return ROBUST_LOSSES[self.kind], 0, float(self.scale), float(self.minScale)


@dataclasses.dataclass(frozen=True)
class PointToPlaneConfiguration:
    """Point-to-plane ICP on the surfaces: ICP's sigma2 schedule (ICP.scala:65, :96-99) with a covariance per vertex that is sigma2 along
    the target's face normal and tangentOverNormal * sigma2 across it.  reject: the three rejection rules of the surface ICP.
    maxDistance (against a point-cloud target only): a vertex farther than this from its nearest target point is not observed.
    robust: M-estimator weights on top (RobustLoss); None: plain."""
    maxIterations: int = 100
    initialSigma: float = 100.0
    endSigma: float = 1.0
    tangentOverNormal: float = 100.0
    reject: bool = False
    threshold: float = 1e-10
    converged: Callable = _never_converged
    useLandmarkCorrespondence: bool = True
    maxDistance: Optional[float] = None
    robust: Optional[RobustLoss] = None

    @property
    def sigmaStep(self) -> float:
        return (self.initialSigma - self.endSigma) / float(self.maxIterations)


@dataclasses.dataclass(frozen=True)
class PointToPlaneRegistrationState:
    general: GeneralRegistrationState
    config: PointToPlaneConfiguration
    # against a point-cloud target: an (N, 3) array of normals, one per target point, or "estimate" (from targetNeighbours nearest
    # neighbours on the device); None: the surface route, normals of the target's triangles
    targetNormals: object = None
    targetNeighbours: int = 16

    def updateGeneral(self, update: GeneralRegistrationState) -> "PointToPlaneRegistrationState":
        return dataclasses.replace(self, general=update)


def _empty_pairs() -> CorrespondencePairs:
    return CorrespondencePairs(np.empty(0, dtype=np.int64), np.empty((0, 3)))

