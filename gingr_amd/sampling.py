"""Host side of GiNGR's probabilistic registration (BASELINE config 5: Metropolis-Hastings over GiNGR updates): evaluators,
proposal generators, the chain and the accuracy metrics, with every data-parallel step on the GPU --

  the informed proposal                  GingrAlgorithm.update(probabilistic = true)        (native posterior sample)
  its transition density                 GingrAlgorithm.logTransitionProbability            (native posterior log-density)
  the likelihood                         IndependentPointDistanceEvaluator                  (native closest-point reduction)
  re-instantiating a random-walk proposal GingrAlgorithm.proposeParameters                  (native model instance)

and only r-sized arithmetic and control flow here.  Mirrors (G/ = src/main/scala/gingr/):

  IndependentPointDistanceEvaluator, EvaluationMode      G/api/sampling/evaluators/IndependentPointDistanceEvaluator.scala:27-84
  ModelEvaluator, AcceptAllEvaluator, EvaluatorWrapper   G/api/sampling/evaluators/{ModelEvaluator,AcceptAllEvaluator,EvaluatorWrapper}.scala
  IndependentPoints, AcceptAll                           G/api/sampling/Evaluator.scala:33-60
  RandomShapeUpdateProposal                              G/api/sampling/generators/RandomShapeUpdateProposal.scala:22-50
  GaussianAxisRotation/TranslationProposal               G/api/sampling/generators/RandomPoseUpdateProposal.scala:28-117
  Generator (RandomShape/Rotation/Translation/Pose, DefaultRandom)   G/api/sampling/Generator.scala:25-88
  GeneratorWrapperStochastic / Deterministic             G/api/sampling/generators/GeneratorWrapper{Stochastic,Deterministic}.scala
  BestAndCurrentSampleLogger, JSONStateLogger            G/api/sampling/loggers/{BestAndCurrentSampleLogger,JSONStateLogger}.scala
  run(...)                                               G/api/GingrAlgorithm.scala:115-190
  RegistrationComparison                                 G/api/helper/RegistrationComparison.scala:22-99

scalismo's MixtureProposal and MetropolisHastings (1.0-RC1, not vendored) are restated from their published behaviour
[SCALISMO-RECALL, parity unpinned]: a mixture picks the first component whose cumulative normalised weight reaches one
uniform draw, its transition density is the weighted sum of the components' densities; a Metropolis-Hastings step accepts when
a = log p(proposal) - log p(current) - (log q(current -> proposal) - log q(proposal -> current)) is positive or a uniform draw is
below exp(a), where the bracket counts as 0 when both densities are -inf (the deterministic wrapper).

Random numbers: the JVM streams (scala.util.Random behind scalismo.utils.Random, and breeze's FixedSeed basis used by the pose
proposals) cannot be reproduced; `Random` below carries two numpy generators in their place and the call ORDER of the reference
is kept, including the discarded draw of GaussianAxisTranslationProposal (RandomPoseUpdateProposal.scala:89).
"""
from __future__ import annotations

import dataclasses
import math
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from .api import (Context, EulerAngles, FittingStatuses, GingrAlgorithm, ModelFittingParameters)

ModelToTargetEvaluation = "ModelToTargetEvaluation"
TargetToModelEvaluation = "TargetToModelEvaluation"
SymmetricEvaluation = "SymmetricEvaluation"


class Random:
    """scalismo.utils.Random (`scalaRandom`) plus breeze's Rand.FixedSeed basis."""

    def __init__(self, seed: int, breeze_seed: int = 0):
        self.scalaRandom = np.random.default_rng(seed)
        self.breeze = np.random.default_rng(breeze_seed)

    def nextDouble(self) -> float:
        return float(self.scalaRandom.random())

    def nextGaussian(self, n: Optional[int] = None):
        return self.scalaRandom.standard_normal(n) if n is not None else float(self.scalaRandom.standard_normal())

    def breezeGaussian(self, sdev: float) -> float:
        return float(self.breeze.standard_normal()) * sdev


def gaussian_logpdf(x: float, sdev: float) -> float:
    """breeze Gaussian(0, sdev).logPdf(x) / scalismo GaussianEvaluator.logDensity(x, 0, sdev)."""
    d = x / sdev
    return -d * d / 2.0 - (math.log(math.sqrt(2.0 * math.pi)) + math.log(sdev))


class _Memoize:
    """scalismo.utils.Memoize(f, n): the last n results, keyed by the state object."""

    def __init__(self, f: Callable, n: int):
        self.f, self.n, self.keys, self.vals = f, n, [], []

    def __call__(self, state):
        for i, k in enumerate(self.keys):
            if k is state:
                v = self.vals[i]
                if i != len(self.keys) - 1:      # least recently USED goes first: the current sample of a chain is asked about every
                    self.keys.append(self.keys.pop(i))   # step and must not age out behind three rejected proposals (a cache only:
                    self.vals.append(self.vals.pop(i))   # the values are the same either way)
                return v
        v = self.f(state)
        self.keys.append(state)
        self.vals.append(v)
        if len(self.keys) > self.n:
            self.keys.pop(0)
            self.vals.pop(0)
        return v


# ------------------------------------------------------------------------------------------------------------ evaluators
class IndependentPointDistanceEvaluator:
    """Sum over the compared points of log N(|p - closestPointOnSurface(p)|; 0, uncertainty), reduced on the GPU.

    `uncertainty` stands for the reference's `likelihoodModel = Gaussian(0, uncertainty)` (Evaluator.scala:47).  The reference's
    numberOfPointsForComparison decimates instance and target (:44-50); scalismo's mesh decimation is not restated, so the vertex
    clustering of this package stands in for it (`Context.mesh_decimate` on the algorithm's context, the result of
    `simple.cluster_decimate`): `sample`'s fit with the model's cells and its target are decimated once, here.  What the
    comparison then uses -- the first n' vertices of a sample (point ids of the decimated instance, :49-50,55) and the points of
    the decimated target (:49) -- can be passed in directly as modelPointCount / targetPoints instead; both at once is an error."""

    def __init__(self, algorithm: GingrAlgorithm, sample, uncertainty: float, evaluationMode: str = ModelToTargetEvaluation,
                 numberOfPointsForComparison: Optional[int] = None, modelPointCount: Optional[int] = None, targetPoints=None):
        if evaluationMode not in (ModelToTargetEvaluation, TargetToModelEvaluation, SymmetricEvaluation):
            raise ValueError(evaluationMode)
        if numberOfPointsForComparison is not None:
            if modelPointCount is not None or targetPoints is not None:
                raise ValueError("numberOfPointsForComparison and modelPointCount / targetPoints exclude each other")
            g, n = sample.general, int(numberOfPointsForComparison)
            kept, _, _ = algorithm.ctx.mesh_decimate(g.fit, g.model.cells, n)
            modelPointCount = int(kept.shape[0])
            target = np.ascontiguousarray(g.target, dtype=np.float64).reshape(-1, 3)
            tkept, _, _ = algorithm.ctx.mesh_decimate(target, g.targetCells, n)
            targetPoints = target[tkept]
        self.algorithm, self.uncertainty, self.evaluationMode = algorithm, float(uncertainty), evaluationMode
        self.modelPointCount = modelPointCount
        self.targetPoints = None if targetPoints is None else np.ascontiguousarray(targetPoints, dtype=np.float64)
        self._memo = _Memoize(self.computeLogValue, 3)       # EvaluationCaching (EvaluationCaching.scala:26-37)

    def distModelToTarget(self, state) -> float:
        return self.algorithm.surfaceDistanceStats(state, 0, self.modelPointCount or 0, None, False, self.uncertainty)[3]

    def distTargetToModel(self, state) -> float:
        return self.algorithm.surfaceDistanceStats(state, 1, 0, self.targetPoints, False, self.uncertainty)[3]

    def computeLogValue(self, state) -> float:
        if self.evaluationMode == ModelToTargetEvaluation:
            return self.distModelToTarget(state)
        if self.evaluationMode == TargetToModelEvaluation:
            return self.distTargetToModel(state)
        return 0.5 * self.distModelToTarget(state) + 0.5 * self.distTargetToModel(state)

    def logValue(self, state) -> float:
        return self._memo(state)


class ModelEvaluator:
    """log N(shape coefficients; 0, I_r)  (ModelEvaluator.scala:25-33)."""

    def __init__(self, modelrank: int):
        self.modelrank = modelrank

    def logValue(self, state) -> float:
        a = np.asarray(state.general.modelParameters.shape, dtype=np.float64)
        return float(-0.5 * (a @ a) - 0.5 * self.modelrank * math.log(2.0 * math.pi))


class AcceptAllEvaluator:
    def logValue(self, state) -> float:
        return 0.0


class ProductEvaluator:
    """scalismo.sampling.evaluators.ProductEvaluator: the sum of the log values."""

    def __init__(self, evaluators: Sequence):
        self.evaluators = list(evaluators)

    def logValue(self, state) -> float:
        return float(sum(e.logValue(state) for e in self.evaluators))


@dataclasses.dataclass
class EvaluatorIdentifier:
    name: str
    evaluator: object


class AcceptAll:
    def evaluator(self) -> List[EvaluatorIdentifier]:
        return [EvaluatorIdentifier("AcceptAll", AcceptAllEvaluator())]

    def productEvaluator(self) -> ProductEvaluator:
        return ProductEvaluator([e.evaluator for e in self.evaluator()])


class IndependentPoints(AcceptAll):
    """Prior on the coefficients x independent point distances (Evaluator.scala:41-60)."""

    def __init__(self, algorithm: GingrAlgorithm, state, uncertainty: float, mode: str = ModelToTargetEvaluation,
                 evaluatedPoints: Optional[int] = None, modelPointCount: Optional[int] = None, targetPoints=None):
        self._evals = [
            EvaluatorIdentifier("Prior", ModelEvaluator(state.general.model.rank)),
            EvaluatorIdentifier("Distance", IndependentPointDistanceEvaluator(algorithm, state, uncertainty, mode, evaluatedPoints,
                                                                              modelPointCount, targetPoints)),
        ]

    def evaluator(self) -> List[EvaluatorIdentifier]:
        return self._evals


class EvaluatorWrapper:
    def __init__(self, probabilistic: bool, evaluator: AcceptAll):
        self.probabilistic, self._eval = probabilistic, evaluator.productEvaluator()

    def logValue(self, state) -> float:
        return self._eval.logValue(state) if self.probabilistic else 0.0


@dataclasses.dataclass
class ProbabilisticSettings:
    evaluators: AcceptAll
    randomMixture: float = 0.5
    fusedSteps: bool = True      # (no reference counterpart) one native call per Metropolis-Hastings step where the set-up allows it

    def __post_init__(self):
        if not (0.0 <= self.randomMixture <= 1.0):
            raise ValueError("requirement failed: randomMixture in [0, 1]")


# ------------------------------------------------------------------------------------------------------------ generators
def _same_parameters(a: ModelFittingParameters, b: ModelFittingParameters) -> bool:
    return (a.scale == b.scale and tuple(a.translation) == tuple(b.translation) and a.rotation == b.rotation
            and tuple(a.center) == tuple(b.center) and np.array_equal(np.asarray(a.shape), np.asarray(b.shape)))


_last_diff = [None, None, frozenset()]
_skip_sets: dict = {}


def _differing_fields(a: ModelFittingParameters, b: ModelFittingParameters) -> frozenset:
    """The fields in which two parameter sets differ, remembered for the pair of OBJECTS last asked about (either order): one
    Metropolis-Hastings step puts the same (from, to) pair to nine random-walk components, twice."""
    c = _last_diff
    if (c[0] is a and c[1] is b) or (c[0] is b and c[1] is a):
        return c[2]
    d = []
    if a.scale != b.scale:
        d.append("scale")
    if a.translation is not b.translation and tuple(a.translation) != tuple(b.translation):
        d.append("translation")
    if a.rotation is not b.rotation and a.rotation != b.rotation:
        d.append("rotation")
    if a.center is not b.center and tuple(a.center) != tuple(b.center):
        d.append("center")
    if a.shape is not b.shape and not _shapes_equal(a.shape, b.shape):
        d.append("shape")
    c[0], c[1], c[2] = a, b, frozenset(d)
    return c[2]


def _same_except(a: ModelFittingParameters, b: ModelFittingParameters, skip: Tuple[str, ...]) -> bool:
    """a == b in every field but `skip` -- what `to.copy(field = from.field) == from` of the reference's proposals tests, without
    building the copy (a Metropolis-Hastings step asks nine random-walk components twice; the shape vectors of two states that
    differ by a pose proposal are the same object)."""
    if a is b:
        return True
    allowed = _skip_sets.get(skip)
    if allowed is None:
        allowed = _skip_sets[skip] = frozenset(skip)
    return _differing_fields(a, b) <= allowed


_last_shape_pair = [None, None, False]


def _shapes_equal(x, y) -> bool:
    """np.array_equal of two coefficient vectors, remembered for the pair of OBJECTS last asked about: one Metropolis-Hastings step
    puts the same (from, to) pair to six pose components in both directions (arrays are treated as immutable, like everywhere here)."""
    c = _last_shape_pair
    if (c[0] is x and c[1] is y) or (c[0] is y and c[1] is x):
        return c[2]
    eq = bool(np.array_equal(np.asarray(x), np.asarray(y)))
    c[0], c[1], c[2] = x, y, eq
    return eq


class RandomShapeUpdateProposal:
    symmetric = True   # q(to | from) is a function of (to - from)^2 and of which fields agree: the same bits for the swapped pair

    def __init__(self, algorithm: GingrAlgorithm, stdev: float, rnd: Random, generatedBy: str = "RandomShapeUpdateProposal"):
        self.algorithm, self.stdev, self.rnd, self.generatedBy = algorithm, float(stdev), rnd, generatedBy

    def propose(self, theta):
        mp = theta.general.modelParameters
        a = np.asarray(mp.shape, dtype=np.float64)
        if a.shape[0] == 0:
            raise ValueError("requirement failed: cannot propose change on empty vector")
        new = a + self.stdev * self.rnd.nextGaussian(a.shape[0])            # GaussianDenseVectorProposal.propose (:29-32)
        return self.algorithm.proposeParameters(theta, dataclasses.replace(mp, shape=new), self.generatedBy)

    def logTransitionProbability(self, frm, to) -> float:
        f, t = frm.general.modelParameters, to.general.modelParameters
        if not _same_except(t, f, ("shape",)):
            return -math.inf
        d = (np.asarray(t.shape, dtype=np.float64) - np.asarray(f.shape, dtype=np.float64)) / self.stdev
        terms = -d * d / 2.0 - (math.log(math.sqrt(2.0 * math.pi)) + math.log(self.stdev))    # GaussianEvaluator.logDensity per entry
        return float(terms.sum())


RollAxis, PitchAxis, YawAxis = "phi", "theta", "psi"


class GaussianAxisRotationProposal:
    symmetric = True   # q(to | from) is a function of (to - from)^2 and of which fields agree: the same bits for the swapped pair

    def __init__(self, algorithm: GingrAlgorithm, sdevRot: float, axis: str, rnd: Random, generatedBy: str = "RotationProposal"):
        self.algorithm, self.sdev, self.axis, self.rnd, self.generatedBy = algorithm, float(sdevRot), axis, rnd, generatedBy

    def propose(self, theta):
        mp = theta.general.modelParameters
        rot = dataclasses.replace(mp.rotation, **{self.axis: getattr(mp.rotation, self.axis) + self.rnd.breezeGaussian(self.sdev)})
        return self.algorithm.proposeParameters(theta, dataclasses.replace(mp, rotation=rot), self.generatedBy)

    def logTransitionProbability(self, frm, to) -> float:
        f, t = frm.general.modelParameters, to.general.modelParameters
        if not _same_except(t, f, ("rotation", "center")):
            return -math.inf
        return gaussian_logpdf(getattr(t.rotation, self.axis) - getattr(f.rotation, self.axis), self.sdev)


class GaussianAxisTranslationProposal:
    symmetric = True   # q(to | from) is a function of (to - from)^2 and of which fields agree: the same bits for the swapped pair

    def __init__(self, algorithm: GingrAlgorithm, sdevTrans: float, axis: int, rnd: Random, generatedBy: str = "TranslationProposal"):
        if not axis < 3:
            raise ValueError("requirement failed")
        self.algorithm, self.sdev, self.axis, self.rnd, self.generatedBy = algorithm, float(sdevTrans), axis, rnd, generatedBy

    def propose(self, theta):
        self.rnd.breezeGaussian(self.sdev)                                   # the discarded sample (:89)
        mp = theta.general.modelParameters
        t = list(mp.translation)
        t[self.axis] = t[self.axis] + self.rnd.breezeGaussian(self.sdev)
        return self.algorithm.proposeParameters(theta, dataclasses.replace(mp, translation=tuple(t)), self.generatedBy)

    def logTransitionProbability(self, frm, to) -> float:
        f, t = frm.general.modelParameters, to.general.modelParameters
        if not _same_except(t, f, ("translation",)):
            return -math.inf
        return gaussian_logpdf(t.translation[self.axis] - f.translation[self.axis], self.sdev)


class MixtureProposal:
    """scalismo MixtureProposal with transition probability [SCALISMO-RECALL]."""

    def __init__(self, components: Sequence[Tuple[float, object]], rnd: Random):
        tot = float(sum(w for w, _ in components))
        self.factors = [w / tot for w, _ in components]
        self.generators = [g for _, g in components]
        self.cumulative = list(np.cumsum(self.factors))
        self.rnd = rnd
        # a mixture of symmetric random walks is symmetric: a Metropolis-Hastings step asks for q(to | from) and q(from | to) of the same
        # pair of state objects, the second answer is the first (thirteen component calls less per step for the stock mixture)
        self.symmetric = all(getattr(g, "symmetric", False) for g in self.generators)
        self._sym = None

    def propose(self, current):
        r = self.rnd.nextDouble()
        i = next((k for k, c in enumerate(self.cumulative) if c >= r), len(self.generators) - 1)
        return self.generators[i].propose(current)

    def logTransitionProbability(self, frm, to) -> float:
        if self.symmetric:
            m = self._sym
            if m is not None and ((m[0] is frm and m[1] is to) or (m[0] is to and m[1] is frm)):
                return m[2]
        s = 0.0
        for f, g in zip(self.factors, self.generators):
            t = g.logTransitionProbability(frm, to)
            if t != t:
                raise ArithmeticError("NaN transition probability encountered!")
            if t != -math.inf:
                s += f * math.exp(t)
        out = math.log(s) if s > 0 else -math.inf
        if self.symmetric:
            self._sym = (frm, to, out)
        return out


class Generator:
    """The reference's stock random-walk mixtures (Generator.scala:25-88)."""

    defaultTranslation = 0.1
    defaultRotation = 0.01

    def __init__(self, algorithm: GingrAlgorithm, rnd: Random):
        self.algorithm, self.rnd = algorithm, rnd

    def RandomShape(self, steps: Sequence[float] = (1.0, 0.1, 0.01)) -> MixtureProposal:
        return MixtureProposal([(1.0 / len(steps), RandomShapeUpdateProposal(self.algorithm, d, self.rnd, f"RandomShape-{d}"))
                                for d in steps], self.rnd)

    def RandomRotation(self, rotYaw=None, rotPitch=None, rotRoll=None) -> MixtureProposal:
        y, p, r = (self.defaultRotation if v is None else v for v in (rotYaw, rotPitch, rotRoll))
        return MixtureProposal([(0.5, GaussianAxisRotationProposal(self.algorithm, y, YawAxis, self.rnd, f"RotationYaw-{y}")),
                                (0.5, GaussianAxisRotationProposal(self.algorithm, p, PitchAxis, self.rnd, f"RotationPitch-{p}")),
                                (0.5, GaussianAxisRotationProposal(self.algorithm, r, RollAxis, self.rnd, f"RotationRoll-{r}"))],
                               self.rnd)

    def RandomTranslation(self, transX=None, transY=None, transZ=None) -> MixtureProposal:
        x, y, z = (self.defaultTranslation if v is None else v for v in (transX, transY, transZ))
        return MixtureProposal([(0.5, GaussianAxisTranslationProposal(self.algorithm, x, 0, self.rnd, f"TranslationX-{x}")),
                                (0.5, GaussianAxisTranslationProposal(self.algorithm, y, 1, self.rnd, f"TranslationY-{y}")),
                                (0.5, GaussianAxisTranslationProposal(self.algorithm, z, 2, self.rnd, f"TranslationZ-{z}"))],
                               self.rnd)

    def RandomPose(self, **kw) -> MixtureProposal:
        rot = {k: v for k, v in kw.items() if k.startswith("rot")}
        tr = {k: v for k, v in kw.items() if k.startswith("trans")}
        return MixtureProposal([(0.5, self.RandomRotation(**rot)), (0.5, self.RandomTranslation(**tr))], self.rnd)

    def DefaultRandom(self) -> MixtureProposal:
        return MixtureProposal([(0.5, self.RandomPose()), (0.5, self.RandomShape())], self.rnd)


class GeneratorWrapperStochastic:
    """The informed proposal: update(current, probabilistic = true); transition density from the posterior of `from`."""

    def __init__(self, algorithm: GingrAlgorithm, rnd: Random, generatedBy: str = "InformedProposal"):
        self.algorithm, self.rnd, self.generatedBy = algorithm, rnd, generatedBy
        self._memo = _Memoize(lambda pair: self.algorithm.logTransitionProbability(pair[0], pair[1]), 1)

    def propose(self, current):
        new = self.algorithm.update(current, True, self.rnd.scalaRandom)
        if new.general.generatedBy == self.generatedBy:   # (update names its states after the algorithm: the stock set-up's label)
            return new
        out = new.updateGeneral(dataclasses.replace(new.general, generatedBy=self.generatedBy))
        self.algorithm._adopt_state(new, out)
        return out

    def logTransitionProbability(self, frm, to) -> float:
        return self.algorithm.logTransitionProbability(frm, to)


class GeneratorWrapperDeterministic:
    def __init__(self, algorithm: GingrAlgorithm, generatedBy: str = "Deterministic"):
        self.algorithm, self.generatedBy = algorithm, generatedBy

    def propose(self, current):
        new = self.algorithm.update(current, False)
        if new.general.generatedBy == self.generatedBy:
            return new
        out = new.updateGeneral(dataclasses.replace(new.general, generatedBy=self.generatedBy))
        self.algorithm._adopt_state(new, out)
        return out

    def logTransitionProbability(self, frm, to) -> float:
        return -math.inf


# ------------------------------------------------------------------------------------------------------------ the chain
class BestAndCurrentSampleLogger:
    def __init__(self, evaluator):
        self.evaluator, self._best, self._bestValue, self._current = evaluator, None, None, None

    def logState(self, sample):
        v = self.evaluator.logValue(sample)
        if self._best is None or v > self._bestValue:
            self._best, self._bestValue = sample, v
        self._current = sample

    def currentSample(self):
        return self._current

    def currentBestSample(self):
        return self._best

    def currentBestValue(self):
        return self._bestValue


class JSONStateLogger:
    """JSONStateLogger (G/api/sampling/loggers/JSONStateLogger.scala:52-201): accept / reject logger that records, per proposal, the
    generator's name, the value of every evaluator plus their product, and -- for accepted proposals only -- the parameters (a
    rejected entry means "the state of the last accepted entry", :128-130).  File layout: gingr_amd.io (write_log / read_log)."""

    def __init__(self, evaluators: AcceptAll, filePath: Optional[str] = None):
        import os
        from . import io as _io
        self._io = _io
        self.evaluators, self.filePath = evaluators, filePath
        self._product = evaluators.productEvaluator()
        self.numOfRejected = self.numOfAccepted = 0
        self.generatedBy = set()
        self.log = []
        if filePath is not None:
            parent = os.path.dirname(os.path.abspath(filePath))
            if not os.path.isdir(parent):
                raise IOError(f"JSON log path does not exist: {parent}!")
            if os.path.exists(filePath) and not os.access(filePath, os.W_OK):
                raise IOError(f"JSON file exist and cannot be overwritten: {filePath}!")

    @property
    def totalSamples(self) -> int:
        return self.numOfRejected + self.numOfAccepted

    def _values(self, sample) -> dict:
        vals = {e.name: float(e.evaluator.logValue(sample)) for e in self.evaluators.evaluator()}
        vals["product"] = float(self._product.logValue(sample))
        return vals

    def accept(self, current, sample, generator, evaluator):
        self.generatedBy.add(sample.general.generatedBy)
        self.log.append(self._io.log_entry(self.totalSamples, sample.general, self._values(sample), True))
        self.numOfAccepted += 1

    def reject(self, current, sample, generator, evaluator):
        self.generatedBy.add(sample.general.generatedBy)
        self.log.append(self._io.log_entry(self.totalSamples, sample.general, self._values(sample), False))
        self.numOfRejected += 1

    @property
    def percentRejected(self) -> float:
        return round(self.numOfRejected / self.totalSamples + 1e-12, 2)    # BigDecimal HALF_UP to two digits (:149-150)

    @property
    def percentAccepted(self) -> float:
        return 1.0 - self.percentRejected

    def percentAcceptedOfType(self, name: str, log=None) -> float:
        rows = [e for e in (self.log if log is None else log) if e.name == name]
        return sum(1 for e in rows if e.status) / len(rows)

    def writeLog(self):
        if self.filePath is None:
            print("JSON logFile NOT written - no filepath given")
            return
        self._io.write_log(self.log, self.filePath)
        print("Log written to: " + self.filePath)

    def printAcceptInfo(self, id: str = ""):
        lastX = 100
        print(f"{id} Total accepted ({self.totalSamples}): {self.percentAccepted}")
        names = sorted(n for n in self.generatedBy if n)
        for n in names:
            print(f"{id} {n}: {self.percentAcceptedOfType(n)}")
        if len(self.log) > lastX:
            tail = self.log[-lastX:]
            print(f"{id} Last {lastX} samples accepted ({lastX}): {sum(1.0 for e in tail if e.status) / lastX}")
            for n in names:
                if any(e.name == n for e in tail):
                    print(f"{id} {n}: {self.percentAcceptedOfType(n, tail)}")

    def __str__(self):
        return (f"# of Accepted: {self.numOfAccepted} = {self.percentAccepted}%\n"
                f"# of Rejected: {self.numOfRejected} = {self.percentRejected}%")


class MetropolisHastings:
    """scalismo.sampling.algorithms.MetropolisHastings [SCALISMO-RECALL]."""

    def __init__(self, generator, evaluator, rnd: Random):
        self.generator, self.evaluator, self.rnd = generator, evaluator, rnd

    def logTransitionRatio(self, start, end) -> float:
        fw = self.generator.logTransitionProbability(start, end)
        bw = self.generator.logTransitionProbability(end, start)
        if math.isnan(fw) or math.isnan(bw):
            raise ArithmeticError("NaN transition probability encountered!")
        if fw == -math.inf and bw == -math.inf:
            return 0.0
        return fw - bw

    def next(self, current, logger=None):
        proposal = self.generator.propose(current)
        currentP = self.evaluator.logValue(current)
        proposalP = self.evaluator.logValue(proposal)
        t = self.logTransitionRatio(current, proposal)
        a = proposalP - currentP - t
        if a > 0.0 or self.rnd.nextDouble() < math.exp(a):
            if logger is not None:
                logger.accept(current, proposal, self.generator, self.evaluator)
            return proposal
        if logger is not None:
            logger.reject(current, proposal, self.generator, self.evaluator)
        return current


def generatorCombined(algorithm: GingrAlgorithm, probabilisticSettings: Optional[ProbabilisticSettings], mixing, rnd: Random):
    """GingrAlgorithm.generatorCombined (GingrAlgorithm.scala:177-190)."""
    if probabilisticSettings is None:
        return GeneratorWrapperDeterministic(algorithm, algorithm.name)
    mix = mixing if mixing is not None else Generator(algorithm, rnd).DefaultRandom()
    informed = GeneratorWrapperStochastic(algorithm, rnd, algorithm.name)
    w = probabilisticSettings.randomMixture
    return MixtureProposal([(w, mix), (1.0 - w, informed)], rnd)


def run(algorithm: GingrAlgorithm, initialState, acceptRejectLogger=None, callBackLogger: Optional[Callable] = None,
        probabilisticSettings: Optional[ProbabilisticSettings] = None, generators=None, rnd: Optional[Random] = None):
    """GingrAlgorithm.run (GingrAlgorithm.scala:115-175).  The chain yields the initial state first, so take(maxIterations)
    makes maxIterations - 1 Metropolis-Hastings steps.  Deterministic (no settings): every proposal is accepted, the run stops
    on convergence or ModelFlexibilityError and returns the last state; probabilistic: stops on ModelFlexibilityError only and
    returns the best state under the evaluator."""
    rnd = rnd if rnd is not None else Random(0)
    probabilistic = probabilisticSettings is not None
    settings = probabilisticSettings if probabilistic else ProbabilisticSettings(AcceptAll(), 0.0)
    evaluator = EvaluatorWrapper(probabilistic, settings.evaluators)
    generator = generatorCombined(algorithm, probabilisticSettings, generators, rnd)
    best = BestAndCurrentSampleLogger(evaluator)
    chain = MetropolisHastings(generator, evaluator, rnd)
    # One native call per step (GingrAlgorithm.enableFusedSteps) when the likelihood is the model-to-target point distance of this
    # algorithm: the call measures it together with the proposal and both transition densities.  Same draws, same decisions.
    fused = False
    if probabilistic and settings.fusedSteps:
        dist = [e.evaluator for e in settings.evaluators.evaluator() if isinstance(e.evaluator, IndependentPointDistanceEvaluator)]
        if len(dist) == 1 and dist[0].algorithm is algorithm and dist[0].evaluationMode == ModelToTargetEvaluation:
            algorithm.enableFusedSteps(dist[0].uncertainty, dist[0].modelPointCount or 0)
            fused = True
    try:
        if acceptRejectLogger is not None:
            acceptRejectLogger.accept(initialState, initialState, generator, evaluator)
        state, last_general, converged, k = initialState, None, False, 0
        while True:
            if callBackLogger is not None:
                callBackLogger(state)
            best.logState(state)
            if not probabilistic and last_general is not None:
                converged = bool(state.config.converged(last_general, state.general, state.config.threshold))
            error = state.general.status == FittingStatuses.ModelFlexibilityError
            last_general = state.general
            k += 1
            if converged or error or k >= state.config.maxIterations:
                break
            state = chain.next(state, acceptRejectLogger)
    finally:
        if fused:
            algorithm.disableFusedSteps()
    fit = best.currentBestSample() if probabilistic else best.currentSample()
    if fit.general.status == FittingStatuses.None_:
        fit = fit.updateGeneral(fit.general.updateStatus(FittingStatuses.Converged if converged else FittingStatuses.MaxIteration))
    return fit


# ------------------------------------------------------------------------------------------------------------ metrics
@dataclasses.dataclass(frozen=True)
class TriangleMesh3D:
    points: np.ndarray   # (n, 3) float64
    cells: np.ndarray    # (T, 3) int


class RegistrationComparison:
    """Accuracy metrics of a registration (G/api/helper/RegistrationComparison.scala:22-99); every closest-point scan and
    reduction runs on the GPU (gingr_mesh_distance_stats)."""

    def __init__(self, ctx: Context, verbose: bool = True):
        self.ctx, self.verbose = ctx, verbose

    def _stats(self, m1: TriangleMesh3D, m2: TriangleMesh3D, boundary_aware: bool = False):
        return self.ctx.mesh_distance_stats(m1.points, m2.points, m2.cells, boundary_aware)

    def avgDistance(self, m1: TriangleMesh3D, m2: TriangleMesh3D) -> float:
        """scalismo MeshMetrics.avgDistance: mean distance of m1's vertices to the surface of m2."""
        s, _, n, _ = self._stats(m1, m2)
        return s / n

    def maxDistance(self, m1: TriangleMesh3D, m2: TriangleMesh3D) -> float:
        return self._stats(m1, m2)[1]

    def hausdorffDistance(self, m1: TriangleMesh3D, m2: TriangleMesh3D) -> float:
        return max(self.maxDistance(m1, m2), self.maxDistance(m2, m1))

    def evaluateReconstruction2GroundTruth(self, id: str, reconstruction: TriangleMesh3D, groundTruth: TriangleMesh3D):
        avg = self.avgDistance(reconstruction, groundTruth)
        hd = self.hausdorffDistance(reconstruction, groundTruth)
        md = self.maxDistance(reconstruction, groundTruth)
        if self.verbose:
            print(f"ID: {id} average2surface: {avg} max: {md}, hausdorff: {hd}")
        return avg, md, hd

    def evaluateReconstruction2GroundTruthDouble(self, id: str, reconstruction: TriangleMesh3D, groundTruth: TriangleMesh3D):
        avg = (self.avgDistance(reconstruction, groundTruth) + self.avgDistance(groundTruth, reconstruction)) / 2.0
        hd = self.hausdorffDistance(reconstruction, groundTruth)
        if self.verbose:
            print(f"ID: {id} average2surface: {avg} hausdorff: {hd}")
        return avg, hd

    def avgDistanceBoundaryAware(self, m1: TriangleMesh3D, m2: TriangleMesh3D) -> Tuple[float, float]:
        s, mx, n, _ = self._stats(m1, m2, True)
        return s / n, mx

    def evaluateReconstruction2GroundTruthBoundaryAware(self, id: str, reconstruction: TriangleMesh3D, groundTruth: TriangleMesh3D):
        a1, m1 = self.avgDistanceBoundaryAware(reconstruction, groundTruth)
        a2, m2 = self.avgDistanceBoundaryAware(groundTruth, reconstruction)
        avg, mx = (a1 + a2) / 2.0, max(m1, m2)
        if self.verbose:
            print(f"ID: {id} average2surface: {avg} max: {mx}")
        return avg, mx
