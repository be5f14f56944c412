"""The algorithms: `GingrAlgorithm` (one native call sequence per iteration, the fused Metropolis-Hastings step, the queries about a
state) and its correspondence flavours `CpdRegistration`, `IcpRegistration`, `TemplateRegistration` and `PointToPlaneIcpRegistration`.

  GingrAlgorithm                                                G/api/GingrAlgorithm.scala:52-75,192-258
  CpdRegistration                                               G/api/registration/config/CPD.scala:52-155
  IcpRegistration                                               G/api/registration/config/ICP.scala:54-107
  TemplateRegistration                                          G/api/registration/config/Template.scala:46-60
"""
from __future__ import annotations

import ctypes
import dataclasses
from ctypes import c_void_p
from typing import Callable, Optional, Sequence, Tuple

import numpy as np

from . import _native as nat
from ._native import GingrNativeError, f64, dptr, iptr
from .context import Context, _check
from .models import DeviceModel, PointDistributionModel, PosteriorDevicePointDistributionModel, _landmarks_native
from .states import (CorrespondencePairs, CpdConfiguration, CpdRegistrationState, EulerAngles, FittingStatuses, GeneralRegistrationState,
                     GlobalTranformationType, IcpConfiguration, IcpRegistrationState, LandmarkCorrespondences, ModelFittingParameters,
                     PointToPlaneConfiguration, PointToPlaneRegistrationState, RobustLoss, TemplateConfiguration, TemplateRegistrationState,
                     _cpd_converged, _empty_pairs, _never_converged, _with_fields)


# ----------------------------------------------------------------------------- the algorithm
class GingrAlgorithm:
    """HIP-backed GingrAlgorithm: `update` is ONE native call sequence per iteration
    (GingrAlgorithm.scala:192-254 + GingrGeneratorWrapper.propose).  Sub-classes supply the correspondence flavour."""

    name = "GiNGR"

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._lib = ctx._lib
        self._dev_model: Optional[DeviceModel] = None
        self._fitter = None
        # The objects currently bound on the device.  Strong references compared with `is` (an id() of a collected object can be
        # reused by a new one of the same shape); arrays are treated as immutable, like the reference's case-class fields.
        self._bound_model = None
        self._bound_target = None
        self._bound_lm = None
        self._bound_mesh = None
        self._device_state = None         # the python state currently mirrored on the device (strong reference, compared with `is`)
        self._mh = None                   # fused Metropolis-Hastings steps: {"sdev", "points"} of the likelihood evaluated with them
        self._mh_last = None              # what the last fused step measured: {"from", "to", "stats", "fw", "bw"}
        self._plan_memo = None            # (config object, what _correspondence said about it + the argument its entry points take)
        self._mh_plan_memo = None         # (config object, what _mh_flavour said about it + ctypes pointers)
        self._mh_req = None               # the request / result structs of the fused step, reused (the call is synchronous)
        self._warp_model = None           # (model, its DeviceModel) of transformPoints for a model that is not the bound one
        self._sel = {}                    # selections already made on the current fitter (options, direction, surface method): set again only when they change

    # -- native plumbing ------------------------------------------------------------------
    def _bind(self, general: GeneralRegistrationState, use_landmarks: bool):
        if self._bound_model is not general.model:
            self._release()
            self._dev_model = DeviceModel(self.ctx, general.model)
            h = c_void_p()
            _check(self.ctx.handle, self._lib.gingr_fitter_create(self.ctx.handle, self._dev_model.handle, ctypes.byref(h)),
                   "gingr_fitter_create")
            self._fitter = h
            self._sel = {}
            self._bound_model = general.model
            self._bound_target = None
            self._bound_lm = None
            self._bound_mesh = None
        if self._bound_target is not general.target:
            x = f64(general.target)
            _check(self.ctx.handle, self._lib.gingr_fitter_set_target(self._fitter, x.shape[0], dptr(x)), "gingr_fitter_set_target")
            self._bound_target = general.target
            self._device_state = None
            self._bound_mesh = None
            self._sel = {}
        mcells = getattr(general.model, "cells", None)
        if mcells is not None and general.targetCells is not None and not (
                self._bound_mesh is not None and self._bound_mesh[0] is mcells and self._bound_mesh[1] is general.targetCells):
            mt = np.ascontiguousarray(mcells, dtype=np.int32).reshape(-1, 3)
            tt = np.ascontiguousarray(general.targetCells, dtype=np.int32).reshape(-1, 3)
            _check(self.ctx.handle, self._lib.gingr_fitter_set_meshes(self._fitter, mt.shape[0], iptr(mt), tt.shape[0], iptr(tt)),
                   "gingr_fitter_set_meshes")
            self._bound_mesh = (mcells, general.targetCells)
            self._sel = {}                # (new meshes: the library starts from the forward direction again)
        lm = general.landmarkCorrespondences if use_landmarks else None
        if not (self._bound_lm is not None and self._bound_lm[0] is lm and self._bound_lm[1] == use_landmarks):
            n, lp, lx, lc = _landmarks_native(lm)
            _check(self.ctx.handle, self._lib.gingr_fitter_set_landmarks(self._fitter, n, iptr(lp), dptr(lx), dptr(lc)),
                   "gingr_fitter_set_landmarks")
            self._bound_lm = (lm, use_landmarks)
        opts = (int(general.globalTransformation), float(general.stepLength))
        if self._sel.get("options") != opts:        # (one native call less per Metropolis-Hastings step)
            _check(self.ctx.handle, self._lib.gingr_fitter_set_options(self._fitter, opts[0], opts[1]), "gingr_fitter_set_options")
            self._sel["options"] = opts

    def _drop_warp_model(self):
        if self._warp_model is not None:
            self._warp_model[1].close()
            self._warp_model = None

    def _release(self):
        self._drop_warp_model()
        if self._fitter:
            if getattr(self.ctx, "handle", None):   # (never into a context that has been closed)
                self._lib.gingr_fitter_destroy(self._fitter)
            self._fitter = None
        if self._dev_model is not None:
            self._dev_model.close()
            self._dev_model = None
        self._bound_model = self._bound_target = self._bound_lm = self._bound_mesh = None
        self._device_state = None
        self._sel = {}

    def close(self):
        self._release()

    def transformPoints(self, state, points) -> np.ndarray:
        """The state's fit carried to arbitrary points (n x 3): s (R (x + u(x) - c) + c + t) with u the deformation field of the
        state's shape coefficients, evaluated by the model's kernel extension (DeviceModel.warpPoints) -- landmarks that are no
        vertices, an inner structure, a finer mesh.  At the model's own points this is the state's fit.  The model must carry the
        extension (a device-built kernel model, truncated or extended); others raise GingrNativeError (GINGR_ERR_STATE)."""
        general = getattr(state, "general", state)
        mp = general.modelParameters
        if self._bound_model is general.model and self._dev_model is not None:
            dm = self._dev_model
        else:                                       # not the bound model: made resident once and kept until another one is asked for
            if self._warp_model is None or self._warp_model[0] is not general.model:
                self._drop_warp_model()
                self._warp_model = (general.model, DeviceModel(self.ctx, general.model))
            dm = self._warp_model[1]
        return dm.warpPoints(points, mp.shape, (mp.rotation.phi, mp.rotation.theta, mp.rotation.psi), mp.center, mp.translation, mp.scale)

    @property
    def retryCounter(self) -> int:
        """`retryCounter` of this algorithm instance (GingrAlgorithm.scala:69-70); it lives on the device next to the state."""
        if not self._fitter:
            return 10
        v = ctypes.c_int32()
        _check(self.ctx.handle, self._lib.gingr_fitter_retry_counter(self._fitter, -1, ctypes.byref(v)), "gingr_fitter_retry_counter")
        return int(v.value)

    def _push_state(self, general: GeneralRegistrationState):
        mp = general.modelParameters
        s = nat.StateScalars()
        s.euler[:] = [mp.rotation.phi, mp.rotation.theta, mp.rotation.psi]
        s.center[:] = list(mp.center)
        s.translation[:] = list(mp.translation)
        s.scale = mp.scale
        s.sigma2 = general.sigma2
        s.iteration = general.iteration
        s.status = general.status
        a = f64(mp.shape)
        _check(self.ctx.handle, self._lib.gingr_fitter_set_state(self._fitter, dptr(a), ctypes.byref(s)), "gingr_fitter_set_state")

    def _pull_state(self, general: GeneralRegistrationState) -> GeneralRegistrationState:
        r = general.model.rank
        M = general.model.numberOfPoints
        alpha = np.empty(r)
        fit = np.empty((M, 3))
        s = nat.StateScalars()
        _check(self.ctx.handle, self._lib.gingr_fitter_get_state(self._fitter, dptr(alpha), ctypes.byref(s), dptr(fit)),
               "gingr_fitter_get_state")
        mp = ModelFittingParameters(scale=s.scale, translation=tuple(s.translation),
                                    rotation=EulerAngles(*list(s.euler)), center=tuple(s.center), shape=alpha)
        return dataclasses.replace(general, modelParameters=mp, fit=fit, sigma2=s.sigma2, iteration=s.iteration,
                                   status=s.status, generatedBy=self.name)

    # -- the correspondence flavour: what a sub-class says once, and the five operations named after it ------------------------------
    def _correspondence(self, state):
        """(flavour, its parameter struct or None): enum Flavour of gingr_amd/csrc/correspondence.h"""
        raise NotImplementedError

    def _prepare_native(self, state):
        """selections on the fitter that the flavour's entry points read (direction, surface method, the caller's pairs)"""

    def _plan(self, state):
        """_correspondence(state) and the parameter argument of its entry points, remembered for the configuration OBJECT (frozen
        dataclasses shared by all the states of a run)"""
        c = state.config
        memo = self._plan_memo
        if memo is not None and memo[0] is c:
            return memo[1]
        flavour, p = self._correspondence(state)
        plan = (flavour, p, () if p is None else (ctypes.byref(p),))
        self._plan_memo = (c, plan)
        return plan

    def _native(self, state, op: int, *args):
        self._prepare_native(state)
        flavour, _, p = self._plan(state)
        name = nat.FITTER_OPS[flavour][op]
        _check(self.ctx.handle, getattr(self._lib, name)(self._fitter, *p, *args), name)

    def _native_update(self, current, n: int):
        self._native(current, nat.OP_UPDATE, n)

    def _native_update_sample(self, current, z: np.ndarray):
        self._native(current, nat.OP_UPDATE_SAMPLE, dptr(z))

    def _native_logpdf(self, state, mesh: np.ndarray) -> float:
        out = ctypes.c_double()
        self._native(state, nat.OP_LOGPDF, dptr(mesh), ctypes.byref(out))
        return out.value

    def _native_posterior_covariance(self, state, out: np.ndarray):
        self._native(state, nat.OP_POSTERIOR_COVARIANCE, dptr(out))

    def _native_posterior_model(self, state, out):
        self._native(state, nat.OP_POSTERIOR_MODEL, ctypes.byref(out))

    # -- the reference surface ----------------------------------------------------------------
    def initializeState(self, general: GeneralRegistrationState, config):
        raise NotImplementedError

    def update(self, current, probabilistic: bool = False, rnd: Optional[np.random.Generator] = None):
        """One GiNGR iteration.  Failure handling as in the reference's Try(...) logic, decided on the device (post_solve_kernel):
        a failed posterior leaves the state unchanged at iteration 0, gives ModelFlexibilityError in a deterministic update,
        and in a probabilistic one uses up one of the instance's 10 retries (state unchanged) before it gives
        ModelFlexibilityError (:194-208; successes give retries back, :210); a failed coefficient projection is a
        ModelFlexibilityError at any iteration (:248-251).
        probabilistic=True proposes posterior.sample() instead of posterior.mean (:211); the standard-normal draws come from
        `rnd` (the reference's `implicit rnd: Random`)."""
        g = current.general
        if probabilistic and rnd is not None and self._mh_usable(current):
            return self._mh_step(current, 0, f64(rnd.standard_normal(g.model.rank)), None, self.name)
        self._bind(g, current.config.useLandmarkCorrespondence)
        if self._device_state is not current:
            self._push_state(g)
        if probabilistic:
            if rnd is None:
                raise ValueError("probabilistic update needs a random generator (rnd)")
            self._native_update_sample(current, f64(rnd.standard_normal(g.model.rank)))
        else:
            self._native_update(current, 1)
        new_general = self._pull_state(g)
        out = current.updateGeneral(new_general)
        self._device_state = out
        return out

    # -- one Metropolis-Hastings step per native call (gingr_fitter_mh_step) ---------------------------------------------------
    def enableFusedSteps(self, uncertainty: float, modelPointCount: int = 0):
        """From now on a probabilistic `update` / `proposeParameters` runs the WHOLE device side of a Metropolis-Hastings step in one
        native call -- proposal, model-to-target likelihood N(0, uncertainty) over the first modelPointCount vertices (0 = all), both
        transition densities of the informed proposal -- and the queries MetropolisHastings.next makes afterwards
        (`surfaceDistanceStats`, `logTransitionProbability`) are answered from what that call measured.  Same numbers, same order
        of random draws as the call-by-call path; states with stepLength != 1 or without meshes keep using that path."""
        self._mh = {"sdev": float(uncertainty), "points": int(modelPointCount or 0)}
        self._mh_last = None

    def disableFusedSteps(self):
        self._mh = self._mh_last = None

    def _mh_flavour(self, state):
        """(flavour, CpdParams | None, IcpParams | None) of gingr_mh_request, a view of _correspondence; None when this configuration has
        no fused step: the pairs come from the host, and the reversed direction keeps the call-by-call path"""
        flavour, p, _ = self._plan(state)
        if flavour == nat.FLAVOUR_PAIRS or getattr(state.config, "reverseCorrespondenceDirection", False):
            return None
        return (flavour, p, None) if flavour == nat.FLAVOUR_CPD else (flavour, None, p)

    def _mh_plan(self, state):
        """_mh_flavour(state) with its ctypes pointers, remembered for the configuration OBJECT (frozen dataclasses shared by all the
        states of a chain): one Metropolis-Hastings step asks twice."""
        c = state.config
        memo = self._mh_plan_memo
        if memo is not None and memo[0] is c:
            return memo[1]
        fl = self._mh_flavour(state)
        plan = None
        if fl is not None:
            flavour, cp, ip = fl
            plan = (flavour, cp, ip, ctypes.pointer(cp) if cp is not None else None, ctypes.pointer(ip) if ip is not None else None)
        self._mh_plan_memo = (c, plan)
        return plan

    def _mh_usable(self, state) -> bool:
        g = state.general
        return (self._mh is not None and g.stepLength == 1.0 and getattr(g.model, "cells", None) is not None
                and g.targetCells is not None and self._mh_plan(state) is not None)

    def _adopt_state(self, old, new):
        """`new` is `old` with host-side fields rewritten (generatedBy): it stands for the same device state and measurements"""
        if self._device_state is old:
            self._device_state = new
        if self._mh_last is not None and self._mh_last["to"] is old:
            self._mh_last["to"] = new

    def _mh_step(self, current, kind: int, z, modelParameters, generatedBy: str):
        g = current.general
        self._bind(g, current.config.useLandmarkCorrespondence)
        last = self._mh_last
        if self._device_state is not current:
            if last is not None and last["from"] is current and self._device_state is last["to"]:
                _check(self.ctx.handle, self._lib.gingr_fitter_mh_restore(self._fitter), "gingr_fitter_mh_restore")   # rejected
            else:
                self._push_state(g)
            self._device_state = current
        self._prepare_native(current)
        flavour, _, _, cpp, ipp = self._mh_plan(current)
        if self._mh_req is None:
            self._mh_req = (nat.MhRequest(), nat.MhResult())
        req, res = self._mh_req
        req.flavour, req.kind = flavour, kind
        req.cpd, req.icp = cpp, ipp
        req.z = req.alpha = None
        req.scalars = None
        req.eval_sdev, req.eval_points = self._mh["sdev"], self._mh["points"]
        # q(.|current) projects current.fit (step length 1): a number of `current` alone, known when a fused step produced or started
        # from this very state
        fw = last["bw"] if last is not None and last["to"] is current else (last["fw"] if last is not None and last["from"] is current else None)
        req.need_forward = 1 if fw is None else 0
        keep = None
        if kind == 0:
            req.z = dptr(z)
        else:
            mp = modelParameters
            keep = (f64(mp.shape), nat.StateScalars())
            sc = keep[1]
            sc.euler[:] = [mp.rotation.phi, mp.rotation.theta, mp.rotation.psi]
            sc.center[:] = list(mp.center)
            sc.translation[:] = list(mp.translation)
            sc.scale, sc.sigma2, sc.iteration, sc.status = mp.scale, g.sigma2, g.iteration + 1, g.status
            req.alpha, req.scalars = dptr(keep[0]), ctypes.pointer(sc)
        r, M = g.model.rank, g.model.numberOfPoints
        alpha, fit = np.empty(r), np.empty((M, 3))
        try:
            _check(self.ctx.handle, self._lib.gingr_fitter_mh_step(self._fitter, ctypes.byref(req), dptr(alpha), dptr(fit), ctypes.byref(res)),
                   "gingr_fitter_mh_step")
        except BaseException:
            # a step that failed half way leaves the device state undefined (the library refuses to continue from it): forget what
            # this object believes to be mirrored there, so that the next call pushes a state again
            self._device_state = None
            self._mh_last = None
            raise
        s = res.scalars
        e, t, c0 = s.euler, s.translation, s.center
        mp = ModelFittingParameters(scale=s.scale, translation=(t[0], t[1], t[2]), rotation=EulerAngles(e[0], e[1], e[2]),
                                    center=(c0[0], c0[1], c0[2]), shape=alpha)
        new_general = _with_fields(g, modelParameters=mp, fit=fit, sigma2=s.sigma2, iteration=s.iteration, status=s.status,
                                   generatedBy=generatedBy)
        out = _with_fields(current, general=new_general)
        self._device_state = out
        self._mh_last = {"from": current, "to": out, "sdev": self._mh["sdev"], "points": self._mh["points"],
                         "stats": (float(res.dist_sum), float(res.dist_max), int(res.count), float(res.log_value)),
                         "fw": float(res.log_q_forward) if fw is None else fw, "bw": float(res.log_q_backward)}
        return out

    def _ensure_device_state(self, state):
        """Make the fitter hold `state` (model, target, meshes, parameters; the fit is re-instantiated on the device)."""
        g = state.general
        self._bind(g, state.config.useLandmarkCorrespondence)
        if self._device_state is not state:
            self._push_state(g)
            self._device_state = state

    def proposeParameters(self, current, modelParameters: ModelFittingParameters, generatedBy: str):
        """GingrGeneratorWrapper.propose for a proposal that only rewrites the parameters (GingrGeneratorWrapper.scala:28-39):
        fit = modelInstanceShapePoseScale(model, parameters) -- instantiated on the device -- and iteration + 1."""
        if self._mh_usable(current):
            return self._mh_step(current, 1, None, modelParameters, generatedBy)
        g = dataclasses.replace(current.general, modelParameters=modelParameters, iteration=current.general.iteration + 1)
        self._bind(g, current.config.useLandmarkCorrespondence)
        self._push_state(g)
        new_general = dataclasses.replace(self._pull_state(g), generatedBy=generatedBy)
        out = current.updateGeneral(new_general)
        self._device_state = out
        return out

    def surfaceDistanceStats(self, state, direction: int, n_points: int = 0, points=None, boundary_aware: bool = False,
                             sdev: float = 0.0) -> Tuple[float, float, int, float]:
        """(sum, max, count, sum of log N(d; 0, sdev)) of the closest-point distances between the fit of `state` and the target
        surface: direction 0 = fit vertices -> target surface, 1 = target vertices (or `points`) -> fit surface."""
        g = state.general
        if getattr(g.model, "cells", None) is None or g.targetCells is None:
            raise ValueError("surface distances need model.cells and targetCells")
        last = self._mh_last
        if (last is not None and last["to"] is state and direction == 0 and points is None and not boundary_aware
                and float(sdev) == last["sdev"] and int(n_points or 0) == last["points"]):
            return last["stats"]          # measured by the fused step that produced this state
        self._ensure_device_state(state)
        out = np.zeros(4)
        pts = None if points is None else f64(points)
        n = int(n_points) if pts is None else pts.shape[0]
        _check(self.ctx.handle, self._lib.gingr_fitter_surface_distance_stats(
            self._fitter, int(direction), n, None if pts is None else dptr(pts), int(bool(boundary_aware)), float(sdev), dptr(out)),
            "gingr_fitter_surface_distance_stats")
        return float(out[0]), float(out[1]), int(out[2]), float(out[3])

    def logTransitionProbability(self, from_state, to_state) -> float:
        """GeneratorWrapperStochastic.logTransitionProbability (GeneratorWrapperStochastic.scala:42-63): log-density, under
        the posterior model of `from_state`, of the mesh the reference projects -- from.fit when stepLength == 1, otherwise
        the unposed instance of the step-compensated coefficients.  -inf when the posterior cannot be computed."""
        g = from_state.general
        last = self._mh_last
        if last is not None and g.stepLength == 1.0:   # both densities of the step that made `to` from `from` came with it
            if last["from"] is from_state and last["to"] is to_state:
                return last["fw"]
            if last["from"] is to_state and last["to"] is from_state:
                return last["bw"]
        if g.stepLength != 1.0:
            a0, a1 = f64(g.modelParameters.shape), f64(to_state.general.modelParameters.shape)
            comp = a0 + (a1 - a0) / g.stepLength
            dm = DeviceModel(self.ctx, g.model)
            try:
                mesh = dm.instance(comp)
            finally:
                dm.close()
        else:
            mesh = f64(g.fit)
        self._ensure_device_state(from_state)     # the query leaves the device state as it is: no push when it already holds `from`
        try:
            return self._native_logpdf(from_state, mesh)
        except GingrNativeError as e:
            if e.code in (nat.ERR_NOT_SPD, nat.ERR_NONFINITE):
                return float("-inf")
            raise

    def posteriorCovariance(self, state) -> np.ndarray:
        """(M, 6): the 3 x 3 posterior covariance block {xx, xy, xz, yy, yz, zz} of every vertex under the posterior model of
        `state` -- posterior.gp.cov(pid, pid) of model.transform(rigid).posterior(observations) (GingrAlgorithm.scala:297-301; no
        scale) -- computed exactly on the device: the quantity DemoPosteriorVisualizationFemur estimates from a chain of samples.
        The state is left as it is.  A posterior that cannot be computed raises GingrNativeError."""
        self._ensure_device_state(state)
        out = np.empty((state.general.model.numberOfPoints, 6))
        self._native_posterior_covariance(state, out)
        return out

    def posteriorModel(self, state) -> DeviceModel:
        """The posterior model of `state` -- computePosterior (GingrAlgorithm.scala:281-302): model.transform(rigid).posterior(
        observations), no scale -- as a new model resident in HBM (gingr_fitter_posterior_model_*): sample from it, save it,
        truncate it, condition it again, or register with it as the prior.  The state is left as it is.  A posterior that cannot be
        computed raises GingrNativeError."""
        self._ensure_device_state(state)
        h = c_void_p()
        self._native_posterior_model(state, h)
        return PosteriorDevicePointDistributionModel(self.ctx, h, cells=getattr(state.general.model, "cells", None)).device()

    def run(self, initialState, callBackLogger: Optional[Callable] = None, acceptRejectLogger=None, probabilisticSettings=None,
            generators=None, rnd=None):
        """GingrAlgorithm.run (:115-175).  Without probabilisticSettings: the deterministic registration loop -- the chain
        yields the initial state first, so take(maxIterations) performs maxIterations-1 updates; stops on convergence or
        ModelFlexibilityError.  With them: the Metropolis-Hastings chain of gingr_amd.sampling (informed + random-walk
        proposals, evaluator, best sample)."""
        if probabilisticSettings is not None or acceptRejectLogger is not None or generators is not None:
            from . import sampling
            return sampling.run(self, initialState, acceptRejectLogger, callBackLogger, probabilisticSettings, generators, rnd)
        state = initialState
        last_general = None
        converged = False
        k = 0
        if callBackLogger is None and state.config.converged in (_cpd_converged, _never_converged) \
                and state.general.status != FittingStatuses.ModelFlexibilityError and state.config.maxIterations > 1:
            return self._run_resident(state)
        while True:
            # dropWhile body (:142-153)
            if last_general is not None:
                converged = bool(state.config.converged(last_general, state.general, state.config.threshold))
            error = state.general.status == FittingStatuses.ModelFlexibilityError
            last_general = state.general
            if callBackLogger is not None:
                callBackLogger(state)
            k += 1
            if converged or error or k >= state.config.maxIterations:
                break
            state = self.update(state, False)
        if state.general.status == FittingStatuses.None_:
            state = state.updateGeneral(state.general.updateStatus(
                FittingStatuses.Converged if converged else FittingStatuses.MaxIteration))
        return state

    def _run_resident(self, state):
        """The deterministic loop of `run` with the state resident on the device: nobody watches the intermediate states (no
        call-back) and the convergence rule is one of the reference's own (|sigma2 - last sigma2| < threshold for CPD, never for ICP).
        Updates are enqueued in blocks and only the state a block ends in is looked at; coefficients and fit come back once, at the end.
        That is sound because the chain cannot run past its last state on the device: a failed fit stays as it is (post_solve_kernel commits
        nothing once the status is ModelFlexibilityError; GingrAlgorithm.scala:149-157 stops at that very state), and so does a state the
        CPD rule stopped at (gingr_fitter_set_stop_threshold: the comparison the dropWhile makes, made by the kernel that commits sigma2).
        ICP has no rule: the whole run is one block.  CPD: updates enqueued behind the stopping state are wasted work, so the block is
        one update where an update is long and a few where the synchronisation would be a fifth of it.
        Same states, same stopping iteration, same status as the generic loop."""
        g = state.general
        self._bind(g, state.config.useLandmarkCorrespondence)
        if self._device_state is not state:
            self._push_state(g)
        cpd_rule = state.config.converged is _cpd_converged
        left = state.config.maxIterations - 1
        if cpd_rule:
            pairs = float(g.model.numberOfPoints) * float(np.asarray(g.target).shape[0])
            block = 4 if pairs <= 4e6 else (2 if pairs <= 3e7 else 1)
        else:
            block = left
        hit, sc = ctypes.c_int32(0), nat.StateScalars()
        _check(self.ctx.handle, self._lib.gingr_fitter_set_stop_threshold(self._fitter, float(state.config.threshold) if cpd_rule else -1.0),
               "gingr_fitter_set_stop_threshold")
        try:
            while left > 0:
                n = min(block, left)
                self._native_update(state, n)
                left -= n
                _check(self.ctx.handle, self._lib.gingr_fitter_get_state(self._fitter, None, ctypes.byref(sc), None), "gingr_fitter_get_state")
                _check(self.ctx.handle, self._lib.gingr_fitter_stop_rule_hit(self._fitter, ctypes.byref(hit)), "gingr_fitter_stop_rule_hit")
                if hit.value or sc.status == FittingStatuses.ModelFlexibilityError:
                    break
        finally:
            # (also clears the mark: the state on the device takes updates again)
            self._lib.gingr_fitter_set_stop_threshold(self._fitter, -1.0)
        out = state.updateGeneral(self._pull_state(g))
        self._device_state = out
        converged = bool(hit.value)
        if out.general.status == FittingStatuses.None_:
            out = out.updateGeneral(out.general.updateStatus(FittingStatuses.Converged if converged else FittingStatuses.MaxIteration))
        return out


def _initial_general(ctx: Context, model: PointDistributionModel, target: np.ndarray, sigma2: float,
                     transform: int, stepLength: float, landmarks: Optional[LandmarkCorrespondences],
                     initial_pose: Optional[Tuple[Sequence[float], Sequence[float]]] = None,
                     targetCells: Optional[np.ndarray] = None) -> GeneralRegistrationState:
    """GeneralRegistrationState.apply (:135-179): alpha = 0, optional initial pose, fit = instance."""
    mp = ModelFittingParameters.zero(model.rank)
    if initial_pose is not None:
        euler, t = initial_pose
        mp = dataclasses.replace(mp, rotation=EulerAngles(*euler), translation=tuple(t))
    dm = DeviceModel(ctx, model)
    try:
        fit = dm.instance(mp.shape, [mp.rotation.phi, mp.rotation.theta, mp.rotation.psi], mp.center, mp.translation, mp.scale)
    finally:
        dm.close()
    return GeneralRegistrationState(model=model, modelParameters=mp, target=f64(target), fit=fit, sigma2=sigma2,
                                    globalTransformation=transform, stepLength=stepLength,
                                    landmarkCorrespondences=landmarks, targetCells=targetCells)


class CpdRegistration(GingrAlgorithm):
    name = "CPD"

    def createInitialState(self, model: PointDistributionModel, target, config: CpdConfiguration,
                           transform: int = GlobalTranformationType.RigidTransforms, stepLength: float = 1.0,
                           landmarks: Optional[LandmarkCorrespondences] = None, initial_pose=None,
                           targetCells: Optional[np.ndarray] = None) -> CpdRegistrationState:
        """targetCells (with model.cells): the target's triangulation -- CPD itself works on the vertices; the surface
        likelihood of a probabilistic run (sampling.IndependentPointDistanceEvaluator) needs both meshes."""
        g = _initial_general(self.ctx, model, target, 1.0, transform, stepLength, landmarks, initial_pose, targetCells)
        return self.initializeState(g, config)

    def initializeState(self, general: GeneralRegistrationState, config: CpdConfiguration) -> CpdRegistrationState:
        # CpdRegistrationState.apply (CPD.scala:92-102): sigma2 = initialSigma or sum|x - y|^2/(3MN) over model MEAN vs target
        if config.initialSigma is not None:
            s2 = float(config.initialSigma)
        else:
            mean_pts = f64(general.model.reference) + f64(general.model.mean)
            s2 = self.ctx.cpd_initial_sigma2(mean_pts, general.target)
        return CpdRegistrationState(general.updateSigma2(s2), config)

    def _correspondence(self, state: CpdRegistrationState):
        return nat.FLAVOUR_CPD, nat.CpdParams(state.config.w, state.config.lambda_)

    # plugin accessors served from one streaming evaluation (the reference recomputes P for each of them)
    def _stats(self, state: CpdRegistrationState) -> dict:
        if getattr(self, "_stats_state", None) is not state:
            self._stats_cache = self.ctx.cpd_stats(state.general.fit, state.general.target, state.general.sigma2, state.config.w)
            self._stats_state = state
            self._stats_keep = state
        return self._stats_cache

    def getCorrespondence(self, state: CpdRegistrationState) -> CorrespondencePairs:
        st = self._stats(state)                                                       # CPD.scala:32-49
        y = f64(state.general.fit)
        with np.errstate(invalid="ignore", divide="ignore"):
            td = y + (st["PX"] * (1.0 / st["P1"])[:, None] - y)
        return CorrespondencePairs(np.arange(y.shape[0]), td)

    def getUncertainty(self, pid: int, state: CpdRegistrationState) -> np.ndarray:
        st = self._stats(state)                                                       # CPD.scala:120-128
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.eye(3) * state.general.sigma2 * state.config.lambda_ * (1.0 / st["P1"][int(pid)])

    def updateSigma2(self, state: CpdRegistrationState) -> float:
        return self._stats(state)["sigma2_next"]                                      # CPD.scala:133-147


class IcpRegistration(GingrAlgorithm):
    name = "ICP"
    _METHODS = ("PointcloudClosestPoint", "TriangularClosestPoint", "AlongNormalClosestPoint")

    @staticmethod
    def _surface(config: IcpConfiguration) -> bool:
        return config.correspondenceMethod in ("TriangularClosestPoint", "AlongNormalClosestPoint")

    def _select_surface_method(self, config: IcpConfiguration):
        method = 1 if config.correspondenceMethod == "AlongNormalClosestPoint" else 0
        if self._sel.get("method") != method:
            _check(self.ctx.handle, self._lib.gingr_fitter_set_surface_method(self._fitter, method), "gingr_fitter_set_surface_method")
            self._sel["method"] = method

    def _select_direction(self, config: IcpConfiguration):
        rev = 1 if config.reverseCorrespondenceDirection else 0
        if self._sel.get("direction") != rev:
            _check(self.ctx.handle, self._lib.gingr_fitter_set_correspondence_direction(self._fitter, rev),
                   "gingr_fitter_set_correspondence_direction")
            self._sel["direction"] = rev

    def _phase0(self, state: "IcpRegistrationState"):
        g, c = state.general, state.config
        self._bind(g, c.useLandmarkCorrespondence)
        self._push_state(g)
        self._device_state = None
        self._prepare_native(state)
        flavour, _, p = self._plan(state)
        name = "gingr_fitter_icp_surface_phase_async" if flavour == nat.FLAVOUR_ICP_SURFACE else "gingr_fitter_icp_phase_async"
        _check(self.ctx.handle, getattr(self._lib, name)(self._fitter, *p, 0), name)

    def reversedCorrespondence(self, state: "IcpRegistrationState") -> Tuple[np.ndarray, np.ndarray]:
        """closestPointCorrespondenceReversal (ClosestPointRegistrator.scala:34-49) for the state's fit: per TARGET vertex the
        template vertex it is assigned to and its weight in {0, 1}."""
        if not state.config.reverseCorrespondenceDirection:
            raise ValueError("the configuration does not reverse the correspondence direction")
        self._phase0(state)
        N = np.asarray(state.general.target).shape[0]
        tid, w = np.empty(N, dtype=np.int32), np.empty(N)
        _check(self.ctx.handle, self._lib.gingr_fitter_get_reversed_correspondence(self._fitter, iptr(tid), dptr(w)),
               "gingr_fitter_get_reversed_correspondence")
        return tid, w

    def createInitialState(self, model: PointDistributionModel, target, config: IcpConfiguration,
                           transform: int = GlobalTranformationType.RigidTransforms, stepLength: float = 1.0,
                           landmarks: Optional[LandmarkCorrespondences] = None, initial_pose=None,
                           targetCells: Optional[np.ndarray] = None) -> IcpRegistrationState:
        g = _initial_general(self.ctx, model, target, 1.0, transform, stepLength, landmarks, initial_pose, targetCells)
        return self.initializeState(g, config)

    def initializeState(self, general: GeneralRegistrationState, config: IcpConfiguration) -> IcpRegistrationState:
        if config.correspondenceMethod not in self._METHODS:
            raise NotImplementedError("ICP flavours: PointcloudClosestPoint, TriangularClosestPoint, AlongNormalClosestPoint (ICP.scala:32-44)")
        if self._surface(config) and (getattr(general.model, "cells", None) is None or general.targetCells is None):
            raise ValueError(config.correspondenceMethod + " needs the triangulations (model.cells and targetCells); for point "
                             "clouds choose correspondenceMethod=\"PointcloudClosestPoint\"")
        return IcpRegistrationState(general.updateSigma2(float(config.initialSigma)), config)   # ICP.scala:73-85

    def _correspondence(self, state: IcpRegistrationState):
        c = state.config
        return (nat.FLAVOUR_ICP_SURFACE if self._surface(c) else nat.FLAVOUR_ICP), nat.IcpParams(c.initialSigma, c.endSigma, c.maxIterations)

    def _prepare_native(self, state: IcpRegistrationState):
        self._select_direction(state.config)
        if self._surface(state.config):
            self._select_surface_method(state.config)

    def surfaceCorrespondence(self, state: IcpRegistrationState) -> Tuple[np.ndarray, np.ndarray]:
        """ClosestPointTriangleMesh3D.closestPointCorrespondence(fit, target) (ClosestPointRegistrator.scala:75-100) for the
        state's fit: (closest surface points (M,3), weights in {0,1})."""
        g, c = state.general, state.config
        if c.reverseCorrespondenceDirection:
            raise ValueError("reversed direction: use reversedCorrespondence (entries are per target vertex)")
        if not self._surface(c):
            raise ValueError("surfaceCorrespondence needs a surface correspondenceMethod (the state uses " + c.correspondenceMethod + ")")
        self._phase0(state)
        M = g.model.numberOfPoints
        cp, w = np.empty((M, 3)), np.empty(M)
        _check(self.ctx.handle, self._lib.gingr_fitter_get_surface_correspondence(self._fitter, dptr(cp), dptr(w)),
               "gingr_fitter_get_surface_correspondence")
        return cp, w

    def getCorrespondence(self, state: IcpRegistrationState) -> CorrespondencePairs:
        if state.config.reverseCorrespondenceDirection:                               # ICP.scala:46-50
            tid, w = self.reversedCorrespondence(state)
            keep = np.flatnonzero(w == 1.0)
            return CorrespondencePairs(tid[keep].astype(np.int64), f64(state.general.target)[keep])
        if self._surface(state.config):                                               # ICP.scala:40-41,50
            cp, w = self.surfaceCorrespondence(state)
            keep = np.flatnonzero(w == 1.0)
            return CorrespondencePairs(keep, cp[keep])
        idx, _, _ = self.ctx.nn(state.general.fit, state.general.target)              # ICP.scala:36-52
        return CorrespondencePairs(np.arange(idx.shape[0]), f64(state.general.target)[idx])

    def getUncertainty(self, pid: int, state: IcpRegistrationState) -> np.ndarray:
        return np.eye(3) * state.general.sigma2                                       # ICP.scala:90-92

    def updateSigma2(self, state: IcpRegistrationState) -> float:
        return max(state.general.sigma2 - state.config.sigmaStep, state.config.endSigma)   # ICP.scala:96-99

    def last_correspondence_indices(self) -> np.ndarray:
        M = self._dev_model.M_local
        idx = np.empty(M, dtype=np.int32)
        _check(self.ctx.handle, self._lib.gingr_fitter_get_icp_idx(self._fitter, iptr(idx), None), "gingr_fitter_get_icp_idx")
        return idx


def normalTangentCovariances(normals, varNormal, varTangent) -> np.ndarray:
    """(K, 3, 3) covariances varTangent I + (varNormal - varTangent) n n^T for K directions: variance varNormal along n, varTangent in
    the plane across it -- small along the surface normal and large in the tangent plane lets a vertex slide on the target surface
    (point-to-plane ICP).  normals (K, 3) are normalised, a zero normal gives varTangent I; the variances are scalars or (K,) arrays."""
    n = np.asarray(normals, dtype=np.float64)
    if n.ndim != 2 or n.shape[1] != 3:
        raise ValueError(f"normalTangentCovariances: normals of shape {n.shape}; need (K, 3)")
    K = n.shape[0]
    vn = np.broadcast_to(np.asarray(varNormal, dtype=np.float64), (K,))
    vt = np.broadcast_to(np.asarray(varTangent, dtype=np.float64), (K,))
    length = np.linalg.norm(n, axis=1)
    unit = np.where(length[:, None] > 0.0, n / np.where(length > 0.0, length, 1.0)[:, None], 0.0)
    return vt[:, None, None] * np.eye(3)[None] + (vn - vt)[:, None, None] * (unit[:, :, None] * unit[:, None, :])


class TemplateRegistration(GingrAlgorithm):
    """A registration algorithm from its three inputs (Template.scala:46-60; the plugin surface of GingrAlgorithm.scala:65-74,256-258):

    getCorrespondence(state) -> CorrespondencePairs   pids in any order, repeated or not, any subset.  Default: no pairs.
    getUncertainty(pids, state)                       a scalar variance, a (K,) array of variances or a (K, 3, 3) array of covariances
                                                      for the K pairs AT ONCE -- vectorised, where the reference asks pid by pid.
                                                      Default: variance 1 (the identity covariance, Template.scala:50-52).
    updateSigma2(newState) -> float                   Default: sigma2 stays (GingrAlgorithm.scala:256-258).  Called with the state an
                                                      update committed, fit already refreshed; not called after a failed update.

    Covariances that are exact multiples of the identity go to the fitter's isotropic list (one consolidated observation per
    vertex, the weighted Gram pass), the others to its covariance list (the landmark pass: meant for few pairs) or, with
    covariancePass="gram", to its dense covariance list (one consolidated precision per vertex, the 3 x 3-weighted Gram pass: meant
    for a covariance per vertex, as point-to-plane ICP has -- normalTangentCovariances).  Everything else
    -- posterior, projections, step length, global transform, failure rules and retries, the sampled proposal, the transition
    density, posteriorCovariance / posteriorModel -- is the device's, as for CPD and ICP (flavour 3 of the fitter).
    The callbacks run once per `update`; a later query about the SAME state object (logTransitionProbability, posteriorCovariance
    ...) reuses what they returned, and the lists are uploaded again only when a callback returned other objects than the fitter
    holds (arrays are treated as immutable).  There is no fused Metropolis-Hastings step for this algorithm (the correspondences
    come from the host): enableFusedSteps keeps the call-by-call path."""
    name = "Template"

    def __init__(self, ctx: Context, getCorrespondence: Optional[Callable] = None, getUncertainty: Optional[Callable] = None,
                 updateSigma2: Optional[Callable] = None, covariancePass: str = "landmark"):
        super().__init__(ctx)
        if covariancePass not in ("landmark", "gram"):
            raise ValueError(f"covariancePass: {covariancePass!r}; need \"landmark\" or \"gram\"")
        self.covariancePass = covariancePass
        self.getCorrespondence = getCorrespondence if getCorrespondence is not None else (lambda state: _empty_pairs())
        self.getUncertainty = getUncertainty if getUncertainty is not None else (lambda pids, state: 1.0)
        self._update_sigma2 = updateSigma2
        self._observed = None      # (state, pairs, uncertainty, split lists): what the callbacks said about `state`
        self._held = None          # (pids, points, uncertainty) objects behind the lists the fitter holds

    def updateSigma2(self, state) -> float:
        return float(state.general.sigma2) if self._update_sigma2 is None else float(self._update_sigma2(state))

    @staticmethod
    def splitObservations(pairs: CorrespondencePairs, uncertainty):
        """(pids, points, variances), (pids, points, covariances): the isotropic and the full-covariance list of the fitter.  Raises
        ValueError for pids / points of different length and for an uncertainty that is neither a scalar, (K,) nor (K, 3, 3)."""
        pids = np.asarray(pairs.pids)
        pts = np.asarray(pairs.points, dtype=np.float64)
        if pids.ndim != 1 or pts.shape != (pids.shape[0], 3):
            raise ValueError(f"getCorrespondence: {pids.shape[0] if pids.ndim == 1 else pids.shape} pids but points of shape {pts.shape}; "
                             "need (K,) and (K, 3)")
        K = pids.shape[0]
        pid32 = np.ascontiguousarray(pids, dtype=np.int32)
        pts = np.ascontiguousarray(pts)
        u = np.asarray(uncertainty, dtype=np.float64)
        none = (np.empty(0, dtype=np.int32), np.empty((0, 3)), np.empty((0, 3, 3)))
        if u.ndim == 0:
            return (pid32, pts, np.full(K, float(u))), none
        if u.shape == (K,):
            return (pid32, pts, np.ascontiguousarray(u)), none
        if u.shape != (K, 3, 3):
            raise ValueError(f"getUncertainty: shape {u.shape} for {K} pairs; need a scalar, ({K},) variances or ({K}, 3, 3) covariances")
        d = u[:, 0, 0]
        iso = np.all(u == d[:, None, None] * np.eye(3)[None], axis=(1, 2))      # exact multiples of the identity
        ki, kc = np.flatnonzero(iso), np.flatnonzero(~iso)
        return ((np.ascontiguousarray(pid32[ki]), np.ascontiguousarray(pts[ki]), np.ascontiguousarray(d[ki])),
                (np.ascontiguousarray(pid32[kc]), np.ascontiguousarray(pts[kc]), np.ascontiguousarray(u[kc])))

    def _observe(self, state):
        """The callbacks' answer for `state`, asked once per state object."""
        if self._observed is None or self._observed[0] is not state:
            pairs = self.getCorrespondence(state)
            unc = self.getUncertainty(pairs.pids, state)
            self._observed = (state, pairs, unc, self.splitObservations(pairs, unc))
        return self._observed

    def _push_pairs(self, state):
        _, pairs, unc, (iso, cov) = self._observe(state)
        h = self._held
        same_unc = h is not None and (h[2] is unc or (np.ndim(unc) == 0 and np.ndim(h[2]) == 0 and float(h[2]) == float(unc)))
        if h is not None and h[0] is pairs.pids and h[1] is pairs.points and same_unc:
            return
        n = h[3] if h is not None else (0, 0)          # what the fitter holds: nothing to clear in an empty list
        if iso[0].shape[0] or n[0]:
            k = iso[0].shape[0]
            _check(self.ctx.handle, self._lib.gingr_fitter_set_pairs(self._fitter, k, iptr(iso[0]) if k else None, dptr(iso[1]) if k else None,
                                                                     dptr(iso[2]) if k else None), "gingr_fitter_set_pairs")
        if cov[0].shape[0] or n[1]:
            k = cov[0].shape[0]
            name = "gingr_fitter_set_pairs_cov_dense" if self.covariancePass == "gram" else "gingr_fitter_set_pairs_cov"
            _check(self.ctx.handle, getattr(self._lib, name)(self._fitter, k, iptr(cov[0]) if k else None, dptr(cov[1]) if k else None,
                                                             dptr(cov[2]) if k else None), name)
        self._held = (pairs.pids, pairs.points, unc, (iso[0].shape[0], cov[0].shape[0]))

    def _release(self):
        super()._release()
        self._held = None          # (the lists went with the fitter)

    def createInitialState(self, model: PointDistributionModel, target, config: Optional[TemplateConfiguration] = None,
                           transform: int = GlobalTranformationType.RigidTransforms, stepLength: float = 1.0,
                           landmarks: Optional[LandmarkCorrespondences] = None, initial_pose=None,
                           targetCells: Optional[np.ndarray] = None, sigma2: float = 1.0) -> TemplateRegistrationState:
        g = _initial_general(self.ctx, model, target, float(sigma2), transform, stepLength, landmarks, initial_pose, targetCells)
        return self.initializeState(g, config if config is not None else TemplateConfiguration())

    def initializeState(self, general: GeneralRegistrationState, config: TemplateConfiguration) -> TemplateRegistrationState:
        return TemplateRegistrationState(general, config)                      # Template.scala:55-60

    def update(self, current, probabilistic: bool = False, rnd: Optional[np.random.Generator] = None):
        self._observe(current)     # (argument errors of the callbacks' results surface before anything is sent to the device)
        out = super().update(current, probabilistic, rnd)
        if self._update_sigma2 is None:
            return out
        err = ctypes.c_int32()
        _check(self.ctx.handle, self._lib.gingr_fitter_last_update_error(self._fitter, ctypes.byref(err)), "gingr_fitter_last_update_error")
        if err.value != 0:         # the update did not commit: no newState, no updateSigma2 (GingrAlgorithm.scala:238-247)
            return out
        s2 = float(self._update_sigma2(out))
        if s2 == out.general.sigma2:
            return out
        _check(self.ctx.handle, self._lib.gingr_fitter_set_sigma2(self._fitter, s2), "gingr_fitter_set_sigma2")
        new = out.updateGeneral(out.general.updateSigma2(s2))
        self._device_state = new
        return new

    def _run_resident(self, state):
        # the callbacks run on the host every iteration: the generic loop of `run`, never a block of updates enqueued at once
        return GingrAlgorithm.run(self, state, callBackLogger=lambda s: None)

    def _correspondence(self, state: TemplateRegistrationState):
        return nat.FLAVOUR_PAIRS, None

    def _prepare_native(self, state: TemplateRegistrationState):
        self._push_pairs(state)

    def _native_update(self, current: TemplateRegistrationState, n: int):
        if n != 1:
            raise ValueError("Template: one update per call (the correspondences of the next one come from the host)")
        super()._native_update(current, n)

    def pairObservations(self, state) -> Tuple[np.ndarray, np.ndarray]:
        """The isotropic pairs of `state` as the device consolidated them: (observed point (M, 3), weight (M,)) per vertex -- the
        precision-weighted mean of a vertex's pairs and their summed precision; weight 0 = no pair."""
        self._ensure_device_state(state)
        self._push_pairs(state)
        M = state.general.model.numberOfPoints
        obs, w = np.empty((M, 3)), np.empty(M)
        _check(self.ctx.handle, self._lib.gingr_fitter_get_pair_observations(self._fitter, dptr(obs), dptr(w)), "gingr_fitter_get_pair_observations")
        return obs, w

    def pairPrecisions(self, state) -> Tuple[np.ndarray, np.ndarray]:
        """The covariance pairs of `state` as the device consolidated them for covariancePass="gram": (observed point (M, 3),
        precision (M, 6): xx, xy, xz, yy, yz, zz) per vertex -- the summed precision of a vertex's pairs and their precision-weighted
        mean; all zero = no pair (and everywhere with covariancePass="landmark")."""
        self._ensure_device_state(state)
        self._push_pairs(state)
        M = state.general.model.numberOfPoints
        obs, prec = np.empty((M, 3)), np.empty((M, 6))
        _check(self.ctx.handle, self._lib.gingr_fitter_get_pair_precisions(self._fitter, dptr(obs), dptr(prec)), "gingr_fitter_get_pair_precisions")
        return obs, prec


class PointToPlaneIcpRegistration(GingrAlgorithm):
    """Point-to-plane ICP on the surfaces as a resident algorithm: per model vertex the closest point of the target surface, observed
    with the covariance v_t I + (v_n - v_t) n n^T -- v_n = sigma2 along the face normal n of the target triangle the point lies on,
    v_t = tangentOverNormal * sigma2 across it -- and ICP's sigma2 schedule.  Correspondence, planes, update and schedule all run on the
    device (gingr_fitter_update_plane_async): `update` is one such iteration, `run` without call-backs enqueues all of them in one call
    and reads the state once.  What TemplateRegistration does with closest-point and normalTangentCovariances callbacks on the host,
    without the host: no transfer and no synchronisation per iteration.

    The update itself is the fitter's pairs flavour, so the sampled update, logTransitionProbability, posteriorCovariance and
    posteriorModel are its queries; each refreshes the planes from the state it is asked about first.  Needs both triangulations
    (model.cells and targetCells) -- or, against a target that is a point cloud (a depth or laser scan: no triangles), a normal per
    target point: createInitialState(..., targetNormals=an (N, 3) array | "estimate").  There the observed point is the nearest target
    point and n its normal (gingr_fitter_update_plane_cloud_async); "estimate" takes the normals from the PCA of each target point's
    targetNeighbours nearest neighbours, on the device (Context.cloud_normals).  There is no fused Metropolis-Hastings step:
    enableFusedSteps keeps the call-by-call path."""
    name = "PointToPlaneICP"

    def __init__(self, ctx: Context):
        super().__init__(ctx)
        self._params_memo = None   # (config object, PlaneParams, PlaneCloudParams, IcpParams)
        self._planes = None        # (state, closest points, weights, precisions): what the device used for `state`
        self._held_normals = None  # (model, target, normals, neighbours) behind the target normals the fitter holds
        self._held_robust = None   # native parameters of the robust setting the fitter holds; None: off

    def createInitialState(self, model: PointDistributionModel, target, config: PointToPlaneConfiguration,
                           transform: int = GlobalTranformationType.RigidTransforms, stepLength: float = 1.0,
                           landmarks: Optional[LandmarkCorrespondences] = None, initial_pose=None,
                           targetCells: Optional[np.ndarray] = None, targetNormals=None,
                           targetNeighbours: int = 16) -> PointToPlaneRegistrationState:
        """targetCells (with model.cells): the surface route.  targetCells None and targetNormals an (N, 3) array or "estimate": the
        target is a point cloud with a normal per point; model.cells is not needed."""
        if targetCells is not None or targetNormals is None:
            if getattr(model, "cells", None) is None or targetCells is None:
                raise ValueError("point-to-plane ICP needs the triangulations (model.cells and targetCells)")
            targetNormals = None
        g = _initial_general(self.ctx, model, target, 1.0, transform, stepLength, landmarks, initial_pose, targetCells)
        return self.initializeState(g, config, targetNormals, targetNeighbours)

    def initializeState(self, general: GeneralRegistrationState, config: PointToPlaneConfiguration, targetNormals=None,
                        targetNeighbours: int = 16) -> PointToPlaneRegistrationState:
        if targetNormals is None:
            if getattr(general.model, "cells", None) is None or general.targetCells is None:
                raise ValueError("point-to-plane ICP needs the triangulations (model.cells and targetCells)")
        else:
            if config.reject:
                raise ValueError("reject=True needs the triangulations: the three rejection rules of the surface ICP do not apply to a "
                                 "point-cloud target (maxDistance does)")
            if not isinstance(targetNormals, str):
                targetNormals = f64(targetNormals)
                if targetNormals.shape != np.shape(general.target):
                    raise ValueError(f"targetNormals of shape {targetNormals.shape} for a target of shape {np.shape(general.target)}")
            elif targetNormals != "estimate":
                raise ValueError(f"targetNormals: {targetNormals!r}; need an (N, 3) array or \"estimate\"")
        if not (np.isfinite(config.tangentOverNormal) and config.tangentOverNormal >= 1.0):
            raise ValueError(f"tangentOverNormal: {config.tangentOverNormal!r}; need a finite ratio >= 1")
        if config.robust is not None and not isinstance(config.robust, RobustLoss):
            raise ValueError(f"robust: {config.robust!r}; need a RobustLoss or None")
        return PointToPlaneRegistrationState(general.updateSigma2(float(config.initialSigma)), config, targetNormals, int(targetNeighbours))

    def _params(self, config: PointToPlaneConfiguration):
        memo = self._params_memo
        if memo is None or memo[0] is not config:
            memo = (config, nat.PlaneParams(float(config.tangentOverNormal), 1 if config.reject else 0),
                    nat.PlaneCloudParams(float(config.tangentOverNormal), float(config.maxDistance or 0.0)),
                    nat.IcpParams(float(config.initialSigma), float(config.endSigma), int(config.maxIterations)))
            self._params_memo = memo
        return memo[1:]

    def _correspondence(self, state: PointToPlaneRegistrationState):
        return nat.FLAVOUR_PAIRS, None

    def _release(self):
        super()._release()
        self._held_normals = None  # (the normals went with the fitter)
        self._held_robust = None

    def _push_robust(self, config: PointToPlaneConfiguration):
        """the robust setting of `config` onto the fitter, once per (fitter, setting)"""
        want = None if config.robust is None else config.robust.native
        if self._held_robust == want:       # (a new fitter holds none: _release)
            return
        rp = None if want is None else nat.RobustParams(*want)
        _check(self.ctx.handle, self._lib.gingr_fitter_set_plane_robust(self._fitter, None if rp is None else ctypes.byref(rp)),
               "gingr_fitter_set_plane_robust")
        self._held_robust = want

    def _push_normals(self, state: PointToPlaneRegistrationState):
        """the target normals of a point-cloud state onto the fitter, once per (model, target, normals)"""
        want = (self._bound_model, self._bound_target, state.targetNormals, state.targetNeighbours)
        held = self._held_normals
        if held is not None and all(a is b for a, b in zip(held[:3], want[:3])) and held[3] == want[3]:
            return
        if isinstance(state.targetNormals, str):
            _check(self.ctx.handle, self._lib.gingr_fitter_estimate_target_normals(self._fitter, int(state.targetNeighbours), None, None),
                   "gingr_fitter_estimate_target_normals")
        else:
            _check(self.ctx.handle, self._lib.gingr_fitter_set_target_normals(self._fitter, dptr(state.targetNormals)),
                   "gingr_fitter_set_target_normals")
        self._held_normals = want

    def targetNormals(self, state: PointToPlaneRegistrationState) -> np.ndarray:
        """(N, 3): the unit (or zero) normals per target point the device uses for a point-cloud state"""
        self._ensure_device_state(state)
        self._push_normals(state)
        out = np.empty((np.shape(state.general.target)[0], 3))
        _check(self.ctx.handle, self._lib.gingr_fitter_get_target_normals(self._fitter, dptr(out)), "gingr_fitter_get_target_normals")
        return out

    def _prepare_native(self, state: PointToPlaneRegistrationState):
        # the queries of the pairs flavour read the planes as they stand: make them the ones of the state the device holds
        pp, pc, _ = self._params(state.config)
        self._push_robust(state.config)
        if state.targetNormals is not None:
            self._push_normals(state)
            _check(self.ctx.handle, self._lib.gingr_fitter_set_pairs_plane_cloud_async(self._fitter, ctypes.byref(pc)),
                   "gingr_fitter_set_pairs_plane_cloud_async")
            return
        _check(self.ctx.handle, self._lib.gingr_fitter_set_pairs_plane_async(self._fitter, ctypes.byref(pp)),
               "gingr_fitter_set_pairs_plane_async")

    def _native_update(self, current: PointToPlaneRegistrationState, n: int):
        pp, pc, ip = self._params(current.config)
        self._push_robust(current.config)
        if current.targetNormals is not None:
            self._push_normals(current)
            _check(self.ctx.handle, self._lib.gingr_fitter_update_plane_cloud_async(self._fitter, ctypes.byref(pc), ctypes.byref(ip), int(n)),
                   "gingr_fitter_update_plane_cloud_async")
            return
        _check(self.ctx.handle, self._lib.gingr_fitter_update_plane_async(self._fitter, ctypes.byref(pp), ctypes.byref(ip), int(n)),
               "gingr_fitter_update_plane_async")

    def updateSigma2(self, state: PointToPlaneRegistrationState) -> float:
        return max(state.general.sigma2 - state.config.sigmaStep, state.config.endSigma)   # ICP.scala:96-99

    def update(self, current, probabilistic: bool = False, rnd: Optional[np.random.Generator] = None):
        out = super().update(current, probabilistic, rnd)
        if not probabilistic:
            return out             # (the schedule ran on the device, behind the update)
        err = ctypes.c_int32()
        _check(self.ctx.handle, self._lib.gingr_fitter_last_update_error(self._fitter, ctypes.byref(err)), "gingr_fitter_last_update_error")
        if err.value != 0 or out.general.status == FittingStatuses.ModelFlexibilityError:
            return out             # the update did not commit: sigma2 stays
        s2 = self.updateSigma2(out)
        if s2 == out.general.sigma2:
            return out
        _check(self.ctx.handle, self._lib.gingr_fitter_set_sigma2(self._fitter, s2), "gingr_fitter_set_sigma2")
        new = out.updateGeneral(out.general.updateSigma2(s2))
        self._device_state = new
        return new

    def _observed(self, state):
        """(closest points (M, 3), weights (M,), precisions (M, 6)) the device makes for `state`, asked once per state object"""
        if self._planes is None or self._planes[0] is not state:
            self._ensure_device_state(state)
            self._prepare_native(state)
            M = state.general.model.numberOfPoints
            cp, w, obs, prec = np.empty((M, 3)), np.empty(M), np.empty((M, 3)), np.empty((M, 6))
            if state.targetNormals is not None:    # the nearest target points, and who lies within maxDistance
                idx, d2 = np.empty(M, dtype=np.int32), np.empty(M)
                _check(self.ctx.handle, self._lib.gingr_fitter_get_icp_idx(self._fitter, iptr(idx), dptr(d2)), "gingr_fitter_get_icp_idx")
                cp = f64(state.general.target)[idx]
                far = float(state.config.maxDistance or 0.0)
                w = np.where(d2 > far * far, 0.0, 1.0) if far > 0.0 else np.ones(M)
            else:
                _check(self.ctx.handle, self._lib.gingr_fitter_get_surface_correspondence(self._fitter, dptr(cp), dptr(w)),
                       "gingr_fitter_get_surface_correspondence")
            _check(self.ctx.handle, self._lib.gingr_fitter_get_pair_precisions(self._fitter, dptr(obs), dptr(prec)),
                   "gingr_fitter_get_pair_precisions")
            robust = None
            if state.config.robust is not None:    # the inflation per vertex; a vertex Tukey removed is not observed
                u, c, n = np.empty(M), ctypes.c_double(), ctypes.c_int64()
                _check(self.ctx.handle, self._lib.gingr_fitter_get_plane_robust(self._fitter, None, dptr(u), None, ctypes.byref(c), ctypes.byref(n)),
                       "gingr_fitter_get_plane_robust")
                w = np.where(u > 0.0, w, 0.0)
                robust = (u, float(c.value), int(n.value))
            self._planes = (state, cp, w, prec, robust)
        return self._planes[1:4]

    def robustWeights(self, state) -> Tuple[np.ndarray, float, int]:
        """(weights (M,), c, nObserved) the device used for `state` under config.robust: the weight 1 / u of every vertex -- 1 = taken at
        sigma2, towards 0 = discounted, 0 = not observed (rejected, beyond maxDistance, or removed by Tukey's loss) -- the scale c and
        the number of vertices the correspondence observed (the ones the median is taken over)."""
        if state.config.robust is None:
            raise ValueError("robustWeights: the state's configuration has no robust loss")
        self._observed(state)
        u, c, n = self._planes[4]
        return np.where(u > 0.0, 1.0 / np.where(u > 0.0, u, 1.0), 0.0), c, n

    def surfaceCorrespondence(self, state) -> Tuple[np.ndarray, np.ndarray]:
        """(closest surface points (M, 3), weights in {0, 1}) as the device used them for the state's fit; against a point-cloud
        target the nearest target points"""
        cp, w, _ = self._observed(state)
        return cp, w

    def pairPrecisions(self, state) -> np.ndarray:
        """(M, 6): the precision planes xx, xy, xz, yy, yz, zz the device used for `state`; all zero = no observation"""
        return self._observed(state)[2]

    def getCorrespondence(self, state) -> CorrespondencePairs:
        cp, w, _ = self._observed(state)
        keep = np.flatnonzero(w == 1.0)
        return CorrespondencePairs(keep, cp[keep])

    def getUncertainty(self, pid: int, state) -> np.ndarray:
        """v_t I + (v_n - v_t) n n^T with the face normal the device used for vertex `pid` (read back from its precision)"""
        _, _, prec = self._observed(state)
        vn = float(state.general.sigma2)
        if state.config.robust is not None:        # the inflated variance sigma2 * u the device used
            u = self._planes[4][0][int(pid)]
            vn *= float(u) if u > 0.0 else np.inf
        vt = float(state.config.tangentOverNormal) * vn
        a, b = 1.0 / vt, 1.0 / vn - 1.0 / vt
        xx, xy, xz, yy, yz, zz = prec[int(pid)]
        lam = np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])
        nnt = (lam - a * np.eye(3)) / b if b > 0.0 else np.zeros((3, 3))
        return vt * np.eye(3) + (vn - vt) * nnt
