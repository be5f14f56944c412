"""Host mirror of the reference's classic Coherent Point Drift family (G/other/algorithms/: cpd/CPDFactory.scala, cpd/RigidCPD.scala,
cpd/AffineCPD.scala, cpd/NonRigidCPD.scala, CPDRegistration.scala) over the device-resident engine of csrc/classic_cpd.hip:

    cpd = CPDFactory(ctx, templatePoints, lambda_=2, beta=2, w=0)
    fit = cpd.registerNonRigidly(targetPoints).Registration(max_iteration=100, tolerance=0.001)

Expectation / Maximization run on the GPU (streaming statistics instead of the M x N matrix P; blocked Cholesky for the non-rigid
M x M system); this module keeps the Registration loop with its convergence test (RigidCPD.scala:59-83)."""
from __future__ import annotations

import ctypes
from ctypes import c_void_p
from typing import Optional, Tuple

import numpy as np

from .api import Context, _check
from ._native import f64, dptr

RIGID, AFFINE, NONRIGID = 0, 1, 2


def _transform_points(ctx: Context, entry, handle, points, name: str) -> np.ndarray:
    pts = f64(points)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError("points: (P, 3) expected")
    out = np.empty_like(pts)
    _check(ctx.handle, entry(handle, pts.shape[0], dptr(pts), dptr(out)), name)
    return out


class LowRankG:
    """The non-rigid kind over a low-rank factor of the kernel matrix, G ~ L L^T (Myronenko & Song 2010, "fast implementation"):
    the pivoted Cholesky of the Gaussian over the template, stopped when the residual trace falls below relativeTolerance * trace or
    at maxColumns (0: the library's ceiling of 512 columns).  No M x M matrix is formed: templates past the dense limit register."""

    def __init__(self, relativeTolerance: float = 1e-8, maxColumns: int = 0):
        self.relativeTolerance, self.maxColumns = float(relativeTolerance), int(maxColumns)


class RigidCPD:
    """RigidCPD / AffineCPD / NonRigidCPD (one class, `kind` selects the Maximization; lowRank: a LowRankG, non-rigid only)."""

    def __init__(self, factory: "CPDFactory", targetPoints, kind: int, lowRank: Optional[LowRankG] = None):
        if lowRank is not None and kind != NONRIGID:
            raise ValueError("lowRank applies to the non-rigid kind only")
        self.cpd, self.kind = factory, kind
        self.target = f64(targetPoints)
        self.N = self.target.shape[0]
        self._lib = factory.ctx._lib
        self._h, self.lowRankInfo = None, None
        h = c_void_p()
        if lowRank is None:
            _check(factory.ctx.handle, self._lib.gingr_classic_cpd_create(factory.ctx.handle, kind, factory.M, dptr(factory.template), self.N,
                                                                          dptr(self.target), float(factory.lambda_), float(factory.beta),
                                                                          float(factory.w), ctypes.byref(h)), "gingr_classic_cpd_create")
        else:
            from ._native import ClassicCpdLowRankInfo
            info = ClassicCpdLowRankInfo()
            _check(factory.ctx.handle, self._lib.gingr_classic_cpd_create_lowrank(
                factory.ctx.handle, factory.M, dptr(factory.template), self.N, dptr(self.target), float(factory.lambda_), float(factory.beta),
                float(factory.w), float(lowRank.relativeTolerance), int(lowRank.maxColumns), ctypes.byref(info), ctypes.byref(h)),
                "gingr_classic_cpd_create_lowrank")
            self.lowRankInfo = {"columns": int(info.columns), "tolerance_reached": bool(info.tolerance_reached),
                                "residual_fraction": float(info.residual_fraction), "factor_bytes": int(info.factor_bytes)}
        self._h = h
        self._sigma2_init = self.sigma2()      # initializeGaussianKernel of the factory's template against this target

    def close(self):
        if self._h:
            self._lib.gingr_classic_cpd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- device state ---------------------------------------------------------------------------------------------
    def state(self) -> Tuple[np.ndarray, float]:
        ty = np.empty((self.cpd.M, 3))
        s2 = ctypes.c_double()
        _check(self.cpd.ctx.handle, self._lib.gingr_classic_cpd_get(self._h, dptr(ty), ctypes.byref(s2), None, None), "gingr_classic_cpd_get")
        return ty, s2.value

    def sigma2(self) -> float:
        s2 = ctypes.c_double()
        _check(self.cpd.ctx.handle, self._lib.gingr_classic_cpd_get(self._h, None, ctypes.byref(s2), None, None), "gingr_classic_cpd_get")
        return s2.value

    def set_state(self, ty, sigma2: float):
        ty = f64(ty)
        _check(self.cpd.ctx.handle, self._lib.gingr_classic_cpd_set(self._h, dptr(ty), float(sigma2)), "gingr_classic_cpd_set")

    def transform(self) -> Tuple[float, np.ndarray, np.ndarray]:
        """(s, R or B, t) of the last rigid / affine Maximization: TY = s Y R^T + 1 t^T."""
        p = np.zeros(13)
        _check(self.cpd.ctx.handle, self._lib.gingr_classic_cpd_get(self._h, None, None, dptr(p), None), "gingr_classic_cpd_get")
        return float(p[0]), p[1:10].reshape(3, 3).copy(), p[10:13].copy()

    def W(self) -> np.ndarray:
        w = np.empty((self.cpd.M, 3))
        _check(self.cpd.ctx.handle, self._lib.gingr_classic_cpd_get(self._h, None, None, None, dptr(w)), "gingr_classic_cpd_get")
        return w

    def factor(self) -> np.ndarray:
        """L (M, k) of a low-rank task: G ~ L @ L.T"""
        k = ctypes.c_int32()
        _check(self.cpd.ctx.handle, self._lib.gingr_classic_cpd_get_factor(self._h, ctypes.byref(k), None), "gingr_classic_cpd_get_factor")
        L = np.empty((self.cpd.M, k.value))
        _check(self.cpd.ctx.handle, self._lib.gingr_classic_cpd_get_factor(self._h, None, dptr(L)), "gingr_classic_cpd_get_factor")
        return L

    def transformPoints(self, points) -> np.ndarray:
        """The map of the last Iteration at any points (P, 3), on the device (csrc/kernel_warp.hip).  Rigid / affine: s B z + t with
        transform(); non-rigid: z + sum_m g(z, y_m) W_m with y the factory's template, W() and the true Gaussian -- at the template
        points the TY of an Iteration that started from the template (low-rank: to the factor's tolerance).  As transform() and W(),
        it is the last step alone: Registration feeds TY back into the next Iteration.  GINGR_ERR_STATE before the first Iteration
        and after set_state."""
        return _transform_points(self.cpd.ctx, self._lib.gingr_classic_cpd_transform_points, self._h, points,
                                 "gingr_classic_cpd_transform_points")

    # -- the reference surface ------------------------------------------------------------------------------------
    def Iteration(self, Y=None, sigma2: Optional[float] = None) -> Tuple[np.ndarray, float]:
        """Iteration(X, Y, sigma2) (RigidCPD.scala:85-88) = Maximization(Expectation(...)); without arguments it advances the
        device state."""
        if Y is not None:
            self.set_state(Y, sigma2)
        _check(self.cpd.ctx.handle, self._lib.gingr_classic_cpd_iterate(self._h, 1), "gingr_classic_cpd_iterate")
        return self.state()

    def Registration(self, max_iteration: int, tolerance: float = 0.001, verbose: bool = False) -> np.ndarray:
        """RigidCPD.Registration (:59-83): iterate until |sigma2' - sigma2| < tolerance or max_iteration non-converged iterations."""
        i, converged = 0, False
        # the reference always starts from cpd.template and the initial variance (RigidCPD.scala:59-62), whatever Iteration or an
        # earlier Registration left on the device
        self.set_state(self.cpd.template, self._sigma2_init)
        current = self._sigma2_init
        while i < max_iteration and not converged:
            if verbose:
                print(f"CPD, iteration: {i}, variance: {current}")
            _check(self.cpd.ctx.handle, self._lib.gingr_classic_cpd_iterate(self._h, 1), "gingr_classic_cpd_iterate")
            new = self.sigma2()
            if abs(new - current) < tolerance:
                if verbose:
                    print("Converged")
                converged = True
            else:
                i += 1
            current = new
        self.iterations, self.converged = i, converged
        return self.state()[0]


class CPDFactory:
    def __init__(self, ctx: Context, templatePoints, lambda_: float = 2.0, beta: float = 2.0, w: float = 0.0):
        if not (0.0 <= w <= 1.0) or not beta > 0 or not lambda_ > 0:
            raise ValueError("requirement failed")          # CPDFactory.scala:43-45
        self.ctx, self.lambda_, self.beta, self.w = ctx, lambda_, beta, w
        self.template = f64(templatePoints)
        self.M, self.dim = self.template.shape[0], 3

    def registerRigidly(self, targetPoints) -> RigidCPD:
        return RigidCPD(self, targetPoints, RIGID)

    def registerNonRigidly(self, targetPoints, lowRank: Optional[LowRankG] = None) -> RigidCPD:
        return RigidCPD(self, targetPoints, NONRIGID, lowRank)

    def registerAffine(self, targetPoints) -> RigidCPD:
        return RigidCPD(self, targetPoints, AFFINE)


class RigidCPDRegistration:
    """RigidCPDRegistration / NonRigidCPDRegistration / AffineCPDRegistration (CPDRegistration.scala:23-73): register(target)
    returns the warped template points; register(target, points) the pair (warped template, transformPoints(points)) of the task.
    The two do not correspond once Registration has taken more than one Iteration: the first is the whole registration, the second
    the map of its LAST Iteration alone (the reference feeds TY back, and transform() / W() / transformPoints are one step's; close to
    the identity at convergence).  To carry a whole classic registration to other points, take the Iterations one by one and compose
    the rigid / affine steps, or add up the non-rigid steps' displacements transformPoints(points) - points (G is fixed over the
    template, TY = Y + G sum_i W_i) as examples/demo_classic_cpd.py does; BCPDRegistration.register(target, points) is the whole map."""

    _kind = RIGID

    def __init__(self, ctx: Context, template, lambda_: float = 2.0, beta: float = 2.0, w: float = 0.0, max_iterations: int = 100,
                 lowRank: Optional[LowRankG] = None):
        if lowRank is not None and self._kind != NONRIGID:
            raise ValueError("lowRank applies to the non-rigid kind only")
        self.cpd, self.max_iterations, self.lowRank = CPDFactory(ctx, template, lambda_, beta, w), max_iterations, lowRank

    def register(self, target, points=None):
        task = RigidCPD(self.cpd, target, self._kind, self.lowRank)
        try:
            warped = task.Registration(self.max_iterations)
            return warped if points is None else (warped, task.transformPoints(points))
        finally:
            task.close()


class NonRigidCPDRegistration(RigidCPDRegistration):
    _kind = NONRIGID


class AffineCPDRegistration(RigidCPDRegistration):
    _kind = AFFINE


# ------------------------------------------------------------------------------------------------ Bayesian coherent point drift
class BCPD:
    """Bayesian coherent point drift (Hirose 2020) over csrc/bcpd.hip -- the method of the reference's draft cpd/BCPD.scala in this
    package's definition (include/gingr_hip.h; DESIGN.md section 5 lists where it follows the paper against the draft).  The reference
    takes any PDKernel; here the kernel is the Gaussian of CPDFactory, g(a, b) = exp(-|a - b|^2 / (2 beta^2)).  `k` is the paper's
    kappa (math.inf: constant mixing weights 1 / M).  The state (yhat, sigma_m^2, <alpha_m>, s, R, t, sigma2) lives on the device.
    lowRank: a LowRankG -- the deformation step over G ~ L L^T (csrc/bcpd_lowrank.hip: the acceleration the paper proposes), for
    templates past the dense limit of 32 768 points; `lowRankInfo` and `factor()` are those of the classic low-rank task."""

    def __init__(self, ctx: Context, templatePoints, targetPoints, w: float = 0.0, lambda_: float = 2.0, gamma: float = 1.0,
                 k: float = 1.0, beta: float = 2.0, lowRank: Optional[LowRankG] = None):
        self.ctx, self._lib = ctx, ctx._lib
        self.template, self.target = f64(templatePoints), f64(targetPoints)
        self.M, self.N = self.template.shape[0], self.target.shape[0]
        self.w, self.lambda_, self.gamma, self.k, self.beta = w, lambda_, gamma, k, beta
        self._h, self.lowRankInfo = None, None
        h = c_void_p()
        if lowRank is None:
            _check(ctx.handle, self._lib.gingr_bcpd_create(ctx.handle, self.M, dptr(self.template), self.N, dptr(self.target), float(w),
                                                           float(lambda_), float(gamma), float(k), float(beta), ctypes.byref(h)),
                   "gingr_bcpd_create")
        else:
            from ._native import ClassicCpdLowRankInfo
            info = ClassicCpdLowRankInfo()
            _check(ctx.handle, self._lib.gingr_bcpd_create_lowrank(
                ctx.handle, self.M, dptr(self.template), self.N, dptr(self.target), float(w), float(lambda_), float(gamma), float(k),
                float(beta), float(lowRank.relativeTolerance), int(lowRank.maxColumns), ctypes.byref(info), ctypes.byref(h)),
                "gingr_bcpd_create_lowrank")
            self.lowRankInfo = {"columns": int(info.columns), "tolerance_reached": bool(info.tolerance_reached),
                                "residual_fraction": float(info.residual_fraction), "factor_bytes": int(info.factor_bytes)}
        self._h = h
        self._sigma2_init = self.sigma2()

    def close(self):
        if self._h:
            self._lib.gingr_bcpd_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _get(self, *args):
        _check(self.ctx.handle, self._lib.gingr_bcpd_get(self._h, *args), "gingr_bcpd_get")

    # -- device state ---------------------------------------------------------------------------------------------
    def state(self) -> dict:
        """the state and the by-products of the iteration that left it: yhat, vhat (M x 3), sigma_diag, alpha, nu (M), nu_prime (N),
        s, R, t, sigma2, Nhat, sigma_bar2"""
        yh, vh = np.empty((self.M, 3)), np.empty((self.M, 3))
        sig, alpha, nu, nup = np.empty(self.M), np.empty(self.M), np.empty(self.M), np.empty(self.N)
        p, sc = np.empty(13), np.empty(3)
        self._get(dptr(yh), dptr(vh), dptr(sig), dptr(alpha), dptr(nu), dptr(nup), dptr(p), dptr(sc))
        return dict(yhat=yh, vhat=vh, sigma_diag=sig, alpha=alpha, nu=nu, nu_prime=nup, s=float(p[0]), R=p[1:10].reshape(3, 3).copy(),
                    t=p[10:13].copy(), sigma2=float(sc[0]), Nhat=float(sc[1]), sigma_bar2=float(sc[2]))

    def points(self) -> np.ndarray:
        yh = np.empty((self.M, 3))
        self._get(dptr(yh), None, None, None, None, None, None, None)
        return yh

    def sigma2(self) -> float:
        sc = np.empty(3)
        self._get(None, None, None, None, None, None, None, dptr(sc))
        return float(sc[0])

    def set_state(self, yhat=None, sigma_diag=None, alpha=None, s=None, R=None, t=None, sigma2=None):
        """inject any part of the state (None: left as it is; s, R, t go together)"""
        p = None
        if s is not None or R is not None or t is not None:
            p = np.concatenate([[float(s)], f64(R).reshape(9), f64(t).reshape(3)])
        yhat, sigma_diag, alpha = (None if a is None else f64(a) for a in (yhat, sigma_diag, alpha))
        if (yhat is not None and yhat.shape != (self.M, 3)) or any(a is not None and a.shape != (self.M,) for a in (sigma_diag, alpha)):
            raise ValueError("BCPD.set_state: shape mismatch")
        _check(self.ctx.handle, self._lib.gingr_bcpd_set(self._h, dptr(yhat), dptr(sigma_diag), dptr(alpha), dptr(p),
                                                         0.0 if sigma2 is None else float(sigma2)), "gingr_bcpd_set")

    def reset(self):
        """back to the start: (template, 1, 1 / M, s = 1, R = I, t = 0, the initial variance)"""
        self.set_state(self.template, np.ones(self.M), np.full(self.M, 1.0 / self.M), 1.0, np.eye(3), np.zeros(3), self._sigma2_init)

    def transform(self) -> Tuple[float, np.ndarray, np.ndarray]:
        """(s, R, t) of the last iteration: yhat = s (y + vhat) R^T + 1 t^T"""
        p = np.empty(13)
        self._get(None, None, None, None, None, None, dptr(p), None)
        return float(p[0]), p[1:10].reshape(3, 3).copy(), p[10:13].copy()

    def factor(self) -> np.ndarray:
        """L (M, k) of a low-rank task: G ~ L @ L.T"""
        k = ctypes.c_int32()
        _check(self.ctx.handle, self._lib.gingr_bcpd_get_factor(self._h, ctypes.byref(k), None), "gingr_bcpd_get_factor")
        L = np.empty((self.M, k.value))
        _check(self.ctx.handle, self._lib.gingr_bcpd_get_factor(self._h, None, dptr(L)), "gingr_bcpd_get_factor")
        return L

    def correspondenceWeights(self) -> Tuple[np.ndarray, np.ndarray]:
        """(nu = P 1, nu' = P^T 1) of the last iteration: how much of the target a template point explains, and the probability that a
        target point is no outlier"""
        nu, nup = np.empty(self.M), np.empty(self.N)
        self._get(None, None, None, None, dptr(nu), dptr(nup), None, None)
        return nu, nup

    def transformPoints(self, points) -> np.ndarray:
        """The map of the last iteration at any points (P, 3), on the device (csrc/kernel_warp.hip):
        s R (z + sum_m g(z, y_m) c_m) + t with c = deformationCoefficients() -- the Gaussian-process posterior mean of the
        displacement field at z (the interpolation step of BCPD++, Hirose 2021), then the similarity; at the template points it is
        points().  GINGR_ERR_STATE before the first iteration and after set_state."""
        return _transform_points(self.ctx, self._lib.gingr_bcpd_transform_points, self._h, points, "gingr_bcpd_transform_points")

    def deformationCoefficients(self) -> np.ndarray:
        """c (M, 3) with vhat = G c (low-rank: L L^T c): (c2 / lambda) (r - nu o vhat) of the last iteration"""
        c = np.empty((self.M, 3))
        _check(self.ctx.handle, self._lib.gingr_bcpd_get_coefficients(self._h, dptr(c)), "gingr_bcpd_get_coefficients")
        return c

    # -- the reference surface ------------------------------------------------------------------------------------
    def Iteration(self) -> Tuple[np.ndarray, float]:
        _check(self.ctx.handle, self._lib.gingr_bcpd_iterate(self._h, 1), "gingr_bcpd_iterate")
        return self.points(), self.sigma2()

    def Registration(self, max_iteration: int, tolerance: float = 1e-6, verbose: bool = False) -> np.ndarray:
        """the reference's loop: from the start, iterate until |sigma2' - sigma2| < tolerance or max_iteration non-converged iterations;
        returns the state left on the device (yhat)"""
        self.reset()
        i, converged, current = 0, False, self._sigma2_init
        while i < max_iteration and not converged:
            if verbose:
                print(f"BCPD, iteration: {i}, variance: {current}")
            _check(self.ctx.handle, self._lib.gingr_bcpd_iterate(self._h, 1), "gingr_bcpd_iterate")
            new = self.sigma2()
            if abs(new - current) < tolerance:
                if verbose:
                    print("Converged")
                converged = True
            else:
                i += 1
            current = new
        self.iterations, self.converged = i, converged
        return self.points()


class BCPDRegistration:
    """BCPDRegistration.scala with its defaults: register(target) returns the warped template points; register(target, points) the
    pair (warped template, transformPoints(points)) of the task -- here the two correspond: y^ = s R (y + v^) + t starts from the template
    in every iteration, so the last iteration's map is the whole registration (unlike the classic wrappers, whose second value is the
    last step alone)."""

    def __init__(self, ctx: Context, template, w: float = 0.0, lambda_: float = 2.0, gamma: float = 1.0, k: float = 1.0, beta: float = 2.0,
                 max_iterations: int = 100, lowRank: Optional[LowRankG] = None):
        self.ctx, self.template, self.max_iterations, self.lowRank = ctx, f64(template), max_iterations, lowRank
        self.w, self.lambda_, self.gamma, self.k, self.beta = w, lambda_, gamma, k, beta

    def register(self, target, points=None):
        task = BCPD(self.ctx, self.template, target, self.w, self.lambda_, self.gamma, self.k, self.beta, self.lowRank)
        try:
            warped = task.Registration(self.max_iterations)
            return warped if points is None else (warped, task.transformPoints(points))
        finally:
            task.close()


# ------------------------------------------------------------------------------------------------ classic rigid ICP
RIGID_REGISTRATOR, AFFINE_REGISTRATOR = 0, 1   # PoseRegistrator.RigidRegistrator3D / AffineRegistrator3D (= similarity)


class RigidICP:
    """G/other/algorithms/icp/RigidICP.scala:24-84 over csrc/rigid_icp.hip: closest points, Umeyama and the transform of the
    template run on the GPU; this class keeps `Registration`'s loop and convergence test."""

    def __init__(self, factory: "ICPFactory", targetPoints):
        self.icp = factory
        self.target = f64(targetPoints)
        self._lib = factory.ctx._lib
        h = c_void_p()
        _check(factory.ctx.handle, self._lib.gingr_rigid_icp_create(factory.ctx.handle, int(factory.registrator), factory.M,
                                                                    dptr(factory.template), self.target.shape[0], dptr(self.target),
                                                                    ctypes.byref(h)), "gingr_rigid_icp_create")
        self._h = h

    def close(self):
        if self._h:
            self._lib.gingr_rigid_icp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def points(self) -> np.ndarray:
        p = np.empty((self.icp.M, 3))
        _check(self.icp.ctx.handle, self._lib.gingr_rigid_icp_get(self._h, dptr(p), None), "gingr_rigid_icp_get")
        return p

    def transform(self) -> Tuple[float, np.ndarray, np.ndarray]:
        """(s, R, t) of the last iteration: p -> s R p + t"""
        t = np.empty(13)
        _check(self.icp.ctx.handle, self._lib.gingr_rigid_icp_get(self._h, None, dptr(t)), "gingr_rigid_icp_get")
        return float(t[0]), t[1:10].reshape(3, 3).copy(), t[10:13].copy()

    def Iteration(self, template=None) -> Tuple[np.ndarray, float]:
        """(registered points, mean closest-point distance BEFORE the move)  (:75-82)"""
        if template is not None:
            tp = f64(template)
            _check(self.icp.ctx.handle, self._lib.gingr_rigid_icp_set(self._h, dptr(tp)), "gingr_rigid_icp_set")
        d = np.empty(1)
        _check(self.icp.ctx.handle, self._lib.gingr_rigid_icp_iterate(self._h, 1, dptr(d)), "gingr_rigid_icp_iterate")
        return self.points(), float(d[0])

    def Registration(self, max_iteration: int, tolerance: float = 0.001, verbose: bool = False) -> np.ndarray:
        """:30-55: stop when the mean distance changes by less than `tolerance` between two iterations (first comparison against
        0.0); the converged iteration's points are the result."""
        _check(self.icp.ctx.handle, self._lib.gingr_rigid_icp_set(self._h, dptr(self.icp.template)), "gingr_rigid_icp_set")
        last = 0.0
        i, converged = 0, False
        self.iterations = 0
        d = np.empty(1)
        while i < max_iteration and not converged:
            _check(self.icp.ctx.handle, self._lib.gingr_rigid_icp_iterate(self._h, 1, dptr(d)), "gingr_rigid_icp_iterate")
            if verbose:
                print(f"ICP, iteration: {i}, distance: {d[0]}")
            if abs(d[0] - last) < tolerance:
                if verbose:
                    print("Converged")
                converged = True
            last = float(d[0])
            i += 1
        self.iterations, self.converged, self.distance = i, converged, last
        return self.points()


class ICPFactory:
    """G/other/algorithms/icp/ICPFactory.scala:28-38 (`registrator`: RIGID_REGISTRATOR or AFFINE_REGISTRATOR, the implicit
    Registrator of the reference)."""

    def __init__(self, ctx: Context, templatePoints, registrator: int = RIGID_REGISTRATOR):
        self.ctx, self.template, self.registrator = ctx, f64(templatePoints), registrator
        self.M = self.template.shape[0]

    def registerRigidly(self, targetPoints) -> RigidICP:
        return RigidICP(self, targetPoints)


class RigidICPRegistration:
    """G/other/algorithms/RigidICPRegistration.scala:24-46.  As in the reference the warp field pairs the TARGET's points with the
    registered template points by index (`target.points zip registration.points`, :40-43), i.e. the result is the registered
    template carried on the target's topology -- both point sets must have the same size for that to mean anything."""

    def __init__(self, ctx: Context, template, max_iterations: int = 100, registrator: int = RIGID_REGISTRATOR):
        self.icp, self.max_iterations = ICPFactory(ctx, template, registrator), max_iterations

    def register(self, target) -> np.ndarray:
        task = self.icp.registerRigidly(target)
        try:
            reg = task.Registration(self.max_iterations)
        finally:
            task.close()
        tgt = f64(target)
        n = min(tgt.shape[0], reg.shape[0])
        return tgt[:n] + (reg[:n] - tgt[:n])


# ------------------------------------------------------------------------------------------------ global rigid pre-alignment
class GlobalRigidAlignment:
    """From an arbitrary pose to the start the local methods need (no reference counterpart: its demos ship pre-aligned data).
    register(target): Context.rigid_search over `starts` spiral rotations (or an (S, 3, 3) array), `iterations` iterations, the `overlap`
    fraction of closest pairs kept -- on every stride-th template point when the template has more than maxPoints points, stride =
    ceil(M / maxPoints) -- then the best pose refined on ALL points by the RigidICP task (its convergence test, at most
    refineIterations iterations), started from the transformed template; the two transforms are composed.  With overlap < 1 the
    task, which does not trim, gets the ceil(overlap M) template points closest to the target at the search's pose (ties included;
    .refineInliers, else None) and the composed transform is applied to all points.  Returns the aligned
    template points; .transform = (R, t) with aligned = template R^T + t, .searchResult = the search's record.
    Trimming from a centroid start does not recover PARTIAL targets reliably (README): use FeatureRigidAlignment below there."""

    def __init__(self, ctx: Context, template, starts=64, iterations: int = 10, overlap: float = 1.0, maxPoints: int = 2000,
                 refineIterations: int = 50, tolerance: float = 0.001):
        if int(maxPoints) < 1:
            raise ValueError("maxPoints >= 1 required")
        if int(refineIterations) < 0:
            raise ValueError("refineIterations >= 0 required")
        self.ctx, self.template = ctx, f64(template).reshape(-1, 3)
        self.starts, self.iterations, self.overlap = starts, int(iterations), float(overlap)
        self.maxPoints, self.refineIterations, self.tolerance = int(maxPoints), int(refineIterations), float(tolerance)
        self.transform: Optional[Tuple[np.ndarray, np.ndarray]] = None
        self.searchResult = None
        self.refineIterationsDone = 0
        self.refineInliers = None

    def searchPoints(self) -> np.ndarray:
        """the template points the search runs on: every stride-th one, stride = ceil(M / maxPoints)"""
        M = self.template.shape[0]
        stride = -(-M // self.maxPoints) if M > self.maxPoints else 1
        return np.ascontiguousarray(self.template[::stride])

    def register(self, target) -> np.ndarray:
        tgt = f64(target).reshape(-1, 3)
        res = self.ctx.rigid_search(self.searchPoints(), tgt, self.starts, self.iterations, self.overlap)
        self.searchResult = res
        R, t = res.R.copy(), res.t.copy()
        points = self.template @ R.T + t
        self.refineIterationsDone = 0
        M = points.shape[0]
        keep = min(M, max(1, int(np.ceil(self.overlap * M))))
        inliers = None
        if keep < M:
            # RigidICP does not trim, and the points the search trimmed away (clutter) would pull it off again (8 degrees with 15 %
            # clutter on the femur): it runs on the template points the trimming keeps at the search's pose, ties included
            d2 = self.ctx.nn(points, tgt)[1]
            inliers = d2 <= np.partition(d2, keep - 1)[keep - 1]
        self.refineInliers = inliers
        if self.refineIterations > 0:
            task = ICPFactory(self.ctx, points if inliers is None else points[inliers]).registerRigidly(tgt)
            lib, h = self.ctx._lib, self.ctx.handle
            try:
                last, d = 0.0, np.empty(1)
                for _ in range(self.refineIterations):              # RigidICP.Registration's loop, with the steps composed
                    _check(h, lib.gingr_rigid_icp_iterate(task._h, 1, dptr(d)), "gingr_rigid_icp_iterate")
                    _, Rk, tk = task.transform()
                    R, t = Rk @ R, Rk @ t + tk
                    self.refineIterationsDone += 1
                    if abs(d[0] - last) < self.tolerance:
                        break
                    last = float(d[0])
                points = task.points() if inliers is None else self.template @ R.T + t
            finally:
                task.close()
        self.transform = (R, t)
        return points


# ------------------------------------------------------------------------------------------------ feature-based global alignment
class FeatureRigidAlignment:
    """From an arbitrary pose when the target is only a PART of the template (or the other way round): correspondences from local shape
    descriptors instead of starts about the centroids (no reference counterpart).  register(target, targetNormals=None):
      1. the template on every stride-th point as GlobalRigidAlignment.searchPoints (stride = ceil(M / maxPoints));
      2. normals where not given: Context.cloud_normals(points, normalsK, viewpoint = the cloud's own centroid) -- the orientation turns
         with the cloud, which is all the descriptor needs; both clouds by the same rule;
      3. Context.cloud_fpfh (descriptorK neighbours within `radius`) on both clouds, Context.feature_match both ways; the pool is the
         template points whose match is mutual, all of them when fewer than 10 are;
      4. `hypotheses` triples from numpy.random.default_rng(seed), one rng.choice(pool, 3, replace=False) each: the library draws nothing;
      5. a triple is kept when the smallest ratio, shorter over longer, of its three corresponding edge lengths is >= edgeSimilarity;
      6. Context.rigid_poses_from_triples, then ONE Context.rigid_search_poses over all kept triples with no iteration: the pose with
         the most template points within inlierDistance of the target wins (then the smaller score, then the lowest index);
      7. that pose refined by rigid_search_poses alone: refineIterations iterations of trimmed ICP at the given overlap.
    The non-trimming RigidICP task is not run afterwards.  Returns the aligned template points; .transform = (R, t) with aligned =
    template R^T + t, .searchResult = the record of step 6, .refineResult that of step 7, .info = dict(matches, mutual, drawn, kept,
    degenerate, inliers), .triples / .matches = the kept triples and the template -> target match.
    inlierDistance=None takes half the median distance of a target point to its nearest other target point (Context.cloud_knn); that
    default is UNMEASURED: every recorded run of this route gave the distance explicitly (3.0 on the femur, spacing 4.6)."""

    def __init__(self, ctx: Context, template, radius: float, normalsK: int = 12, descriptorK: int = 64, hypotheses: int = 2000,
                 edgeSimilarity: float = 0.8, inlierDistance: Optional[float] = None, overlap: float = 0.6, refineIterations: int = 30,
                 maxPoints: int = 2000, seed: int = 0, templateNormals=None):
        if int(maxPoints) < 1 or int(hypotheses) < 1 or int(refineIterations) < 0:
            raise ValueError("maxPoints >= 1, hypotheses >= 1 and refineIterations >= 0 required")
        if not float(radius) > 0.0:
            raise ValueError("radius > 0 required")
        self.ctx, self.template, self.radius = ctx, f64(template).reshape(-1, 3), float(radius)
        self.normalsK, self.descriptorK, self.hypotheses = int(normalsK), int(descriptorK), int(hypotheses)
        self.edgeSimilarity, self.inlierDistance, self.overlap = float(edgeSimilarity), inlierDistance, float(overlap)
        self.refineIterations, self.maxPoints, self.seed = int(refineIterations), int(maxPoints), int(seed)
        self.templateNormals = None if templateNormals is None else f64(templateNormals).reshape(-1, 3)
        if self.templateNormals is not None and self.templateNormals.shape != self.template.shape:
            raise ValueError("one normal per template point required")
        self.transform: Optional[Tuple[np.ndarray, np.ndarray]] = None
        self.searchResult = self.refineResult = self.triples = self.matches = None
        self.info: dict = {}

    def _stride(self) -> int:
        M = self.template.shape[0]
        return -(-M // self.maxPoints) if M > self.maxPoints else 1

    def searchPoints(self) -> np.ndarray:
        """the template points the descriptors and the search run on: every stride-th one, stride = ceil(M / maxPoints)"""
        return np.ascontiguousarray(self.template[::self._stride()])

    def _descriptors(self, points, normals):
        if normals is None:
            normals = self.ctx.cloud_normals(points, min(self.normalsK, points.shape[0]), viewpoint=points.mean(0))[0]
        return self.ctx.cloud_fpfh(points, normals, min(self.descriptorK, points.shape[0]), self.radius)[0]

    def register(self, target, targetNormals=None) -> np.ndarray:
        ctx = self.ctx
        x, y = self.searchPoints(), f64(target).reshape(-1, 3)
        nx = None if self.templateNormals is None else np.ascontiguousarray(self.templateNormals[::self._stride()])
        ny = None if targetNormals is None else f64(targetNormals).reshape(-1, 3)
        fx, fy = self._descriptors(x, nx), self._descriptors(y, ny)
        match, back = ctx.feature_match(fx, fy)[0].astype(np.int64), ctx.feature_match(fy, fx)[0].astype(np.int64)
        mutual = np.nonzero(back[match] == np.arange(match.shape[0]))[0]
        pool = mutual if mutual.size >= 10 else np.arange(match.shape[0])
        if pool.size < 3:
            raise ValueError("fewer than three template points to draw a triple from")
        rng = np.random.default_rng(self.seed)
        tri = np.stack([rng.choice(pool, 3, replace=False) for _ in range(self.hypotheses)]).astype(np.int64)
        a, b = x[tri], y[match[tri]]
        keep = np.ones(tri.shape[0], dtype=bool)
        for p, q in ((0, 1), (0, 2), (1, 2)):
            la, lb = np.linalg.norm(a[:, p] - a[:, q], axis=1), np.linalg.norm(b[:, p] - b[:, q], axis=1)
            hi = np.maximum(la, lb)
            keep &= np.where(hi > 0, np.minimum(la, lb) / np.where(hi > 0, hi, 1.0), 0.0) >= self.edgeSimilarity
        tri = tri[keep]
        self.matches, self.triples = match, tri
        self.info = dict(matches=int(match.shape[0]), mutual=int(mutual.size), drawn=self.hypotheses, kept=int(tri.shape[0]), degenerate=0,
                         inliers=0)
        if tri.shape[0] == 0:
            raise ValueError("no triple passed the edge test: lower edgeSimilarity or raise hypotheses")
        distance = self.inlierDistance
        if distance is None:
            distance = 0.5 * float(np.median(np.sqrt(ctx.cloud_knn(y, 3)[1][:, 1])))
        poses, degenerate = ctx.rigid_poses_from_triples(x, y, tri, match[tri])
        self.info["degenerate"] = int(degenerate.sum())
        scored = ctx.rigid_search_poses(x, y, poses, 0, 1.0, distance, 1)
        self.searchResult = scored
        self.info["inliers"] = int(scored.inliers[scored.best])
        start = np.concatenate([scored.R.reshape(9), scored.t])[None]
        refined = ctx.rigid_search_poses(x, y, start, self.refineIterations, self.overlap, distance, 1)
        self.refineResult = refined
        self.transform = (refined.R.copy(), refined.t.copy())
        return self.template @ refined.R.T + refined.t


# ------------------------------------------------------------------------------------------------ optimal-step non-rigid ICP
NICP_DEFAULT_ALPHA = [1e1] * 11   # NonRigidOptimalStepICP.scala:63-65: the scanLeft / reverse chain ends in `.map(_ => 1e1)`


def nicp_edges(cells) -> np.ndarray:
    """trianglesToEdges (:67-76): the unique sorted vertex pairs of the triangles, (E, 2) int32 with p1 < p2 (the reference keeps
    them in a Set's iteration order; the order of the rows of M does not change the least-squares solution)."""
    t = np.sort(np.asarray(cells, dtype=np.int64).reshape(-1, 3), axis=1)
    e = np.concatenate([t[:, [0, 1]], t[:, [0, 2]], t[:, [1, 2]]])
    return np.ascontiguousarray(np.unique(e, axis=0), dtype=np.int32)


class NonRigidOptimalStepICP:
    """G/other/algorithms/icp/NonRigidOptimalStepICP.scala:31-284 (Amberg et al., "Optimal Step Nonrigid ICP Algorithms for Surface
    Registration"): `kind` "T" = N-ICP-T (one displacement per vertex), "A" = N-ICP-A (one affine 4 x 3 map per vertex).
    Both halves of an iteration run on the GPU: the correspondence (closest target surface point + the three rejection tests of
    ClosestPointTriangleMesh3D: the surface-ICP query of the GiNGR path, asked for the current template through
    gingr_fitter_set_fit_points) and the least-squares step.  `solver`: "dense" (gingr_nicp_solve: the normal equations as a dense
    matrix, blocked MFMA Cholesky; templates of a few thousand vertices) or "sparse" (gingr_nicp_step: the same equations matrix-free,
    block-Jacobi preconditioned conjugate gradients over the edge graph; no size limit but the card's memory for a dozen vectors).
    relTol / maxSolverIterations: the sparse solver's stop (None: 1e-12, 20 000); `solveInfo` holds its last info block.
    Landmarks: two mappings id -> point; the common ids are used (:45-55)."""

    def __init__(self, ctx: Context, templateMesh, targetMesh, templateLandmarks=None, targetLandmarks=None, gamma: float = 1.0,
                 kind: str = "T", solver: str = "dense", relTol: Optional[float] = None, maxSolverIterations: Optional[int] = None):
        from . import api as ga
        if gamma < 0:
            raise ValueError("gamma >= 0 required")
        if kind not in ("T", "A"):
            raise ValueError("kind is 'T' or 'A'")
        if solver not in ("dense", "sparse"):
            raise ValueError("solver is 'dense' or 'sparse'")
        if relTol is not None and not 0.0 < relTol <= 1.0:
            raise ValueError("0 < relTol <= 1 required")
        if maxSolverIterations is not None and maxSolverIterations < 1:
            raise ValueError("maxSolverIterations >= 1 required")
        self.ctx, self.kind, self.gamma = ctx, kind, float(gamma)
        self.solver, self.relTol, self.maxSolverIterations = solver, relTol, maxSolverIterations
        self.solveInfo = None
        self._nicp = None
        self.template = f64(templateMesh[0])
        self.cells = np.ascontiguousarray(templateMesh[1], dtype=np.int32).reshape(-1, 3)
        self.target = f64(targetMesh[0])
        self.targetCells = np.ascontiguousarray(targetMesh[1], dtype=np.int32).reshape(-1, 3)
        self.n = self.template.shape[0]
        self.edges = nicp_edges(self.cells)
        tl, gl = dict(templateLandmarks or {}), dict(targetLandmarks or {})
        common = [k for k in tl if k in gl]
        if common:
            tp = f64(np.array([tl[k] for k in common]))
            gp = f64(np.array([gl[k] for k in common]))
            self.lmIdsOnTemplate = ctx.nn(tp, self.template)[0].astype(np.int32)       # closest template VERTEX of each landmark
            self.UL = self.target[ctx.nn(gp, self.target)[0]].copy()                    # closest target VERTEX (not the landmark)
        else:
            self.lmIdsOnTemplate, self.UL = np.zeros(0, dtype=np.int32), np.zeros((0, 3))
        # carrier of the correspondence query: a fitter over the template's topology (the basis is never used)
        M = self.n
        self._model = ga.PointDistributionModel(self.template, np.zeros((M, 3)), np.zeros((3 * M, 1)), np.ones(1), cells=self.cells)
        self._algo = ga.IcpRegistration(ctx)
        cfg = ga.IcpConfiguration(maxIterations=1, initialSigma=1.0, endSigma=1.0, correspondenceMethod="TriangularClosestPoint")
        self._state = self._algo.createInitialState(self._model, self.target, cfg, transform=ga.GlobalTranformationType.NoTransforms,
                                                    targetCells=self.targetCells)
        self._lib = ctx._lib
        if solver == "sparse":
            from ._native import iptr
            h = c_void_p()
            L = self.lmIdsOnTemplate.shape[0]
            _check(ctx.handle, self._lib.gingr_nicp_create(ctx.handle, 0 if kind == "T" else 1, self.n, self.edges.shape[0], iptr(self.edges), L,
                                                           iptr(self.lmIdsOnTemplate) if L else None, ctypes.byref(h)), "gingr_nicp_create")
            self._nicp = h

    def close(self):
        if getattr(self, "_nicp", None):
            self._lib.gingr_nicp_destroy(self._nicp)
            self._nicp = None
        if getattr(self, "_algo", None) is not None:
            self._algo.close()
            self._algo = None

    def __del__(self):
        try:
            if getattr(self, "_nicp", None):
                self._lib.gingr_nicp_destroy(self._nicp)
                self._nicp = None
        except Exception:
            pass

    def solution(self) -> np.ndarray:
        """the unknowns X of the last sparse step: (n, 3) displacements (T) or (4 n, 3), row 4 i + a of vertex i (A)"""
        if self._nicp is None:
            raise ValueError("solver='sparse' required")
        x = np.empty(((1 if self.kind == "T" else 4) * self.n, 3))
        _check(self.ctx.handle, self._lib.gingr_nicp_get_solution(self._nicp, dptr(x)), "gingr_nicp_get_solution")
        return x

    def getClosestPoints(self, template) -> Tuple[np.ndarray, np.ndarray, float]:
        """(:118-128) (closest target surface points, weights in {0, 1}, mean distance) of the given template points."""
        from . import _native as nat
        a, st = self._algo, self._state
        g, c = st.general, st.config
        pts = f64(template)
        a._bind(g, c.useLandmarkCorrespondence)
        a._push_state(g)
        a._device_state = None
        a._select_direction(c)
        a._select_surface_method(c)
        _check(self.ctx.handle, self._lib.gingr_fitter_set_fit_points(a._fitter, dptr(pts)), "gingr_fitter_set_fit_points")
        p = nat.IcpParams(c.initialSigma, c.endSigma, c.maxIterations)
        _check(self.ctx.handle, self._lib.gingr_fitter_icp_surface_phase_async(a._fitter, ctypes.byref(p), 0),
               "gingr_fitter_icp_surface_phase_async")
        cp, w = np.empty((self.n, 3)), np.empty(self.n)
        _check(self.ctx.handle, self._lib.gingr_fitter_get_surface_correspondence(a._fitter, dptr(cp), dptr(w)),
               "gingr_fitter_get_surface_correspondence")
        dd = cp - pts
        dist = float(np.sqrt((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]).sum() / self.n)
        return cp, w, dist

    def Iteration(self, template, alpha: float, beta: float):
        """(:151-190 / :241-283) -> (moved template points, mean distance BEFORE the move, moved landmark vertices)"""
        if alpha < 0 or beta < 0:
            raise ValueError("alpha, beta >= 0 required")
        from ._native import iptr
        pts = f64(template)
        cp, w, dist = self.getClosestPoints(pts)
        out, lm = np.empty((self.n, 3)), np.empty((self.lmIdsOnTemplate.shape[0], 3))
        if self.solver == "sparse":
            from ._native import NicpInfo
            info = NicpInfo()
            rc = self._lib.gingr_nicp_step(self._nicp, dptr(pts), dptr(w), dptr(cp), dptr(self.UL) if len(self.UL) else None, float(alpha),
                                           float(beta), self.gamma, float(self.relTol or 0.0), int(self.maxSolverIterations or 0), dptr(out),
                                           dptr(lm) if len(lm) else None, ctypes.byref(info))
            self.solveInfo = {"iterations": int(info.iterations), "converged": bool(info.converged),
                              "residual": np.array(info.residual[:]), "rhs_norm": np.array(info.rhs_norm[:])}
            _check(self.ctx.handle, rc, "gingr_nicp_step")
            return out, dist, lm
        _check(self.ctx.handle, self._lib.gingr_nicp_solve(
            self.ctx.handle, 0 if self.kind == "T" else 1, self.n, dptr(pts), self.edges.shape[0], iptr(self.edges), dptr(w), dptr(cp),
            self.lmIdsOnTemplate.shape[0], iptr(self.lmIdsOnTemplate) if len(self.lmIdsOnTemplate) else None,
            dptr(self.UL) if len(self.UL) else None, float(alpha), float(beta), self.gamma, dptr(out), dptr(lm) if len(lm) else None),
            "gingr_nicp_solve")
        return out, dist, lm

    def Registration(self, max_iteration: int, tolerance: float = 0.001, alpha=None, beta=None, verbose: bool = False) -> np.ndarray:
        """(:89-121): one stage per (alpha, beta) pair, each up to max_iteration steps or until the mean distance measured before
        a step is below the tolerance."""
        alpha = NICP_DEFAULT_ALPHA if alpha is None else list(alpha)
        beta = alpha if beta is None else list(beta)
        if len(alpha) != len(beta):
            raise ValueError("alpha and beta need the same length")
        fit = self.template
        self.iterations = 0
        for j, (a, b) in enumerate(zip(alpha, beta)):
            dist, i = float("inf"), 0
            while i < max_iteration and dist >= tolerance:
                fit, dist, _ = self.Iteration(fit, a, b)
                if verbose:
                    print(f"ICP, iteration: {j * max_iteration + i}/{max_iteration * len(alpha)}, alpha: {a}, beta: {b}, "
                          f"average distance to target: {dist}")
                i += 1
                self.iterations += 1
        return fit


def NonRigidOptimalStepICP_T(ctx, templateMesh, targetMesh, templateLandmarks=None, targetLandmarks=None, gamma: float = 1.0,
                             solver: str = "dense", relTol: Optional[float] = None, maxSolverIterations: Optional[int] = None):
    return NonRigidOptimalStepICP(ctx, templateMesh, targetMesh, templateLandmarks, targetLandmarks, gamma, "T", solver, relTol,
                                  maxSolverIterations)


def NonRigidOptimalStepICP_A(ctx, templateMesh, targetMesh, templateLandmarks=None, targetLandmarks=None, gamma: float = 1.0,
                             solver: str = "dense", relTol: Optional[float] = None, maxSolverIterations: Optional[int] = None):
    return NonRigidOptimalStepICP(ctx, templateMesh, targetMesh, templateLandmarks, targetLandmarks, gamma, "A", solver, relTol,
                                  maxSolverIterations)
