"""The bits of the fitter behind every correspondence flavour and every operation of the C ABI, against
tests/golden/fitter_flavour_bits.npz -- recorded (twice, with equal bits in every output) from a build of the commit before the
flavour became one descriptor (gingr_amd/csrc/correspondence.h).  That change touches host code only: for any sequence of ABI calls
the kernels launched, their order and their arguments stay the same, so every output keeps every bit.

Inputs: femur_case(24) of tests/test_gpu_template_pairs.py (600 template vertices, 800 target vertices) with the femur triangles
that survive the same sub-sampling, three landmarks where a configuration asks for them, and femur_case(136) for one wide CPD case.
The sizes reach every host branch; the work under test is dispatch, not kernels.

Per configuration (CONFIGS): alpha, scalars and fit after two deterministic updates; the same after one sampled update with fixed z;
the transition density of a fixed mesh; the posterior covariance map; mean and variances of the posterior model; for flavours 0..2
in the forward direction the result struct, alpha and fit of one gingr_fitter_mh_step.  Then, for flavours 0..2, an update, a
sampled update and the transition density through a one-device gingr_group.

The golden keeps the float64 fit of the deterministic updates; the fits of the sampled update, of the Metropolis-Hastings step and of
the group (functions of the alpha and scalars recorded next to them) are kept as SHA-256 digests of their bytes."""
import ctypes
import functools
import hashlib
import os

import numpy as np
import pytest

from tests.test_gpu_posterior_covariance import ga_model, three_landmarks
from tests.test_gpu_surface_icp import femur
from tests.test_gpu_template_pairs import EULER, TRANSLATION, femur_case, pair_lists

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fitter_flavour_bits.npz")
CPD, ICP, SURFACE, PAIRS = 0, 1, 2, 3
CPD_PARAMS, ICP_PARAMS = (0.1, 1.0), (4.0, 1.0, 10)
SIGMA2 = 4.0
OPT_GRAM_DOWNDATE = 5

# name -> (flavour, rank, landmarks, reversed, surface method, GINGR_OPT_GRAM_DOWNDATE or None, pairs: None / "iso" / "cov")
CONFIGS = {
    "cpd": (CPD, 24, True, False, 0, None, None),
    "cpd_wide": (CPD, 136, False, False, 0, None, None),
    "icp": (ICP, 24, False, False, 0, None, None),                 # uniform weights: scaled moment, eigen solve
    "icp_landmarks": (ICP, 24, True, False, 0, None, None),
    "icp_reversed": (ICP, 24, False, True, 0, None, None),
    "surface_triangular": (SURFACE, 24, True, False, 0, None, None),
    "surface_along_normal": (SURFACE, 24, False, False, 1, None, None),
    "surface_downdate": (SURFACE, 24, False, False, 0, 1, None),   # both Gram cases at this size
    "surface_no_downdate": (SURFACE, 24, False, False, 0, 0, None),
    "pairs_isotropic": (PAIRS, 24, True, False, 0, None, "iso"),
    "pairs_covariance": (PAIRS, 24, False, False, 0, None, "cov"),
}
# what each operation is called per flavour (include/gingr_hip.h)
SUFFIX = {CPD: "cpd", ICP: "icp", SURFACE: "icp_surface", PAIRS: "pairs"}


@functools.lru_cache(maxsize=None)
def sub_triangles():
    """the femur triangles whose three vertices survive femur_case's sub-sampling (every second vertex, the first 600 of the
    template and 800 of the target), in the new vertex numbers"""
    _, cells, _, tcells = femur()

    def sub(c, n):
        keep = (c % 2 == 0).all(1) & (c < 2 * n).all(1)
        return np.ascontiguousarray(c[keep] // 2, dtype=np.int32)
    return sub(cells, 600), sub(tcells, 800)


@functools.lru_cache(maxsize=None)
def fixed_inputs(rank):
    """(alpha of the start state, z of the sampled update, z of the Metropolis-Hastings step, the mesh of the transition density)"""
    from oracle import gingr_oracle as go
    mo, _ = femur_case(rank)
    rng = np.random.default_rng(1000 + rank)
    alpha, z, z_mh = rng.normal(0, 0.3, mo.rank), rng.standard_normal(mo.rank), rng.standard_normal(mo.rank)
    mesh = mo.instance(rng.normal(0, 0.4, mo.rank)) @ go.euler_to_rot(*EULER).T + np.array(TRANSLATION)
    return alpha, z, z_mh, np.ascontiguousarray(mesh)


def scalars_array(s):
    return np.array(list(s.euler) + list(s.center) + list(s.translation) + [s.scale, s.sigma2, s.iteration, s.status], dtype=np.float64)


def params_of(flavour):
    from gingr_amd import _native as nat
    cp = nat.CpdParams(*CPD_PARAMS) if flavour == CPD else None
    ip = nat.IcpParams(*ICP_PARAMS) if flavour in (ICP, SURFACE) else None
    return cp, ip


class Fitter:
    """one single-shard fitter behind the C ABI, set up for one configuration"""

    def __init__(self, ctx, name):
        from gingr_amd._native import dptr, iptr
        from gingr_amd.sharded import ShardedFitter
        self.flavour, rank, landmarks, rev, method, downdate, pairs = CONFIGS[name]
        self.ctx, self.lib = ctx, ctx._lib
        self.mo, self.target = femur_case(rank)
        self.restore_option = None
        if downdate is not None:
            old = ctypes.c_int32()
            self.ok(self.lib.gingr_ctx_get_option(ctx.handle, OPT_GRAM_DOWNDATE, ctypes.byref(old)), "ctx_get_option")
            self.restore_option = old.value
            self.ok(self.lib.gingr_ctx_set_option(ctx.handle, OPT_GRAM_DOWNDATE, downdate), "ctx_set_option")
        self.sf = ShardedFitter(ctx, ga_model(self.mo), self.target)
        self.h = self.sf.handle
        if self.flavour != PAIRS:
            self.sf.set_meshes(*sub_triangles(), method=method)
            self.sf.set_correspondence_direction(rev)
        if landmarks:
            lm = three_landmarks(self.mo, self.target)
            lp, lx, lc = np.ascontiguousarray(lm.pids, dtype=np.int32), np.ascontiguousarray(lm.points), np.ascontiguousarray(lm.covs)
            self.ok(self.lib.gingr_fitter_set_landmarks(self.h, 3, iptr(lp), dptr(lx), dptr(lc)), "set_landmarks")
        if pairs is not None:
            pids, pts, var = pair_lists(rank)
            p = np.ascontiguousarray(pids, dtype=np.int32)
            self.ok(self.lib.gingr_fitter_set_pairs(self.h, p.shape[0], iptr(p), dptr(pts), dptr(var)), "set_pairs")
            if pairs == "cov":
                rng = np.random.default_rng(9)
                k = 5
                A = rng.normal(0, 1, (k, 3, 3))
                covs = np.ascontiguousarray(A @ A.transpose(0, 2, 1) + np.diag([0.2, 1.0, 3.0])[None])
                cp, cx = np.ascontiguousarray(p[:k]), np.ascontiguousarray(pts[:k] + 0.5)
                self.ok(self.lib.gingr_fitter_set_pairs_cov(self.h, k, iptr(cp), dptr(cx), dptr(covs)), "set_pairs_cov")
        self.cp, self.ip = params_of(self.flavour)
        self.p = [ctypes.byref(x) for x in (self.cp, self.ip) if x is not None]   # the parameter argument of this flavour, if any
        self.alpha0, self.z, self.z_mh, self.mesh = fixed_inputs(rank)
        self.can_mh = self.flavour != PAIRS and not rev

    def ok(self, rc, what):
        from gingr_amd.api import _check
        _check(self.ctx.handle, rc, what)

    def fn(self, pattern):
        return getattr(self.lib, pattern.format(SUFFIX[self.flavour]))

    def start(self):
        self.sf.set_state(self.alpha0, SIGMA2, euler=EULER, translation=TRANSLATION)

    def state(self, prefix, out):
        alpha, s, fit = self.sf.get_state()
        out[prefix + "_alpha"], out[prefix + "_scalars"], out[prefix + "_fit"] = alpha, scalars_array(s), fit

    def results(self):
        from gingr_amd import _native as nat
        from gingr_amd._native import dptr
        out = {}
        M, r = self.mo.M, self.mo.rank
        self.start()
        self.ok(self.fn("gingr_fitter_update_{}_async")(self.h, *self.p, 2), "update")
        self.state("update", out)
        self.start()
        self.ok(self.fn("gingr_fitter_update_{}_sample_async")(self.h, *self.p, dptr(self.z)), "update_sample")
        self.state("sample", out)
        self.start()
        lp = ctypes.c_double()
        self.ok(self.fn("gingr_fitter_posterior_logpdf_{}")(self.h, *self.p, dptr(self.mesh), ctypes.byref(lp)), "posterior_logpdf")
        out["logpdf"] = np.array([lp.value])
        cov = np.empty((M, 6))
        self.ok(self.fn("gingr_fitter_posterior_covariance_{}")(self.h, *self.p, dptr(cov)), "posterior_covariance")
        out["covariance"] = cov
        pm = ctypes.c_void_p()
        self.ok(self.fn("gingr_fitter_posterior_model_{}")(self.h, *self.p, ctypes.byref(pm)), "posterior_model")
        try:
            rank = self.lib.gingr_model_rank(pm)
            mean, var = np.empty((M, 3)), np.empty(rank)
            self.ok(self.lib.gingr_model_download(self.ctx.handle, pm, None, dptr(mean), None, dptr(var)), "model_download")
            out["posterior_mean"], out["posterior_variance"] = mean, var
        finally:
            self.lib.gingr_model_destroy(pm)
        if self.can_mh:
            self.start()
            req, res = nat.MhRequest(), nat.MhResult()
            req.flavour, req.kind = self.flavour, 0
            req.cpd = ctypes.pointer(self.cp) if self.cp is not None else None
            req.icp = ctypes.pointer(self.ip) if self.ip is not None else None
            req.z = dptr(self.z_mh)
            req.eval_sdev, req.eval_points, req.need_forward = 1.5, 0, 1
            alpha, fit = np.empty(r), np.empty((M, 3))
            self.ok(self.lib.gingr_fitter_mh_step(self.h, ctypes.byref(req), dptr(alpha), dptr(fit), ctypes.byref(res)), "mh_step")
            out["mh_alpha"], out["mh_fit"], out["mh_scalars"] = alpha, fit, scalars_array(res.scalars)
            out["mh_result"] = np.array([res.log_value, res.dist_sum, res.dist_max, res.count, res.log_q_forward, res.log_q_backward,
                                         res.forward_status, res.backward_status], dtype=np.float64)
        return out

    def close(self):
        self.sf.close()
        if self.restore_option is not None:
            self.lib.gingr_ctx_set_option(self.ctx.handle, OPT_GRAM_DOWNDATE, self.restore_option)


def config_results(ctx, name):
    f = Fitter(ctx, name)
    try:
        return {name + "." + k: v for k, v in f.results().items()}
    finally:
        f.close()


def group_results():
    """a one-device gingr_group: it hands every call to its only fitter"""
    from gingr_amd.group import DeviceGroup
    mo, target = femur_case(24)
    alpha0, z, _, mesh = fixed_inputs(24)
    out = {}
    g = DeviceGroup([0])
    try:
        g.upload_model(mo.ref, mo.mean, mo.U, mo.lam)
        g.set_target(target)
        g.set_meshes(*sub_triangles())
        for flavour, params in ((CPD, CPD_PARAMS), (ICP, ICP_PARAMS), (SURFACE, ICP_PARAMS)):
            name = "group." + SUFFIX[flavour]
            g.set_state(alpha0, SIGMA2, euler=EULER, translation=TRANSLATION)
            g.update(flavour, params, 2)
            alpha, s, fit = g.get_state()
            out[name + "_update_alpha"], out[name + "_update_scalars"], out[name + "_update_fit"] = alpha, scalars_array(s), fit
            g.set_state(alpha0, SIGMA2, euler=EULER, translation=TRANSLATION)
            g.update(flavour, params, 1, z=z)
            alpha, s, fit = g.get_state()
            out[name + "_sample_alpha"], out[name + "_sample_scalars"], out[name + "_sample_fit"] = alpha, scalars_array(s), fit
            g.set_state(alpha0, SIGMA2, euler=EULER, translation=TRANSLATION)
            out[name + "_logpdf"] = np.array([g.posterior_logpdf(flavour, params, mesh)])
    finally:
        g.close()
    return out


def all_results(ctx):
    """what tests/golden/fitter_flavour_bits.npz records, before reduce()"""
    out = {}
    for name in CONFIGS:
        out.update(config_results(ctx, name))
    out.update(group_results())
    return out


def reduce(results):
    """every fit but that of the deterministic updates as the SHA-256 digest of its bytes"""
    out = {}
    for k, v in results.items():
        v = np.ascontiguousarray(v, dtype=np.float64)
        if k.endswith("_fit") and (k.startswith("group.") or not k.endswith(".update_fit")):
            v = np.frombuffer(hashlib.sha256(v.tobytes()).digest(), dtype=np.uint8)
        out[k] = v
    return out


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


def compare(got, prefix):
    want = {k: v for k, v in golden().items() if k.startswith(prefix + ".")}
    got = reduce(got)
    assert sorted(want) == sorted(got)
    for k in sorted(want):
        assert want[k].dtype == got[k].dtype and np.array_equal(want[k], got[k], equal_nan=True), k


def test_every_recorded_output_is_a_number():
    for k, v in golden().items():
        assert np.isfinite(v).all(), k


@pytest.mark.parametrize("name", list(CONFIGS))
def test_the_flavour_keeps_its_bits(ctx, name):
    compare(config_results(ctx, name), name)


def test_the_one_device_group_keeps_its_bits(ctx):
    compare(group_results(), "group")
