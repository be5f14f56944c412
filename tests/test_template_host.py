"""Host-side checks of the "pairs given" flavour and TemplateRegistration (no GPU): the new entry points exist in the header, the
ctypes table and the built library; the identity the device consolidation rests on, with the oracle alone; and the argument errors
TemplateRegistration raises before anything is sent to the device."""
import os
import re
import subprocess
import types

import numpy as np
import pytest

from oracle import gingr_oracle as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = [
    "gingr_fitter_set_pairs", "gingr_fitter_set_pairs_cov", "gingr_fitter_get_pair_observations", "gingr_fitter_set_sigma2",
    "gingr_fitter_last_update_error", "gingr_fitter_update_pairs_async", "gingr_fitter_pairs_phase_async",
    "gingr_fitter_update_pairs_sample_async", "gingr_fitter_posterior_logpdf_pairs", "gingr_fitter_posterior_covariance_pairs",
    "gingr_fitter_posterior_model_pairs",
]


def test_new_symbols_in_header_signatures_and_library():
    from gingr_amd import _native as nat
    header = open(os.path.join(ROOT, "include", "gingr_hip.h")).read()
    declared = set(re.findall(r"^\w[\w \*]*?\b(gingr_\w+)\(", header, flags=re.M))
    lib = os.path.join(ROOT, "gingr_amd", "libgingr_hip.so")
    assert os.path.exists(lib), "build the library first (__graft_entry__.build)"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (gingr_\w+)", out))
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} not declared in include/gingr_hip.h"
        assert name in nat.SIGNATURES, f"{name} not in _native.SIGNATURES"
        assert name in exported, f"{name} not exported by libgingr_hip.so"
    import gingr_amd as ga
    assert ga.TemplateRegistration.name == "Template"
    cfg = ga.TemplateConfiguration()                                            # Template.scala:24-29
    assert (cfg.maxIterations, cfg.threshold, cfg.useLandmarkCorrespondence) == (1, 1e-5, True) and cfg.converged(None, None, 0.0) is False


@pytest.mark.parametrize("seed", range(20))
def test_repeated_observations_are_one_observation_of_their_weighted_mean(seed):
    """k isotropic observations of one point = one observation of their precision-weighted mean with the summed precision: both the
    Gram matrix and the right-hand side of the regression agree, so PDM.posterior_mean does.  1e-12 relative."""
    rng = np.random.default_rng(seed)
    M = int(rng.integers(5, 60))
    ref = rng.normal(0, 30, (M, 3))
    mo = go.build_gaussian_gpmm(ref, 40.0, 20.0, rel_tol=1e-9, max_rank=int(rng.integers(3, 12)))
    if seed % 3 == 0:
        mo = mo.transform(go.euler_to_rot(0.2, -0.1, 0.3), np.array([1.0, -2.0, 0.5]), np.array([0.5, 0.5, -1.0]))
    K = int(rng.integers(1, 4 * M))
    seen = rng.permutation(M)[: max(1, M // 2)]
    pids = rng.choice(seen, K)
    pts = (mo.ref + mo.mean)[pids] + rng.normal(0, 3.0, (K, 3))
    var = 10.0 ** rng.uniform(-2, 2, K)
    mesh_a, a = mo.posterior_mean(pids, pts, var[:, None, None] * np.eye(3)[None])
    w, s = np.zeros(M), np.zeros((M, 3))
    for k in range(K):                                                          # the device's consolidation, in its order
        w[pids[k]] += 1.0 / var[k]
        s[pids[k]] += pts[k] / var[k]
    one = np.flatnonzero(w)
    mesh_b, b = mo.posterior_mean(one, s[one] / w[one][:, None], (1.0 / w[one])[:, None, None] * np.eye(3)[None])
    assert np.linalg.norm(mesh_b - mesh_a) <= 1e-12 * np.linalg.norm(mesh_a)
    assert np.linalg.norm(b - a) <= 1e-12 * max(np.linalg.norm(a), 1.0)


def _host_state(M=6, r=3):
    import gingr_amd as ga
    model = ga.PointDistributionModel(np.zeros((M, 3)), np.zeros((M, 3)), np.zeros((3 * M, r)), np.ones(r))
    g = ga.GeneralRegistrationState(model=model, modelParameters=ga.ModelFittingParameters.zero(r), target=np.zeros((4, 3)), fit=np.zeros((M, 3)))
    return ga.TemplateRegistrationState(g, ga.TemplateConfiguration())


def test_argument_errors_are_raised_before_any_native_call():
    import gingr_amd as ga
    no_device = types.SimpleNamespace(_lib=None, handle=None)                   # any native call through it would raise AttributeError
    state = _host_state()
    pairs = ga.CorrespondencePairs(np.array([0, 2, 2]), np.zeros((3, 3)))
    for bad in (np.ones((3, 2, 2)), np.ones((2, 3, 3)), np.ones(4), np.ones((3, 3))):
        algo = ga.TemplateRegistration(no_device, lambda s: pairs, lambda p, s, bad=bad: bad)
        with pytest.raises(ValueError, match="getUncertainty"):
            algo.update(state)
    algo = ga.TemplateRegistration(no_device, lambda s: ga.CorrespondencePairs(np.array([0, 1]), np.zeros((3, 3))))
    with pytest.raises(ValueError, match="getCorrespondence"):
        algo.update(state)


def test_split_of_isotropic_and_full_covariances():
    import gingr_amd as ga
    pairs = ga.CorrespondencePairs(np.array([4, 1, 4, 0]), np.arange(12.0).reshape(4, 3))
    aniso = np.diag([1.0, 2.0, 3.0])
    almost = 2.0 * np.eye(3)
    almost[0, 1] = 1e-300                                                        # not an EXACT multiple of the identity
    covs = np.stack([0.5 * np.eye(3), aniso, almost, 7.0 * np.eye(3)])
    (ip, ix, iv), (cp, cx, cc) = ga.TemplateRegistration.splitObservations(pairs, covs)
    assert ip.dtype == np.int32 and np.array_equal(ip, [4, 0]) and np.array_equal(iv, [0.5, 7.0]) and np.array_equal(ix, pairs.points[[0, 3]])
    assert np.array_equal(cp, [1, 4]) and np.array_equal(cc, covs[[1, 2]]) and np.array_equal(cx, pairs.points[[1, 2]])
    (ip, ix, iv), (cp, _, _) = ga.TemplateRegistration.splitObservations(pairs, 2.5)        # a scalar: every pair
    assert np.array_equal(iv, np.full(4, 2.5)) and cp.shape[0] == 0
    (ip, ix, iv), (cp, _, _) = ga.TemplateRegistration.splitObservations(pairs, np.array([1.0, 2.0, np.inf, 4.0]))
    assert np.array_equal(iv, [1.0, 2.0, np.inf, 4.0]) and cp.shape[0] == 0
    empty = ga.TemplateRegistration(types.SimpleNamespace(_lib=None, handle=None)).getCorrespondence(None)   # Template.scala:47-48
    (ip, _, _), (cp, _, _) = ga.TemplateRegistration.splitObservations(empty, 1.0)
    assert ip.shape[0] == 0 and cp.shape[0] == 0
