"""Host-side pieces of the posterior model: the r x r identity behind gingr_amd/csrc/posterior_model.hip, restated in numpy and
pinned against the oracle's restatement of scalismo's regression, and the declarations of the C ABI."""
import os
import re

import numpy as np
import pytest

from oracle import gingr_oracle as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ["gingr_model_posterior", "gingr_fitter_posterior_model_cpd", "gingr_fitter_posterior_model_icp",
             "gingr_fitter_posterior_model_icp_surface"]


def factored_posterior(model, pids, pts, covs):
    """(Q_new, lambda_p, mean mesh) the way the device builds them: W = L^-T with L L^T = I + G, H = W^T diag(lambda) W =
    V diag(lambda_p) V^T, T = W V, Q_new = Q T, a = W W^T rhs -- no division by a prior variance"""
    r = model.rank
    Q = model.U * np.sqrt(model.lam)[None, :]
    G, rhs = np.zeros((r, r)), np.zeros(r)
    for k, pid in enumerate(pids):
        Qk = Q[3 * pid:3 * pid + 3]
        G += Qk.T @ np.linalg.solve(covs[k], Qk)
        rhs += Qk.T @ np.linalg.solve(covs[k], pts[k] - model.ref[pid] - model.mean[pid])
    W = np.linalg.inv(np.linalg.cholesky(np.eye(r) + G)).T
    H = W.T @ (model.lam[:, None] * W)
    lam_p, V = np.linalg.eigh(H)
    lam_p, V = lam_p[::-1], V[:, ::-1]
    a = W @ (W.T @ rhs)
    return Q @ (W @ V), lam_p, model.ref + model.mean + (Q @ a).reshape(-1, 3)


@pytest.mark.parametrize("M,r,sigma2,zero_variance", [(60, 12, 1.0, False), (40, 30, 0.01, False), (50, 9, 1.0, True)])
def test_factored_route_is_the_oracles_posterior_model(M, r, sigma2, zero_variance):
    rng = np.random.default_rng(M + r)
    U, _ = np.linalg.qr(rng.normal(0, 1, (3 * M, r)))
    lam = 50.0 * 0.8 ** np.arange(r)
    if zero_variance:
        lam[-2:] = 0.0                                                          # directions the prior does not have stay at zero
    model = go.PDM(rng.normal(0, 30, (M, 3)), rng.normal(0, 1, (M, 3)), U, lam).transform(go.euler_to_rot(0.3, -0.2, 0.1), np.array([1.0, -2.0, 0.5]))
    pids = np.sort(rng.permutation(M)[: M - M // 5])
    pts = (model.ref + model.mean)[pids] + rng.normal(0, 2.0, (pids.shape[0], 3))
    covs = np.tile(sigma2 * np.eye(3), (pids.shape[0], 1, 1))
    A = rng.normal(0, 1, (3, 3))
    covs[0] = A @ A.T + np.diag([0.2, 1.0, 3.0])
    want = model.posterior_model(pids, pts, covs)
    Qn, lam_p, mesh = factored_posterior(model, pids, pts, covs)
    Qw = want.U * np.sqrt(want.lam)[None, :]
    assert np.abs(Qn @ Qn.T - Qw @ Qw.T).max() <= 1e-11 * np.abs(Qw @ Qw.T).max()
    assert np.abs(lam_p - want.lam).max() <= 1e-11 * want.lam.max()
    assert np.abs(mesh - want.ref - want.mean).max() <= 1e-11 * np.abs(want.ref + want.mean).max()
    keep = lam_p > 1e-9 * lam_p.max()
    Un = Qn[:, keep] / np.sqrt(lam_p[keep])[None, :]
    assert np.abs(Un.T @ Un - np.eye(int(keep.sum()))).max() <= 1e-10             # Q T = U_p sqrt(lambda_p): unit columns
    assert keep.sum() == r - (2 if zero_variance else 0) and np.abs(Qn[:, ~keep]).max(initial=0.0) <= 1e-6 * np.abs(Qn).max()


def test_header_and_prototypes_declare_the_new_names():
    from gingr_amd import _native
    header = open(os.path.join(ROOT, "include", "gingr_hip.h")).read()
    for name in NEW_NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _native.SIGNATURES, name
    assert "GingrAlgorithm.scala:281-302" in header                              # each entry cites the Scala it replaces
