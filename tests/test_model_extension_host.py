"""CPU: the kernel-extension formula (tests/model_extension_restatement.py) on the oracle's own factor -- it gives back the model's
rows at the model's vertices, and leaves a non-negative residual variance off them."""
import numpy as np
import pytest

from tests import model_extension_restatement as mr

SPEC = {"kind": "gauss", "sigmas": [60.0], "scalings": [25.0], "mirror": 0.0}


@pytest.fixture(scope="module")
def hull():
    return mr.hull()


@pytest.fixture(scope="module", params=[1e-2, 1e-6], ids=["tol1e-2", "tol1e-6"])
def built(request, hull):
    specs = [SPEC] * 3
    Q, coeffs, lam = mr.oracle_model(hull, specs, request.param)
    return request.param, specs, Q, coeffs


def test_the_formula_reproduces_the_models_own_rows(hull, built):
    tol, specs, Q, coeffs = built
    Qx = mr.extension_rows(specs, hull, coeffs, hull, np.float64)
    err = mr.reproduction_error(Q, Qx)
    print(f"tolerance {tol:g}: pivots per coordinate {[len(i) for i, _ in coeffs]}, rank {Q.shape[2]}, own-vertex reproduction error {err:.3g}")
    # the triangular solve loses what the conditioning of the pivot rows takes, which grows as the tolerance falls: measured 5.5e-15
    # and 1.3e-12; two and three orders above that would mean a wrong formula, not rounding
    assert err <= (1e-9 if tol < 1e-3 else 1e-12), (tol, err)


def test_the_residual_variance_off_the_reference_is_not_negative(hull, built):
    tol, specs, Q, coeffs = built
    rng = np.random.default_rng(5)
    Z = 0.9 * hull[:300] + rng.normal(0.0, 1.0, (300, 3))
    res, kzz = mr.residual_diagonal(specs, hull, coeffs, Z)
    print(f"tolerance {tol:g}: smallest residual diagonal {res.min() / 25.0:.3g} x scaling, largest {res.max() / 25.0:.3g} x scaling")
    assert res.min() >= 0.0
    assert res.max() <= kzz.max()
