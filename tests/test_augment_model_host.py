"""The numpy restatement of gingr_model_augment (tests/augment_restatement.py) against closed forms, its two routes against each other,
the rank rules, and the shared cases' fitness for a rank comparison.  CPU only."""
import numpy as np
import pytest

from tests import augment_restatement as ar
from tests.augment_restatement import CASES, ROUTE_SPREAD


def orthogonal_pair(M, ra, rb, seed=1):
    rng = np.random.default_rng(seed)
    ref = rng.normal(0.0, 30.0, (M, 3))
    U, _ = np.linalg.qr(rng.normal(size=(3 * M, ra + rb)))
    la, lb = ar.spectrum(ra, 400.0), ar.spectrum(rb, 90.0, 1e-3)
    a = ar.Model(ref, rng.normal(0, 5, (M, 3)), la, U[:, :ra] * np.sqrt(la)[None])
    b = ar.Model(ref, rng.normal(0, 5, (M, 3)), lb, U[:, ra:] * np.sqrt(lb)[None])
    return a, b


@pytest.mark.parametrize("route", [ar.augment, ar.augment_by_gram])
def test_orthogonal_models_give_the_merged_spectra(route):
    a, b = orthogonal_pair(60, 7, 12)
    m = route(a, b)
    want = np.sort(np.concatenate([a.variance, b.variance]))[::-1]
    assert m.rank == 19
    np.testing.assert_allclose(m.variance, want, rtol=0, atol=1e-13 * want[0])
    np.testing.assert_array_equal(m.mean, a.mean + b.mean)
    np.testing.assert_array_equal(m.reference, a.reference)
    P = ar.probes(180)
    np.testing.assert_allclose(m.operator(P), a.operator(P) + b.operator(P), rtol=0, atol=1e-12 * np.abs(a.operator(P)).max())
    # the basis is orthonormal and sorted
    np.testing.assert_allclose(m.basis.T @ m.basis, np.eye(19), rtol=0, atol=1e-10)


@pytest.mark.parametrize("route", [ar.augment, ar.augment_by_gram])
def test_a_model_augmented_with_itself_doubles_its_variance(route):
    a, _ = ar.case(150, 17, 100)
    m = route(a, a)
    assert m.rank == a.rank
    np.testing.assert_allclose(m.variance, 2.0 * a.variance, rtol=0, atol=1e-13 * a.variance[0])
    np.testing.assert_array_equal(m.mean, 2.0 * a.mean)
    assert m.all_variance.shape[0] == 2 * a.rank and m.all_variance[a.rank:].max() <= 1e-13 * m.variance[0]


@pytest.mark.parametrize("route", [ar.augment, ar.augment_by_gram])
def test_more_columns_than_coordinates(route):
    a, b = ar.case(5, 10, 10)
    m = route(a, b)
    assert m.rank <= 15
    P = ar.probes(15)
    np.testing.assert_allclose(m.operator(P), a.operator(P) + b.operator(P), rtol=0, atol=1e-12 * np.abs(m.operator(P)).max())


def test_route_spread_svd_against_gram():
    worst = 0.0
    for c in CASES:
        x, y = ar.expected(*c), ar.augment_by_gram(*ar.case(*c))
        d_lam, d_op = ar.spread(x, y)
        print(f"{c}: rank {x.rank}, eigenvalues {d_lam:.2e} of lambda_1, operator {d_op:.2e} of the result")
        worst = max(worst, d_lam, d_op)
    print(f"largest: {worst:.2e}; ROUTE_SPREAD = {ROUTE_SPREAD:.2e}")
    assert worst <= ROUTE_SPREAD


def test_rank_rules():
    a, b = ar.case(150, 17, 100)
    full = ar.expected(150, 17, 100)
    assert full.rank == 117
    for route in (ar.augment, ar.augment_by_gram):
        m = route(a, b, max_rank=9)
        assert m.rank == 9
        np.testing.assert_allclose(m.variance, full.variance[:9], rtol=0, atol=ROUTE_SPREAD * full.variance[0])
        tol = 0.5 * (full.variance[30] + full.variance[31]) / full.variance[0]
        assert route(a, b, relative_tolerance=tol).rank == 31
        assert route(a, b, relative_tolerance=tol, max_rank=12).rank == 12
        assert route(a, b, max_rank=4000).rank == 117
        with pytest.raises(ValueError, match="rank 0"):
            route(a, b, relative_tolerance=1.0)
    with pytest.raises(ValueError, match="512"):
        ar.augment(ar.case(300, 200, 312)[1], ar.case(300, 200, 312)[1])
    other = ar.Model(a.reference + 1e-9, b.mean, b.variance, b.Q0)
    with pytest.raises(ValueError, match="reference"):
        ar.augment(a, other)


@pytest.mark.parametrize("M,ra,rb", CASES)
def test_every_shared_case_has_an_unambiguous_rank(M, ra, rb):
    """no eigenvalue of the sum between 1e-13 and 1e-7 of the largest: the cutoff 1e-10 decides the same way on every route"""
    m = ar.expected(M, ra, rb)
    rel = m.all_variance / m.all_variance[0]
    print(f"({M}, {ra}, {rb}): rank {m.rank} of {ra + rb} columns, smallest kept {rel[m.rank - 1]:.2e}, largest dropped "
          f"{rel[m.rank] if m.rank < rel.shape[0] else 0.0:.2e}")
    assert not np.any((rel > 1e-13) & (rel < 1e-7))
    assert m.rank == min(ra + rb, 3 * M) == ar.augment_by_gram(*ar.case(M, ra, rb)).rank
    # the means are large enough that the row orders of a, b and the result have nothing to do with each other
    a, b = ar.case(M, ra, rb)
    assert np.abs(a.mean).max() > 10.0 and np.abs(b.mean).max() > 10.0 and np.abs(a.mean - b.mean).max() > 10.0
