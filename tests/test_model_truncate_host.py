"""CPU tests of PointDistributionModel.truncate (the host dataclass): slices, bounds, independence from the source."""
import numpy as np
import pytest


def model(M=7, r=5, cells=True):
    import gingr_amd as ga
    rng = np.random.default_rng(3)
    U, _ = np.linalg.qr(rng.normal(size=(3 * M, r)))
    return ga.PointDistributionModel(reference=rng.normal(size=(M, 3)), mean=rng.normal(size=(M, 3)), basis=np.asfortranarray(U),
                                     variance=np.sort(rng.uniform(1, 9, r))[::-1].copy(),
                                     cells=np.arange(6, dtype=np.int32).reshape(2, 3) if cells else None)


@pytest.mark.parametrize("k", [1, 3, 5])
def test_truncate_keeps_the_leading_basis_functions(k):
    m = model()
    t = m.truncate(k)
    assert t.rank == k and t.numberOfPoints == m.numberOfPoints
    assert np.array_equal(t.reference, m.reference) and np.array_equal(t.mean, m.mean)
    assert np.array_equal(t.basis, m.basis[:, :k]) and np.array_equal(t.variance, m.variance[:k])
    assert np.array_equal(t.cells, m.cells)
    assert model(cells=False).truncate(k).cells is None


@pytest.mark.parametrize("k", [0, -1, 6])
def test_truncate_bounds(k):
    with pytest.raises(ValueError):
        model().truncate(k)


def test_truncated_model_shares_no_memory_with_its_source():
    m = model()
    t = m.truncate(3)
    for a, b in ((t.reference, m.reference), (t.mean, m.mean), (t.basis, m.basis), (t.variance, m.variance), (t.cells, m.cells)):
        assert not np.shares_memory(a, b)
    t.basis[:] = 0.0
    t.variance[:] = 0.0
    t.reference[:] = 0.0
    assert m.basis.any() and m.variance.all() and m.reference.any()
