"""Host tests of the spatially varying / non-Gaussian kernel layer: the weight fields and the term construction of
GPMMTriangleMesh3D (nothing here builds a model, so no device is touched), the selectors of gingr_amd.simple, and the restatement the
GPU tests compare against (tests/varying_kernel_restatement.py)."""
import numpy as np
import pytest

from tests import varying_kernel_restatement as vk


def patch(M=60, seed=2):
    rng = np.random.default_rng(seed)
    i, j = np.divmod(np.arange(M), 6)
    return np.stack([5.0 * i, 5.0 * j, 3.0 * np.sin(i / 3.0)], axis=1) + rng.uniform(-1.5, 1.5, (M, 3))


def builder(ref):
    import gingr_amd as ga
    return ga.GPMMTriangleMesh3D(None, ref, relativeTolerance=0.01)          # no context: nothing is built


def test_new_names_import_from_api():
    from gingr_amd import api
    for name in ("RadialKernelTerm", "sigmoidField", "GPMMTriangleMesh3D"):
        assert hasattr(api, name)
    for name in ("RadialMixture", "RationalQuadratic", "InverseMultiquadric", "ScaledGaussian", "ChangePoint"):
        assert callable(getattr(api.GPMMTriangleMesh3D, name))
    import gingr_amd as ga
    assert ga.RadialKernelTerm is api.RadialKernelTerm and ga.sigmoidField is api.sigmoidField


def test_sigmoid_field():
    import gingr_amd as ga
    ref = patch()
    point, normal = np.array([20.0, 10.0, 0.0]), np.array([3.0, 0.0, 4.0])
    s = ga.sigmoidField(ref, point, normal, 7.0)
    assert s.shape == (60,) and s.dtype == np.float64
    assert np.array_equal(s, vk.sigmoid_field(ref, point, normal, 7.0))
    assert np.all((s > 0.0) & (s < 1.0))
    # on the plane 1/2; the normal's length does not matter; the opposite normal is the complement
    assert ga.sigmoidField(point[None, :], point, normal, 7.0)[0] == 0.5
    assert np.allclose(ga.sigmoidField(ref, point, 10.0 * normal, 7.0), s, rtol=1e-14, atol=0)
    assert np.allclose(ga.sigmoidField(ref, point, -normal, 7.0), 1.0 - s, rtol=0, atol=1e-15)
    # far away it saturates without a warning or a NaN
    far = ga.sigmoidField(np.array([[1e6, 0, 0], [-1e6, 0, 0]]), [0, 0, 0], [1, 0, 0], 1.0)
    assert far[0] == 1.0 and far[1] == 0.0
    for bad in ([0.0, 0.0, 0.0], [np.nan, 0.0, 1.0]):
        with pytest.raises(ValueError):
            ga.sigmoidField(ref, point, bad, 7.0)
    for width in (0.0, -1.0):
        with pytest.raises(ValueError):
            ga.sigmoidField(ref, point, normal, width)


def test_change_point_terms_weights_and_order():
    import gingr_amd as ga
    ref = patch()
    s = ga.sigmoidField(ref, [20.0, 10.0, 0.0], [1.0, 0.0, 0.0], 5.0)
    A = [ga.GaussianKernelParameters(40.0, 20.0), ga.GaussianKernelParameters(25.0, 8.0)]
    B = [ga.GaussianKernelParameters(12.0, 5.0)]
    m = builder(ref).ChangePoint(A, B, s)
    kx, ky, kz = m._radial
    assert kx is ky and ky is kz                                    # one kernel: the scalar route
    assert [(t.family, t.parameter, t.scaling) for t in kx] == [("gaussian", 40.0, 20.0), ("gaussian", 25.0, 8.0), ("gaussian", 12.0, 5.0)]
    assert np.array_equal(kx[0].weight, s) and kx[1].weight is kx[0].weight          # the terms of A share the indicator
    assert np.array_equal(kx[2].weight, 1.0 - s)
    # the restatement's change point is the same list
    for t, (fam, par, sc, w) in zip(kx, vk.change_point_terms([(40.0, 20.0), (25.0, 8.0)], [(12.0, 5.0)], s)):
        assert (t.family, t.parameter, t.scaling) == (fam, par, sc) and np.array_equal(t.weight, w)
    for bad in (s + 0.5, s - 0.5, np.where(np.arange(60) == 3, np.nan, s)):
        with pytest.raises(ValueError):
            builder(ref).ChangePoint(A, B, bad)
    with pytest.raises(ValueError):                                  # a field of the wrong length
        builder(ref).ChangePoint(A, B, s[:-1])
    with pytest.raises(ValueError):                                  # a term that already has a field
        builder(ref).ChangePoint([ga.RadialKernelTerm("gaussian", 10.0, 1.0, s)], B, s)


def test_scaled_gaussian_and_radial_mixture_terms():
    import gingr_amd as ga
    ref = patch()
    a = 0.2 + 2.8 * ga.sigmoidField(ref, [20.0, 10.0, 0.0], [0.0, 1.0, 0.0], 9.0)
    m = builder(ref).ScaledGaussian([ga.GaussianKernelParameters(30.0, 6.0), ga.GaussianKernelParameters(10.0, 2.0)], a)
    terms = m._radial[0]
    assert [(t.family, t.parameter, t.scaling) for t in terms] == [("gaussian", 30.0, 6.0), ("gaussian", 10.0, 2.0)]
    assert terms[0].weight is terms[1].weight and np.array_equal(terms[0].weight, a)
    assert builder(ref).RationalQuadratic(30.0, 4.0)._radial[0][0].family_code == 1
    imq = builder(ref).InverseMultiquadric(30.0, 4.0)._radial[0][0]
    assert (imq.family_code, imq.parameter, imq.scaling, imq.weight) == (2, 30.0, 4.0, None)
    # three lists: the coordinates keep their own
    tx, ty = [ga.RadialKernelTerm("gaussian", 30.0, 6.0, a)], [ga.RadialKernelTerm("rationalQuadratic", 30.0, 6.0)]
    m3 = builder(ref).RadialMixture((tx, ty, ty))
    assert m3._radial[0][0] is tx[0] and m3._radial[1][0] is ty[0] and m3._radial[2][0] is ty[0]
    # a truncation keeps the terms
    assert m3.truncate(5)._radial == m3._radial and m3.truncate(5)._keep == 5
    with pytest.raises(ValueError):
        ga.RadialKernelTerm("cubic", 1.0, 1.0)
    with pytest.raises(ValueError):
        ga.RadialKernelTerm("gaussian", 1.0, 1.0, np.ones((4, 2)))
    with pytest.raises(ValueError):
        builder(ref).RadialMixture([ga.RadialKernelTerm("gaussian", 1.0, 1.0, np.ones(59))])
    with pytest.raises(TypeError):
        builder(ref).RadialMixture([("gaussian", 1.0, 1.0)])


def test_simple_selectors_printpars():
    from gingr_amd import simple
    assert simple.RationalQuadraticKernel(scaling=4.0, beta=30.0).printpars == "4.0_30.0"
    assert simple.RationalQuadraticKernel(4.0, 30.0).name == "RationalQuadratic"
    assert simple.InverseMultiquadricKernel(scaling=2.5, beta=12.0).printpars == "2.5_12.0"
    assert simple.InverseMultiquadricKernel(2.5, 12.0).name == "InverseMultiquadric"
    cp = simple.ChangePointKernel(20.0, 40.0, 5.0, 12.0, (1.0, 2.0, 3.0), (0.0, 0.0, 1.0), 8.0)
    assert cp.printpars == "20.0_40.0_5.0_12.0_8.0" and cp.name == "ChangePoint"


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restated_kernel_is_positive_semidefinite(seed):
    """sum_t D_t K_t D_t is positive semi-definite for ANY real weights: smallest eigenvalue >= -1e-10 of the largest."""
    rng = np.random.default_rng(seed)
    ref = patch(60, seed + 10)
    terms = [(vk.GAUSSIAN, 20.0, 5.0, rng.normal(0, 1, 60)),                     # fields with negative values
             (vk.RATIONAL_QUADRATIC, 15.0, 2.0, rng.uniform(-2, 2, 60)),
             (vk.INVERSE_MULTIQUADRIC, 10.0, 30.0, rng.normal(0, 1, 60)),
             (vk.GAUSSIAN, 8.0, 1.0, None)]
    K = vk.dense(ref, terms)
    assert np.array_equal(K, K.T) or np.abs(K - K.T).max() <= 1e-15 * np.abs(K).max()
    ev = np.linalg.eigvalsh(0.5 * (K + K.T))
    assert ev[0] >= -1e-10 * ev[-1], (ev[0], ev[-1])
    # the diagonal the device starts from: sum_t scaling_t f_t(0) w_t^2, f_t(0) = 1, 1, 1 / beta
    d = 5.0 * terms[0][3] ** 2 + 2.0 * terms[1][3] ** 2 + (30.0 / 10.0) * terms[2][3] ** 2 + 1.0
    assert np.allclose(np.diag(K), d, rtol=1e-14, atol=0)


def test_restatement_all_ones_field_is_no_field():
    ref = patch()
    one = np.ones(60)
    a = vk.dense(ref, [(vk.GAUSSIAN, 20.0, 5.0, None), (vk.INVERSE_MULTIQUADRIC, 10.0, 30.0, None)])
    b = vk.dense(ref, [(vk.GAUSSIAN, 20.0, 5.0, one), (vk.INVERSE_MULTIQUADRIC, 10.0, 30.0, one)])
    assert np.array_equal(a, b)
