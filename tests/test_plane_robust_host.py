"""CPU tests of robust point-to-plane ICP: the numpy restatement (tests/robust_pairs_restatement.py) against direct closed forms, the
plan header of the selection (gingr_amd/csrc/robust_select_plan.h) through a stand-alone C++ driver built with the address and
undefined-behaviour sanitizers (tests/c/robust_select_plan_driver.cpp), and the C ABI / Python surface."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import plane_pairs_restatement as pp
from tests import robust_pairs_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
FUNCTIONS = ["gingr_fitter_set_plane_robust", "gingr_fitter_get_plane_robust", "gingr_order_statistic"]
SIZES = [1, 2, 255, 256, 257, 1000, 65537]


# ------------------------------------------------------------------------------------------------------ the restatement
def unit(rng, k):
    n = rng.normal(0, 1, (k, 3))
    return n / np.linalg.norm(n, axis=1)[:, None]


@pytest.mark.parametrize("ratio", [1.0, 100.0, 1e8])
def test_residual_is_the_distance_in_the_metric_of_the_observation(ratio):
    rng = np.random.default_rng(3)
    n, d = unit(rng, 200), rng.normal(0, 2.0, (200, 3))
    sigma2 = 1.7
    L = pp.closed_form(n, sigma2, ratio, np.longdouble)                                   # the plane the vertex gets
    want = sigma2 * np.einsum("ki,kij,kj->k", d.astype(np.longdouble), L, d.astype(np.longdouble))
    s = rr.residual(d, n, ratio, np.longdouble)
    assert np.abs(s - want).max() <= 64 * pp.U53 * np.abs(want).max()
    if ratio == 1.0:
        assert np.abs(s - (d.astype(np.longdouble) ** 2).sum(1)).max() <= 8 * pp.U53 * (d * d).sum(1).max()
    zero = rr.residual(d, np.zeros_like(n), ratio)                                        # no normal: |d|^2 / rho, as plane_precision
    assert np.allclose(zero, (d * d).sum(1) / ratio, rtol=1e-14, atol=0)
    along = rr.residual(3.0 * n, n, ratio)                                                # d along the normal: the tangential part clamps
    assert (along >= 0).all() and np.allclose(along, 9.0, rtol=1e-12)


def test_cauchy_at_ratio_one_is_the_demo_formula():
    rng = np.random.default_rng(4)
    d, n = rng.normal(0, 1.5, (300, 3)), unit(rng, 300)
    sigma2, tau = 2.5, 1.3
    s = rr.residual(d, n, 1.0)
    u = rr.inflation("cauchy", s, tau)
    d2 = (d * d).sum(1)
    assert np.allclose(sigma2 * u, sigma2 * (1.0 + d2 / tau ** 2), rtol=1e-14, atol=0)    # examples/demo_template.py: sigma2 (1 + d^2 / tau^2)


def test_losses_scale_and_degenerate_cases():
    s = np.array([0.0, 0.25, 1.0, 3.9999, 4.0, 9.0])
    c = 2.0
    assert np.array_equal(rr.inflation("huber", s, c), [1.0, 1.0, 1.0, 1.0, 1.0, 1.5])
    assert np.allclose(rr.inflation("cauchy", s, c), 1.0 + s / 4.0)
    tk = rr.inflation("tukey", s, c)
    assert tk[0] == 1.0 and tk[4] == 0.0 and tk[5] == 0.0 and (tk[1:4] > 1.0).all()
    assert np.allclose(tk[1:4], 1.0 / (1.0 - s[1:4] / 4.0) ** 2)
    for kind in rr.LOSSES:                                                                # c = 0 (perfect fit, nothing observed): u = 1
        assert np.array_equal(rr.inflation(kind, s, 0.0), np.ones(6))
    assert np.array_equal(rr.inflation("huber", s, 1e300), np.ones(6))                     # a robust setting that never weights
    # the lower median is an element of the data and does not depend on the weights
    assert rr.lower_median([5.0, 1.0, 3.0, 2.0]) == 2.0 and rr.lower_median([7.0]) == 7.0 and rr.lower_median([4.0, 2.0, 9.0]) == 4.0
    sel, cc = rr.scale([4.0, 1.0, 9.0], 1, 2.385)
    assert sel == 4.0 and cc == (2.385 * 1.4826) * 2.0
    assert rr.scale([4.0, 1.0, 9.0], 1, 2.385, min_scale=100.0)[1] == 100.0 and rr.scale([], 1, 2.385) == (0.0, 0.0)
    assert rr.scale([4.0], 0, 3.0) == (4.0, 3.0)
    # Tukey's removed vertices still count in the median
    fit, pts = np.zeros((5, 3)), np.array([[0.1, 0, 0], [0.2, 0, 0], [0.3, 0, 0], [50.0, 0, 0], [60.0, 0, 0]])
    s, u, sel, cc, n = rr.weigh(fit, pts, np.zeros((5, 3)), np.ones(5, bool), 1.0, "tukey", 1, 4.685)
    assert n == 5 and sel == s[2] and (u[3:] == 0).all() and (u[:3] >= 1).all()
    assert rr.TUNINGS == {"cauchy": 2.385, "huber": 1.345, "tukey": 4.685}


def test_covariances_are_the_planes_at_the_inflated_variance():
    rng = np.random.default_rng(6)
    n, u = unit(rng, 50), rng.uniform(1.0, 30.0, 50)
    cov = rr.covariances(n, 1.5, u, 100.0)
    for k in range(50):
        L = pp.closed_form(n[k:k + 1], 1.5 * u[k], 100.0)[0]
        assert np.abs(cov[k] @ L - np.eye(3)).max() < 1e-9


# ------------------------------------------------------------------------------------------------------ the plan header
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("robust_select_plan") / "robust_select_plan_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gingr_amd", "csrc"), os.path.join(ROOT, "tests", "c", "robust_select_plan_driver.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, check=True, text=True).stdout
    assert "FAIL" not in out and "ok 0" in out, out
    return out


def test_digits_cover_the_key(driver):
    m = re.search(r"digits (\d+) bits x (\d+) passes, (\d+) bins, (\d+) threads, covered ([0-9a-f]+)", driver)
    bits, passes, bins, threads = (int(m.group(i)) for i in range(1, 5))
    assert bits * passes == 64 and bins == 1 << bits and threads == bins and m.group(5) == "f" * 16


def test_grid_sizing(driver):
    groups = {int(n): (int(g), int(w)) for n, g, w in re.findall(r"groups (\d+) (\d+) (\d+)", driver)}
    assert set(SIZES) <= set(groups)
    for n, (g, words) in groups.items():
        assert 1 <= g <= 64 and words == 8 * g * 256
        assert g == 64 or g * 2048 >= n                                                    # every key has a thread before the grid strides
    assert [groups[n][0] for n in SIZES] == [1, 1, 1, 1, 1, 1, 33] and groups[2049][0] == 2 and groups[1000000][0] == 64


def test_key_order_and_selection(driver):
    m = re.search(r"keys zero ([0-9a-f]+) denormal ([0-9a-f]+) inf ([0-9a-f]+) sentinel ([0-9a-f]+)", driver)
    zero, den, inf, sentinel = (int(m.group(i), 16) for i in range(1, 5))
    assert zero == 0 and den == 1 and inf == 0x7FF0000000000000 and sentinel == 2 ** 64 - 1
    assert zero < den < inf < sentinel
    assert int(re.search(r"selections (\d+)", driver).group(1)) == 7 * 5 * 3
    # the same order in numpy: non-negative doubles sort as their bit patterns
    v = np.array([0.0, 5e-324, 2.2e-308, 1.0, np.inf, 3.0, 1e-320])
    assert np.array_equal(np.argsort(v, kind="stable"), np.argsort(v.view(np.uint64), kind="stable"))


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_entries_are_declared_exported_and_loaded():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gingr_hip.h")).read(), flags=re.S)
    from gingr_amd import _native
    lib = ctypes.CDLL(_native.LIB_PATH)
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", text), f
        assert f in _native.SIGNATURES and hasattr(lib, f), f
    assert re.search(r"typedef struct gingr_robust_params\s*\{\s*int32_t loss;\s*int32_t scale_mode;\s*double scale;\s*double min_scale;", text)
    assert ctypes.sizeof(_native.RobustParams) == 24
    assert [n for n, _ in _native.RobustParams._fields_] == ["loss", "scale_mode", "scale", "min_scale"]
    srcs = open(os.path.join(ROOT, "gingr_amd", "csrc", "Makefile")).read()
    assert " robust_select.hip" in srcs and "robust_select_plan.h" in srcs


def test_configuration_and_keywords():
    import inspect
    import gingr_amd as ga
    from gingr_amd import api
    assert api.RobustLoss is ga.RobustLoss
    assert ga.PointToPlaneConfiguration().robust is None
    assert list(inspect.signature(ga.PointToPlaneConfiguration).parameters)[-1] == "robust"            # appended last
    assert ga.PointToPlaneConfiguration(100, 100.0, 1.0, 100.0, False, 1e-10).maxIterations == 100       # positional order unchanged
    sig = inspect.signature(ga.RobustLoss).parameters
    assert list(sig) == ["kind", "scale", "tuning", "minScale"]
    assert sig["scale"].default == "median" and sig["tuning"].default is None and sig["minScale"].default == 0.0
    assert ga.RobustLoss("cauchy").native == (1, 1, 2.385, 0.0)
    assert ga.RobustLoss("huber").native == (2, 1, 1.345, 0.0)
    assert ga.RobustLoss("tukey", minScale=0.5).native == (3, 1, 4.685, 0.5)
    assert ga.RobustLoss("tukey", tuning=3.0).native == (3, 1, 3.0, 0.0)
    assert ga.RobustLoss("cauchy", scale=1.5).native == (1, 0, 1.5, 0.0)
    for bad in (dict(kind="l2"), dict(kind="cauchy", scale=0.0), dict(kind="cauchy", scale=np.nan), dict(kind="cauchy", scale="mad"),
                dict(kind="huber", tuning=-1.0), dict(kind="huber", scale=2.0, tuning=1.0), dict(kind="huber", minScale=-1.0),
                dict(kind="huber", minScale=np.inf)):
        with pytest.raises(ValueError):
            ga.RobustLoss(**bad)
    assert cfg_with_loss().robust.kind == "cauchy"
    assert callable(ga.PointToPlaneIcpRegistration.robustWeights)
    assert list(inspect.signature(ga.Context.order_statistic).parameters) == ["self", "values", "k"]


def cfg_with_loss():
    import gingr_amd as ga
    return ga.PointToPlaneConfiguration(maxIterations=5, robust=ga.RobustLoss("cauchy"))
