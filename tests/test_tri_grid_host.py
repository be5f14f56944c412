"""CPU pins of the target-triangle grid's host side (gingr_amd/csrc/tri_grid_plan.h), compiled for the host with the address and
undefined-behaviour sanitizers into a stand-alone driver (tests/c/tri_grid_plan_driver.cpp):

1. the clamped cell index -- the one expression the binning and every grid kernel evaluate -- at values that follow from its definition;
2. the plan of a mesh has the properties the grid searches rely on (checked with numpy from the plan's own geometry; the binning is not
   restated): every finite triangle listed once, in the cell of its box's lower corner, ascending inside a cell, spans as measured,
   the wide ones in the short list, records equal to the triangles, and every triangle whose box meets a ball found in the cells the
   searches scan for that ball."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.tri_grid_cases import sheet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if CXX is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("tri_grid") / "tri_grid_plan_driver"
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "gingr_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c", "tri_grid_plan_driver.cpp"), "-o", str(exe)])
    return str(exe)


def cell_of(driver, x, lo, inv_h, gd):
    x = np.asarray(x, dtype=np.float64)
    rows = np.stack(np.broadcast_arrays(x, np.float64(lo), np.float64(inv_h), np.float64(gd)), -1).reshape(-1, 4)
    out = subprocess.run([driver, "cell"], input=np.ascontiguousarray(rows).tobytes(), capture_output=True, check=True).stdout
    return np.frombuffer(out, dtype=np.int64).reshape(x.shape)


def plan(driver, v, tri, orig=None):
    n, T = v.shape[0], tri.shape[0]
    raw = np.array([n, T, orig is not None], dtype=np.int64).tobytes() + np.ascontiguousarray(v.T, dtype=np.float64).tobytes() + \
        np.ascontiguousarray(tri, dtype=np.int32).tobytes() + (b"" if orig is None else np.ascontiguousarray(orig, dtype=np.int32).tobytes())
    out = subprocess.run([driver, "plan"], input=raw, capture_output=True, check=True).stdout
    ints, reals = np.frombuffer(out, dtype=np.int64, count=13), np.frombuffer(out, dtype=np.float64, count=5, offset=104)
    p = dict(ready=bool(ints[0]), max_span=int(ints[1]), rec=int(ints[2]), g=ints[3:6], span=ints[6:9], n_listed=int(ints[9]),
             n_big=int(ints[10]), lo=reals[:3], h=float(reals[3]), inv_h=float(reals[4]))
    if not p["ready"]:
        assert len(out) == 144
        return p
    ns, nl = int(ints[11]), int(ints[12])
    at = 144
    p["start"] = np.frombuffer(out, dtype=np.int32, count=ns, offset=at)
    at += 4 * ns
    p["list"] = np.frombuffer(out, dtype=np.int32, count=nl, offset=at)
    at += 4 * nl
    p["boxes"] = np.frombuffer(out[at:at + 48 * nl], dtype=np.float64).reshape(nl, 6)
    at += 48 * nl
    p["recs"] = np.frombuffer(out[at:at + 8 * p["rec"] * nl], dtype=np.float64).reshape(nl, p["rec"])
    assert at + 8 * p["rec"] * nl == len(out)
    return p


def check_plan(driver, v, tri, orig, seed):
    p = plan(driver, v, tri, orig)
    assert p["ready"] and p["rec"] == 10
    g, span, lo, inv_h = p["g"], p["span"], p["lo"], p["inv_h"]
    n_listed, n_big = p["n_listed"], p["n_big"]
    total = n_listed + n_big
    corners = v[tri]                                                   # (T, 3 corners, 3 axes)
    finite = np.isfinite(corners).all((1, 2))
    box_lo, box_hi = corners.min(1), corners.max(1)
    assert p["h"] > 0.0 and inv_h == 1.0 / p["h"] and np.all(g >= 1) and p["start"].shape[0] == g.prod() + 1
    assert p["start"][0] == 0 and p["start"][-1] == n_listed and np.all(np.diff(p["start"]) >= 0)
    # a permutation of exactly the triangles with finite corners
    lst = p["list"][:total]
    assert np.array_equal(np.sort(lst), np.flatnonzero(finite))
    # every listed entry sits in the cell of its box's lower corner, by the shared clamped floor
    with np.errstate(invalid="ignore"):
        ca = np.stack([cell_of(driver, box_lo[:, d], lo[d], inv_h, g[d]) for d in range(3)], 1)      # (T, 3)
        cb = np.stack([cell_of(driver, box_hi[:, d], lo[d], inv_h, g[d]) for d in range(3)], 1)
    home = np.searchsorted(p["start"], np.arange(n_listed), side="right") - 1
    listed = lst[:n_listed]
    assert np.array_equal(home, (ca[listed, 2] * g[1] + ca[listed, 1]) * g[0] + ca[listed, 0])
    # positions ascend inside a cell
    same_cell = home[1:] == home[:-1]
    assert np.all(listed[1:][same_cell] > listed[:-1][same_cell])
    # span[d] = the largest cell extent among the listed triangles; the short list = exactly the triangles wider than the limit
    extent = cb - ca
    wide = finite & (extent > p["max_span"]).any(1)
    assert np.array_equal(np.sort(lst[n_listed:]), np.flatnonzero(wide)) and n_big == wide.sum()
    assert np.array_equal(span, extent[listed].max(0) if n_listed else np.zeros(3, dtype=np.int64))
    # each entry's box and nine corner doubles are its triangle's; the tenth packs original << 32 | position
    assert np.array_equal(p["boxes"][:total], np.concatenate([box_lo[lst], box_hi[lst]], 1))
    assert np.array_equal(p["recs"][:total, :9], corners[lst].reshape(-1, 9))
    meta = p["recs"][:total, 9].copy().view(np.uint64)
    want_orig = lst if orig is None else orig[lst]
    assert np.array_equal(meta, (want_orig.astype(np.uint64) << np.uint64(32)) | lst.astype(np.uint64))
    # 200 random balls: every triangle whose box meets the ball is listed in the cells [c0 - span, c1], or is in the short list
    rng = np.random.default_rng(seed)
    vf = v[np.isfinite(v).all(1)]
    ext = float((vf.max(0) - vf.min(0)).max())
    centres = rng.uniform(vf.min(0) - 0.3 * ext, vf.max(0) + 0.3 * ext, (200, 3))
    radii = ext * 10.0 ** rng.uniform(-2.5, -0.3, 200)
    c0 = np.stack([cell_of(driver, centres[:, d] - radii, lo[d], inv_h, g[d]) for d in range(3)], 1)  # (200, 3)
    c1 = np.stack([cell_of(driver, centres[:, d] + radii, lo[d], inv_h, g[d]) for d in range(3)], 1)
    hx = np.stack([home % g[0], (home // g[0]) % g[1], home // (g[0] * g[1])], 1)                    # (n_listed, 3)
    in_short = np.zeros(tri.shape[0], dtype=bool)
    in_short[lst[n_listed:]] = True
    met = 0
    for k in range(200):
        gap = np.maximum(np.maximum(box_lo - centres[k], centres[k] - box_hi), 0.0)
        meets = finite & ((gap * gap).sum(1) <= radii[k] * radii[k])
        scanned = np.zeros(tri.shape[0], dtype=bool)
        scanned[listed[np.all((hx >= np.maximum(c0[k] - span, 0)) & (hx <= c1[k]), 1)]] = True
        assert np.all(scanned[meets] | in_short[meets]), k
        met += int(meets.sum())
    assert met > 200                                                    # the balls do meet triangles
    return p


def wide_sheet():
    v, tri = sheet()
    idx = np.arange(169).reshape(13, 13)
    extra = np.array([[idx[0, 0], idx[6, 0], idx[0, 6]], [idx[12, 12], idx[5, 12], idx[12, 4]], [idx[2, 3], idx[9, 4], idx[3, 10]],
                      [idx[0, 12], idx[0, 5], idx[1, 12]], [idx[6, 6], idx[12, 6], idx[6, 7]]], dtype=np.int32)
    return v, np.concatenate([tri[:100], extra[:2], tri[100:], extra[2:]])


def test_plan_of_a_bumpy_sheet(driver):
    v, tri = sheet()
    assert tri.shape == (288, 3)
    p = check_plan(driver, v, tri, None, 1)
    assert p["n_listed"] == 288 and p["n_big"] == 0 and np.all(p["g"] > 1)


def test_plan_of_a_flat_sheet_has_one_layer_of_cells(driver):
    v, tri = sheet(bumpy=False)
    p = check_plan(driver, v, tri, np.random.default_rng(5).permutation(288).astype(np.int32), 2)
    assert p["g"][2] == 1 and p["span"][2] == 0 and p["n_listed"] == 288


def test_plan_with_five_wide_triangles(driver):
    v, tri = wide_sheet()
    p = check_plan(driver, v, tri, np.random.default_rng(6).permutation(293).astype(np.int32), 3)
    assert p["n_big"] == 5 and p["n_listed"] == 288


def test_plan_skips_triangles_with_a_non_finite_corner(driver):
    v, tri = sheet()
    v = v.copy()
    v[84, 1] = np.inf                                                   # an inner vertex: six triangles
    p = check_plan(driver, v, tri, None, 4)
    assert p["n_listed"] + p["n_big"] == 288 - 6


def test_no_grid_when_all_vertices_are_equal(driver):
    v, tri = sheet()
    assert not plan(driver, np.full_like(v, 0.25), tri)["ready"]
    assert not plan(driver, np.full_like(v, np.nan), tri)["ready"]     # no finite triangle at all


def test_no_grid_when_more_than_256_triangles_are_wide(driver):
    v, tri = sheet(n=65)                                                # 8192 triangles of extent 1 / 64: a fine grid
    rng = np.random.default_rng(7)
    idx = np.arange(65 * 65).reshape(65, 65)

    def long_ones(k):                                                   # triangles across half the sheet: dozens of cells wide
        i, j = rng.integers(0, 32, k), rng.integers(0, 32, k)
        return np.stack([idx[i, j], idx[i + 32, j], idx[i, j + 32]], 1).astype(np.int32)

    p = check_plan(driver, v, np.concatenate([tri, long_ones(256)]), None, 8)
    assert p["n_big"] == 256                                            # the limit itself still gives a grid
    assert not plan(driver, v, np.concatenate([tri, long_ones(257)]))["ready"]


def test_clamped_cell(driver):
    inf, nan = np.inf, np.nan
    # lo = 1, h = 1 / 4, eight cells: [1, 1.25) is cell 0, ..., [2.75, 3) is cell 7 (all of it exact in binary)
    x = np.array([0.5, 1.0, 1.2, 1.25, 1.6, 2.74, 2.75, 2.99, 3.0, 100.0, 1e300, inf, -inf, nan, -1e300])
    want = np.array([0, 0, 0, 1, 2, 6, 7, 7, 7, 7, 7, 7, 0, 0, 0])
    assert np.array_equal(cell_of(driver, x, 1.0, 4.0, 8), want)
    assert np.array_equal(cell_of(driver, x, 1.0, 4.0, 1), np.zeros_like(want))                      # one cell: always cell 0
    # an infinite or undefined scale (the degenerate grids never get here; the kernels' flags do): still inside [0, gd - 1]
    assert np.array_equal(cell_of(driver, np.array([0.0, 2.0, 1.0]), 1.0, inf, 8), np.array([0, 7, 0]))   # (1 - 1) * inf is NaN
