"""Element-wise tests of the two CPD pair passes with exact-zero culling ON, at every kernel instance and arithmetic form.

The stateless `Context.cpd_stats` runs `cpd_colsum_kernel` / `cpd_rowstats_kernel` (gingr_amd/csrc/cpd_pairs.hip) without boxes,
so the dense-reference tests never see `PartWalk` with boxes, the MASKED tile loops, the FINE kernels or the `tile_bad`
exemption.  Here the statistics come out of the fitter (the only caller that culls): set_state -> one update -> get_cpd_stats,
which are the statistics of the evaluation at the state that was set, and are compared

  (1) bit for bit between GINGR_OPT_CULL = 0, culling with the plain kernels and culling with the FINE kernels, and
  (2) element by element with the strict C restatement `oracle.c_oracle.cpd_stats`.

`den` includes the outlier constant c on both sides: gingr_fitter_get_cpd_stats returns exchange segment 0, which
cpd_den_finalize_kernel overwrote with colsum + c, and oracle_cpd_stats stores den[j] = colsum + c as well.

Inputs are clustered clouds (seven boxes of half-width 6 on corners of a cube of side 200), so that whole tiles are certain to
be skipped, and the cluster sizes are off the 64 grid, so that tiles and 64-point quarters straddling two clusters give partly
set slot masks.  Which arithmetic form a case runs (norm expansion / plain differences / clamped differences) and whether
anything can be culled is asserted in numpy from the actual inputs with the kernels' own predicates (`regime_of`): a later
change of the thresholds in cpd_pairs.hip, cpd_plan.h or fastexp.h makes these tests fail instead of silently testing another branch.
"""
import functools

import numpy as np
import pytest

from oracle import c_oracle as co

pytestmark = pytest.mark.gpu

REL_STATS = 1e-10   # tests/test_gpu_parity.py: streaming sums against the float64 restatement
REL_SIGMA2 = 1e-9   # tests/test_gpu_parity.py: sigma2_next

SEP, HALF = 200.0, 6.0
# corners of the cube (the eighth stays empty) and the clusters' shares of a cloud: uneven, and chosen so that the centroid
# stays near the middle of the cube (the expansion predicate depends on the extent about the target centroid)
CORNERS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [1, 0, 1], [0, 1, 1]], dtype=np.float64)
SHARES = np.array([0.10, 0.11, 0.12, 0.13, 0.20, 0.19, 0.18])
SEED = 1

# (M fit, N target): the smallest shapes that select each instance (colsum_pt / rowstats_pt: thresholds 2048 and 16384), all off
# the 64 and 256 grids
SHAPES = [(1500, 1700),     # column sums <1, false>,      row statistics <1, false>
          (6000, 5500),     #             <2, false>,                     <2, false / true>
          (2341, 16584),    #             <4, false / true>,              <4, false / true>
          (16584, 2341)]    #             <2, false>,                     <4, false / true>

# name -> (sigma2, w, noise of the fit points)
REGIMES = {
    "expansion_culled": (SEP * SEP / 2200.0, 0.1, 0.3),
    "plain_culled": (1.0, 0.1, 0.3),
    "clamped_culled": (1e-5, 0.1, 0.002),
    "expansion_all_live": (400.0, 0.1, 0.3),     # the control: nothing can be culled
}
# name -> (norm expansion, clamped differences, tiles of other clusters are culled)
EXPECT = {
    "expansion_culled": (True, False, True),
    "plain_culled": (False, False, True),
    "plain_culled_w0": (False, False, True),
    "clamped_culled": (False, True, True),
    "expansion_all_live": (True, False, False),
}


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def maxrel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


def cluster_sizes(n):
    s = np.floor(SHARES / SHARES.sum() * n).astype(np.int64)
    s[-1] += n - s.sum()
    for k in range(len(s) - 1):     # no size on the 64 grid: a tile or a quarter then straddles two clusters
        if s[k] % 64 == 0:
            s[k] += 1
            s[k + 1] -= 1
    assert s.sum() == n and np.all(s > 0) and np.all(s % 64 != 0), s
    return s


def clustered(M, N, noise, seed=SEED):
    """targets: seven uniform boxes, shuffled; fit points: targets drawn with replacement plus normal(0, noise)"""
    rng = np.random.default_rng(seed)
    x = np.concatenate([SEP * CORNERS[k] + rng.uniform(-HALF, HALF, (n, 3)) for k, n in enumerate(cluster_sizes(N))])
    x = x[rng.permutation(N)]
    y = x[rng.integers(0, N, M)] + rng.normal(0, noise, (M, 3))
    return np.ascontiguousarray(y), np.ascontiguousarray(x)


def regime_of(fit, target, sigma2):
    """The wave-uniform choices of cpd_colsum_kernel / cpd_rowstats_kernel, restated.  aux[0] / aux[1] = largest |coordinate -
    target centroid| of the targets (cloud_absmax_kernel, fitter.hip set_target) and of the fit (tile_bbox_kernel with the same
    centre, fit_boxes_now / the fit sweep); c = fastexp_scale_for_variance<11>(2 sigma2)."""
    ctr = target.mean(axis=0)
    a_tgt, a_fit = float(np.abs(target - ctr).max()), float(np.abs(fit - ctr).max())
    negc = 2048.0 * 1.4426950408889634074 / (2.0 * sigma2)
    am = a_tgt + a_fit
    # use_expansion(fmax(aux0, aux1), c)
    expand = 3.0 * max(a_tgt, a_fit) ** 2 * negc * (0.69314718055994530942 / 2048.0) * 7.7e-16 < 1e-12
    # fastexp_needs_clamp(3 am^2, c)
    clamp = not (3.0 * am * am * negc < 2199023255552.0)
    # GINGR_CULL_SCALED(2048): a tile pair is skipped when box_gap2 * (-c) > 1084 * 2048.  Two clusters differ in at least one
    # coordinate, and on every axis the points sit either near 0 or near SEP: the smallest per-axis gap bounds every gap
    # between boxes of different clusters from below; 3 am^2 bounds every squared distance from above.
    pts = np.concatenate([fit, target])

    def side_gap(d):    # (a cloud that is no clustered one -- tests/test_gpu_fastexp.py -- has no two sides: no gap, nothing is culled)
        far, near = pts[:, d][pts[:, d] > SEP / 2], pts[:, d][pts[:, d] < SEP / 2]
        return float(far.min() - near.max()) if far.size and near.size else 0.0

    gap = min(side_gap(d) for d in range(3))
    culls_clusters = gap * gap * negc > 1084.0 * 2048.0
    culls_nothing = not (3.0 * am * am * negc > 1084.0 * 2048.0)
    return {"expand": expand, "clamp": clamp, "culls_clusters": culls_clusters, "culls_nothing": culls_nothing}


def check_regime(name, fit, target, sigma2):
    got = regime_of(fit, target, sigma2)
    expand, clamp, culls = EXPECT[name]
    assert got["expand"] == expand, (name, got)
    assert got["clamp"] == clamp, (name, got)
    assert got["culls_clusters"] == culls and got["culls_nothing"] == (not culls), (name, got)


@functools.lru_cache(maxsize=None)
def case(M, N, name):
    """inputs and the C reference of one (shape, regime), computed once; never modified"""
    sigma2, w, noise = REGIMES[name] if name in REGIMES else (0.25, 0.0, 0.3)
    y, x = clustered(M, N, noise)
    want = co.cpd_stats(y, x, sigma2, w)
    for a in (y, x, want.den, want.P1, want.PX, want.Pt1):
        a.setflags(write=False)
    return y, x, sigma2, w, want


OPTION_SETTINGS = (("cull off", 0, None), ("cull on, plain kernels", 1, 0), ("cull on, FINE kernels", 1, 1))


def run_fitter(fit_points, target, sigma2, w):
    """set_state -> update_cpd -> get_cpd_stats under each option setting, each in a context of its own.  The rank 4 model has the
    fit points as its reference shape and a zero mean, so the state (alpha = 0, identity pose) instantiates the fit points."""
    import gingr_amd as ga
    from gingr_amd import _native as nat
    from gingr_amd.sharded import ShardedFitter
    M = fit_points.shape[0]
    rng = np.random.default_rng(SEED + M)
    U, _ = np.linalg.qr(rng.normal(0, 1, (3 * M, 4)))
    model = ga.PointDistributionModel(np.array(fit_points), np.zeros((M, 3)), U, np.array([4.0, 3.0, 2.0, 1.0]))
    runs = []
    for label, cull, fine in OPTION_SETTINGS:
        c = ga.Context(0)
        try:
            c.set_option(nat.OPT_CULL, cull)
            if fine is not None:
                c.set_option(nat.OPT_FINE_CULL, fine)
                assert c.get_option(nat.OPT_FINE_CULL) == fine
            assert c.get_option(nat.OPT_CULL) == cull
            f = ShardedFitter(c, model, np.array(target))
            f.set_state(np.zeros(4), sigma2)
            _, _, fit0 = f.get_state()
            f.update_cpd(w, 1.0, 1)
            c.synchronize()
            stats = f.get_cpd_stats()
            # the three terms of sigma2_next, which ShardedFitter.get_cpd_stats leaves out: scalars6 = {Np, xPx, trPXY, yPy, ..}
            sc6 = np.empty(6)
            assert f._lib.gingr_fitter_get_cpd_stats(f.handle, None, None, None, nat.dptr(sc6)) == 0
            stats.update(xPx=float(sc6[1]), trPXY=float(sc6[2]), yPy=float(sc6[3]))
            alpha, sc, fit = f.get_state()
            runs.append({"label": label, "fit0": fit0, "stats": stats, "alpha": alpha.copy(), "fit": fit.copy(),
                         "sigma2": float(sc.sigma2), "status": int(sc.status)})
            f.close()
        finally:
            c.close()
    return runs


def assert_bit_identical(runs):
    a = runs[0]
    for b in runs[1:]:
        assert np.array_equal(a["fit0"], b["fit0"]), b["label"]
        for k in ("den", "P1", "PX"):
            assert np.array_equal(a["stats"][k], b["stats"][k], equal_nan=True), (k, b["label"])
        for k in ("Np", "sigma2_next", "c", "xPx", "trPXY", "yPy"):
            assert np.array_equal(a["stats"][k], b["stats"][k], equal_nan=True), (k, b["label"], a["stats"][k], b["stats"][k])
        assert a["status"] == b["status"], b["label"]
        assert np.array_equal(a["fit"], b["fit"], equal_nan=True) and np.array_equal(a["alpha"], b["alpha"], equal_nan=True), b["label"]
        assert np.array_equal(a["sigma2"], b["sigma2"], equal_nan=True), b["label"]


# every shape in every regime; "plain_culled_w0" is plain differences at sigma2 = 0.25 with w = 0 (no outlier constant under den)
CASES = [(M, N, name) for (M, N) in SHAPES for name in list(REGIMES) + ["plain_culled_w0"]]


# sigma2_next: |C restatement - dense restatement| / dense on the same input, where that exceeds the 1e-9 bound
REFERENCES_DIFFER = {(16584, 2341, "plain_culled_w0"): 1.28e-9}


def sigma2_next_terms(fit, target, want):
    """xPx, trPXY, yPy of sigma2_next = (xPx - 2 trPXY + yPy) / (3 Np) from the reference's statistics (oracle_cpd_stats forms them
    the same way), and the condition number kappa of their combination"""
    xPx = float(np.sum(want.Pt1 * np.sum(target * target, axis=1)))
    yPy = float(np.sum(want.P1 * np.sum(fit * fit, axis=1)))
    trPXY = float(np.sum(fit * want.PX))
    return {"xPx": xPx, "trPXY": trPXY, "yPy": yPy}, (xPx + 2.0 * abs(trPXY) + yPy) / abs(xPx - 2.0 * trPXY + yPy)


@pytest.mark.parametrize("M,N,name", CASES, ids=[f"{M}x{N}-{name}" for M, N, name in CASES])
def test_culled_pair_passes_bitwise_and_against_c_reference(M, N, name):
    """Bounds: REL_STATS = 1e-10 on den and P1 (largest relative error over ALL elements), PX (norm), Np and each of the three terms
    xPx, trPXY, yPy of sigma2_next, in every regime -- the clamped one (sigma2 = 1e-5, |ln K| up to 745 before the flush) included:
    fastexp.h bounds the error of one K by the polynomial's 2.02e-13 plus |ln K| 2^-53 for the rounded product (twice that at
    worst in round-down mode), and only pairs with |ln K| of a few tens can matter at 1e-10 of a sum, i.e. another ~1e-14.
    Measured on an MI355X over the cases of this test: den <= 3.2e-13, P1 <= 3.7e-13, PX <= 1.2e-13, Np, xPx, trPXY, yPy <= 8.5e-14
    (<= 1e-15 in the difference forms); the clamped regime is no worse than the others (den 2.03e-13, P1 3.6e-13).

    sigma2_next = (xPx - 2 trPXY + yPy) / (3 Np) is the reference's expanded form (CPD.scala:133-147) on both sides, and ANY
    float64 evaluation of it loses a factor kappa = (xPx + 2 |trPXY| + yPy) / |xPx - 2 trPXY + yPy| to cancellation: the terms are
    of the order of Np SEP^2, their combination of the order of Np noise^2 (kappa is printed with the figures: 4e3 to 6e5 with
    noise 0.3, 2e10 with noise 0.002).  Its bound is 1e-9 wherever the reference itself is determined that well, measured as the
    difference between oracle.c_oracle.cpd_stats and oracle.gingr_oracle.cpd_stats_dense on the same input (den, P1, PX and Np
    of the two agree to 5e-16 everywhere).  It is not in two places, and there the bound comes from the references alone:
      * the clamped regime: on the 1500 x 1700 input the two references differ by 1.0e-5 in sigma2_next (kappa 2.1e10, i.e. 4 kappa
        2^-53).  No term of fastexp.h is involved: it is the rounding of the three sums, sqrt(n) 2^-53 each in the usual
        probabilistic model, n = max(M, N).  Bound: 10 kappa sqrt(n) 2^-53 (1e-3 to 4e-3; measured 3.8e-6 to 4.3e-5).  What that
        width no longer sees, the separate 1e-10 bounds on xPx, trPXY and yPy do.
      * w = 0 at 16584 x 2341 (kappa 5.9e5, the largest outside the clamped regime): the two references differ by 1.28e-9 in
        sigma2_next (1.1e-10 at 1500 x 1700, 4.7e-11 at 6000 x 5500, where 1e-9 stays).  Bound: ten times that difference; measured
        1.41e-9, with xPx, trPXY and yPy each within 9e-16 of the reference -- rounding of the last digits of the terms times kappa,
        nothing the kernels could do better.
    The bit identity of sigma2_next and of its terms across the kernel variants is asserted everywhere."""
    y, x, sigma2, w, want = case(M, N, name)
    check_regime(name, y, x, sigma2)
    # the condition under which a largest relative error over all elements means something (nothing is masked out)
    assert want.P1.min() > 1e-3 and want.den.min() > 1e-12, (want.P1.min(), want.den.min())
    runs = run_fitter(y, x, sigma2, w)
    assert np.array_equal(runs[0]["fit0"], y)       # the zero state instantiates the reference shape bit for bit
    got = runs[0]["stats"]
    terms, kappa = sigma2_next_terms(y, x, want)
    figures = {"den": maxrel(got["den"], want.den), "P1": maxrel(got["P1"], want.P1), "PX": rel(got["PX"], want.PX),
               "Np": abs(got["Np"] - want.Np) / abs(want.Np),
               "xPx": abs(got["xPx"] - terms["xPx"]) / abs(terms["xPx"]),
               "trPXY": abs(got["trPXY"] - terms["trPXY"]) / abs(terms["trPXY"]),
               "yPy": abs(got["yPy"] - terms["yPy"]) / abs(terms["yPy"]),
               "sigma2_next": abs(got["sigma2_next"] - want.sigma2_next) / abs(want.sigma2_next)}
    print(f"\n{M}x{N} {name}: " + " ".join(f"{k} {v:.3e}" for k, v in figures.items()) +
          f" | sigma2_next {want.sigma2_next:.6e} kappa {kappa:.2e} status {runs[0]['status']}")
    assert_bit_identical(runs)
    assert figures["den"] < REL_STATS, figures
    assert figures["P1"] < REL_STATS, figures
    assert figures["PX"] < REL_STATS, figures
    assert figures["Np"] <= REL_STATS, figures
    assert max(figures["xPx"], figures["trPXY"], figures["yPy"]) <= REL_STATS, figures
    bound = REL_SIGMA2
    if name == "clamped_culled":
        bound = 10.0 * kappa * np.sqrt(max(M, N)) * 2.0 ** -53
    elif (M, N, name) in REFERENCES_DIFFER:
        bound = 10.0 * REFERENCES_DIFFER[(M, N, name)]
    assert figures["sigma2_next"] <= bound, (figures, kappa, bound)


@pytest.mark.parametrize("M,N", [(6000, 5500), (2341, 16584)])
def test_deep_tail_columns_are_computed_not_culled(M, N):
    """The margin of the culling constant from below.  900 extra targets without fit points sit 31 to 32 in front of a face of
    the first cluster, w = 0, sigma2 = 1: every K of theirs is between exp(-480) and the flush at exp(-745), so their den is
    ~1e-210 to 1e-260 -- normal doubles that only a walk which still visits box pairs 31 apart can produce (box_gap2 * (-c) is
    ~0.64 of GINGR_CULL_SCALED there; a constant of 600 instead of 1084 skips them and den becomes 0).  Each of those columns
    has Pt1 = 1, so P1 and PX of the fit points at that face depend on them as well.  Bounds as everywhere: |ln K| 2^-52 (round-down mode: at
    worst twice the header's 2^-53) for the rounded product is 1.6e-13 at |ln K| = 745, next to the polynomial's 2.02e-13."""
    sigma2, w = 1.0, 0.0
    y, x0 = clustered(M, N, 0.3)
    rng = np.random.default_rng(SEED + 7)
    face = float(min(y[:, 0].min(), x0[:, 0].min()))
    ghosts = np.stack([rng.uniform(face - 32.0, face - 31.0, 900), rng.uniform(-1, 1, 900), rng.uniform(-1, 1, 900)], axis=1)
    x = np.ascontiguousarray(np.concatenate([x0, ghosts]))
    negc = 2048.0 * 1.4426950408889634074 / (2.0 * sigma2)
    gap = face - float(ghosts[:, 0].max())
    assert 600.0 * 2048.0 < 0.9 * gap * gap * negc and 1.1 * gap * gap * negc < 1084.0 * 2048.0
    reg = regime_of(y, x, sigma2)
    assert not reg["expand"] and not reg["clamp"] and reg["culls_clusters"], reg
    want = co.cpd_stats(y, x, sigma2, w)
    tail = want.den[N:]
    assert 1e-290 < tail.min() and tail.max() < 1e-200, (tail.min(), tail.max())
    assert want.P1.min() > 1e-3 and want.den[:N].min() > 1e-12
    runs = run_fitter(y, x, sigma2, w)
    got = runs[0]["stats"]
    figures = {"den": maxrel(got["den"], want.den), "P1": maxrel(got["P1"], want.P1), "PX": rel(got["PX"], want.PX),
               "Np": abs(got["Np"] - want.Np) / abs(want.Np)}
    print(f"\n{M}x{N} deep tail: " + " ".join(f"{k} {v:.3e}" for k, v in figures.items()) + f" | tail den {tail.min():.2e}..{tail.max():.2e}")
    assert_bit_identical(runs)
    assert np.array_equal(runs[0]["fit0"], y)
    assert max(figures.values()) < REL_STATS, figures


def test_underflowed_column_stays_nan_under_culling():
    """w = 0 and one target far from every fit point: the reference has den = 0 there and, through 0 * (1 / 0), NaN in every P1
    (CPD.scala:66,71-74).  The far target's tile must not be culled away (tile_bad), with the PT = 4 kernels, plain and FINE."""
    y, x0, sigma2, w = clustered(2341, 16584, 0.3) + (1.0, 0.0)
    x = np.concatenate([x0, [[1e4, 1e4, 1e4]]])
    reg = regime_of(y, x, sigma2)       # the far target stretches the extent: still plain differences, unclamped
    assert not reg["expand"] and not reg["clamp"] and reg["culls_clusters"], reg
    want = co.cpd_stats(y, x, sigma2, w)
    assert want.den[-1] == 0.0 and np.all(np.isnan(want.P1))
    runs = run_fitter(y, x, sigma2, w)
    for r in runs:
        assert r["stats"]["den"][-1] == 0.0, r["label"]
        assert np.all(np.isnan(r["stats"]["P1"])), r["label"]
        assert maxrel(r["stats"]["den"][:-1], want.den[:-1]) < REL_STATS, r["label"]
    assert_bit_identical(runs)


def test_stateless_stats_at_a_four_points_per_thread_shape(ctx):
    """The stateless path (no boxes) at the smallest shape that runs <4, false> in both passes: every element against the C
    reference (the 50k / 100k tests sample 16 to 48 rows)."""
    y, x, sigma2, w, want = case(2341, 16584, "plain_culled")
    got = ctx.cpd_stats(y, x, sigma2, w)
    assert maxrel(got["den"], want.den) < REL_STATS
    assert maxrel(got["P1"], want.P1) < REL_STATS
    assert rel(got["PX"], want.PX) < REL_STATS
    assert maxrel(got["Pt1"], want.Pt1) < REL_STATS
    assert abs(got["Np"] - want.Np) <= REL_STATS * abs(want.Np)
    assert abs(got["sigma2_next"] - want.sigma2_next) <= REL_SIGMA2 * abs(want.sigma2_next)
