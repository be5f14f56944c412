"""The 3 x 3 rotation step (gingr_amd/csrc/svd3.h: polar3_rotation, svd3, kabsch3_rotation, the Euler round trip and its one-wave forms)
on the device at its degenerate inputs, through the four callers and the public API only: PCA alignment (align_finish_kernel), rigid /
similarity ICP (icp_transform_kernel), classic rigid CPD (transform_finish_kernel) and the GiNGR update (post_pose_step).  The inputs
come from tests/rot3_cases.py; every case asserts its guard -- the branch it is built for, evaluated on the oracle's numbers alone.

Tolerances.  Well-conditioned cases (A, B, F outside the window, H, thickness 1e-2) use those of the sibling test of the same caller
(test_gpu_pca_model.py, test_gpu_rigid_icp.py, test_gpu_classic_cpd.py, test_gpu_parity.py), absolute ones multiplied for H by the
largest coordinate over the sibling's.  Ill-conditioned cases (thickness 1e-4, F at delta = 0.02 and inside the gimbal window) use 10 x the
oracle's own spread -- its largest change over 8 seeded perturbations of 2^-52 of its inputs (rot3_cases.oracle_spread), one decimal
digit for the different route, polar iteration against SVD -- where that exceeds the well-conditioned tolerance.  No tolerance depends
on device output.  Every case prints the oracle's spread and the device's deviation.

Left out on purpose: planar (D) and collinear (E) data through the rigid ICP and through the GiNGR update.  With a determinant at
rounding level scalismo's rule "det Sigma < 0" may return an improper matrix, which the Euler round trip then turns into an arbitrary
rotation: the reference is ill-posed there.  D and E run through the PCA alignment, where the aligned points are unique although the
rotation is not, and D through the classic CPD, whose det(U V^T) convention is well posed on planar data.

Measured on an MI355X (largest over the cases of a row; deviation and spread in the units of the bound):

caller       family              quantity      cases   spread  deviation    bound
pca          A B C-1e-2 D E H    aligned          41  1.5e-15    3.8e-15  6.2e-12   (of the largest coordinate)
pca          C-1e-4              aligned           4  1.2e-15    1.1e-15  6.2e-12
rigid icp    B C-1e-2            points            8  4.3e-14    1.7e-13  1.0e-09
rigid icp    B C-1e-2            R                 8  4.6e-16    5.6e-15  1.0e-11
rigid icp    B C-1e-2            scale             8  3.3e-16    4.4e-16  1.0e-11
rigid icp    C-1e-4              points            4  3.6e-14    7.1e-14  1.0e-09
rigid icp    C-1e-4              R                 4  4.4e-16    1.9e-15  1.0e-11
rigid icp    C-1e-4              scale             4  3.3e-16    2.2e-16  1.0e-11
rigid icp    C-1e-4              t                 4  5.8e-15    7.4e-15  1.0e-08
rigid icp    H                   points            8  1.2e-05    3.8e-06  2.4e-02   (absolute, at the scaled coordinates)
rigid icp    H                   R                 8  1.6e-12    4.5e-15  1.0e-11
rigid icp    H                   t                 8  1.3e-02    7.6e-06  2.4e-01
classic cpd  B C-1e-2 D          TY (relative)     6  3.5e-15    4.1e-15  1.0e-10
classic cpd  B C-1e-2 D          R                 6  1.2e-15    5.4e-15  1.0e-10
classic cpd  C-1e-4              TY (relative)     2  4.2e-15    1.6e-15  1.0e-10
classic cpd  C-1e-4              sigma2            2  5.3e-13    4.4e-13  2.2e-11
classic cpd  C-1e-4              R                 2  1.1e-15    2.0e-15  1.0e-10
update       A B                 fit (relative)   42  6.0e-15    4.5e-15  1.0e-08
update       A B                 sigma2 (rel.)    42  3.2e-11    1.3e-10  1.0e-08
update       A B                 R                42  1.1e-15    5.8e-15  1.0e-08
update       F delta 0           fit / R           4  3.3e-15 / 4.4e-16    2.1e-15 / 2.4e-15  1.0e-08
update       F delta 0.01        fit / R           4  4.0e-15 / 3.9e-16    2.2e-15 / 2.6e-15  1.0e-08
update       F delta 0.02        fit / R           4  1.4e-13 / 2.8e-14    1.3e-14 / 1.5e-14  1.0e-08
update       F (all)             sigma2 (rel.)    12  3.2e-11    1.3e-10  1.0e-08

Ten times the oracle's spread stayed below the well-conditioned tolerance in every ill-conditioned case, so that tolerance was the
bound everywhere; no case came within a factor 50 of its bound.
"""
import functools
import os

import numpy as np
import pytest

from oracle import gingr_oracle as go
from tests import pca_restatement as pr
from tests import rot3_cases as rc
from tests.pca_restatement import ROUTE_SPREAD

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL_PCA = 1000.0 * ROUTE_SPREAD                       # test_gpu_pca_model.py


def report(what, name, **rows):
    """rows: quantity -> (deviation, oracle spread, bound)"""
    print(f"{what} {name}: " + "; ".join(f"{k} dev {d:.2e} spread {s:.2e} bound {b:.2e}" for k, (d, s, b) in rows.items()))
    for k, (d, s, b) in rows.items():
        assert d <= b, (what, name, k, d, s, b)


# ------------------------------------------------------------------------------------------------------------- PCA alignment
@pytest.mark.parametrize("name", sorted(rc.pairs()))
def test_pca_alignment(ctx, name):
    """families A B C D E H: correspondence by index, any S exactly; the aligned shape against pr.align"""
    import gingr_amd as ga
    p = rc.pairs()[name]
    assert p.guard.holds(S=p.S), name
    ref, x = np.array(p.target), np.array(p.x)
    want, spread = rc.oracle_spread(lambda a, b: {"aligned": pr.align(a, b)}, (x, ref))
    dev = ga.PointDistributionModel.createUsingPCA(ctx, ref, np.stack([x, ref]), alignment="rigid")
    aligned = 2.0 * (dev.reference + dev.mean) - ref
    dev.device().close()
    scale = np.abs(np.stack([x, ref])).max()
    d = np.abs(aligned - want["aligned"]).max() / scale
    s = spread["aligned"] / scale
    report("pca", name, aligned=(d, s, rc.bound(TOL_PCA, s, p.ill)))


# ----------------------------------------------------------------------------------------------------------------- rigid ICP
@functools.lru_cache(maxsize=None)
def femur_scale():
    d = np.load(os.path.join(HERE, "golden", "inputs.npz"))
    return float(max(np.abs(d["femur"]).max(), np.abs(d["femur_target"]).max()))


ICP_SLABS = [n for n, s in rc.slabs().items() if s.guard.kind != "rank2"]


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", ICP_SLABS)
def test_rigid_icp(ctx, name, kind):
    """families B C H on lattice slabs; kind 1: the similarity scale, (d1 + d2 - d3) / var_x on the mirrored ones"""
    from gingr_amd import classic
    s = rc.slabs()[name]
    idx, _, _ = go.icp_closest_point(s.tpl, s.tgt)
    assert np.array_equal(idx, s.partner) and s.guard.holds(S=rc.cross_covariance(s.tpl, s.tgt[idx])), name

    def oracle(tpl, tgt):
        pts, dist, (sc, R, t) = go.rigid_icp_iteration(tpl, tgt, similarity=bool(kind))
        return {"points": pts, "dist": dist, "scale": sc, "R": R, "t": t}

    want, spread = rc.oracle_spread(oracle, (s.tpl, s.tgt))
    task = classic.ICPFactory(ctx, np.array(s.tpl), kind).registerRigidly(np.array(s.tgt))
    got, dist = task.Iteration()
    gs, gR, gt = task.transform()
    task.close()
    # absolute bounds of test_gpu_rigid_icp.py times (largest coordinate here / largest coordinate of its femur pair) for family H
    f = max(np.abs(s.tpl).max(), np.abs(s.tgt).max()) / femur_scale() if name.startswith("H-") else 1.0
    wd = float(want["dist"])
    report(f"icp kind {kind}", name,
           dist=(abs(dist - wd) / wd, spread["dist"] / wd, rc.bound(1e-11, spread["dist"] / wd, s.ill)),
           points=(np.abs(got - want["points"]).max(), spread["points"], rc.bound(1e-9 * f, spread["points"], s.ill)),
           scale=(abs(gs - float(want["scale"])), spread["scale"], rc.bound(1e-11, spread["scale"], s.ill)),
           R=(np.abs(gR - want["R"]).max(), spread["R"], rc.bound(1e-11, spread["R"], s.ill)),
           t=(np.abs(gt - want["t"]).max(), spread["t"], rc.bound(1e-8 * f, spread["t"], s.ill)))
    assert abs(np.linalg.det(gR) - 1) < 1e-12
    if kind == 0:
        assert gs == 1.0


# --------------------------------------------------------------------------------------------------------- classic rigid CPD
CPD_SLABS = [n for n, s in rc.slabs().items() if s.scale == 1.0]


@pytest.mark.parametrize("name", CPD_SLABS)
def test_classic_rigid_cpd(ctx, name):
    """families B C D: one Iteration from the template at variance 1 against go.classic_cpd_maximization_rigid"""
    from gingr_amd import classic as cl
    s = rc.slabs()[name]
    assert s.guard.holds(S=rc.classic_cpd_A(s)), name
    X, Y = np.array(s.tgt), np.array(s.tpl)
    want, spread = rc.oracle_spread(rc.classic_cpd_outputs, (X, Y))
    reg = cl.CPDFactory(ctx, Y, w=0.0).registerRigidly(X)
    gTY, gs2 = reg.Iteration(Y, 1.0)
    gs, gR, gt = reg.transform()
    reg.close()
    nTY = np.linalg.norm(want["TY"])
    os2 = float(want["sigma2"])
    report("classic cpd", name,
           TY=(np.linalg.norm(gTY - want["TY"]) / nTY, spread["TY"] * np.sqrt(gTY.size) / nTY,
               rc.bound(1e-10, spread["TY"] * np.sqrt(gTY.size) / nTY, s.ill)),
           sigma2=(abs(gs2 - os2), spread["sigma2"], rc.bound(1e-9 * abs(os2) + 1e-12, spread["sigma2"], s.ill)),
           scale=(abs(gs - float(want["scale"])), spread["scale"], rc.bound(1e-10, spread["scale"], s.ill)),
           R=(np.abs(gR - want["R"]).max(), spread["R"], rc.bound(1e-10, spread["R"], s.ill)),
           t=(np.abs(gt - want["t"]).max(), spread["t"], rc.bound(1e-8, spread["t"], s.ill)))
    assert abs(np.linalg.det(gR) - 1) < 1e-12


# ------------------------------------------------------------------------------------------------------------ the GiNGR update
def to_ga(mo):
    import gingr_amd as ga
    return ga.PointDistributionModel(mo.ref, mo.mean, mo.U, mo.lam)


def oracle_update(mo, target, st, flavour):
    if flavour == "cpd":
        return go.cpd_update(mo, target, st, w=0.0)
    return go.icp_update(mo, target, st, 1.0, 0.5, 5)[0]


def check_update(ctx, label, name, mo, target, make_state, flavour, transform, guard, ill):
    """one update on the device against the oracle's, both from make_state(model); the guards on the oracle's cross-covariance"""
    import gingr_amd as ga
    st0 = make_state(mo)
    S = rc.update_sigma_xy(mo, target, st0, flavour)
    for g in guard:
        assert g.holds(S=S, R=rc.svd_rotation(S)), (name, g, S)

    def oracle(ref, tgt):
        m = go.PDM(ref, mo.mean, mo.U, mo.lam)
        st = oracle_update(m, tgt, make_state(m), flavour)
        assert st.status == 0
        return {"fit": st.fit, "sigma2": st.sigma2, "scale": st.scale, "translation": st.translation, "R": go.euler_to_rot(*st.euler)}

    want, spread = rc.oracle_spread(oracle, (mo.ref, target))
    if flavour == "cpd":
        algo, cfg = ga.CpdRegistration(ctx), ga.CpdConfiguration(maxIterations=5, w=0.0, initialSigma=1.0)
    else:
        algo = ga.IcpRegistration(ctx)
        cfg = ga.IcpConfiguration(maxIterations=5, initialSigma=1.0, endSigma=0.5, correspondenceMethod="PointcloudClosestPoint")
    state = algo.createInitialState(to_ga(mo), target, cfg, transform=transform, initial_pose=(tuple(st0.euler), tuple(st0.translation)))
    assert np.linalg.norm(state.general.fit - st0.fit) <= 1e-13 * np.linalg.norm(st0.fit)
    g = algo.update(state).general
    algo.close()
    assert g.status == 0
    rot = g.modelParameters.rotation
    gR = go.euler_to_rot(rot.phi, rot.theta, rot.psi)
    nfit = np.linalg.norm(want["fit"])
    rms = np.sqrt(want["fit"].size)
    os2 = float(want["sigma2"])
    # test_gpu_parity.py: fit 1e-8 relative, sigma2 1e-8 relative, scale 1e-9, translation 1e-6, Euler angles 1e-8 (here: the matrix)
    report(label, name,
           fit=(np.linalg.norm(g.fit - want["fit"]) / nfit, spread["fit"] * rms / nfit, rc.bound(1e-8, spread["fit"] * rms / nfit, ill)),
           sigma2=(abs(g.sigma2 - os2) / os2, spread["sigma2"] / os2, rc.bound(1e-8, spread["sigma2"] / os2, ill)),
           scale=(abs(g.modelParameters.scale - float(want["scale"])), spread["scale"], rc.bound(1e-9, spread["scale"], ill)),
           translation=(np.abs(np.asarray(g.modelParameters.translation) - want["translation"]).max(), spread["translation"],
                        rc.bound(1e-6, spread["translation"], ill)),
           R=(np.abs(gR - want["R"]).max(), spread["R"], rc.bound(1e-8, spread["R"], ill)))


# (flavour, transform): everything for the CPD flavour with rigid transforms, a subset of family A for the other three
SUBSET_A = ("random0", "pi-x", "pi-random-axis", "phi-q2-psi-q3", "phi-q3-psi-q2")
UPDATE_A = [("cpd", go.RIGID_TRANSFORMS, n) for n in rc.rotations_A()] + \
           [(f, t, n) for f, t in (("cpd", go.SIMILARITY_TRANSFORMS), ("icp", go.RIGID_TRANSFORMS), ("icp", go.SIMILARITY_TRANSFORMS))
            for n in SUBSET_A]


@pytest.mark.parametrize("flavour,transform,name", UPDATE_A)
def test_update_returns_a_large_rotation(ctx, flavour, transform, name):
    """family A: a stiff model posed by R0, target the posed reference: the Umeyama step returns the state's total rotation"""
    R0 = rc.rotations_A()[name]
    mo = rc.stiff_model()
    target = rc.posed_target(mo, R0, rc.T0)
    check_update(ctx, f"update {flavour} transform {transform}", "A-" + name, mo, target,
                 lambda m: rc.state_at(m, 1.0, R0, rc.T0, transform), flavour, transform,
                 (rc.Guard("det+"), rc.Guard("euler", 0.3, 1.0)), False)


@pytest.mark.parametrize("flavour,transform", [("cpd", go.RIGID_TRANSFORMS), ("icp", go.SIMILARITY_TRANSFORMS)])
@pytest.mark.parametrize("name", sorted(rc.rotations_F()))
def test_update_near_gimbal_lock(ctx, name, flavour, transform):
    """family F: locked, inside the window, outside it with cos(theta) = 0.02.  The angles themselves are not compared: they are
    ill-conditioned near the lock, and that is no defect; the rotation matrix rebuilt from them is."""
    R0, guard, ill = rc.rotations_F()[name]
    mo = rc.stiff_model()
    target = rc.posed_target(mo, R0, rc.T0)
    check_update(ctx, f"update {flavour} transform {transform}", "F-" + name, mo, target,
                 lambda m: rc.state_at(m, 1.0, R0, rc.T0, transform, direct=True), flavour, transform, (rc.Guard("det+"), guard), ill)


@pytest.mark.parametrize("flavour", ["cpd", "icp"])
@pytest.mark.parametrize("transform", [go.RIGID_TRANSFORMS, go.SIMILARITY_TRANSFORMS])
def test_update_towards_a_mirrored_slab(ctx, transform, flavour):
    """family B: the posterior mean crosses the plane, det Sigma_xy < 0 in the oracle's update: svd3 with s3 = -1, and for similarity
    transforms the scale from d1 + d2 - d3"""
    mo, target = rc.mirror_model()
    check_update(ctx, f"update {flavour} transform {transform}", "B-mirror", mo, target,
                 lambda m: go.initial_state(m, 1.0, global_transformation=transform), flavour, transform, (rc.Guard("det-"),), False)
