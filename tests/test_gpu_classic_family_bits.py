"""The bits of the classic family (classic CPD dense and low-rank, BCPD, dense and sparse N-ICP, rigid ICP) against
tests/golden/classic_family_bits.npz, recorded from a build of the commit before the family's shared pieces got one home each
(cloud_sums.h, upload_cloud / download_cloud, nicp_dense.hip).  Every path here adds in a fixed order, so a refactor that keeps the
operations keeps every bit.  The clouds are those of test_gpu_bcpd.unchanged_inputs (M = 300, N = 257: no multiple of 64 or 256, live
padding rows in the 64-wide Cholesky, two chunks in both BCPD pair passes); the N-ICP mesh has 150 vertices (A: 600 unknowns)."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import bcpd_restatement as br
from tests.test_gpu_bcpd import unchanged_inputs
from tests.test_gpu_nicp import sphere_mesh
from tests.test_gpu_nicp_sparse import create, step

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "classic_family_bits.npz")
LOWRANK_TOLERANCE = 0.05  # the pivoted Cholesky of this template's kernel (beta = 6) passes it near 135 columns: three column blocks


@functools.lru_cache(maxsize=None)
def nicp_task():
    """a closed mesh, a moved copy of it as closest points, weights with zeros, three landmarks"""
    from gingr_amd import classic as cl
    v, tris = sphere_mesh(150, 21)
    rng = np.random.default_rng(77)
    cp = 1.04 * v + np.array([0.4, -0.3, 0.2]) + rng.normal(0, 0.3, v.shape)
    w = np.ones(150)
    w[rng.permutation(150)[:40]] = 0.0
    ids = np.array([5, 61, 140], dtype=np.int32)
    ul = cp[ids] + rng.normal(0, 0.2, (3, 3))
    return v, cl.nicp_edges(tris), w, cp, ids, ul


def family_results(ctx):
    """what tests/golden/classic_family_bits.npz records"""
    from gingr_amd import classic as cl
    from gingr_amd._native import dptr, iptr
    Y, X = unchanged_inputs()
    out = {}
    factory = cl.CPDFactory(ctx, Y, lambda_=2.0, beta=6.0, w=0.1)
    for kind, name, low in ((cl.RIGID, "cpd_rigid", None), (cl.AFFINE, "cpd_affine", None), (cl.NONRIGID, "cpd_nonrigid", None),
                            (cl.NONRIGID, "cpd_lowrank", cl.LowRankG(LOWRANK_TOLERANCE))):
        reg = cl.RigidCPD(factory, X, kind, low)
        try:
            for _ in range(3):
                ty, s2 = reg.Iteration()
            out[name + "_ty"], out[name + "_sigma2"] = ty, np.array([s2])
            if low is None:
                s, L, t = reg.transform()
                out[name + "_transform"] = np.concatenate([[s], L.reshape(9), t])
            else:
                assert 64 < reg.lowRankInfo["columns"] < 300
                out[name + "_columns"] = np.array([reg.lowRankInfo["columns"]])
            if kind == cl.NONRIGID:
                out[name + "_W"] = reg.W()
        finally:
            reg.close()
    for w, name in ((0.0, "bcpd_w0"), (0.1, "bcpd_w01")):
        reg = cl.BCPD(ctx, Y, X, w=w, lambda_=br.PARAMS["lambda_"], gamma=br.PARAMS["gamma"], k=br.PARAMS["kappa"], beta=6.0)
        try:
            for _ in range(3):
                reg.Iteration()
            for k, v in reg.state().items():
                out[name + "_" + k] = np.asarray(v, dtype=float)
        finally:
            reg.close()
    v, edges, w, cp, ids, ul = nicp_task()
    for kind, name in ((0, "nicp_t"), (1, "nicp_a")):
        moved, lm = np.empty_like(v), np.empty((3, 3))
        rc = ctx._lib.gingr_nicp_solve(ctx.handle, kind, v.shape[0], dptr(v), edges.shape[0], iptr(edges), dptr(w), dptr(cp), 3, iptr(ids),
                                       dptr(ul), 10.0, 4.0, 0.7, dptr(moved), dptr(lm))
        assert rc == 0, ctx._lib.gingr_last_error(ctx.handle)
        out[name + "_dense_points"], out[name + "_dense_landmarks"] = moved, lm
        rc, h = create(ctx, kind, v.shape[0], edges, ids)
        assert rc == 0
        try:
            rc, moved, lm, _ = step(ctx, h, v.shape[0], v, w, cp, ul, 10.0, 4.0, 0.7, n_lm=3)
            assert rc == 0, ctx._lib.gingr_last_error(ctx.handle)
            out[name + "_sparse_points"] = moved
        finally:
            ctx._lib.gingr_nicp_destroy(h)
    for registrator, name in ((cl.RIGID_REGISTRATOR, "icp_rigid"), (cl.AFFINE_REGISTRATOR, "icp_similarity")):
        task = cl.ICPFactory(ctx, Y, registrator).registerRigidly(X)
        try:
            d = np.empty(3)
            rc = ctx._lib.gingr_rigid_icp_iterate(task._h, 3, dptr(d))
            assert rc == 0, ctx._lib.gingr_last_error(ctx.handle)
            s, R, t = task.transform()
            out[name + "_points"], out[name + "_distances"] = task.points(), d
            out[name + "_transform"] = np.concatenate([[s], R.reshape(9), t])
        finally:
            task.close()
    return out


def test_the_classic_family_keeps_its_bits(ctx):
    want = np.load(GOLDEN)
    got = family_results(ctx)
    assert sorted(want.files) == sorted(got)
    for k in want.files:
        assert np.array_equal(want[k], got[k], equal_nan=False), k
