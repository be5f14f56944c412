"""Inputs, references and guards of the BCPD edge tests (tests/test_gpu_bcpd_edges.py; the guards alone: tests/test_bcpd_host.py).
Everything here comes from the numpy restatement (tests/bcpd_restatement.py): no device, and nothing is modified after it is built."""
import functools
from dataclasses import replace

import numpy as np

from tests import bcpd_restatement as br

BASE = dict(w=0.1, beta=1.5, **br.PARAMS)

# ------------------------------------------------------------------------------------------------------------ size edges
# (M, N): (Mp, padded rows, 64-row blocks nb, chunks of the column pass, chunks of the row pass) -- what the shape is there for
SIZE_EDGES = {
    (64, 64): (64, 0, 1, 1, 1),            # no padding, nb = 1
    (63, 300): (64, 1, 1, 1, 2),           # one padded row; two row-pass chunks
    (65, 255): (128, 63, 2, 1, 1),         # 63 padded rows; N one short of a tile
    (256, 256): (256, 0, 4, 1, 1),         # both clouds fill their owner tile exactly
    (255, 257): (256, 1, 4, 1, 2),         # one short of / one past the owner tile
    (257, 255): (320, 63, 5, 2, 1),        # the other way round; a column chunk of one row
    (320, 513): (320, 0, 5, 2, 3),         # no padding past one block; a row chunk of one point
    (576, 700): (576, 0, 9, 3, 3),         # three chunks in both passes
    (1025, 300): (1088, 63, 17, 5, 2),     # five column chunks, the last of one row
    (5, 40): (64, 59, 1, 1, 1),            # fewer rows than the 16 lanes of one row group
    (17, 1000): (64, 47, 1, 1, 4),         # one row past a row group; four row chunks
}
# the shapes whose chunks are longer than one tile: (M, N): {pass: (count, length)}
MULTI_TILE = {
    (64, 65537): {"row": (129, 512)},                               # N <= 65536 never gives a two-tile chunk; the last chunk holds one point
    (513, 130817): {"col": (2, 512), "row": (256, 512)},            # the smallest N at which M = 513 gives a two-tile column chunk
}
STARTS = ("initial", "crafted")


def chunks(M, N):
    """{pass: (count, length)} as the handle plans them"""
    return {"col": br.plan_chunks(N, M), "row": br.plan_chunks(M, N)}


def size_guard(M, N):
    plan = chunks(M, N)
    assert br.padded(M) + (plan["col"][0], plan["row"][0]) == SIZE_EDGES[(M, N)], (M, N, br.padded(M), plan)
    assert plan["col"][1] == plan["row"][1] == br.TILE, (M, N, plan)             # the multi-tile chunks are MULTI_TILE's business


def multi_tile_guard(M, N):
    plan = chunks(M, N)
    for which, want in MULTI_TILE[(M, N)].items():
        assert plan[which] == want, (M, N, which, plan)
        assert want[1] == 2 * br.TILE


@functools.lru_cache(maxsize=None)
def cloud_problem(M, N, w):
    y, x = br.cloud_case(M, N, seed=1000 + M)
    return br.Problem(y, x, **{**BASE, "w": w})


@functools.lru_cache(maxsize=None)
def cloud_state(M, N, w, start):
    p = cloud_problem(M, N, w)
    return p.initial() if start == "initial" else br.crafted_state(p, seed=M + N)


@functools.lru_cache(maxsize=None)
def cloud_reference(M, N, w, start):
    return cloud_problem(M, N, w).iterate(cloud_state(M, N, w, start))


# ---------------------------------------------------------------------------------------------------------- clamp branch
FAR, FAR_INDEX = 1e6, 17
CLAMP_CASES = ("far_target", "far_row", "unmoved")


@functools.lru_cache(maxsize=None)
def clamp_case(which):
    """(problem, state, reference): g6, w = 0.1, from the restatement's state after 10 iterations; far_target: x[17] += 1e6;
    far_row: the row 17 of the injected yhat moved by 1e6, target unchanged"""
    y, x = br.grid_case(6)
    p = br.Problem(y, x, **BASE)
    st = p.run(10, keep=(10,))[10]
    if which == "far_target":
        x = x.copy()
        x[FAR_INDEX] += FAR
        p = br.Problem(y, x, **BASE)
    elif which == "far_row":
        st = st.copy()
        st.yhat[FAR_INDEX] += FAR
    return p, st, p.iterate(st)


def clamp_guard(which):
    p, st, want = clamp_case(which)
    figure = br.clamp_figure(p.x, st.yhat, st.sigma2)
    assert all(np.isfinite(np.asarray(v)).all() for v in want.__dict__.values()), which
    if which == "unmoved":
        assert figure < br.CLAMP_AT / 1e3, figure
        assert want.nu_prime[FAR_INDEX] > 0.5 and want.nu[FAR_INDEX] > 0.0
    else:
        assert figure >= 1e3 * br.CLAMP_AT, figure
        assert (want.nu_prime[FAR_INDEX] if which == "far_target" else want.nu[FAR_INDEX]) == 0.0
    return figure


# ------------------------------------------------------------------------------------------------------------ parameters
PARAMETER_CASES = {
    "kappa=1e-3": dict(kappa=1e-3), "kappa=0.5": dict(kappa=0.5), "kappa=7": dict(kappa=7.0), "kappa=1e6": dict(kappa=1e6),
    "beta=0.3": dict(beta=0.3), "beta=6": dict(beta=6.0), "lambda=0.1": dict(lambda_=0.1), "lambda=1e4": dict(lambda_=1e4),
    "w=0.9": dict(w=0.9), "gamma=10": dict(gamma=10.0),
}
PARAMETER_STATES = (0, 1, 10)
OFFSET, OFFSET_STATES = 1e4, (0, 10)
ALPHA_FLOOR = 1e-300


def _states_and_references(p, keep):
    states = p.run(max(keep), keep=keep)
    return p, states, {it: p.iterate(st) for it, st in states.items()}


@functools.lru_cache(maxsize=None)
def parameter_case(name):
    """(problem, {iteration: state}, {iteration: reference}): g6 with one parameter changed, states of a run under those parameters"""
    y, x = br.grid_case(6)
    return _states_and_references(br.Problem(y, x, **{**BASE, **PARAMETER_CASES[name]}), PARAMETER_STATES)


def parameter_guard(name):
    p, states, refs = parameter_case(name)
    assert all(np.isfinite(r.yhat).all() and np.isfinite(r.sigma2) for r in refs.values()), name
    if name == "kappa=1e-3":                                   # psi(kappa) - psi(kappa M + N^) < log of the smallest double
        assert min(r.alpha.min() for r in refs.values()) == 0.0


@functools.lru_cache(maxsize=None)
def offset_case():
    """g6 with template and target both shifted by 1e4"""
    y, x = br.grid_case(6)
    return _states_and_references(br.Problem(y + OFFSET, x + OFFSET, **BASE), OFFSET_STATES)


# ------------------------------------------------------------------------------------------- the restatement's own spread
def iteration_outputs(p, st):
    """fn(yhat, x) -> the quantities of one iteration, for rot3_cases.oracle_spread over (yhat, x)"""
    def fn(yhat, x):
        q = br.Problem(p.y, x, w=p.w, lambda_=p.lam, gamma=p.gamma, kappa=p.kappa, beta=p.beta)
        new = q.iterate(replace(st, yhat=yhat))
        return dict(yhat=new.yhat, vhat=new.vhat, uhat=p.y + new.vhat, alpha=new.alpha, nu=new.nu, nu_prime=new.nu_prime, sigma_diag=new.sig,
                    s=new.s, R=new.R, t=new.t, sigma2=new.sigma2, Nhat=new.Nhat, sigma_bar2=new.sigma_bar2)
    return fn


def spread_on_figure_scale(base, spread, p):
    """oracle_spread's largest element-wise changes on the scales of test_gpu_bcpd.figures: vectors by norm (a change of `d` in every
    entry moves the norm by d sqrt(size)), sigma_m^2 by the largest K_mm, scalars by their value, R absolute"""
    out = {}
    for k, d in spread.items():
        v = base[k]
        if k == "R":
            out[k] = d
        elif k == "sigma_diag":
            out[k] = d / float(np.diag(p.G).max() / p.lam)
        elif v.ndim == 0:
            out[k] = d / abs(float(v))
        else:
            out[k] = d * np.sqrt(v.size) / float(np.linalg.norm(v))
    return out
