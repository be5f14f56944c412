"""Small seeded point sets that put the 3 x 3 rotation step (gingr_amd/csrc/svd3.h) on each of its branches through the public API, and
the oracle's numbers about them: the 3 x 3 cross-covariance, its singular values, its determinant.  No tests in here;
test_rotation_step_host.py checks the builders against the oracle on the CPU, test_gpu_rotation_step.py runs them on the device.

Every case names the branch it is built for as a GUARD (`Guard`), evaluated on the oracle's numbers alone: the sign of det S with
|det S| >= 1e-6 s1 s2 s3, or rank deficiency with s3 / s1 <= 1e-14, or the branch of rot_to_euler that |R[2,0]| selects.  Both test
modules assert the guard of every case they run: a change of the data, or of a threshold, must fail there and not test another branch.

Families: A large proper rotations; B mirrored (det S < 0); C thin slabs along a tilted normal (thickness ratio 1e-2 and 1e-4, both
signs); D exactly planar on a tilted plane; E collinear; F near gimbal lock; H far from the origin (centroid at 1e4 x the extent,
coordinates scaled by 1e-3 and 1e+4)."""
from __future__ import annotations

import dataclasses
import functools
import math

import numpy as np

from oracle import gingr_oracle as go

TILT = go.euler_to_rot(0.7, 0.5, -0.4)          # no slab, plane or line in here is aligned with a coordinate axis
LOCK_WINDOW = 1e-4                               # rot_to_euler: | |R[2,0]| - 1 | <= 1e-4 is the gimbal branch


# ------------------------------------------------------------------------------------------------------------------------- guards
@dataclasses.dataclass(frozen=True)
class Guard:
    kind: str                                    # "det+", "det-", "rank2", "rank1", "euler", "lock+", "lock-"
    min_ct: float = 0.0                          # "euler": cos(theta) must lie in [min_ct, max_ct]
    max_ct: float = 1.0

    def holds(self, S=None, R=None) -> bool:
        """S: the oracle's cross-covariance (det / rank guards); R: the rotation the oracle's Umeyama step hands to rot_to_euler"""
        if self.kind in ("det+", "det-"):
            s = np.linalg.svd(S, compute_uv=False)
            det = float(np.linalg.det(S))
            return (det > 0) == (self.kind == "det+") and abs(det) >= 1e-6 * s[0] * s[1] * s[2] and s[2] > 1e-12 * s[0]
        if self.kind in ("rank2", "rank1"):
            s = np.linalg.svd(S, compute_uv=False)
            r = 2 if self.kind == "rank2" else 1
            return s[r] <= 1e-14 * s[0] and s[r - 1] >= 1e-3 * s[0]
        locked = not abs(abs(R[2, 0]) - 1) > LOCK_WINDOW
        if self.kind == "euler":
            ct = math.cos(math.asin(-R[2, 0])) if not locked else 0.0
            return not locked and self.min_ct <= ct <= self.max_ct and abs(abs(abs(R[2, 0]) - 1) - LOCK_WINDOW) > 1e-6
        return locked and (abs(R[2, 0] + 1) < LOCK_WINDOW) == (self.kind == "lock+")


def cross_covariance(x, target):
    """the 3 x 3 matrix of kabsch / umeyama: sum (target - ct)(x - cx)^T / M"""
    x, target = np.asarray(x, dtype=np.float64), np.asarray(target, dtype=np.float64)
    return (target - target.mean(0)).T @ (x - x.mean(0)) / x.shape[0]


def svd_rotation(S):
    """what umeyama / kabsch make of S before any Euler step: U diag(1, 1, sign det S) V^T"""
    U, _, Vt = np.linalg.svd(S)
    return U @ np.diag([1.0, 1.0, -1.0 if np.linalg.det(S) < 0 else 1.0]) @ Vt


def rot_axis(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def half_turn(axis):
    """rotation by exactly pi about `axis`: 2 a a^T - I (no sine of pi)"""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    return 2.0 * np.outer(a, a) - np.eye(3)


def random_rotation(rng):
    Q, R = np.linalg.qr(rng.normal(size=(3, 3)))
    Q = Q * np.sign(np.diag(R))[None]
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    return Q


QUADRANT_ANGLES = (0.6, 2.2, -2.2, -0.6)         # one angle in each atan2 quadrant


def rotations_A():
    """name -> rotation: family A"""
    rng = np.random.default_rng(41)
    out = {f"random{k}": random_rotation(rng) for k in range(3)}
    out["pi-x"] = np.diag([1.0, -1.0, -1.0])
    out["pi-y"] = np.diag([-1.0, 1.0, -1.0])
    out["pi-z"] = np.diag([-1.0, -1.0, 1.0])
    out["pi-random-axis"] = half_turn(rng.normal(size=3))
    for i, phi in enumerate(QUADRANT_ANGLES):
        for j, psi in enumerate(QUADRANT_ANGLES):
            out[f"phi-q{i + 1}-psi-q{j + 1}"] = go.euler_to_rot(phi, 0.4, psi)
    return out


def rotations_F():
    """name -> (rotation, guard, ill-conditioned): theta = +-(pi/2 - delta); delta = 0 locked, 0.01 inside the 1e-4 window (its edge is
    at delta = 0.01414), 0.02 outside it with cos(theta) = 0.02"""
    out = {}
    for sign, tag in ((1.0, "+"), (-1.0, "-")):
        for delta in (0.0, 0.01, 0.02):
            R = go.euler_to_rot(0.8, sign * (math.pi / 2 - delta), -1.9)
            g = Guard("euler", 0.019, 0.021) if delta == 0.02 else Guard("lock" + tag)
            out[f"theta{tag}-delta{delta:g}"] = (R, g, True)
    return out


# --------------------------------------------------------------------------------------------- pairs with correspondence by index
@dataclasses.dataclass(frozen=True)
class Pair:
    """x is to be aligned to target, point m to point m"""
    name: str
    x: np.ndarray
    target: np.ndarray
    guard: Guard
    ill: bool = False                            # thickness 1e-4: the bound comes from the oracle's own spread

    @property
    def S(self):
        return cross_covariance(self.x, self.target)


def cloud(seed, M=300):
    """anisotropic Gaussian cloud (deviations 30, 20, 10 along tilted axes): three well separated singular values"""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(M, 3)) * np.array([30.0, 20.0, 10.0])) @ TILT.T + np.array([5.0, -3.0, 2.0])


def flatten(P, normal, ratio):
    """P with its extent along `normal` scaled by `ratio` about the centroid"""
    c = P.mean(0)
    h = (P - c) @ normal
    return P - np.outer(h * (1.0 - ratio), normal)


def _moved(target, Q, rng, mirror_normal=None, noise=0.05, keep=None):
    """x = Q (target [mirrored in the plane through its centroid] + noise) + t; keep: projector that confines the noise"""
    P = target.copy()
    if mirror_normal is not None:
        c = P.mean(0)
        P = P - 2.0 * np.outer((P - c) @ mirror_normal, mirror_normal)
    e = rng.normal(0.0, noise, P.shape)
    if keep is not None:
        e = e @ keep
    return (P + e) @ Q.T + np.array([7.0, -11.0, 4.0])


def _far(x, target, scale):
    """family H: the centroid 1e4 x the extent away, then every coordinate scaled"""
    extent = np.ptp(target, axis=0).max()
    off = 1e4 * extent * np.array([0.6, -0.64, 0.48])
    return scale * (x + off), scale * (target + off)


@functools.lru_cache(maxsize=None)
def pairs():
    """name -> Pair, families A B C D E H"""
    out = {}
    normal = TILT[:, 2]                          # the thin direction of the cloud, tilted

    def add(name, x, target, guard, ill=False):
        x.setflags(write=False)
        target.setflags(write=False)
        out[name] = Pair(name, x, target, guard, ill)

    rots = rotations_A()
    for k, (name, Q) in enumerate(rots.items()):
        tgt = cloud(100 + k)
        add("A-" + name, _moved(tgt, Q, np.random.default_rng(200 + k)), tgt, Guard("det+"))
    rngB = np.random.default_rng(43)
    mirrors = {"B-mirror-thin-axis": TILT[:, 2], "B-mirror-long-axis": TILT[:, 0], "B-mirror-random": rngB.normal(size=3)}
    for k, (name, n) in enumerate(mirrors.items()):
        tgt = cloud(300 + k)
        add(name, _moved(tgt, random_rotation(rngB), np.random.default_rng(310 + k), mirror_normal=n / np.linalg.norm(n)), tgt, Guard("det-"))
    for ratio, tag, ill in ((1e-2 / (1.0 / 3.0), "1e-2", False), (1e-4 / (1.0 / 3.0), "1e-4", True)):
        # the cloud's own ratio of its thin to its long axis is 1/3: after flatten() it is 1e-2 resp. 1e-4, s3/s1 of S its square
        for sign, mirror in (("pos", None), ("neg", TILT[:, 0])):
            for k in range(2):
                tgt = flatten(cloud(400 + k), normal, ratio)
                rng = np.random.default_rng(420 + k)
                x = _moved(tgt, random_rotation(rng) if k else half_turn(rng.normal(size=3)), rng, mirror_normal=mirror,
                           noise=0.05 * ratio)
                add(f"C-{tag}-{sign}-{k}", x, tgt, Guard("det+" if sign == "pos" else "det-"), ill)
    for k in range(3):
        rng = np.random.default_rng(500 + k)
        ab = rng.normal(size=(300, 2)) * np.array([30.0, 20.0])
        tgt = ab[:, :1] * TILT[:, 0][None] + ab[:, 1:] * TILT[:, 1][None]      # through the origin: no offset to round
        cd = ab + rng.normal(0.0, 0.05, ab.shape)
        Q = random_rotation(rng)
        x = (cd[:, :1] * (Q @ TILT[:, 0])[None] + cd[:, 1:] * (Q @ TILT[:, 1])[None])
        add(f"D-planar-{k}", x, tgt, Guard("rank2"))
    for k in range(2):
        rng = np.random.default_rng(600 + k)
        a = rng.normal(0.0, 30.0, 300)
        d1, d2 = TILT[:, 0], random_rotation(rng) @ TILT[:, 0]
        add(f"E-collinear-{k}", np.outer(a + rng.normal(0.0, 0.05, 300), d2), np.outer(a, d1), Guard("rank1"))
    for scale, tag in ((1e-3, "1e-3"), (1e4, "1e+4")):
        for base in ("A-random0", "A-pi-random-axis", "B-mirror-random"):
            p = out[base]
            x, tgt = _far(np.array(p.x), np.array(p.target), scale)
            add(f"H-{tag}-{base}", x, tgt, p.guard)
    return out


# ------------------------------------------------------------------------------------- lattice slabs: callers that find the partners
@dataclasses.dataclass(frozen=True)
class Slab:
    """tpl is registered to tgt; partner[i] is the index in tgt of the point built as the counterpart of tpl[i]"""
    name: str
    tpl: np.ndarray
    tgt: np.ndarray
    partner: np.ndarray
    guard: Guard
    ill: bool = False
    scale: float = 1.0                           # largest coordinate / that of the unscaled slab at the origin (family H)

    @property
    def S(self):
        return cross_covariance(self.tpl, self.tgt[self.partner])


SMALL_MOTION = (go.euler_to_rot(0.02, -0.015, 0.01), np.array([0.3, -0.2, 0.1]))


def lattice_slab(name, seed, sign, ratio=None, planar=False, far_scale=None):
    """Nodes of a y-z lattice (spacings 10 and 7, 10 x 10 nodes about the origin) with random asymmetric x offsets in +-2; the
    counterpart has the offsets mirrored (sign = -1) or kept (+1) -- 0.8 of them plus a tenth of fresh ones, so that it is no exact
    copy --, is moved by a small rigid motion (0.02 rad, 0.3) and listed in another order.  Neighbours are 7 apart, partners at most
    about 5: every point's nearest neighbour is its partner.  ratio: the x offsets scaled to that ratio of deviations x : y.  Both
    clouds are then tilted, and for family H moved away and scaled."""
    rng = np.random.default_rng(seed)
    j, k = np.meshgrid(np.arange(10) - 4.5, np.arange(10) - 4.5, indexing="ij")
    y, z = 10.0 * j.ravel(), 7.0 * k.ravel()
    M = y.shape[0]
    xo, fresh = rng.uniform(-2.0, 2.0, M), rng.uniform(-2.0, 2.0, M)
    f = 0.0 if planar else (1.0 if ratio is None else ratio * y.std() / xo.std())
    tpl = np.stack([f * xo, y, z], axis=1)
    jit = rng.uniform(-0.3, 0.3, (M, 2))                                       # in-plane: the counterpart is no copy in y, z either
    tgt = np.stack([f * (sign * 0.8 * xo + 0.1 * fresh), y + jit[:, 0], z + jit[:, 1]], axis=1)
    Rm, tm = SMALL_MOTION
    tgt = tgt @ Rm.T + tm
    perm = rng.permutation(M)
    partner = np.empty(M, dtype=np.int64)
    partner[perm] = np.arange(M)
    tgt = tgt[perm]
    tpl, tgt = tpl @ TILT.T, tgt @ TILT.T
    scale = 1.0
    if far_scale is not None:
        top = max(np.abs(tpl).max(), np.abs(tgt).max())
        tpl, tgt = _far(tpl, tgt, far_scale)
        scale = max(np.abs(tpl).max(), np.abs(tgt).max()) / top
    guard = Guard("rank2") if planar else Guard("det+" if sign > 0 else "det-")
    for a in (tpl, tgt, partner):
        a.setflags(write=False)
    return Slab(name, tpl, tgt, partner, guard, ill=(ratio is not None and ratio < 1e-3), scale=scale)


@functools.lru_cache(maxsize=None)
def slabs():
    """name -> Slab: B, C (both signs), D, H"""
    out = {}
    for k in range(2):
        out[f"B-mirror-{k}"] = lattice_slab(f"B-mirror-{k}", 700 + k, -1.0)
    for ratio, tag in ((1e-2, "1e-2"), (1e-4, "1e-4")):
        for sign, st in ((1.0, "pos"), (-1.0, "neg")):
            out[f"C-{tag}-{st}"] = lattice_slab(f"C-{tag}-{st}", 710 + int(sign), sign, ratio=ratio)
    for k in range(2):
        out[f"D-planar-{k}"] = lattice_slab(f"D-planar-{k}", 720 + k, 1.0, planar=True)
    for scale, tag in ((1e-3, "1e-3"), (1e4, "1e+4")):
        out[f"H-{tag}-mirror"] = lattice_slab(f"H-{tag}-mirror", 730, -1.0, far_scale=scale)
        out[f"H-{tag}-proper"] = lattice_slab(f"H-{tag}-proper", 731, 1.0, far_scale=scale)
    return out


def classic_cpd_A(slab, sigma2=1.0, w=0.0):
    """the 3 x 3 matrix of RigidCPD.Maximization for template slab.tpl, target slab.tgt at variance sigma2 (1: the soft assignment is
    the partner, 7 apart from the next candidate)"""
    X, Y = slab.tgt, slab.tpl
    P = go.classic_cpd_expectation(X, Y, sigma2, w)
    P1 = P.sum(1)
    Np = P1.sum()
    muX = (X.T @ (P.T @ np.ones(Y.shape[0]))) / Np
    muY = (Y.T @ P1) / Np
    return (X - muX).T @ P.T @ (Y - muY)


# ----------------------------------------------------------------------------------------------------------- the GiNGR update
def stiff_model(M=200, seed=800):
    """rank 2, variances 1e-8: a model of negligible flexibility on a cloud, so that the Umeyama step of an update towards the posed
    reference returns the state's total rotation"""
    rng = np.random.default_rng(seed)
    ref = cloud(seed, M)
    U, _ = np.linalg.qr(rng.normal(size=(3 * M, 2)))
    return go.PDM(ref, np.zeros((M, 3)), U, np.array([1e-8, 0.5e-8]))


def posed_target(model, R0, t0, seed=801, noise=0.01):
    return model.ref @ R0.T + t0 + np.random.default_rng(seed).normal(0.0, noise, model.ref.shape)


T0 = np.array([3.0, -2.0, 1.0])


def mirror_model(seed=900):
    """Family B for the update: a lattice slab as reference and a rank-2 model whose first column is the mirror displacement
    (-2 x_i, 0, 0) (tilted with the slab), normalised, with the variance |displacement|^2: coefficient 1 is the mirrored slab, and the
    posterior mean of an update towards the mirrored target crosses the plane.  Returns (model, target)."""
    s = lattice_slab("update-mirror", seed, -1.0)
    M = s.tpl.shape[0]
    xo = (s.tpl @ TILT)[:, 0]                                                    # the offsets along the tilted normal
    d = np.outer(-2.0 * xo, TILT[:, 0]).reshape(-1)
    n = np.linalg.norm(d)
    rng = np.random.default_rng(seed + 1)
    v = rng.normal(size=3 * M)
    v -= (v @ d) / (n * n) * d
    U = np.stack([d / n, v / np.linalg.norm(v)], axis=1)
    return go.PDM(np.array(s.tpl), np.zeros((M, 3)), U, np.array([n * n, 1e-8])), np.array(s.tgt)


def state_at(model, sigma2, R0, t0, transform, direct=False):
    """go.initial_state at the pose (R0, t0).  direct (family F): the Euler angles of R0 are put into the state as they are -- read off
    by Slabaugh's recipe without the gimbal window, which would snap theta to +-pi/2 --, so that the state's rotation, and with it the
    matrix the update's Umeyama step returns, is R0 itself: locked, inside the window, or just outside it."""
    st = go.initial_state(model, sigma2, global_transformation=transform, init_R=R0, init_t=t0)
    if direct:
        theta = math.asin(-R0[2, 0])
        if abs(R0[2, 0]) < 1 - 1e-12:
            euler = (math.atan2(R0[1, 0], R0[0, 0]), theta, math.atan2(R0[2, 1], R0[2, 2]))
        else:
            euler = go.rot_to_euler(R0)
        st = dataclasses.replace(st, euler=euler)
        st.fit = go.model_instance_shape_pose_scale(model, st)
    return st


def classic_cpd_outputs(X, Y, sigma2=1.0, w=0.0):
    TY, s2, (sc, R, t) = go.classic_cpd_maximization_rigid(X, Y, go.classic_cpd_expectation(X, Y, sigma2, w))
    return {"TY": TY, "sigma2": s2, "scale": sc, "R": R, "t": t}


def update_sigma_xy(model, target, st, flavour, w=0.0, lam=1.0):
    """The cross-covariance the Umeyama step of go.cpd_update / go.icp_update decomposes for state st (update_from_observations,
    steps :212-231, restated with the oracle's own parts): for the guards of the update cases."""
    if flavour == "cpd":
        pids, pts, var = go.cpd_observations(model, target, st, w, lam)
    else:
        idx, _, _ = go.icp_closest_point(st.fit, target)
        pids, pts, var = np.arange(model.M), np.asarray(target)[idx], np.full(model.M, st.sigma2)
    shape, _, posed = go.compute_posterior_mean(model, st, pids, pts, var, None)
    alpha1 = posed.coefficients(shape)
    alpha_c = st.alpha + (alpha1 - st.alpha) * st.step_length
    return cross_covariance(model.instance(st.alpha), posed.instance(alpha_c))


# ------------------------------------------------------------------------------------------------------- the oracle's own spread
def oracle_spread(fn, inputs, samples=8, seed=12345):
    """fn(*inputs) -> dict name -> array.  The largest change of each output over `samples` seeded relative perturbations of 2^-52 of
    every entry of the inputs: what the oracle itself makes of the last bit of its data.  Returns (outputs, spread per name)."""
    base = {k: np.asarray(v, dtype=np.float64) for k, v in fn(*inputs).items()}
    rng = np.random.default_rng(seed)
    spread = {k: 0.0 for k in base}
    for _ in range(samples):
        moved = [np.asarray(a, dtype=np.float64) * (1.0 + rng.choice([-1.0, 1.0], size=np.shape(a)) * 2.0 ** -52) for a in inputs]
        for k, v in fn(*moved).items():
            spread[k] = max(spread[k], float(np.abs(np.asarray(v, dtype=np.float64) - base[k]).max()))
    return base, spread


def bound(well, spread, ill):
    """the tolerance of a case: the well-conditioned one, or -- ill-conditioned cases -- 10 x the oracle's spread where that is larger"""
    return max(well, 10.0 * spread) if ill else well
