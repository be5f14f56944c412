"""The kernel extension of a kernel-built model, restated in numpy (the definition gingr_amd/csrc/model_extend.hip is held to).

The pivoted Cholesky reproduces the kernel exactly on its pivot rows, so with L_P the rows of the factor at coordinate d's pivots
(lower triangular in pivot order) and V the eigenvectors the build kept (Q = L V):

    Q(x)[d, :] = sum_j k_d(x, p_dj) C_d[j, :],        L_P^T C_d = V_d.

Kernels are described by plain dicts and evaluated in the dtype asked for (np.longdouble for the reference of the device pass):
    {"kind": "gauss", "sigmas": [...], "scalings": [...], "mirror": 0 | +1 | -1}     sum_i s_i exp(-|x-y|^2 / sigma_i^2) [+ mirror * same at (Mx, y)]
    {"kind": "dot", "scaling": s}                                                      s x.y
    {"kind": "radial", "terms": [(family, parameter, scaling), ...]}                   gaussian / rationalQuadratic / inverseMultiquadric
"""
import numpy as np

U = 2.0 ** -53          # unit roundoff of float64


def hull(n=700, seed=11, radii=(90.0, 60.0, 45.0), jitter=1.0):
    """n points on an ellipsoid hull with unit-scale jitter"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.ascontiguousarray(v * np.asarray(radii) + rng.normal(0.0, jitter, (n, 3)))


def _d2(X, Pv, dtype):
    X, Pv = np.asarray(X, dtype=dtype), np.asarray(Pv, dtype=dtype)
    d = X[:, None, :] - Pv[None, :, :]
    return (d * d).sum(axis=2)


def kernel_matrix(spec, X, Pv, dtype=np.longdouble):
    """k(x_i, p_j) [len(X), len(Pv)]; X takes the non-pivot argument (the one a mirrored copy mirrors)"""
    X, Pv = np.asarray(X, dtype=dtype), np.asarray(Pv, dtype=dtype)
    if spec["kind"] == "dot":
        return (X @ Pv.T) * dtype(spec["scaling"])
    if spec["kind"] == "gauss":
        def mix(d2):
            out = np.zeros_like(d2)
            for sg, sc in zip(spec["sigmas"], spec["scalings"]):
                out = out + dtype(sc) * np.exp(-d2 / (dtype(sg) * dtype(sg)))
            return out
        k = mix(_d2(X, Pv, dtype))
        m = spec.get("mirror", 0.0)
        if m:
            k = k + dtype(m) * mix(_d2(X * np.asarray([-1.0, 1.0, 1.0], dtype=dtype), Pv, dtype))
        return k
    if spec["kind"] == "radial":
        nn = _d2(X, Pv, dtype)
        out = np.zeros_like(nn)
        for family, par, sc in spec["terms"]:
            p2 = dtype(par) * dtype(par)
            if family == "gaussian":
                f = np.exp(-nn / p2)
            elif family == "rationalQuadratic":
                f = 1 - nn / (nn + p2)
            elif family == "inverseMultiquadric":
                f = 1 / np.sqrt(nn + p2)
            else:
                raise ValueError(family)
            out = out + dtype(sc) * f
        return out
    raise ValueError(spec["kind"])


def kernel_error_bound(spec, X, Pv):
    """Bound of |device kernel value - exact value|, entry by entry [len(X), len(Pv)], float64.
    Gaussian terms (table exponential, degree 3, round-to-nearest form): tests/fastexp_cases.py establishes <= 1 ulp of the correctly
    rounded result OF ITS ARGUMENT (ULPS_NEAREST) and puts the argument's own roundings at seven times 2^-52 relative (ARG_ROUNDINGS),
    which enter the value times |ln K| = |x-y|^2 / sigma^2; one more for the rounded exponent constant, one ulp for the scaling and one
    per addition of a mixture or mirror term: relative (4 + 8 |x-y|^2 / sigma_min^2) 2^-52 of the sum of the terms' magnitudes.
    Dot product: three products and two sums, relative to sum |x_i p_i|: 4 u.  Rational quadratic 1 - nn / (nn + b^2): nn carries 5 u,
    the quotient (<= 1) 8 u absolute, the difference one more: 9 u absolute.  Inverse multiquadric: a few u relative (8 u)."""
    X, Pv = np.asarray(X, dtype=np.float64), np.asarray(Pv, dtype=np.float64)
    ulp = 2.0 ** -52
    if spec["kind"] == "dot":
        return 4 * U * (np.abs(X) @ np.abs(Pv).T) * abs(spec["scaling"])
    if spec["kind"] == "gauss":
        smin = min(spec["sigmas"])
        pos = dict(spec, mirror=abs(spec.get("mirror", 0.0)))
        mag = np.asarray(kernel_matrix(pos, X, Pv, np.float64))
        arg = _d2(X, Pv, np.float64)
        if spec.get("mirror", 0.0):
            arg = np.maximum(arg, _d2(X * np.array([-1.0, 1.0, 1.0]), Pv, np.float64))
        return (4 + 8 * arg / smin ** 2) * ulp * mag
    nn = _d2(X, Pv, np.float64)
    out = np.zeros_like(nn)
    for family, par, sc in spec["terms"]:
        one = {"kind": "radial", "terms": [(family, par, sc)]}
        mag = np.asarray(kernel_matrix(one, X, Pv, np.float64))
        if family == "gaussian":
            out += (4 + 8 * nn / par ** 2) * ulp * mag
        elif family == "rationalQuadratic":
            out += 9 * U * abs(sc) + 2 * U * mag
        else:
            out += 8 * U * mag
        out += 2 * U * mag            # the term's place in the sum
    return out


def back_substitute(LP, V):
    """C with LP^T C = V, LP lower triangular (rows from the last to the first), in the dtype of LP"""
    n = LP.shape[0]
    C = np.array(V, dtype=LP.dtype, copy=True)
    for j in range(n - 1, -1, -1):
        if j + 1 < n:
            C[j] = C[j] - LP[j + 1:, j] @ C[j + 1:]
        C[j] = C[j] / LP[j, j]
    return C


def coefficients(L, pivots, V, dtype=np.float64):
    """Per coordinate d: (ids of its pivots' points, C_d [n_d, r]) from a factor L [3M, k] over the (point, coordinate) entries with
    pivot entries `pivots` (oracle.gingr_oracle.pivoted_cholesky_diagonal_kernel(..., return_pivots=True)) and the kept V [k, r]."""
    out = []
    piv = np.asarray(pivots, dtype=np.int64)
    for d in range(3):
        cols = np.nonzero(piv % 3 == d)[0]
        ent = piv[cols]
        LP = np.asarray(L[np.ix_(ent, cols)], dtype=dtype)
        out.append((ent // 3, back_substitute(LP, np.asarray(V[cols], dtype=dtype))))
    return out


def extension_rows(specs, ref, coeffs, Z, dtype=np.longdouble):
    """Q(z) [len(Z), 3, r] by the formula; specs: one kernel dict per coordinate; coeffs: [(ids, C_d)] * 3"""
    Z = np.asarray(Z, dtype=np.float64)
    r = coeffs[0][1].shape[1]
    Q = np.zeros((Z.shape[0], 3, r), dtype=dtype)
    for d, (ids, C) in enumerate(coeffs):
        if len(ids):
            Q[:, d, :] = kernel_matrix(specs[d], Z, ref[ids], dtype) @ np.asarray(C, dtype=dtype)
    return Q


def pass_bound(specs, ref, coeffs, Z):
    """Entry-wise bound [len(Z), 3, r] of the device pass against the exact formula with the SAME C and pivots:
    (2 n u + 8 u) S + E_k |C|,  S = sum_j |k_j| |C_jq|: n float64 multiply-adds of the MFMA chain in any order (2 n u S is the classic
    dot-product bound with room for the products' roundings), the kernel value's own error E_k (kernel_error_bound), 8 u S of slack for
    the accumulator's hand-over between MFMA steps."""
    Z = np.asarray(Z, dtype=np.float64)
    r = coeffs[0][1].shape[1]
    B = np.zeros((Z.shape[0], 3, r))
    for d, (ids, C) in enumerate(coeffs):
        n = len(ids)
        if n == 0:
            continue
        K = np.abs(np.asarray(kernel_matrix(specs[d], Z, ref[ids], np.float64)))
        Ca = np.abs(np.asarray(C, dtype=np.float64))
        B[:, d, :] = (2 * n * U + 8 * U) * (K @ Ca) + kernel_error_bound(specs[d], Z, ref[ids]) @ Ca
    return B


def oracle_model(ref, specs, rel_tol, max_cols=None, dtype=np.float64):
    """The oracle's model of DiagonalKernel(specs) on ref and its extension: (Q [M, 3, r] = L V, coeffs, variances)"""
    from oracle import gingr_oracle as go
    ref = np.asarray(ref, dtype=np.float64)

    def kfun(dim, rows, j):
        return np.asarray(kernel_matrix(specs[dim], ref[rows], ref[j:j + 1], np.float64))[:, 0]
    L, piv = go.pivoted_cholesky_diagonal_kernel(ref.shape[0], kfun, rel_tol, max_cols, return_pivots=True)
    _, _, Vt = np.linalg.svd(L.T @ L)
    V = Vt.T
    Q = (L @ V).reshape(ref.shape[0], 3, -1)
    lam = (Q.reshape(-1, Q.shape[2]) ** 2).sum(axis=0)
    return Q, coefficients(L, piv, V, dtype), lam


def reproduction_error(Q, Qx):
    """relative own-vertex reproduction error: largest |Qx - Q| over the largest |Q|"""
    return float(np.max(np.abs(np.asarray(Qx, dtype=np.float64) - Q)) / np.max(np.abs(Q)))


def residual_diagonal(specs, ref, coeffs, Z, dtype=np.float64):
    """k_d(z, z) - |Q_d(z)|^2  [len(Z), 3] and k_d(z, z) [len(Z), 3]"""
    Z = np.asarray(Z, dtype=np.float64)
    Q = extension_rows(specs, ref, coeffs, Z, dtype)
    kzz = np.stack([np.array([kernel_matrix(specs[d], Z[i:i + 1], Z[i:i + 1], dtype)[0, 0] for i in range(Z.shape[0])]) for d in range(3)], axis=1)
    return np.asarray(kzz - (Q * Q).sum(axis=2), dtype=np.float64), np.asarray(kzz, dtype=np.float64)
