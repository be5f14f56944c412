"""Timing of the PCA model built on the device (gingr_model_from_shapes) and of the host route it replaces: numpy centring, eigh of the
n x n Gram matrix, Q0 = Xc V, then gingr_model_upload of the result.  Both start from the same shapes in host memory and end with a
finalized resident model.  Prints one JSON document.
Usage: python tools/bench_pca_model.py [M] [n] [repeats]      (defaults 50000, 100, 5)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import gingr_amd as ga  # noqa: E402


def host_route(ctx, ref, X, rel_tol=1e-10):
    n = X.shape[0]
    mu = X.mean(axis=0)
    Xc = (X - mu).reshape(n, -1).T / np.sqrt(n - 1.0)
    lam, V = np.linalg.eigh(Xc.T @ Xc)
    lam, V = lam[::-1], V[:, ::-1]
    k = int(min(n - 1, (lam > rel_tol * lam[0]).sum()))
    Q0 = Xc @ V[:, :k]
    model = ga.PointDistributionModel(ref, mu - ref, Q0 / np.sqrt(lam[:k])[None], lam[:k].copy())
    return ga.DeviceModel(ctx, model)


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    rng = np.random.default_rng(5)
    ref = rng.normal(0, 40, (M, 3))
    modes = rng.normal(size=(3 * M, 30)) * (0.8 ** np.arange(30))[None]
    X = ref[None] + (rng.normal(size=(n, 30)) @ modes.T).reshape(n, M, 3) * 3.0 + rng.normal(0, 0.05, (n, M, 3))
    ctx = ga.Context(0)
    out = {"M": M, "n": n, "repeats": repeats, "threads": os.environ.get("OMP_NUM_THREADS", "")}
    for name, make in (("device_none", lambda: ga.PointDistributionModel.createUsingPCA(ctx, ref, X)),
                       ("device_gpa", lambda: ga.PointDistributionModel.createUsingPCA(ctx, ref, X, alignment="gpa")),
                       ("host_numpy_eigh_upload", lambda: host_route(ctx, ref, X))):
        ms = []
        for rep in range(repeats + 1):               # (the first build of a size pays its allocations and code objects)
            t0 = time.perf_counter()
            dm = make()
            ctx.synchronize()
            dt = 1e3 * (time.perf_counter() - t0)
            rank = dm.rank
            (dm.device() if hasattr(dm, "device") else dm).close()
            if rep:
                ms.append(round(dt, 2))
        ms.sort()
        out[name] = {"rank": rank, "median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
