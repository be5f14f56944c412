#!/usr/bin/env python3
"""Timing of the inverse-Laplacian model from the sparse Laplacian's own eigenpairs (gingr_model_from_laplacian) and, where it can
run, of the route it stands beside: InverseLaplacian(maxRank) = dense adjacency + numpy SVD pseudo-inverse on the host, then the
pivoted Cholesky of the lookup kernel on the device.

    python tools/bench_laplacian_model.py [M=50000] [rank=102]

On the femur (1 622 vertices) both routes run.  On a sphere hull of M vertices only the spectral route runs: the existing one would
need an M x M pseudo-inverse (20 GB at 50 000) and an O(M^3) SVD, so there is nothing to compare with.  Per build: wall time (host
clock around the synchronising call, best of three after a warm-up), the solver's gingr_laplacian_info, and the share of the
Chebyshev kernel (timer slot 17, event pairs around its launches, measured in a separate run with timing on).  The degree totals at
k = 34 and k = 170 are what the default budget was set from.  One JSON line on stdout, the same into
profiles/laplacian_model_<M>.json."""
import dataclasses
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import gingr_amd as ga  # noqa: E402
from bench_nicp_sparse import sphere_mesh  # noqa: E402

SCALING = 30.0
CHEB_TIMER = 17


def femur():
    d = np.load(os.path.join(ROOT, "tests", "golden", "inputs.npz"))
    m = np.load(os.path.join(ROOT, "tests", "golden", "femur_mesh.npz"))
    return d["femur"].astype(np.float64), np.ascontiguousarray(m["femur_cells"], dtype=np.int32)


def spectral(ctx, v, c, rank, reps=3):
    g = ga.GPMMTriangleMesh3D(ctx, v, cells=c)

    def once():
        t0 = time.perf_counter()
        dm = g.InverseLaplacianSpectral(SCALING, rank)
        ms = 1e3 * (time.perf_counter() - t0)
        info = dm.laplacianInfo
        dm.device().close()
        return ms, info

    once()                                        # warm-up: code objects, allocator pools
    runs = [once() for _ in range(reps)]
    ctx.timing_enable(True)
    ctx.timing_reset()
    timed_ms, info = once()
    cheb_ms, cheb_n = ctx.timing_read(CHEB_TIMER)
    ctx.timing_enable(False)
    return {"rank": rank, "build_ms": round(min(r[0] for r in runs), 3), "build_ms_all": [round(r[0], 3) for r in runs],
            "info": dataclasses.asdict(info), "chebyshev_kernel_ms": round(cheb_ms, 3), "chebyshev_launches": int(cheb_n),
            "chebyshev_share_of_timed_build": round(cheb_ms / timed_ms, 4), "timed_build_ms": round(timed_ms, 3)}


def lookup_route(ctx, v, c, rank):
    def once():
        t0 = time.perf_counter()
        g = ga.GPMMTriangleMesh3D(ctx, v, relativeTolerance=0.0, maxRank=rank, cells=c)
        dm = g.InverseLaplacian(SCALING)
        t1 = time.perf_counter()
        r = dm.rank                               # (builds: upload of the M x M table + pivoted Cholesky on the device)
        t2 = time.perf_counter()
        dm.device().close()
        return 1e3 * (t1 - t0), 1e3 * (t2 - t1), r

    once()
    runs = [once() for _ in range(2)]
    best = min(runs, key=lambda r: r[0] + r[1])
    return {"rank": best[2], "host_pinv_ms": round(best[0], 3), "device_factorisation_ms": round(best[1], 3),
            "total_ms": round(best[0] + best[1], 3)}


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    rank = int(sys.argv[2]) if len(sys.argv) > 2 else 102
    ctx = ga.Context(0)
    result = {"what": "inverse-Laplacian model: sparse eigensolver against the dense lookup route; one run on one machine",
              "date": time.strftime("%Y-%m-%d"), "build": ctx._lib.gingr_build_info().decode(), "scaling": SCALING}
    fv, fc = femur()
    ranks = sorted({rank, 102, 510})
    result["femur_1622"] = {"vertices": int(fv.shape[0]), "spectral": [spectral(ctx, fv, fc, r) for r in ranks],
                            "lookup_route": lookup_route(ctx, fv, fc, rank)}
    sv, sc = sphere_mesh(M, 0)
    result[f"sphere_{M}"] = {"vertices": int(M), "spectral": [spectral(ctx, sv, sc, r) for r in ranks],
                             "lookup_route": f"not run: an {M} x {M} pseudo-inverse ({M * M * 8 / 1e9:.0f} GB) and its SVD; nothing to compare with"}
    ctx.close()
    print(json.dumps(result))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", f"laplacian_model_{M}.json"), "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
