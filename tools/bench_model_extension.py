"""Timing of the kernel extension (gingr_model_extend, gingr_model_warp_points) on one MI355X: a model built on M points carried to P
points, next to the same formula in blocked numpy on 16 threads, a direct build on the P points where it fits, and the floors of the
extension pass -- 2 P n r flops at the float64 MFMA rate the project measures (78.6 TFLOP/s) and the 24 P rp bytes it writes at the
streaming-copy rate (6.29 TB/s).  One process, one GPU; one warm-up call, then the median of 3.  No speed is promised.

usage: tools/bench_model_extension.py [P=1000000] [M=50000] [rank=100] [--out FILE]
    default output: profiles/model_extension_<P>_<M>_<rank>.json
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("OMP_NUM_THREADS", "16")
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import numpy as np  # noqa: E402

import gingr_amd as ga  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
if out_path in args:
    args.remove(out_path)
P = int(args[0]) if len(args) > 0 else 1000000
M = int(args[1]) if len(args) > 1 else 50000
rank = int(args[2]) if len(args) > 2 else 100
SIGMA, SCALING = 70.0, 50.0
MFMA_FLOPS, COPY_BYTES = 78.6e12, 6.29e12

ctx = ga.Context(0)
rng = np.random.default_rng(1234)
ref = rng.normal(0, 100, (M, 3))
Z = rng.normal(0, 100, (P, 3))
dm = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.0, maxRank=rank).Gaussian(SIGMA, SCALING).device()
ctx.synchronize()
t0 = time.perf_counter()
info = dm.kernelExtension
dm.kernelExtensionCoefficients(0)                                        # the first use forms C (the back substitutions, one-off)
form_s = time.perf_counter() - t0
coeffs = [dm.kernelExtensionCoefficients(d) for d in range(3)]
alpha = rng.normal(0, 1, dm.rank)
n, r, rp = max(info.counts), dm.rank, (dm.rank + 15) // 16 * 16


def timed(fn, reps=3):
    fn()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), times


def extend():
    e = dm.extend(Z)
    ctx.synchronize()
    e.close()


def numpy_formula():
    """the same formula, blocks of 8192 points: three products kvec C_d per block, nothing kept"""
    pts = [ref[ids] for ids, _ in coeffs]
    acc = 0.0
    for b in range(0, P, 8192):
        z = Z[b:b + 8192]
        d2 = (z * z).sum(1)[:, None] + (pts[0] * pts[0]).sum(1)[None, :] - 2.0 * z @ pts[0].T
        K = SCALING * np.exp(-d2 / SIGMA ** 2)
        for d, (ids, C) in enumerate(coeffs):
            acc += float((K[:, :len(ids)] @ C)[0, 0])
    return acc


out = {"what": "gingr_model_extend and gingr_model_warp_points: wall time of the whole call (host arrays in, model or host array out)",
       "date": time.strftime("%Y-%m-%d"), "points": P, "model_points": M, "rank": r, "pivots_per_coordinate": list(info.counts),
       "form_coefficients_s": form_s, "no_speed_is_promised": True}
out["extend_s"], out["extend_s_runs"] = timed(extend)
out["warp_points_s"], out["warp_points_s_runs"] = timed(lambda: dm.warpPoints(Z, alpha))
out["numpy_16_threads_s"], _ = timed(numpy_formula, reps=1)
out["floor_mfma_s"] = 2.0 * P * n * r * 3 / MFMA_FLOPS          # three coordinates of n pivots and r columns each, as executed
out["floor_mfma_useful_s"] = 2.0 * P * n * r / MFMA_FLOPS       # a diagonal kernel's C_d holds only its own third of the columns
out["floor_store_s"] = 24.0 * P * rp / COPY_BYTES
try:
    t0 = time.perf_counter()
    direct = ga.GPMMTriangleMesh3D(ctx, Z, relativeTolerance=0.0, maxRank=rank).Gaussian(SIGMA, SCALING)
    direct.rank
    ctx.synchronize()
    out["direct_build_on_the_points_s"] = time.perf_counter() - t0
    direct.device().close()
except Exception as e:                                                  # (does not fit)
    out["direct_build_on_the_points_s"] = None
    out["direct_build_error"] = str(e)[:200]
print(json.dumps(out))
path = out_path or os.path.join(ROOT, "profiles", f"model_extension_{P}_{M}_{r}.json")
with open(path, "w") as f:
    json.dump(out, f, indent=1)
