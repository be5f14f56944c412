"""Build time of the GPMM entries at one size (one-off model set-up, not the benchmark metric): the old entry
(gingr_gpmm_build_gaussian) next to gingr_gpmm_build_radial with Gaussian terms and no field, one weighted term, two weighted terms
(change point) and the rational quadratic.  One process, one GPU; per path one warm-up build, then the median of 5 blocks of one build.

usage: tools/bench_varying_gpmm.py [M=50000] [rank=100] [--old-entry-only] [--out FILE]
    default output: profiles/varying_gpmm_<M>_<rank>.json
    --old-entry-only   time the old entry alone and write nothing (same-box A/B of two builds of the library: tools/ab_gpmm.sh)
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import numpy as np  # noqa: E402

import gingr_amd as ga  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
old_only = "--old-entry-only" in sys.argv
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
if out_path in args:
    args.remove(out_path)
M = int(args[0]) if len(args) > 0 else 50000
rank = int(args[1]) if len(args) > 1 else 100
BLOCKS = 5

ctx = ga.Context(0)
ref = np.random.default_rng(1234).normal(0, 100, (M, 3))
g = ga.GPMMTriangleMesh3D(ctx, ref, relativeTolerance=0.0, maxRank=rank)
SIGMA, SCALING = 70.0, 50.0


def timed(make):
    times, r = [], 0
    for block in range(BLOCKS + 1):                 # the first build of a path pays its allocations: not counted
        t0 = time.perf_counter()
        dm = make()
        r = dm.rank
        ctx.synchronize()
        dt = time.perf_counter() - t0
        dm.device().close()
        if block > 0:
            times.append(dt)
    return {"rank": r, "build_s_median": statistics.median(times), "build_s_blocks": times}


paths = [("old entry: gingr_gpmm_build_gaussian", lambda: g.Gaussian(SIGMA, SCALING))]
if not old_only:
    amplitude = 0.5 + 1.5 * ga.sigmoidField(ref, [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], 60.0)
    indicator = ga.sigmoidField(ref, [0.0, 0.0, 0.0], [0.0, 1.0, 0.0], 40.0)
    pars = [ga.GaussianKernelParameters(SIGMA, SCALING)]
    paths += [
        ("radial entry: one Gaussian term, no field", lambda: g.RadialMixture([ga.RadialKernelTerm("gaussian", SIGMA, SCALING)])),
        ("radial entry: one weighted Gaussian term", lambda: g.ScaledGaussian(pars, amplitude)),
        ("radial entry: change point, two weighted Gaussian terms",
         lambda: g.ChangePoint(pars, [ga.GaussianKernelParameters(SIGMA / 3.0, SCALING / 4.0)], indicator)),
        ("radial entry: rational quadratic", lambda: g.RationalQuadratic(SIGMA, SCALING)),
    ]
result = {"points": M, "max_rank": rank, "blocks": BLOCKS, "date": time.strftime("%Y-%m-%d"), "library": os.path.basename(os.environ.get("GINGR_HIP_LIB", "")) or "in-tree",
          "paths": []}
for name, make in paths:
    row = {"path": name, **timed(make)}
    result["paths"].append(row)
    print(row, file=sys.stderr)
ctx.close()
if not old_only:
    out_path = out_path or os.path.join(ROOT, "profiles", f"varying_gpmm_{M}_{rank}.json")
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
print(json.dumps(result))
