#!/usr/bin/env python3
"""Time per `update` of the fitter's "pairs given" flavour (gingr_fitter_update_pairs_async) on the synthetic M <-> M workload of
bench.py, with K = M isotropic pairs (every vertex paired with its nearest target vertex):
  pairs_pushed      gingr_fitter_set_pairs (upload + keys + radix sort + gather) before every update -- a host whose
                    correspondences change every iteration
  pairs_in_place    the pairs left as they stand -- a host with fixed correspondences
  icp               gingr_fitter_update_icp_async on the same model and target (nearest neighbour on the device, uniform weights)
  set_pairs_alone   the consolidation call by itself
One JSON line; no pass / fail threshold.   usage: bench_template.py [M] [rank] [out.json]"""
import json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401
import gingr_amd as ga
from gingr_amd._native import dptr, iptr
from gingr_amd.api import _check
from gingr_amd.sharded import ShardedFitter
from bench import synth_clouds, synth_gpmm

M = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
RANK = int(sys.argv[2]) if len(sys.argv) > 2 else 100
OUT = sys.argv[3] if len(sys.argv) > 3 else None
y, x = synth_clouds(M)
basis, lam = synth_gpmm(y, RANK)
ctx = ga.Context(0)
f = ShardedFitter(ctx, ga.PointDistributionModel(y, np.zeros_like(y), basis, lam), x)
lib, h = f._lib, f.handle
idx, _, _ = ctx.nn(y, x)
pids = np.arange(M, dtype=np.int32)
pts = np.ascontiguousarray(x[idx])
var = np.full(M, 100.0)


def set_pairs():
    _check(ctx.handle, lib.gingr_fitter_set_pairs(h, M, iptr(pids), dptr(pts), dptr(var)), "gingr_fitter_set_pairs")


def update_pairs(n):
    _check(ctx.handle, lib.gingr_fitter_update_pairs_async(h, n), "gingr_fitter_update_pairs_async")


def timed(step, n=20, repeats=5):
    """median over `repeats` of the time per iteration of n back-to-back iterations, from the same state"""
    out = []
    for _ in range(repeats):
        f.set_state(np.zeros(RANK), 100.0)
        ctx.synchronize()
        t0 = time.perf_counter()
        step(n)
        ctx.synchronize()
        out.append((time.perf_counter() - t0) / n * 1e6)
    return statistics.median(out), min(out)


def pushed(n):
    for _ in range(n):
        set_pairs()
        update_pairs(1)


set_pairs()
f.set_state(np.zeros(RANK), 100.0)
update_pairs(3)
f.update_icp(100.0, 100.0, 100, 3)
ctx.synchronize()
res = {"what": "time per update of the pairs flavour, synthetic clouds, K = M isotropic pairs", "points": M, "rank": RANK}
res["pairs_in_place_us"], res["pairs_in_place_us_min"] = timed(update_pairs)
res["pairs_pushed_us"], res["pairs_pushed_us_min"] = timed(pushed)
res["icp_us"], res["icp_us_min"] = timed(lambda n: f.update_icp(100.0, 100.0, 100, n))
res["set_pairs_alone_us"], res["set_pairs_alone_us_min"] = timed(lambda n: [set_pairs() for _ in range(n)])
_, sc, fit = f.get_state()
res["status"] = int(sc.status)
res["fit_checksum"] = float(np.abs(fit).sum())
line = json.dumps(res)
print(line)
if OUT:
    with open(OUT, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
f.close()
ctx.close()
