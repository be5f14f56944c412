"""Timing of the to-tolerance GPMM build (gingr_gpmm_build_diagonal_ex) and, on the same matrices in the same session, of the two
eigen kernels that can serve its coordinate blocks of 193 .. 512 columns: the block kernel of eig.hip (sym_eig_blocks) and the
two-sided grid kernel it replaces there (GINGR_EIG_TWO_SIDED=1).  One child process per kernel (the switch is read once);
prints one JSON document.  Usage: python tools/bench_gpmm_to_tolerance.py [repeats]"""
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(repeats):
    import numpy as np
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (first: one HIP runtime per process)
    import gingr_amd as ga
    ctx = ga.Context(0)
    femur = np.load(os.path.join(ROOT, "tests", "golden", "inputs.npz"))["femur"].astype(np.float64)
    cloud = np.random.default_rng(21).normal(0, 40, (1200, 3))
    cases = [("femur template kernels, tolerance 0.01, keep 100", lambda: ga.automaticGPMMfromTemplate(ctx, femur, 0.01, toTolerance=True).truncate(100))]
    for mc in (600, 900, 1536):
        cases.append((f"cloud 1200 Gaussian(18, 10), {mc} columns, keep 100",
                      lambda mc=mc: ga.DevicePointDistributionModel(ctx, cloud, [18.0], [10.0], 0.0, maxRank=mc, toTolerance=True, keepRank=100)))
    for name, make in cases:
        for rep in range(repeats + 1):           # (the first build of a size pays its allocations)
            t0 = time.perf_counter()
            dm = make()
            info = dm.buildInfo
            ctx.synchronize()
            dt = time.perf_counter() - t0
            dm.device().close()
            if rep:
                print(json.dumps({"case": name, "columns": info.columns, "rank": info.rank, "build_ms": 1e3 * dt}), flush=True)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = {}
    for kernel in ("blocks", "two_sided"):
        env = dict(os.environ, GINGR_EIG_TIMING="1")
        if kernel == "two_sided":
            env["GINGR_EIG_TWO_SIDED"] = "1"
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(repeats)], env=env, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit(p.returncode)
        builds = [json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")]
        eig = {}
        for m in re.finditer(r"sym_eig_timing n=(\S+) kernel=(\S+) two_sided_runs=(\d+) ms=(\S+)", p.stderr):
            eig.setdefault(m.group(1), []).append((m.group(2), int(m.group(3)), float(m.group(4))))
        res = {"builds": {}, "eigen": {}}
        for b in builds:
            res["builds"].setdefault(b["case"], {"columns": b["columns"], "rank": b["rank"], "build_ms": []})["build_ms"].append(round(b["build_ms"], 3))
        for n, runs in eig.items():
            runs = runs[1:] if len(runs) > 1 else runs   # (drop the warm-up build's)
            ms = sorted(r[2] for r in runs)
            res["eigen"][n] = {"kernel": runs[0][0], "two_sided_runs": max(r[1] for r in runs), "median_ms": ms[len(ms) // 2], "min_ms": ms[0],
                               "max_ms": ms[-1], "samples": len(ms)}
        for v in res["builds"].values():
            ms = sorted(v["build_ms"])
            v["median_ms"] = ms[len(ms) // 2]
        out[kernel] = res
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        child(int(sys.argv[2]))
    else:
        main()
