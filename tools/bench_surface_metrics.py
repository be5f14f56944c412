"""Timing of the surface-distance model metrics on one MI355X (gingr_mesh_set_distances, gingr_model_generalization_surface,
gingr_model_specificity_surface) and, on the same device in the same run, of the route they replace: DeviceModel.project / .instances,
then one Context.mesh_distance_stats per (projection, shape) or (sample, shape) pair -- every pair for the generalization, a subset of
the pairs for the specificity and the primitive, scaled to all pairs (the scaling is stated in the output).  Beside the whole calls: the
batched scan alone (device timer 23: HIP events on the context's stream), per call and per query point.
The mesh is a jittered triangulated grid of about M vertices, the model a random basis of rank 32 on it; the n shapes are instances
plus noise.  Writes profiles/surface_metrics_<M>_<n>_<S>.json and prints the same document.  Not the benchmark metric; no speed is
promised.
Usage: python tools/bench_surface_metrics.py [M] [n] [S] [n_ranks]      (defaults 1600, 100, 1000, 3; n shapes, S samples)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import gingr_amd as ga  # noqa: E402

RANK = 32
SUBSET_PAIRS = 256


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def timed(call, repeats=3):
    call()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        out.append(1e3 * (time.perf_counter() - t0))
    return {"median": median(out), "min": min(out), "max": max(out)}


def grid(M, rng):
    gx = max(2, int(round(np.sqrt(M))))
    gy = max(2, -(-M // gx))
    x, y = np.meshgrid(np.arange(gx, dtype=np.float64), np.arange(gy, dtype=np.float64), indexing="ij")
    pts = np.stack([x.ravel(), y.ravel(), np.zeros(gx * gy)], axis=1) * 2.0 + rng.normal(0.0, 0.3, (gx * gy, 3))
    idx = np.arange(gx * gy).reshape(gx, gy)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    return pts, np.concatenate([np.stack([a, b, c], axis=1), np.stack([b, d, c], axis=1)]).astype(np.int32)


def scan_time(ctx, call):
    us, launches = [], 0
    for _ in range(3):
        ctx.timing_reset()
        call()
        ms, launches = ctx.timing_read(23)
        us.append(1e3 * ms)
    return {"us_per_call": median(us), "launches_per_call": int(launches), "all_samples_us": us}


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 1600
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    S = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    n_ranks = int(sys.argv[4]) if len(sys.argv) > 4 else 3
    rng = np.random.default_rng(5)
    ref, cells = grid(M, rng)
    Mv = ref.shape[0]
    basis = np.asfortranarray(rng.standard_normal((3 * Mv, RANK)) / np.sqrt(3.0 * Mv))
    model = ga.PointDistributionModel(ref, rng.normal(0, 0.1, (Mv, 3)), basis, 64.0 * (0.25 / 64.0) ** (np.arange(RANK) / (RANK - 1)), cells=cells)
    ctx = ga.Context(0)
    dm = ga.DeviceModel(ctx, model)
    A = rng.standard_normal((S, RANK))
    X = dm.instances(rng.standard_normal((n, RANK))) + rng.normal(0, 0.2, (n, Mv, 3))
    ranks = sorted({int(round(k)) for k in np.linspace(1, RANK, n_ranks)})
    samples = dm.instances(A)

    calls = {"mesh_set_distances_all_pairs_seeded": lambda: ctx.mesh_set_distances(samples, X, cells, "all", True),
             "mesh_set_distances_all_pairs_cold": lambda: ctx.mesh_set_distances(samples, X, cells, "all", False),
             f"generalization_surface_{len(ranks)}_ranks": lambda: dm.project(X, ranks, distance="surface"),
             "specificity_surface_full_rank": lambda: ga.ModelMetrics.specificity(ctx, dm, X, S, alphas=A, distance="surface"),
             f"generalization_vertex_{len(ranks)}_ranks": lambda: dm.project(X, ranks),
             "specificity_vertex_full_rank": lambda: ga.ModelMetrics.specificity(ctx, dm, X, S, alphas=A)}
    whole = {name: timed(call) for name, call in calls.items()}
    ctx.timing_enable(True)
    scans = {name: scan_time(ctx, call) for name, call in calls.items() if "vertex" not in name}
    ctx.timing_enable(False)
    for name, s in scans.items():
        pairs = len(ranks) * n if name.startswith("generalization") else S * n
        s.update(pairs=pairs, query_points=pairs * Mv, ns_per_query_point=1e3 * s["us_per_call"] / (pairs * Mv),
                 share_of_the_whole_call=1e-3 * s["us_per_call"] / whole[name]["median"])

    # the replaced route: the projections / samples on the device as before, then one single call per pair
    def replaced_generalization():
        coef = dm.project(X, ranks)[0]
        out = np.empty((len(ranks), n))
        for q in range(len(ranks)):
            proj = dm.instances(coef[q])
            for i in range(n):
                s, _, cnt, _ = ctx.mesh_distance_stats(proj[i], X[i], cells)
                out[q, i] = s / cnt
        return out

    t0 = time.perf_counter()
    rep_gen = replaced_generalization()
    rep_gen_ms = 1e3 * (time.perf_counter() - t0)
    sub = min(SUBSET_PAIRS, S * n)
    pick = rng.choice(S * n, sub, replace=False)
    t0 = time.perf_counter()
    rep_pairs = np.array([ctx.mesh_distance_stats(samples[p // n], X[p % n], cells)[0] / Mv for p in pick])
    rep_pair_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    dm.instances(A)
    inst_ms = 1e3 * (time.perf_counter() - t0)
    rep_spec_ms = inst_ms + rep_pair_ms * (S * n) / sub
    rep_prim_ms = rep_pair_ms * (S * n) / sub

    got_gen = dm.project(X, ranks, distance="surface")[1]
    got_all = ctx.mesh_set_distances(samples, X, cells, "all", True)[0]
    gname, sname, pname = f"generalization_surface_{len(ranks)}_ranks", "specificity_surface_full_rank", "mesh_set_distances_all_pairs_seeded"
    out = {"M": Mv, "triangles": int(cells.shape[0]), "rank": RANK, "n_shapes": n, "n_samples": S, "ranks": ranks,
           "whole_call_ms": whole, "batched_scan": scans,
           "replaced_route_ms": {"generalization": rep_gen_ms, "specificity_scaled": rep_spec_ms, "all_pairs_scaled": rep_prim_ms,
                                 "pairs_timed": int(sub), "ms_per_single_call": rep_pair_ms / sub,
                                 "scaling": f"the {sub} timed single calls x {S * n} / {sub} pairs (+ one instances call for the specificity); "
                                            "the generalization's pairs are all timed"},
           "replaced_route_over_batched": {"generalization": rep_gen_ms / whole[gname]["median"], "specificity": rep_spec_ms / whole[sname]["median"],
                                           "all_pairs": rep_prim_ms / whole[pname]["median"]},
           "largest_difference_batched_against_replaced_route": {"generalization_avg": float(np.abs(got_gen - rep_gen).max()),
                                                                 "pair_avg": float(np.abs(got_all.ravel()[pick] - rep_pairs).max())}}
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", f"surface_metrics_{M}_{n}_{S}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    dm.close()
    ctx.close()


if __name__ == "__main__":
    main()
