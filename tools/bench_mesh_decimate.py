"""Timing of the mesh decimation (Context.mesh_decimate, gingr_mesh_decimate) beside the host route it replaces
(gingr_amd.simple.cluster_decimate) on the same box, warm:  bench_mesh_decimate.py [M] [n_target]   (default 50176 100).
M = 1622 takes the femur fixture of the tests, any other M a height-field grid of about M vertices (224 x 224 = 50 176 vertices,
99 458 triangles).  The two results are compared (they have to be equal), the device call is timed as a whole (wall clock, median) and
per stage by the context's event timers 13 .. 16 -- once with the bisection's steps enqueued sixteen per read-back of the control
block (the default) and once with one read-back per step --, and everything is written to profiles/mesh_decimate_<M>_<n>.json.
Not the benchmark metric."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: one HIP runtime per process)

import gingr_amd as ga  # noqa: E402
from gingr_amd import _native as nat  # noqa: E402
from gingr_amd.simple import cluster_decimate  # noqa: E402

STAGES = {13: "bounding_box", 14: "bisection", 15: "clusters_and_representatives", 16: "compaction"}


def grid_surface(m: int):
    u = np.linspace(0.0, 1.0, m)
    U, V = np.meshgrid(u, u, indexing="ij")
    rng = np.random.default_rng(m)
    v = np.stack([200.0 * U + rng.normal(0.0, 0.05, U.shape), 200.0 * V + rng.normal(0.0, 0.05, U.shape),
                  30.0 * np.sin(5.0 * U) * np.cos(4.0 * V) + 10.0 * U * V], axis=-1).reshape(-1, 3)
    i = np.arange(m * m).reshape(m, m)
    a, b, c, d = i[:-1, :-1].ravel(), i[1:, :-1].ravel(), i[:-1, 1:].ravel(), i[1:, 1:].ravel()
    return v, np.concatenate([np.stack([a, b, c], axis=1), np.stack([b, d, c], axis=1)], axis=0).astype(np.int32)


def time_device(ctx, v, tri, n_target, reps):
    for _ in range(3):
        ctx.mesh_decimate(v, tri, n_target)                # warm-up: code objects, allocator
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.mesh_decimate(v, tri, n_target)
        wall.append(time.perf_counter() - t0)
    ctx.timing_enable(True)
    ctx.timing_reset()
    for _ in range(reps):
        ctx.mesh_decimate(v, tri, n_target)
    stages = {name: 1e3 * ctx.timing_read(which)[0] / reps for which, name in STAGES.items()}
    ctx.timing_enable(False)
    return {"call_us_median": 1e6 * float(np.median(wall)), "call_us_min": 1e6 * float(np.min(wall)), "stage_us": stages}


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 50176
    n_target = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    if M == 1622:
        v = np.load(os.path.join(ROOT, "tests", "golden", "inputs.npz"))["femur"].astype(np.float64)
        tri = np.asarray(np.load(os.path.join(ROOT, "tests", "golden", "femur_mesh.npz"))["femur_cells"], dtype=np.int32)
    else:
        v, tri = grid_surface(max(2, int(round(M ** 0.5))))
    ctx = ga.Context(0)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        want_v, want_c = cluster_decimate(v, tri, n_target)
        host.append(time.perf_counter() - t0)
    kept, cells, h = ctx.mesh_decimate(v, tri, n_target)
    equal = bool(np.array_equal(v[kept], want_v) and np.array_equal(cells, want_c))
    out = {"vertices": int(v.shape[0]), "triangles": int(tri.shape[0]), "n_target": n_target, "kept_vertices": int(kept.shape[0]),
           "kept_triangles": int(cells.shape[0]), "cube_size": h, "equal_to_the_host_definition": equal,
           "host_cluster_decimate_ms_median": 1e3 * float(np.median(host))}
    reps = 20
    out["device_steps_enqueued_16_per_read_back"] = time_device(ctx, v, tri, n_target, reps)
    ctx.set_option(nat.OPT_DECIMATE_BATCH, 1)
    out["device_one_read_back_per_step"] = time_device(ctx, v, tri, n_target, reps)
    ctx.set_option(nat.OPT_DECIMATE_BATCH, 16)
    out["host_over_device"] = 1e3 * out["host_cluster_decimate_ms_median"] / out["device_steps_enqueued_16_per_read_back"]["call_us_median"]
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    path = os.path.join(ROOT, "profiles", f"mesh_decimate_{v.shape[0]}_{n_target}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    ctx.close()
    if not equal:
        sys.exit("the device result differs from cluster_decimate")


if __name__ == "__main__":
    main()
