#!/usr/bin/env python3
"""Point-to-plane ICP against a point cloud, timed on a closed hull of about N vertices (the ellipsoid of tools/bench_point_to_plane.py)
against a perturbed copy of it whose vertices alone are the target; one run, same process, same device:
  (a) normals      cloud_knn_us / cloud_normals_us: Context.cloud_knn and Context.cloud_normals on the target's N points, call to
                   return (upload, grid build, search, download); estimate_us: gingr_fitter_estimate_target_normals on the target as it
                   lies on the device.  Beside them on the same box: scipy.spatial.cKDTree(...).query(k, workers=16) and a batched
                   numpy.linalg.eigh of the neighbourhoods' covariances (cpu_kdtree_us, cpu_eigh_us).  largest_sin_to_numpy_eigh
                   compares the two sets of normals as a plausibility figure only: the mesh has exact ties at the k-th distance,
                   which the k-d tree resolves otherwise than by index, so a few neighbourhoods differ by a point (the accuracy
                   check is tests/test_gpu_cloud_normals.py).
  (b) iterations   cloud_enqueued_us: gingr_fitter_update_plane_cloud_async, 20 iterations enqueued in one call; in the same run the
                   surface point-to-plane iteration (gingr_fitter_update_plane_async) and the point-cloud ICP iteration
                   (gingr_fitter_update_icp_async).
Each figure is the median over 5 timed blocks after a warm-up (the minimum beside it).  Writes profiles/cloud_normals_<N>_<k>.json and
profiles/point_to_plane_cloud_<N>_<rank>.json and prints both as JSON lines; no pass / fail threshold.
    usage: bench_cloud_point_to_plane.py [N] [k] [rank]"""
import ctypes, json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_point_to_plane import RATIO, SCHEDULE, hull_mesh, perturbed, timed  # noqa: E402


def wall(fn, repeats=5):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out), min(out)


def measure(N, k, rank):
    import torch  # noqa: F401
    import gingr_amd as ga
    from gingr_amd import _native as nat
    from gingr_amd.api import _check
    from bench import synth_gpmm
    v, tris, normals = hull_mesh(N)
    target = np.ascontiguousarray(perturbed(v, normals))
    ctx = ga.Context(0)
    # ---- (a) neighbours and normals
    info = {}
    ctx.cloud_knn(target, k, info)
    dev_normals, _ = ctx.cloud_normals(target, k)                               # warm-up
    na = {"what": "k nearest neighbours and k-NN normals of a cloud, device against scipy + numpy on the same box; one run",
          "points": int(target.shape[0]), "k": k, "grid": list(info["grid"]), "cell_size": info["cell_size"], "flagged": info["flagged"]}
    na["cloud_knn_us"], na["cloud_knn_us_min"] = wall(lambda: ctx.cloud_knn(target, k))
    na["cloud_normals_us"], na["cloud_normals_us_min"] = wall(lambda: ctx.cloud_normals(target, k))
    from scipy.spatial import cKDTree
    keep = {}

    def kdtree():
        keep["idx"] = cKDTree(target).query(target, k, workers=16)[1]

    def eigh():
        q = target[keep["idx"]] - target[:, None, :]
        q = q - q.mean(1, keepdims=True)
        keep["n"] = np.linalg.eigh(np.einsum("nki,nkj->nij", q, q) / k)[1][:, :, 0]

    na["cpu_kdtree_us"], na["cpu_kdtree_us_min"] = wall(kdtree, 3)
    na["cpu_eigh_us"], na["cpu_eigh_us_min"] = wall(eigh, 3)
    na["cpu_over_device_normals"] = (na["cpu_kdtree_us"] + na["cpu_eigh_us"]) / na["cloud_normals_us"]
    ok = np.linalg.norm(dev_normals, axis=1) > 0
    na["zero_normals"] = int((~ok).sum())
    na["largest_sin_to_numpy_eigh"] = float(np.sqrt(1.0 - np.minimum(1.0, np.abs((dev_normals[ok] * keep["n"][ok]).sum(1))) ** 2).max())
    na["median_angle_to_hull_normal_deg"] = float(np.degrees(np.median(np.arccos(np.minimum(1.0, np.abs((dev_normals[ok] * normals[ok]).sum(1)))))))
    # ---- (b) iterations
    basis, lam = synth_gpmm(v, rank)
    rank = int(lam.shape[0])
    model = ga.PointDistributionModel(v, np.zeros_like(v), basis, lam, cells=tris)
    cfg = ga.PointToPlaneConfiguration(maxIterations=SCHEDULE[2], initialSigma=SCHEDULE[0], endSigma=SCHEDULE[1], tangentOverNormal=RATIO)
    res = {"what": "time per iteration: point-to-plane ICP against the target's vertices, the surface route and point-cloud ICP; one run",
           "points": int(v.shape[0]), "rank": rank, "k": k, "tangent_over_normal": RATIO}
    algo = ga.PointToPlaneIcpRegistration(ctx)
    start = algo.createInitialState(model, target, cfg, targetCells=tris)
    algo.update(start)                                                          # binds the fitter (meshes included); warm-up
    lib, h = algo._lib, algo._fitter
    pp_, pc_, ip_ = algo._params(cfg)
    ki = nat.CloudKnnInfo()

    def estimate():
        _check(ctx.handle, lib.gingr_fitter_estimate_target_normals(h, k, None, ctypes.byref(ki)), "gingr_fitter_estimate_target_normals")

    estimate()
    na["estimate_us"], na["estimate_us_min"] = wall(estimate)

    def reset():
        algo._push_state(start.general)
        algo._device_state = None

    def cloud(n):
        _check(ctx.handle, lib.gingr_fitter_update_plane_cloud_async(h, ctypes.byref(pc_), ctypes.byref(ip_), n), "gingr_fitter_update_plane_cloud_async")

    def surface(n):
        _check(ctx.handle, lib.gingr_fitter_update_plane_async(h, ctypes.byref(pp_), ctypes.byref(ip_), n), "gingr_fitter_update_plane_async")

    def icp(n):
        _check(ctx.handle, lib.gingr_fitter_update_icp_async(h, ctypes.byref(ip_), n), "gingr_fitter_update_icp_async")

    def cloud_planes(n):
        for _ in range(n):
            _check(ctx.handle, lib.gingr_fitter_set_pairs_plane_cloud_async(h, ctypes.byref(pc_)), "gingr_fitter_set_pairs_plane_cloud_async")

    for name, step in (("cloud_enqueued_us", cloud), ("surface_enqueued_us", surface), ("pointcloud_icp_us", icp), ("cloud_planes_step_us", cloud_planes)):
        step(2)
        res[name], res[name + "_min"] = timed(ctx, reset, step, 20)
    res["surface_over_cloud"] = res["surface_enqueued_us"] / res["cloud_enqueued_us"]
    # where the two routes end from the same start (20 iterations each), against the true target surface
    for name, step in (("cloud", cloud), ("surface", surface), ("pointcloud_icp", icp)):
        reset()
        step(20)
        g = algo._pull_state(start.general)
        s, mx, n, _ = ctx.mesh_distance_stats(np.asarray(g.fit), target, tris)
        res[name + "_avg_distance_after_20"] = s / n
    algo.close()
    ctx.close()
    return na, res


if __name__ == "__main__":
    nums = [int(x) for x in sys.argv[1:] if not x.startswith("--")]
    N = nums[0] if len(nums) > 0 else 50000
    k = nums[1] if len(nums) > 1 else 16
    rank = nums[2] if len(nums) > 2 else 100
    na, res = measure(N, k, rank)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    for path, out in ((f"cloud_normals_{N}_{k}.json", na), (f"point_to_plane_cloud_{N}_{res['rank']}.json", res)):
        with open(os.path.join(ROOT, "profiles", path), "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
        print(json.dumps(out))
