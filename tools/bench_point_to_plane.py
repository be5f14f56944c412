#!/usr/bin/env python3
"""Time per iteration of point-to-plane ICP on a closed hull of about M vertices (an ellipsoid as a latitude / longitude mesh) against
a perturbed copy of it, for the two routes the algorithm can take, in the same process on the same device:
  native_enqueued_us    gingr_fitter_update_plane_async, 20 iterations enqueued in one call: correspondence, planes, update and
                        sigma2 schedule on the device, nothing transferred or synchronised between iterations
  native_update_us      PointToPlaneIcpRegistration.update: one such iteration per call, the state read back after each
  template_update_us    the route it replaces: TemplateRegistration.update with the callbacks of examples/demo_point_to_plane.py
                        (closest points on the device through Context.mesh_closest_points, asked twice; normalTangentCovariances on
                        the host; the dense list uploaded, sorted and gathered; one pairs update; sigma2 set from the host)
  planes_step_us        gingr_fitter_set_pairs_plane_async alone: the surface scan and the kernel that writes the planes
  surface_icp_us        gingr_fitter_update_icp_surface_async per iteration, for scale (the same scan, isotropic weights)
Each figure is the median over 5 timed blocks from the same start state after a warm-up (the minimum is kept beside it); one run.
Writes profiles/point_to_plane_<M>_<rank>.json and prints it as one JSON line; no pass / fail threshold.
    usage: bench_point_to_plane.py [M] [rank]"""
import ctypes, json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RATIO, SCHEDULE = 100.0, (4.0, 1.0, 50)


def hull_mesh(M):
    """(vertices of the ellipsoid 50 (1, 0.7, 0.5) on a latitude / longitude grid with two poles, its triangles, unit normals)"""
    cols = max(8, int(round(np.sqrt(2.0 * M))))
    rows = max(2, (M - 2) // cols)
    axes = 50.0 * np.array([1.0, 0.7, 0.5])
    th = np.pi * (np.arange(rows) + 1.0) / (rows + 1.0)
    ph = 2.0 * np.pi * np.arange(cols) / cols
    T, P = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], -1).reshape(-1, 3)
    d = np.concatenate([[[0.0, 0.0, 1.0]], d, [[0.0, 0.0, -1.0]]])
    v = d * axes
    idx = 1 + np.arange(rows * cols).reshape(rows, cols)
    nxt = np.roll(idx, -1, axis=1)
    a, b, c, e = idx[:-1].ravel(), idx[1:].ravel(), nxt[:-1].ravel(), nxt[1:].ravel()
    south = 1 + rows * cols
    tris = np.concatenate([np.stack([a, b, c], 1), np.stack([b, e, c], 1),
                           np.stack([np.zeros(cols, dtype=np.int64), idx[0], nxt[0]], 1),
                           np.stack([np.full(cols, south), nxt[-1], idx[-1]], 1)]).astype(np.int32)
    n = v / (axes * axes)
    n /= np.linalg.norm(n, axis=1)[:, None]
    return v, tris, n


def perturbed(v, n):
    """the hull grown by a smooth 2 +- 0.5 along its normals and moved a little"""
    bump = 2.0 + 0.5 * np.sin(v[:, 0] / 9.0) * np.cos(v[:, 1] / 7.0)
    return v + bump[:, None] * n + np.array([0.5, -0.3, 0.2])


def timed(ctx, reset, step, n, repeats=5):
    out = []
    for _ in range(repeats):
        reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        step(n)
        ctx.synchronize()
        out.append((time.perf_counter() - t0) / n * 1e6)
    return statistics.median(out), min(out)


def measure(M, rank):
    import torch  # noqa: F401
    import gingr_amd as ga
    from gingr_amd import _native as nat
    from gingr_amd.api import _check
    from bench import synth_gpmm
    v, tris, normals = hull_mesh(M)
    target = perturbed(v, normals)
    basis, lam = synth_gpmm(v, rank)
    rank = int(lam.shape[0])
    ctx = ga.Context(0)
    model = ga.PointDistributionModel(v, np.zeros_like(v), basis, lam, cells=tris)
    res = {"what": "time per iteration of point-to-plane ICP, native route against the Template route it replaces; one run",
           "points": int(v.shape[0]), "triangles": int(tris.shape[0]), "rank": rank, "tangent_over_normal": RATIO}
    cfg = ga.PointToPlaneConfiguration(maxIterations=SCHEDULE[2], initialSigma=SCHEDULE[0], endSigma=SCHEDULE[1], tangentOverNormal=RATIO)
    algo = ga.PointToPlaneIcpRegistration(ctx)
    start = algo.createInitialState(model, target, cfg, targetCells=tris)
    algo.update(start)                                                          # binds the fitter; warm-up
    lib, h = algo._lib, algo._fitter
    pp_, ip_ = algo._params(cfg)

    def reset():
        algo._push_state(start.general)
        algo._device_state = None

    def enqueue(n):
        _check(ctx.handle, lib.gingr_fitter_update_plane_async(h, ctypes.byref(pp_), ctypes.byref(ip_), n), "gingr_fitter_update_plane_async")

    def planes(n):
        for _ in range(n):
            _check(ctx.handle, lib.gingr_fitter_set_pairs_plane_async(h, ctypes.byref(pp_)), "gingr_fitter_set_pairs_plane_async")

    def surface_icp(n):
        _check(ctx.handle, lib.gingr_fitter_update_icp_surface_async(h, ctypes.byref(ip_), n), "gingr_fitter_update_icp_surface_async")

    def class_updates(which, first):
        def go(n):
            s = first
            for _ in range(n):
                s = which.update(s)
            go.last = s
        return go

    enqueue(2)
    res["native_enqueued_us"], res["native_enqueued_us_min"] = timed(ctx, reset, enqueue, 20)
    res["planes_step_us"], res["planes_step_us_min"] = timed(ctx, reset, planes, 20)
    surface_icp(2)
    res["surface_icp_us"], res["surface_icp_us_min"] = timed(ctx, reset, surface_icp, 20)
    native = class_updates(algo, start)
    res["native_update_us"], res["native_update_us_min"] = timed(ctx, lambda: None, native, 5)

    # the route it replaces: the callbacks of examples/demo_point_to_plane.py, ICP's linear schedule
    a, b, c = (target[tris[:, k]] for k in range(3))
    cell_normals = np.cross(b - a, c - a)

    def closest(state):
        cp, _, tid, _ = ctx.mesh_closest_points(state.general.fit, target, tris)
        return cp, tid

    def correspondence(state):
        return ga.CorrespondencePairs(np.arange(v.shape[0]), closest(state)[0])

    def uncertainty(pids, state):
        s2 = state.general.sigma2
        return ga.normalTangentCovariances(cell_normals[closest(state)[1][pids]], s2, RATIO * s2)

    tmpl = ga.TemplateRegistration(ctx, correspondence, uncertainty, updateSigma2=lambda s: max(s.general.sigma2 - cfg.sigmaStep, cfg.endSigma),
                                   covariancePass="gram")
    tstart = ga.TemplateRegistrationState(start.general, ga.TemplateConfiguration(maxIterations=SCHEDULE[2]))
    tmpl.update(tstart)                                                         # warm-up
    template = class_updates(tmpl, tstart)
    res["template_update_us"], res["template_update_us_min"] = timed(ctx, lambda: None, template, 5)
    res["template_over_native_update"] = res["template_update_us"] / res["native_update_us"]
    res["template_over_native_enqueued"] = res["template_update_us"] / res["native_enqueued_us"]
    fa, fb = np.asarray(native.last.general.fit), np.asarray(template.last.general.fit)
    res["native_against_template_rel_fit_after_5"] = float(np.linalg.norm(fa - fb) / np.linalg.norm(fb))
    res["status"] = [int(native.last.general.status), int(template.last.general.status)]
    tmpl.close()
    algo.close()
    ctx.close()
    return res


if __name__ == "__main__":
    nums = [int(x) for x in sys.argv[1:] if not x.startswith("--")]
    M = nums[0] if len(nums) > 0 else 50000
    rank = nums[1] if len(nums) > 1 else 100
    out = measure(M, rank)
    path = os.path.join(ROOT, "profiles", f"point_to_plane_{M}_{out['rank']}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
