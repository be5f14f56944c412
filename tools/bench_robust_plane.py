#!/usr/bin/env python3
"""Time per iteration of ROBUST point-to-plane ICP on the hull of tools/bench_point_to_plane.py (about M vertices against a perturbed
copy of it), all in the same process on the same device:
  plain_enqueued_us            gingr_fitter_update_plane_async with the robust setting off: the path before this setting existed
  robust_fixed_enqueued_us     the same loop with Cauchy weights at a fixed scale c (the selection still runs: c is chosen behind it)
  robust_median_enqueued_us    ... with the median scale, c = 2.385 * 1.4826 * sqrt(lower median of s) found on the device
  plain_planes_step_us / robust_planes_step_us
                               gingr_fitter_set_pairs_plane_async alone, setting off / on: the surface scan and the plane kernel,
                               against the scan, the residual kernel, the selection's ten launches and the robust plane kernel
  robust_extra_us, _share      their difference -- what the residuals and the selection add to an iteration -- and its share of
                               robust_median_enqueued_us
  template_update_us           TemplateRegistration.update with callbacks that apply the same formula on the host (closest points on
                               the device, residuals, median and covariances in numpy, the dense list uploaded)
Each figure is the median over 5 timed blocks from the same start state after a warm-up (the minimum beside it); one run.
Writes profiles/robust_plane_<M>_<rank>.json and prints it as one JSON line; no pass / fail threshold.
    usage: bench_robust_plane.py [M] [rank]"""
import ctypes, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_point_to_plane import RATIO, SCHEDULE, hull_mesh, perturbed, timed  # noqa: E402

TUNING, MAD, FIXED_C = 2.385, 1.4826, 5.0


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
    res = {"what": "time per iteration of robust point-to-plane ICP (Cauchy), fixed and median scale, against the plain loop and the "
                   "Template route with the same formula; one run",
           "points": int(v.shape[0]), "triangles": int(tris.shape[0]), "rank": rank, "tangent_over_normal": RATIO}
    cfg = ga.PointToPlaneConfiguration(maxIterations=SCHEDULE[2], initialSigma=SCHEDULE[0], endSigma=SCHEDULE[1], tangentOverNormal=RATIO)
    algo = ga.PointToPlaneIcpRegistration(ctx)
    start = algo.createInitialState(model, target, cfg, targetCells=tris)
    algo.update(start)                                                          # binds the fitter; warm-up
    lib, h = algo._lib, algo._fitter
    pp_, _, ip_ = algo._params(cfg)

    def reset():
        algo._push_state(start.general)
        algo._device_state = None

    def setting(params):
        rp = None if params is None else nat.RobustParams(*params)
        _check(ctx.handle, lib.gingr_fitter_set_plane_robust(h, None if rp is None else ctypes.byref(rp)), "gingr_fitter_set_plane_robust")

    def enqueue(n):
        _check(ctx.handle, lib.gingr_fitter_update_plane_async(h, ctypes.byref(pp_), ctypes.byref(ip_), n), "gingr_fitter_update_plane_async")

    def planes(n):
        for _ in range(n):
            _check(ctx.handle, lib.gingr_fitter_set_pairs_plane_async(h, ctypes.byref(pp_)), "gingr_fitter_set_pairs_plane_async")

    for name, params in (("plain", None), ("robust_fixed", (1, 0, FIXED_C, 0.0)), ("robust_median", (1, 1, TUNING, 0.0))):
        setting(params)
        enqueue(2)
        res[name + "_enqueued_us"], res[name + "_enqueued_us_min"] = timed(ctx, reset, enqueue, 20)
        if name != "robust_fixed":
            key = "plain_planes_step_us" if params is None else "robust_planes_step_us"
            res[key], res[key + "_min"] = timed(ctx, reset, planes, 20)
    u, c, n = np.empty(v.shape[0]), ctypes.c_double(), ctypes.c_int64()
    _check(ctx.handle, lib.gingr_fitter_get_plane_robust(h, None, u.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, ctypes.byref(c),
                                                         ctypes.byref(n)), "gingr_fitter_get_plane_robust")
    res["median_scale_c"], res["observed"], res["weighted"] = float(c.value), int(n.value), int((u > 1.0).sum())
    setting(None)
    res["robust_extra_us"] = res["robust_planes_step_us"] - res["plain_planes_step_us"]
    res["robust_extra_share"] = res["robust_extra_us"] / res["robust_median_enqueued_us"]
    res["robust_median_over_plain"] = res["robust_median_enqueued_us"] / res["plain_enqueued_us"]

    # the same formula through callbacks: the route this setting replaces
    a, b, cc = (target[tris[:, k]] for k in range(3))
    cell_normals = np.cross(b - a, cc - a)
    cell_normals /= np.linalg.norm(cell_normals, axis=1)[:, None]
    memo = {}

    def closest(state):
        if memo.get("state") is not state:
            cp, _, tid, _ = ctx.mesh_closest_points(state.general.fit, target, tris)
            d, nrm = state.general.fit - cp, cell_normals[tid]
            en = (d * nrm).sum(1)
            s = en * en + np.maximum((d * d).sum(1) - en * en, 0.0) / RATIO
            k = (s.shape[0] - 1) // 2
            scale = TUNING * MAD * np.sqrt(np.partition(s, k)[k])
            memo.update(state=state, cp=cp, nrm=nrm, u=1.0 + s / scale ** 2 if scale > 0 else np.ones_like(s))
        return memo

    def correspondence(state):
        return ga.CorrespondencePairs(np.arange(v.shape[0]), closest(state)["cp"])

    def uncertainty(pids, state):
        m = closest(state)
        vn = state.general.sigma2 * m["u"][pids]
        return ga.normalTangentCovariances(m["nrm"][pids], vn, RATIO * vn)

    def class_updates(which, first):
        def go(k):
            s = first
            for _ in range(k):
                s = which.update(s)
            go.last = s
        return go

    rcfg = ga.PointToPlaneConfiguration(maxIterations=SCHEDULE[2], initialSigma=SCHEDULE[0], endSigma=SCHEDULE[1], tangentOverNormal=RATIO,
                                        robust=ga.RobustLoss("cauchy"))
    rstart = algo.createInitialState(model, target, rcfg, targetCells=tris)
    native = class_updates(algo, rstart)
    native(1)
    res["robust_update_us"], res["robust_update_us_min"] = timed(ctx, lambda: None, native, 5)
    tmpl = ga.TemplateRegistration(ctx, correspondence, uncertainty, updateSigma2=lambda s: max(s.general.sigma2 - cfg.sigmaStep, cfg.endSigma),
                                   covariancePass="gram")
    tstart = ga.TemplateRegistrationState(start.general, ga.TemplateConfiguration(maxIterations=SCHEDULE[2]))
    tmpl.update(tstart)                                                         # warm-up
    template = class_updates(tmpl, tstart)
    res["template_update_us"], res["template_update_us_min"] = timed(ctx, lambda: None, template, 5)
    res["template_over_robust_enqueued"] = res["template_update_us"] / res["robust_median_enqueued_us"]
    fa, fb = np.asarray(native.last.general.fit), np.asarray(template.last.general.fit)
    res["robust_against_template_rel_fit_after_5"] = float(np.linalg.norm(fa - fb) / np.linalg.norm(fb))
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
    path = os.path.join(ROOT, "profiles", f"robust_plane_{M}_{out['rank']}.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))
