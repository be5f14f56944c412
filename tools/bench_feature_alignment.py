#!/usr/bin/env python3
"""Feature-based global alignment (classic.FeatureRigidAlignment: descriptors, their match, poses from triples, one scoring call, one
refining call), timed stage by stage on a template of M points against a PARTIAL target (its lower third along the longest axis cut
away) under a random rigid motion; one run, same process, same device:
  call_us           FeatureRigidAlignment.register, from call to return
  stages            Context.cloud_normals (both clouds), Context.cloud_fpfh (both), Context.feature_match (both ways), the host's draw
                    and edge filter, Context.rigid_poses_from_triples, the scoring call and the refining call of
                    Context.rigid_search_poses -- each from call to return, uploads and read-backs included
  host_us           the numpy / scipy.spatial.cKDTree restatement (tests/feature_alignment_restatement.py: align) on the host
  rigid_search_us   Context.rigid_search with 64 spiral starts and 10 iterations at the same overlap on the same input, for scale
  split             HIP-event time of one more call by kernel group (gingr_ctx_timing_*): descriptor (SPFH + FPFH), match, triples,
                    and of the two searches: nearest-neighbour search, sums, the rest
Without arguments: the femur pair of tests/golden (template femur[::4], 406 points), radius 25, inlier distance 3.  With M and N: an
asymmetric bumpy ellipsoid sampled with M and with N points, radius and inlier distance from the template's spacing.
Each figure is the median over 5 timed blocks after a warm-up (the minimum beside it; the host restatement: one block above 10 000
target points, else 3).  Writes profiles/feature_alignment_<M>_<N>.json with the date and prints it as a JSON line; no pass / fail
threshold.
    usage: bench_feature_alignment.py [M] [N]"""
import datetime, json, os, statistics, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shape(n, seed):
    """n points of a bumpy ellipsoid without a symmetry (jittered Fibonacci directions)"""
    rng = np.random.default_rng(seed)
    i = np.arange(n) + 0.5
    z = 1.0 - 2.0 * i / n
    phi = i * np.pi * (3.0 - np.sqrt(5.0)) + rng.uniform(0, 0.3, n)
    u = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], axis=1)
    r = 1.0 + 0.35 * u[:, 0] + 0.25 * u[:, 1] * u[:, 2] + 0.2 * np.sin(3.0 * u[:, 2] + u[:, 0])
    return u * r[:, None] * [120.0, 45.0, 30.0]


def wall(fn, repeats=5):
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out), min(out)


def measure(M, N):
    import torch  # noqa: F401
    import gingr_amd as ga
    from gingr_amd import classic
    from tests import feature_alignment_restatement as fa
    from tests import rigid_search_restatement as rs
    rng = np.random.default_rng(2)
    R_true = rs.random_rotation(rng)
    shift = rng.normal(size=3) * 100.0
    if M is None:
        femur, tgt = rs.femur_pair()
        X, whole, radius, distance = np.ascontiguousarray(femur[::4]), tgt, 25.0, 3.0
    else:
        X, whole = shape(M, 1), shape(N, 3)
        spacing = float(np.sqrt(4.0 * np.pi * 60.0 ** 2 / M))                  # (of a sphere of the shape's middle radius: a scale, no more)
        radius, distance = 5.0 * spacing, 0.6 * spacing
    part = fa.partial_target(whole)
    Y = np.ascontiguousarray(part @ R_true.T + shift)
    M, N = X.shape[0], Y.shape[0]
    ctx = ga.Context(0)
    res = {"what": "feature-based global alignment on a partial target, stage by stage, against the host restatement; one run",
           "date": datetime.date.today().isoformat(), "moving_points": M, "target_points": N, "target_points_before_the_cut": int(whole.shape[0]),
           "radius": radius, "inlier_distance": distance, "hypotheses": 2000, "edge_similarity": 0.8, "overlap": 0.6, "refine_iterations": 30}
    align = classic.FeatureRigidAlignment(ctx, X, radius, inlierDistance=distance)
    align.register(Y)                                                          # warm-up
    res["call_us"], res["call_us_min"] = wall(lambda: align.register(Y))
    res["info"] = dict(align.info)
    res["degrees_from_truth_hypothesis"] = rs.angle_deg(align.searchResult.R, R_true)
    res["degrees_from_truth_refined"] = rs.angle_deg(align.transform[0], R_true)

    stages = {}
    nx, ny = ctx.cloud_normals(X, 12, viewpoint=X.mean(0))[0], ctx.cloud_normals(Y, 12, viewpoint=Y.mean(0))[0]
    stages["normals_us"], _ = wall(lambda: (ctx.cloud_normals(X, 12, viewpoint=X.mean(0)), ctx.cloud_normals(Y, 12, viewpoint=Y.mean(0))))
    fx, fy = ctx.cloud_fpfh(X, nx, 64, radius)[0], ctx.cloud_fpfh(Y, ny, 64, radius)[0]
    stages["fpfh_us"], _ = wall(lambda: (ctx.cloud_fpfh(X, nx, 64, radius), ctx.cloud_fpfh(Y, ny, 64, radius)))
    match = ctx.feature_match(fx, fy)[0].astype(np.int64)
    stages["match_us"], _ = wall(lambda: (ctx.feature_match(fx, fy), ctx.feature_match(fy, fx)))
    back = ctx.feature_match(fy, fx)[0].astype(np.int64)
    pool = fa.mutual_pool(match, back)[0]
    drawn = {}

    def draw():
        tri = fa.draw_triples(pool, 2000, 0)
        drawn["tri"] = tri[fa.edge_similar(X, Y, tri, match, 0.8)]

    stages["draw_and_filter_host_us"], _ = wall(draw)
    tri = drawn["tri"]
    assert np.array_equal(tri, align.triples)
    poses = ctx.rigid_poses_from_triples(X, Y, tri, match[tri])[0]
    stages["triples_us"], _ = wall(lambda: ctx.rigid_poses_from_triples(X, Y, tri, match[tri]))
    scored = ctx.rigid_search_poses(X, Y, poses, 0, 1.0, distance, 1)
    stages["score_us"], _ = wall(lambda: ctx.rigid_search_poses(X, Y, poses, 0, 1.0, distance, 1))
    start = np.concatenate([scored.R.reshape(9), scored.t])[None]
    stages["refine_us"], _ = wall(lambda: ctx.rigid_search_poses(X, Y, start, 30, 0.6, distance, 1))
    stages["sum_us"] = sum(stages.values())
    res["stages"] = stages

    host = {}

    def restatement():
        host["res"] = fa.align(X, Y, radius, inlier_distance=distance)

    res["host_us"], res["host_us_min"] = wall(restatement, 1 if N > 10000 else 3)
    res["host_over_call"] = res["host_us"] / res["call_us"]
    res["host_degrees_from_truth_refined"] = rs.angle_deg(host["res"]["R"], R_true)
    res["host_info"] = host["res"]["info"]

    ctx.rigid_search(X, Y, 64, 10, 0.6)
    res["rigid_search_64_10_us"], res["rigid_search_64_10_us_min"] = wall(lambda: ctx.rigid_search(X, Y, 64, 10, 0.6))
    res["rigid_search_64_10_degrees_from_truth"] = rs.angle_deg(ctx.rigid_search(X, Y, 64, 10, 0.6).R, R_true)

    ctx.timing_enable(True)
    ctx.timing_reset()
    align.register(Y)
    ctx.synchronize()
    split = {}
    for name, which in (("descriptor", 27), ("match", 28), ("triples", 29), ("search", 8), ("selection", 24), ("sums", 25), ("rest", 26)):
        ms, n = ctx.timing_read(which)
        split[name + "_us"], split[name + "_launches"] = ms * 1e3, n
    ctx.timing_enable(False)
    split["device_total_us"] = sum(v for k, v in split.items() if k.endswith("_us"))
    res["split"] = split
    ctx.close()
    return res


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if not x.startswith("--")]
    M = int(args[0]) if len(args) > 0 else None
    N = int(args[1]) if len(args) > 1 else (50000 if M is not None else None)
    res = measure(M, N)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    name = f"feature_alignment_{res['moving_points']}_{res['target_points_before_the_cut']}.json"
    with open(os.path.join(ROOT, "profiles", name), "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
