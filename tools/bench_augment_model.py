"""Timing of a resident model augmented with a second one (gingr_model_augment) and of the host route it replaces: download of both
bases, numpy concatenate, Gram matrix, eigh, product, gingr_model_upload of the result.  Both start from two finalized resident models
and end with a finalized resident model.  Beside the whole call: the cross Gram pass and the two-source basis pass alone (device
timers 11 and 12, HIP events on the context's stream) with their share of the float64 MFMA peak and of the HBM bandwidth a streaming
copy reaches, and -- for the comparison per flop -- basis_rotate_kernel (timer 10) on the result, whose one source is as wide as the
two sources together.  The two models carry different per-vertex mean displacements, so their row orders and the result's differ.
Writes profiles/augment_model_<M>_<ra>_<rb>.json and prints the same document.  Not the benchmark metric.
Usage: python tools/bench_augment_model.py [M] [ra] [rb]      (defaults 50000, 8, 256)"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: one HIP runtime per process)
import gingr_amd as ga  # noqa: E402

HBM_BYTES_PER_S = 6.29e12      # a streaming copy on an MI355X
F64_MFMA_FLOPS = 78.6e12       # v_mfma_f64_16x16x4_f64 peak


def pad(r):
    return (r + 15) // 16 * 16


def random_model(rng, ref, r, top, mean_size):
    M = ref.shape[0]
    basis = np.asfortranarray(rng.standard_normal((3 * M, r)) / np.sqrt(3.0 * M))
    return ga.PointDistributionModel(ref, rng.normal(0.0, mean_size, (M, 3)), basis, top * 1e-3 ** (np.arange(r) / max(r - 1, 1)))


def host_route(ctx, da, db, rel_tol=1e-10):
    t = {}
    t0 = time.perf_counter()
    ha, hb = da.download(), db.download()
    t["download"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    F = np.concatenate([np.asarray(ha.basis) * np.sqrt(ha.variance)[None], np.asarray(hb.basis) * np.sqrt(hb.variance)[None]], axis=1)
    t["concatenate"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    G = F.T @ F
    t["gram"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    lam, V = np.linalg.eigh(G)
    lam, V = lam[::-1].copy(), np.ascontiguousarray(V[:, ::-1])      # (a reversed view would take the product off the BLAS path)
    k = int(min(512, (lam > rel_tol * lam[0]).sum()))
    t["eigh"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    Q0 = F @ V[:, :k]
    model = ga.PointDistributionModel(ha.reference, ha.mean + hb.mean, np.asfortranarray(Q0 / np.sqrt(lam[:k])[None]), lam[:k].copy())
    t["product"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    dm = ga.DeviceModel(ctx, model)
    ctx.synchronize()
    t["upload"] = time.perf_counter() - t0
    return dm, t, lam[:k]


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    M = int(sys.argv[1]) if len(sys.argv) > 1 else 50000
    ra = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    rb = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    rng = np.random.default_rng(5)
    ref = rng.normal(0, 100, (M, 3))
    ctx = ga.Context(0)
    ma, mb = random_model(rng, ref, ra, 400.0, 3.0), random_model(rng, ref, rb, 90.0, 2.0)
    da, db = ga.DeviceModel(ctx, ma), ga.DeviceModel(ctx, mb)
    rpa, rpb = pad(ra), pad(rb)

    # the whole call, to the finalized model: median of three after a warm-up, timers off
    whole = []
    for rep in range(4):
        t0 = time.perf_counter()
        dm = da.augment(db)
        ctx.synchronize()
        dt = 1e3 * (time.perf_counter() - t0)
        if rep:
            whole.append(dt)
        if rep < 3:
            dm.close()
    k, kp = dm.rank, pad(dm.rank)
    dev_lam = dm.download(basis=False).variance

    # the two passes alone: HIP events around each launch (timers 11, 12), median of three calls each read on its own
    ctx.timing_enable(True)
    cross, rot2 = [], []
    for rep in range(3):
        ctx.timing_reset()
        da.augment(db).close()
        cross.append(1e3 * ctx.timing_read(11)[0])
        rot2.append(1e3 * ctx.timing_read(12)[0])
    # the same two bases with zero means: all three row orders are the reference's, every gather is the identity
    ma.mean, mb.mean = np.zeros_like(ref), np.zeros_like(ref)
    da0, db0 = ga.DeviceModel(ctx, ma), ga.DeviceModel(ctx, mb)
    da0.augment(db0).close()
    cross0, rot20 = [], []
    for rep in range(3):
        ctx.timing_reset()
        da0.augment(db0).close()
        cross0.append(1e3 * ctx.timing_read(11)[0])
        rot20.append(1e3 * ctx.timing_read(12)[0])
    da0.close()
    db0.close()
    # basis_rotate_kernel on the result (one source of rp = kp columns, result kp columns): the posterior of two landmarks
    lm = ga.LandmarkCorrespondences(np.array([0, M // 2], dtype=np.int32), (ref + dm.host.mean)[[0, M // 2]] + 1.0, np.tile(np.eye(3), (2, 1, 1)))
    dm.posterior(np.zeros((M, 3)), np.zeros(M), landmarks=lm).close()
    rot1 = []
    for rep in range(3):
        ctx.timing_reset()
        dm.posterior(np.zeros((M, 3)), np.zeros(M), landmarks=lm).close()
        rot1.append(1e3 * ctx.timing_read(10)[0])
    ctx.timing_enable(False)
    dm.close()

    # the host route: median of three after a warm-up
    runs = []
    for rep in range(4):
        t0 = time.perf_counter()
        hm, parts, host_lam = host_route(ctx, da, db)
        dt = 1e3 * (time.perf_counter() - t0)
        hm.close()
        if rep:
            runs.append((dt, parts))
    runs.sort(key=lambda x: x[0])
    host_ms, host_parts = runs[len(runs) // 2]

    cross_us, rot2_us, rot1_us = median(cross), median(rot2), median(rot1)
    cross_flop, cross_bytes = 6.0 * M * rpa * rpb, 24.0 * M * (rpa + rpb)
    rot2_flop, rot2_bytes = 6.0 * M * (rpa + rpb) * kp, 24.0 * M * (rpa + rpb + kp)
    rot1_flop, rot1_bytes = 6.0 * M * kp * kp, 48.0 * M * kp

    def kernel(us, flop, nbytes):
        return {"us": us, "gflop": flop / 1e9, "megabytes": nbytes / 1e6, "tflops": flop / us / 1e6,
                "fraction_of_f64_mfma_peak": flop / (us * 1e-6) / F64_MFMA_FLOPS, "fraction_of_hbm_bandwidth": nbytes / (us * 1e-6) / HBM_BYTES_PER_S}

    out = {"M": M, "ra": ra, "rb": rb, "rank": int(k), "threads": os.environ.get("OMP_NUM_THREADS", ""),
           "whole_call_ms": {"median": median(whole), "min": min(whole), "max": max(whole)},
           "cross_gram_kernel": kernel(cross_us, cross_flop, cross_bytes),
           "basis_rotate2_kernel": kernel(rot2_us, rot2_flop, rot2_bytes),
           "basis_rotate_kernel_same_width": dict(kernel(rot1_us, rot1_flop, rot1_bytes), source_columns=kp, result_columns=kp),
           "rotate2_ns_per_gflop_over_rotate_ns_per_gflop": (rot2_us / rot2_flop) / (rot1_us / rot1_flop),
           "same_row_order_us": {"cross_gram_kernel": median(cross0), "basis_rotate2_kernel": median(rot20),
                                 "rotate2_ns_per_gflop_over_rotate_ns_per_gflop": (median(rot20) / rot2_flop) / (rot1_us / rot1_flop)},
           "all_samples_us": {"cross_gram": cross, "basis_rotate2": rot2, "basis_rotate": rot1, "cross_gram_same_row_order": cross0,
                              "basis_rotate2_same_row_order": rot20},
           "host_route_ms": dict({n: 1e3 * v for n, v in host_parts.items()}, total=host_ms),
           "host_route_over_device": host_ms / median(whole),
           "largest_eigenvalue_difference_device_against_host_route": float(np.abs(dev_lam[:min(k, len(host_lam))] - host_lam[:k]).max() / host_lam[0])}
    path = os.path.join(ROOT, "profiles", f"augment_model_{M}_{ra}_{rb}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    da.close()
    db.close()


if __name__ == "__main__":
    main()
