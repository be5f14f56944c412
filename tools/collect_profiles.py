#!/usr/bin/env python3
"""Copy the judged summaries of one `tools/final_profile.sh` run (gpurun_out/final/) into profiles/rNN_*.
    python tools/collect_profiles.py [round=02]"""
import json
import os
import shutil
import sys

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
rnd = sys.argv[1] if len(sys.argv) > 1 else "06"
F, P = os.path.join(root, "gpurun_out", "final"), os.path.join(root, "profiles")


def load(name):
    return json.load(open(os.path.join(F, name)))


shutil.copy(os.path.join(F, "bench.json"), os.path.join(P, f"r{rnd}_bench50k_final.json"))
shutil.copy(os.path.join(F, "kernel_stats.csv"), os.path.join(P, f"r{rnd}_bench50k_kernel_stats_final.csv"))
shutil.copy(os.path.join(F, "pmc_traffic.json"), os.path.join(P, f"r{rnd}_pmc_traffic.json"))
shutil.copy(os.path.join(F, "pmc_sq.txt"), os.path.join(P, f"r{rnd}_pmc_sq_counters.txt"))
for name, dst in (("pmc_mfma.json", f"r{rnd}_pmc_mfma.json"), ("configs.json", f"r{rnd}_configs.json"), ("pmc_wide_r256.json", f"r{rnd}_pmc_wide_r256.json")):
    if os.path.exists(os.path.join(F, name)):
        shutil.copy(os.path.join(F, name), os.path.join(P, dst))

if os.path.exists(os.path.join(F, "kernel_stats_r256.csv")):
    shutil.copy(os.path.join(F, "kernel_stats_r256.csv"), os.path.join(P, f"r{rnd}_bench50k_r256_kernel_stats.csv"))
ranks = {}
for r in (128, 200, 256, 512):
    if os.path.exists(os.path.join(F, f"bench_rank{r}.json")) and os.path.getsize(os.path.join(F, f"bench_rank{r}.json")) > 0:
        d = load(f"bench_rank{r}.json")
        ranks[str(r)] = {"ms_per_step": d["ms_per_step"], "iterations_per_s": d["value"], "valid": d["valid"], "parity_check": d["parity_check"],
                         "kernels": d["kernels"]}
        if r == 256:
            shutil.copy(os.path.join(F, "bench_rank256.json"), os.path.join(P, f"r{rnd}_bench50k_r256.json"))
if ranks:
    json.dump({"what": "the metric workload (50k <-> 50k CPD) at model ranks above 112: python bench.py --full --rank R --no-cpu-baseline", "ranks": ranks},
              open(os.path.join(P, f"r{rnd}_bench50k_wide_ranks.json"), "w"), indent=1)

e50 = {str(n): load(f"emu{n}.json")["ms_per_step"] for n in (1, 2, 4, 8)}
one100 = load("bench_100k.json")
e100 = {"1": one100["ms_per_step"], **{str(n): load(f"emu100k_{n}.json")["ms_per_step"] for n in (2, 4, 8)}}
json.dump({
    "what": "emulated per-rank iteration time of a row shard (one GPU runs rank 0's share of an N-rank job; exchange = the library's "
            "native RCCL path with a ONE-rank communicator, i.e. ncclAllReduce enqueued by libgingr_hip between the phases, no Python "
            "in the loop -- rounds 1-3 measured this through a torch.distributed callback; timing experiment, not a valid registration)",
    "command": "python bench.py --emulate-world N --no-cpu-baseline --no-parity-check --steps 100 --warmup 10 --roofline-steps 0 "
               "(100k: --points 100000 --steps 40 --warmup 5)",
    "ms_per_iteration_50k": e50,
    "ms_per_iteration_100k": e100,
    "ratio_to_one_gpu_50k": {k: e50["1"] / v for k, v in e50.items()},
    "ratio_to_one_gpu_100k": {k: e100["1"] / v for k, v in e100.items() if k != "1"},
}, open(os.path.join(P, f"r{rnd}_emulated_shard_times.json"), "w"), indent=1)


def cfg(d):
    return {"ms_per_step": d["ms_per_step"], "iterations_per_s": d["value"], "valid": d["valid"], "parity_check": d["parity_check"]}


json.dump({
    "config3_15k": cfg(load("bench_15k.json")),
    "config4_100k_one_gpu": cfg(one100),
    "late_regime_sigma2_4_50k": load("bench_sigma2_4.json")["ms_per_step"],
    "device_group_two_logical_shards_50k": load("bench_group_logical2.json")["ms_per_step"],
}, open(os.path.join(P, f"r{rnd}_configs_3_4_and_variants.json"), "w"), indent=1)
for src, dst in (("emu8_kernel_stats.csv", f"r{rnd}_emulated_8gpu_shard_kernel_stats.csv"), ("emu8_kernels.txt", f"r{rnd}_emulated_8gpu_shard_kernel_stats.txt"),
                 ("chain_kernel_stats.csv", f"r{rnd}_mh_chain_femur_kernel_stats.csv"), ("icp50k.json", f"r{rnd}_icp_pointcloud_50k.json"),
                 ("icp_surface.json", f"r{rnd}_icp_surface_41k.json"), ("icp_surface_n50.json", f"r{rnd}_icp_surface_41k_50_iterations.json"),
                 ("stamps_emu8.txt", f"r{rnd}_shard_pair_loop_stamps_final.txt")):
    if os.path.exists(os.path.join(F, src)) and os.path.getsize(os.path.join(F, src)) > 0:
        shutil.copy(os.path.join(F, src), os.path.join(P, dst))
for src, dst in (("gpmm_build.json", f"r{rnd}_gpmm_build.json"), ("gpmm_kernel_stats.csv", f"r{rnd}_gpmm_build_kernel_stats.csv"),
                 ("registration_timeline.txt", f"r{rnd}_registration_timeline.txt"),
                 ("landmarks_kernel_stats.csv", f"r{rnd}_landmarks_cpd50k_kernel_stats.csv"), ("ubench_sym_eig.txt", f"r{rnd}_ubench_sym_eig.txt")):
    if os.path.exists(os.path.join(F, src)) and os.path.getsize(os.path.join(F, src)) > 0:
        shutil.copy(os.path.join(F, src), os.path.join(P, dst))
if os.path.exists(os.path.join(F, "chain_1.json")):
    runs = [load(f"chain_{i}.json") for i in range(1, 6) if os.path.exists(os.path.join(F, f"chain_{i}.json"))]
    best = sorted(runs, key=lambda c: c["steps_per_s"])[len(runs) // 2]     # the median run
    best["runs_steps_per_s"] = sorted(c["steps_per_s"] for c in runs)
    if os.path.exists(os.path.join(F, "chain_call_by_call.json")):
        best["call_by_call_steps_per_s"] = load("chain_call_by_call.json")["steps_per_s"]
    json.dump(best, open(os.path.join(P, f"r{rnd}_mh_chain_femur.json"), "w"))
if os.path.exists(os.path.join(F, "bench_1622.json")):
    shutil.copy(os.path.join(F, "bench_1622.json"), os.path.join(P, f"r{rnd}_bench_1622.json"))
print("profiles updated from", F)
