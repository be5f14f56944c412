#!/bin/bash
# Same-box A/B of the OLD GPMM entry (gingr_gpmm_build_gaussian) between builds of the library, in the manner of tools/abn.sh (whose runs
# are bench.py's): each variant is "name=library.so" (relative to the repository root; empty = the in-tree build), the runs alternate,
# three rounds, one process per run (tools/bench_varying_gpmm.py M rank --old-entry-only, median of 5 builds).  Naming one library twice
# gives the A/A spread against which a difference between two libraries is to be read.
# usage: tools/ab_gpmm.sh "parentA=tools/bin/libgingr_hip_parent.so" "parentB=tools/bin/libgingr_hip_parent.so" "new=" -- 50000 100 512
R=$(cd "$(dirname "$0")/.." && pwd)
VARS=()
while [ $# -gt 0 ] && [ "$1" != "--" ]; do VARS+=("$1"); shift; done
shift
M=$1; shift
O=${AB_GPMM_OUT:-$R/build/ab_gpmm}; rm -rf "$O"; mkdir -p "$O"   # per-run output and ab.json (AB_GPMM_OUT: another directory)
for i in 1 2 3; do
  for rank in "$@"; do
    for v in "${VARS[@]}"; do
      name=${v%%=*}; lib=${v#*=}
      (
        set -o pipefail
        if [ -n "$lib" ]; then export GINGR_HIP_LIB=$R/$lib GINGR_HIP_LIB_ALLOW_OLDER=1; fi
        timeout -k 10 300 python3 $R/tools/bench_varying_gpmm.py $M $rank --old-entry-only 2> $O/${name}_${rank}_$i.err | tail -1 > $O/${name}_${rank}_$i.json
      ) || { echo "run $name rank $rank round $i failed: stopping" >&2; exit 1; }
    done
  done
done
python3 - "$O" "$M" "$@" -- "${VARS[@]}" <<'PY'
import json, statistics, sys, time
O, M = sys.argv[1], int(sys.argv[2])
sep = sys.argv.index("--")
ranks, names = [int(r) for r in sys.argv[3:sep]], [v.split("=")[0] for v in sys.argv[sep + 1:]]
out = {"points": M, "date": time.strftime("%Y-%m-%d"), "entry": "gingr_gpmm_build_gaussian", "rounds": 3, "builds_per_round": 5, "ranks": {}}
for rank in ranks:
    rows = {}
    for name in names:
        meds = [json.load(open(f"{O}/{name}_{rank}_{i}.json"))["paths"][0]["build_s_median"] for i in (1, 2, 3)]
        rows[name] = {"build_s_rounds": meds, "build_s_median": statistics.median(meds)}
        print(f"rank {rank:4d} {name:12s}", " ".join("%.5f" % m for m in meds), "| median %.5f" % rows[name]["build_s_median"])
    out["ranks"][str(rank)] = rows
json.dump(out, open(f"{O}/ab.json", "w"), indent=1)
PY
