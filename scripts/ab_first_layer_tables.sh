#!/bin/bash
# Headline step of a PARENT build against this build, and this build with each first-layer table switched off alone
# (MLQEM_TABLE_CHEB=0 / MLQEM_TABLE_GCN=0), alternating on ONE box; every invocation under its own timeout.
#   bash scripts/ab_first_layer_tables.sh <dir of a built checkout of the parent commit> [rounds] > runs.txt
# One line per run on stdout: label, ms_per_step_p10 / p50 / p90, final loss.  A change counts only if every run with it has a
# lower p50 than every run without it (profiles/first_layer_tables_ab.json holds the recorded runs).
R=$(cd "$(dirname "$0")/.." && pwd)
PARENT=${1:?usage: ab_first_layer_tables.sh <parent checkout> [rounds]}
N=${2:-3}
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
run() {   # label, directory, environment assignment
  ( cd "$2" && env "$3" MLQEM_BENCH_FULL_RECORD="$T/full.json" timeout -k 10 300 python3 bench.py --no-cpu-baseline 2> /dev/null | tail -1 > "$T/line.json" ) || exit 1
  python3 - "$1" "$T/line.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read())
print(sys.argv[1], d["ms_per_step_p10"], d["ms_per_step_p50"], d["ms_per_step_p90"], d["final_loss"])
PY
}
for i in $(seq 1 "$N"); do
  run parent "$PARENT" MLQEM_AB=parent
  run both_tables "$R" MLQEM_AB=both
  run gcn_table_only "$R" MLQEM_TABLE_CHEB=0
  run cheb_table_only "$R" MLQEM_TABLE_GCN=0
done
