#!/bin/bash
# Headline step of a PARENT build against this build with the table forward switched off (MLQEM_TABLE_FWD=0: cheb_conv1 and
# sage_conv1 aggregate their projections, one pooled aggregation per branch) and at its default (both layers pooled projections of
# table rows inside the fan-out's launch), alternating on ONE box.  Every bench invocation runs under its own timeout, the
# invocations are chained and the script stops at the first one that fails.
#   bash scripts/ab_table_fwd.sh <dir of a built checkout of the parent commit> [rounds] > runs.txt
# One line per run on stdout: label, ms_per_step_p10 / p50 / p90, final loss.  The path counts only if every default run has a lower
# p50 than every run of the parent and of the switched-off build (profiles/table_fwd_ab.json holds the recorded runs).  The last
# line is the parent with MLQEM_TABLE_GCN=0 MLQEM_TABLE_CHEB=0: an fp32 reassociation of the same size already in the code, the
# yardstick for the final loss.
R=$(cd "$(dirname "$0")/.." && pwd)
PARENT=${1:?usage: ab_table_fwd.sh <parent checkout> [rounds]}
N=${2:-3}
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
run() {   # label, directory, environment assignments
  local label=$1 dir=$2
  shift 2
  ( set -o pipefail; cd "$dir" && env "$@" MLQEM_BENCH_FULL_RECORD="$T/full.json" timeout -k 10 300 python3 bench.py --no-cpu-baseline 2> "$T/err.log" | tail -1 > "$T/line.json" ) \
    || { echo "$label: bench failed" >&2; tail -5 "$T/err.log" >&2; return 1; }
  python3 - "$label" "$T/line.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read())
print(sys.argv[1], d["ms_per_step_p10"], d["ms_per_step_p50"], d["ms_per_step_p90"], d["final_loss"], flush=True)
PY
}
for i in $(seq 1 "$N"); do
  run parent "$PARENT" MLQEM_AB=parent &&
    run switch_off "$R" MLQEM_TABLE_FWD=0 &&
    run table_fwd "$R" MLQEM_AB=table_fwd || exit 1
done
run parent_no_tables "$PARENT" MLQEM_TABLE_GCN=0 MLQEM_TABLE_CHEB=0
