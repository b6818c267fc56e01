#!/bin/bash
# Headline step of a PARENT build against this build with the table gradients switched off (MLQEM_TABLE_GRAD=0: the aggregating
# backward of cheb_conv1 / sage_conv1), with the pooled gradients written out in front of the pass over the tables
# (MLQEM_TABLE_GRAD_SYNTH=0) and with them computed inside it (the default), alternating on ONE box.  Every bench invocation runs
# under its own timeout, the invocations are chained and the script stops at the first one that fails.
#   bash scripts/ab_table_grad.sh <dir of a built checkout of the parent commit> [rounds] > runs.txt
# One line per run on stdout: label, ms_per_step_p10 / p50 / p90, final loss.  A form counts only if every run with it has a lower
# p50 than every run of the parent and of the switched-off build (profiles/table_grad_ab.json holds the recorded runs).
R=$(cd "$(dirname "$0")/.." && pwd)
PARENT=${1:?usage: ab_table_grad.sh <parent checkout> [rounds]}
N=${2:-3}
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
run() {   # label, directory, environment assignment
  ( set -o pipefail; cd "$2" && env "$3" MLQEM_BENCH_FULL_RECORD="$T/full.json" timeout -k 10 300 python3 bench.py --no-cpu-baseline 2> "$T/err.log" | tail -1 > "$T/line.json" ) \
    || { echo "$1: bench failed" >&2; tail -5 "$T/err.log" >&2; return 1; }
  python3 - "$1" "$T/line.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[2]).read())
print(sys.argv[1], d["ms_per_step_p10"], d["ms_per_step_p50"], d["ms_per_step_p90"], d["final_loss"], flush=True)
PY
}
for i in $(seq 1 "$N"); do
  run parent "$PARENT" MLQEM_AB=parent &&
    run switch_off "$R" MLQEM_TABLE_GRAD=0 &&
    run stage_a_written "$R" MLQEM_TABLE_GRAD_SYNTH=0 &&
    run stage_b_synth "$R" MLQEM_AB=synth || exit 1
done
