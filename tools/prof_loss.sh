#!/bin/bash
# Dev tool: the objective's measurement (DESIGN.md "Objective") into $PROF_OUT/$1 (default prof_out/):
# tools/loss_bench.py timed A/B (bench.jsonl), then one rocprofv3 kernel-stats run
# per variant (base = no objective, A = torch ops, B = RenderLoss; sparse 1e-3) whose
# total launch counts tools/loss_bench.py's docstring explains how to difference.
export TMPDIR=/tmp
O=${PROF_OUT:-prof_out}/${1:-ploss}; mkdir -p $O
N=${2:-12}
timeout -k 10 400 python tools/loss_bench.py > $O/bench.jsonl 2> $O/bench.err || exit 1
for v in base A B; do
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/$v -o run -- \
    python tools/loss_bench.py --variant $v --sparse 1e-3 --profile-steps $N > $O/prof_$v.log 2>&1 || exit 1
done
python - "$O" "$N" <<'PY'
import csv, glob, json, sys
O, N = sys.argv[1], int(sys.argv[2])
calls = {}
for v in ("base", "A", "B"):
    f = glob.glob(f"{O}/{v}/**/*kernel_stats.csv", recursive=True)[0]
    calls[v] = sum(int(r["Calls"]) for r in csv.DictReader(open(f)))
res = {"steps": N, "kernel_launches_total": calls,
       "objective_launches_per_step": {v: round((calls[v] - calls["base"]) / N, 2) for v in ("A", "B")}}
json.dump(res, open(f"{O}/launches.json", "w"))
print(json.dumps(res))
PY
