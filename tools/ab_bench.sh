#!/bin/bash
# The headline of bench.py with several builds of the library alternating in one session on one box:
#   tools/ab_bench.sh OUTDIR RUNS name=/abs/path/lib.so [name=/abs/path/lib.so ...]      (run from the repo root on a GPU box)
# RUNS rounds of `python bench.py --gpus 1 --steps 20 --warmup 5`, every library once per round (PINN_HIP_LIB), then three rounds
# of bench.py's leg_residuals (physics pass + finalize at 1e6 and 1e7 rows, V stage) for the first two libraries.
# OUTDIR/summary.txt: median, min, max and every value per library (what profiles/r04/ab_parent_vs_branch.txt holds).
set -o pipefail
out=$1; runs=$2; shift 2
mkdir -p "$out"
: > "$out/headline.jsonl"; : > "$out/resid.jsonl"
for i in $(seq 1 "$runs"); do
  for nl in "$@"; do
    name=${nl%%=*}; lib=${nl#*=}
    PINN_HIP_LIB=$lib timeout -k 10 120 python bench.py --gpus 1 --steps 20 --warmup 5 > "$out/run.json" 2> "$out/run.err" || { echo "bench failed: $name run $i"; tail -20 "$out/run.err"; exit 1; }
    python -c "import json; d = json.load(open('$out/run.json')); print(json.dumps({'lib': '$name', 'run': $i, 'ms_per_step': d['ms_per_step'], 'final_loss': d['config']['final_loss']}))" | tee -a "$out/headline.jsonl"
  done
done
for i in 1 2 3; do
  for nl in "${@:1:2}"; do
    name=${nl%%=*}; lib=${nl#*=}
    PINN_HIP_LIB=$lib timeout -k 10 120 python -c "
import json, torch, bench
torch.cuda.set_device(0)
print(json.dumps({'lib': '$name', 'residuals': bench.leg_residuals(torch.device('cuda:0'))}))" >> "$out/resid.jsonl" 2> "$out/run.err" || { echo "residual leg failed: $name run $i"; tail -20 "$out/run.err"; exit 1; }
  done
done
python - "$out" <<'PY' | tee "$out/summary.txt"
import json, statistics, sys
o = sys.argv[1]
runs = [json.loads(l) for l in open(o + "/headline.jsonl")]
for v in dict.fromkeys(r["lib"] for r in runs):
    ms = [r["ms_per_step"] for r in runs if r["lib"] == v]
    print("headline %-8s n=%d median %.4f min %.4f max %.4f  all %s" % (v, len(ms), statistics.median(ms), min(ms), max(ms), ["%.4f" % m for m in ms]))
res = [json.loads(l) for l in open(o + "/resid.jsonl")]
for k in sorted({(e["kernel"], e["rows"]) for r in res for e in r["residuals"]}):
    for v in dict.fromkeys(r["lib"] for r in res):
        us = [e["us"] for r in res if r["lib"] == v for e in r["residuals"] if (e["kernel"], e["rows"]) == k]
        print("resid %-55s rows %9d %-8s us %s" % (k[0][:55], k[1], v, ["%.2f" % u for u in us]))
PY
