#!/bin/bash
# bench.py --full over the optimizer / workload / sampler matrix of the batched STREAM kernel (one line each)
R=$(cd "$(dirname "$0")/.." && pwd); O=${BENCH_OUT:-$R/bench_out}; mkdir -p "$O"  # repository root; where the results go
for o in "$@"; do
  python "$R/bench.py" --full --steps 30 --warmup 4 --no-cpu-baseline $o > $O/b.json 2>$O/b.err || tail -5 $O/b.err
  python - "$o" "$O/b.json" <<'PY'
import json, sys
j = json.load(open(sys.argv[2])); r = j["roofline"]
print("%-55s | %7.1f M/s  ms/step %7.3f  kernel %7.3f ms  frac %.3f  loss %.4f" % (
    sys.argv[1], j["value"] / 1e6, j["ms_per_step"], r["kernel_ms_avg"], r["frac"], j["config"]["mean_bpr_loss"]))
PY
done
