#!/bin/bash
# bench.py --full at several pass sizes (samples of a pixel traced concurrently); run on the GPU box. OUT names the output folder
out=${OUT:-results}
mkdir -p "$out"
for s in "$@"; do
  timeout -k 10 250 python bench.py --full --no-cpu-baseline --spp-per-pass $s 2>&1 | tail -1 > "$out/_pp.json"
  python3 - "$s" "$out/_pp.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[2]))
r = d["roofline"]
print("spp_per_pass", sys.argv[1], d["value"], "Mrays/s", d["ms_per_step"], "ms/step; k_trace", r["avg_launch_ms"], "ms x", r["launches_per_step"], "trace fraction", r["trace_fraction_of_step"], flush=True)
PY
done
