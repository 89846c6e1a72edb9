#!/bin/bash
# Single-SST (--batch 1) bench with stage times, then its kernel trace.  Logs go to $SDB_OUT (default bench_out/).
set -u
cd "$(dirname "$0")/.."
export O=${SDB_OUT:-bench_out}
mkdir -p $O
timeout -k 10 200 python3 bench.py --full --batch 1 --streams 1 --steps 100 --warmup 10 --no-cpu --no-verify --single-steps 0 --stage-steps 100 > $O/b1.log 2>&1 || exit 1
python3 - <<'PY'
import json
import os
d = json.loads([l for l in open(os.path.join(os.environ["O"], "b1.log")) if l.startswith("{")][0])
r = d["roofline"]
print("batch1 value", d["value"], "ms/SST", r["device_ms_per_sst"], {k: round(v * 1000, 1) for k, v in r["stage_ms_per_step"].items()})
PY
timeout -k 10 200 rocprofv3 --kernel-trace --stats -d $O/b1prof -o run --output-format csv -- python3 bench.py --batch 1 --streams 1 --steps 100 --warmup 10 > $O/b1prof.log 2>&1 || exit 1
cut -d, -f1-4 $O/b1prof/run_kernel_stats.csv | head -14
