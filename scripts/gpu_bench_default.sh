#!/bin/bash
# The bench with every side measurement (--full, other arguments at their defaults), then a one-line digest
# of its JSON.  Logs go to $SDB_OUT (default bench_out/).
set -u
cd "$(dirname "$0")/.."
export O=${SDB_OUT:-bench_out}
mkdir -p $O
timeout -k 10 600 python3 bench.py --full > $O/bench_default.log 2>&1
rc=$?; echo "bench rc=$rc"; [ $rc -eq 0 ] || { tail -20 $O/bench_default.log; exit $rc; }
python3 - <<'PY'
import json
import os
d = json.loads([l for l in open(os.path.join(os.environ["O"], "bench_default.log")) if l.startswith("{")][0])
r = d["roofline"]
print("value", d["value"], "ms_step", d["ms_per_step"], "single", d["single_sst"]["device_ms_per_sst"],
      "one_stream", d["one_stream"], "copy", r["measured_copy_GBps"], "k_emit", r["k_emit"], "cpu", d["cpu_baseline"]["value"])
PY
