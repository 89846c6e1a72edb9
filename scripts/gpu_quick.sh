#!/bin/bash
# Quick GPU iteration: full -m gpu suite, then the bench with its side measurements (no CPU leg).
# Logs go to $SDB_OUT (default bench_out/).
set -o pipefail
cd "$(dirname "$0")/.."
O=${SDB_OUT:-bench_out}
mkdir -p $O
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread ${TESTS:-} > $O/q_tests.log 2>&1
rc=$?; tail -3 $O/q_tests.log; grep -E "^(FAILED|ERROR)" $O/q_tests.log | head; [ $rc -ne 0 ] && exit $rc
timeout -k 10 300 python -u bench.py --full --steps ${STEPS:-600} --warmup 10 --no-cpu ${BENCH_ARGS:-} > $O/q_bench.json 2> $O/q_bench.err
rc=$?; python3 -c "
import json; d=json.load(open('$O/q_bench.json')); r=d['roofline']
print('value', d['value'], 'ms/SST', r['device_ms_per_sst'], 'frac', r['frac'], 'emit', r['k_emit']['frac'], 'single', d['single_sst'])
print({k: round(v/8*1000,1) for k,v in r['stage_ms_per_step'].items()})" ; tail -2 $O/q_bench.err; exit $rc
