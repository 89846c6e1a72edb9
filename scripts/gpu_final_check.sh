#!/bin/bash
# Final check: the GPU suite, smoke(), then the bench with every side measurement.  Run from the repository
# root; logs go to $SDB_OUT/final (default bench_out/final).
set -u
O=${SDB_OUT:-bench_out}/final
mkdir -p $O
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $O/tests.log 2>&1; rc=$?; echo "tests rc=$rc"; tail -2 $O/tests.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 200 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $O/smoke.log 2>&1; rc=$?; echo "smoke rc=$rc"; tail -2 $O/smoke.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python bench.py --full > $O/bench.log 2>&1; rc=$?; echo "bench rc=$rc"; grep "^{" $O/bench.log | cut -c1-300
