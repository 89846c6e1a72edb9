"""Compaction with a merge operator (sdb_compactor_run_merge) against the same inputs passed through unmerged
(sdb_compactor_run with retention.merge_operands = 1), at the size scripts/bench_configs.py uses for compaction:
4 runs of 578,524 entries, 16-byte keys, 100-byte values, 4 KiB blocks, 10 filter bits per key, max_sst_size 256 MiB.

  python scripts/bench_compact_merge.py [--reps R] [--run-entries N] [--kernel-stats FILE]

The mix: counter-style keys (a big-endian counter in a 16-byte key), every key 1 to 8 merge operands over one base
value, each version in a run drawn at random, newer versions holding higher seqs; the operator is StringConcat
(slatedb_amd/merge.py), called from the library through the runtime's ctypes callback.

Per job one JSON line: wall-clock of the whole job (the call returns after its last synchronisation), medians of R
with min .. max; for the merge job also the time spent inside the operator, the number of operator calls and the
chain counts.  The device time of the new kernels (k_mg_chain, k_mg_chain_scan, k_mg_chain_emit and the unit forms
of k_mg_keys / k_mg_emit) is not visible from the host: run the script once more under
`rocprofv3 --kernel-trace --stats` and pass the kernel statistics CSV it writes as --kernel-stats to get their
line (profile runs slow the host: take the wall-clock lines from a run without the profiler).  A record, not a gate.
"""
import argparse
import csv
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_KERNELS = ("k_mg_chain", "k_mg_chain_scan", "k_mg_chain_emit", "k_mg_keys<true>", "k_mg_emit<true>")


def kernel_stats_line(path):
    rows = list(csv.DictReader(open(path)))
    name = next(k for k in rows[0] if k.lower() == "name")
    total = next(k for k in rows[0] if k.lower().startswith("totalduration"))
    calls = next(k for k in rows[0] if k.lower() == "calls")
    out, new_us, all_ns = {}, 0.0, 0
    for r in rows:
        all_ns += int(r[total])
        m = re.search(r"::(k_(?:mg|cut)\w*(?:<\w+>)?)\(", r[name])
        if m:
            us = int(r[total]) / int(r[calls]) / 1e3
            out[m.group(1)] = {"calls": int(r[calls]), "us_per_call": round(us, 1)}
            if m.group(1) in NEW_KERNELS:
                new_us += us
    return {"what": "kernel statistics of the profiled run (rocprofv3 --kernel-trace --stats); every new kernel runs "
                    "once per merge job", "new_kernels_us_per_job": round(new_us, 1),
            "all_kernels_total_ms": round(all_ns / 1e6, 3), "merge_and_cut_kernels": out}


def make_runs(run_entries, nruns=4, seed=11):
    """-> host Runs: about nruns * run_entries entries over keys of 1..8 operands and a base."""
    from slatedb_amd import _abi
    from slatedb_amd.batch import Batch, Run
    rng = np.random.default_rng(seed)
    total = nruns * run_entries
    nops = rng.integers(1, 9, int(total / 5.5) + 1)
    nops = nops[:np.searchsorted(np.cumsum(nops + 1), total, side="right")]
    nver = nops + 1
    k = np.repeat(np.arange(nver.size), nver)
    first = np.repeat(np.cumsum(nver) - nver, nver)
    j = np.arange(k.size) - first                       # version of its key, 0 = newest
    kind = np.where(j == np.repeat(nops, nver), _abi.KIND_VALUE, _abi.KIND_MERGE).astype(np.uint8)
    seq = (np.repeat(np.cumsum(nver), nver) - j).astype(np.uint64)  # unique, descending within a key
    run = rng.integers(0, nruns, k.size)
    counters = (np.arange(nver.size, dtype=np.uint64) * np.uint64(977) + np.uint64(1 << 40))
    runs = []
    for r in range(nruns):
        sel = np.nonzero(run == r)[0]
        n = sel.size
        keys = np.zeros((n, 16), np.uint8)
        keys[:, 4:12] = counters[k[sel]].astype(">u8").view(np.uint8).reshape(-1, 8)
        vals = rng.integers(97, 123, (n, 100), dtype=np.uint8)
        b = Batch(keys.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(16), vals.reshape(-1),
                  np.arange(n + 1, dtype=np.uint64) * np.uint64(100), kind[sel], seq[sel], None, None, None)
        runs.append(Run.from_batch(b))
    return runs, int(nver.size)


class TimedConcat:
    """StringConcat with the time spent inside it."""

    def __init__(self):
        self.s, self.calls = 0.0, 0

    def merge_batch(self, key, existing, operands):
        t = time.perf_counter()
        r = (existing or b"") + b"".join(operands)
        self.s += time.perf_counter() - t
        self.calls += 1
        return r


def spread(x):
    return {"median": round(float(np.median(x)), 3), "min": round(min(x), 3), "max": round(max(x), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--run-entries", type=int, default=578524)
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_stats_line(a.kernel_stats)), flush=True)
        return
    import torch
    from slatedb_amd import _abi, runtime
    runtime.require_device()
    t0 = time.perf_counter()
    runs, nkeys = make_runs(a.run_entries)
    druns = [runtime.DeviceRun.from_host(r) for r in runs]
    prm = runtime.params(block_size=4096, sst_version=2, bloom_bits_per_key=10)
    logical = sum(int(r.key_off[-1]) + int(r.val_len.sum()) for r in runs)
    print(json.dumps({"what": "inputs", "runs": len(runs), "entries": sum(r.n for r in runs), "keys": nkeys,
                      "logical_bytes": logical, "build_s": round(time.perf_counter() - t0, 1)}), flush=True)
    comp = runtime.Compactor()
    max_sst = 256 << 20

    # the baseline: operands passed through unmerged (retention_min_seq Some(0) as in bench_configs.compact_bench)
    plain = _abi.Retention(0, 0, 0, 1, 0, 0, 1, 0)
    walls = []
    for i in range(a.reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        st, ns = comp.run(druns, plain, prm, max_sst)
        torch.cuda.synchronize()
        assert st == 0, st
        if i:
            walls.append((time.perf_counter() - t) * 1e3)
    _, sm = comp.merged()
    print(json.dumps({"what": "sdb_compactor_run, operands passed unmerged (baseline)", "ms_wall": spread(walls),
                      "entries_out": int(sm.num_out), "val_bytes_out": int(sm.val_bytes), "output_ssts": ns,
                      "GiB_per_s_logical": round(logical / (np.median(walls) * 1e-3) / 2**30, 2)}), flush=True)

    # the merge job: no barrier (retention_min_seq None), so every key collapses to one Value
    ret = _abi.Retention(0, 0, 0, 0, 0, 0, 0, 0)
    walls, ops = [], []
    for i in range(a.reps + 1):
        op = TimedConcat()
        torch.cuda.synchronize()
        t = time.perf_counter()
        st, ns = comp.run_merge(druns, ret, op, prm, max_sst)
        torch.cuda.synchronize()
        assert st == 0, st
        if i:
            walls.append((time.perf_counter() - t) * 1e3)
            ops.append(op.s * 1e3)
    _, sm = comp.merged()
    ms = comp.merge_stats()
    print(json.dumps({"what": "sdb_compactor_run_merge, StringConcat through the ctypes callback", "ms_wall": spread(walls),
                      "ms_inside_operator": spread(ops), "operator_calls": int(ms.operator_calls),
                      "groups": int(ms.groups), "links": int(ms.links), "link_bytes_d2h": int(ms.link_bytes),
                      "merged_bytes_h2d": int(ms.merged_bytes), "entries_out": int(sm.num_out),
                      "val_bytes_out": int(sm.val_bytes), "output_ssts": ns,
                      "GiB_per_s_logical": round(logical / (np.median(walls) * 1e-3) / 2**30, 2)}), flush=True)
    comp.close()


if __name__ == "__main__":
    main()
