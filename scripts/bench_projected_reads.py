"""Projected tree reads (sdb_lsm_scan_projected, sdb_lsm_get_projected) next to the filtered calls on the
device-resident tree of scripts/bench_lsm_scan.py: 8 L0 SSTs plus 3 sorted runs of 8 SSTs, every SST of the
configs[1] shape (16-byte keys, 100-byte values, 4 KiB blocks, 10 filter bits per key).

  python scripts/bench_projected_reads.py [--reps R] [--sst-entries N] [--keys K] [--compare-library FILE]

The batch is workload (a) of bench_lsm_scan.py (4,096 ranges of about 100 keys) and the "spread" mix of bench_get.py
(K keys spread over the levels).  Measured:
  a     sdb_lsm_scan_filtered / sdb_lsm_get_filtered (policies, prefixes and probe_len NULL)
  b     the projected calls with every projection (UNBOUNDED, UNBOUNDED)
  c_lo  every SST projected to the lower half of the key space, [.., mid): one half of a range-split clone
  c_hi  every SST projected to the upper half, [mid, ..): the other half
--compare-library names another build of the library in slatedb_amd/ (the parent commit's, say): (a) is then measured
through both, alternating call by call on the same tree and workspace, and reported as a_other.

One JSON line: per path the device time of a call between two events (median of R with min .. max), blocks_checked,
num_candidates and num_entries (gets: num_found, blocks_checked), and whether (b) returns (a)'s rows and (c_lo) and
(c_hi) together return them.  A record, not a gate.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_get import build_tree, key_of, mixes, stats  # noqa: E402
from bench_lsm_scan import workloads  # noqa: E402
from slatedb_amd import _abi, datasets, runtime  # noqa: E402

U, INC, EXC = _abi.BOUND_UNBOUNDED, _abi.BOUND_INCLUDED, _abi.BOUND_EXCLUDED


def timed(s, calls, reps):
    """calls: name -> a function that enqueues one call on s and returns its result.  Two warm-up rounds, then
    `reps` rounds that go through the names in turn, so drift hits every path alike -> name -> (device times, the
    last result)."""
    ev, last = {k: [] for k in calls}, {}
    for i in range(reps + 2):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            last[name] = fn()
            e1.record(s)
            s.synchronize()
            if i >= 2:
                ev[name].append(e0.elapsed_time(e1))
    return {k: (ev[k], last[k]) for k in calls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sst-entries", type=int, default=datasets.D1_N)
    ap.add_argument("--keys", type=int, default=65536)
    ap.add_argument("--compare-library", default=None)
    a = ap.parse_args()
    reps = max(5, a.reps)
    runtime.require_device()
    own = runtime.lib()
    other = None
    if a.compare_library:
        other = _abi.bind(C.CDLL(os.path.join(ROOT, "slatedb_amd", os.path.basename(a.compare_library))), partial=True)

    def through(lib, fn):
        """fn with the runtime's calls going through `lib`."""
        def run():
            runtime._lib = lib
            try:
                return fn()
            finally:
                runtime._lib = own
        return run

    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    t0 = time.perf_counter()
    views, runs, info = build_tree(a.sst_entries, dev)
    tree = runtime.lsm_tree_device(views, runs)
    build_s = round(time.perf_counter() - t0, 1)
    ns = len(views)
    to_dev = lambda d: {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev) for k, v in d.items()}  # noqa: E731
    mid = key_of(1 << 61)  # the counters are uniform in [0, 2^62)
    proj = {"b": [None] * ns, "c_lo": [(None, U, mid, EXC)] * ns, "c_hi": [(mid, INC, None, U)] * ns}
    proj = {k: dict(to_dev(runtime.projections_columnar(v)), n=ns) for k, v in proj.items()}
    line = {"what": "projected tree reads next to the filtered calls", "ssts": ns, "entries_per_sst": a.sst_entries,
            "total_blocks": tree["total_blocks"], "build_s": build_s, "compare_library": a.compare_library}

    with torch.cuda.stream(s):
        # ---- scans
        ranges = workloads(info)["a"]
        n = len(ranges)
        rt = dict(to_dev(runtime.scan_ranges_columnar(ranges)), n=n)
        sized = runtime.lsm_scan_filtered_device(tree, rt, stream=s)  # the sizing calls of rule 6
        s.synchronize()
        sm = [int(x) for x in sized["summary"].cpu().numpy()]
        kw = dict(stream=s, workspace=sized["_ws"], cand=(sm[2], sm[3]), cap=(sm[0], sm[1]))
        calls = {"a": lambda: runtime.lsm_scan_filtered_device(tree, rt, **kw)}
        if other:
            calls["a_other"] = through(other, calls["a"])
        for name, p in proj.items():
            calls[name] = (lambda p=p: runtime.lsm_scan_projected_device(tree, p, rt, **kw))
        got = timed(s, calls, reps)
        line["ranges"] = n
        rows = {}
        for name, (ev, r) in got.items():
            smr = dict(zip(runtime.LSM_SCAN_SUMMARY, (int(x) for x in r["summary"].cpu().numpy())))
            line["scan_" + name] = {"device": stats(ev), "blocks_checked": smr["blocks_checked"],
                                    "num_candidates": smr["num_candidates"], "num_entries": smr["num_entries"],
                                    "status": smr["status"] & 0xFFFFFFFF}
            ne = smr["num_entries"]
            rows[name] = (r["range_entry_start"].cpu().numpy()[:n + 1],
                          [r[k].cpu().numpy()[:ne] for k in ("seq", "sst", "val_off")], r["key_arena"].cpu().numpy()[:smr["key_bytes"]])
        same = lambda x, y: (np.array_equal(x[0], y[0]) and all(np.array_equal(p, q) for p, q in zip(x[1], y[1])) and  # noqa: E731
                             np.array_equal(x[2], y[2]))
        line["scan_b_same_rows_as_a"] = bool(same(rows["a"], rows["b"]))
        if other:
            line["scan_a_other_same_rows_as_a"] = bool(same(rows["a"], rows["a_other"]))
        # the two halves hold every row once (a range that straddles mid has its rows in both, in order)
        line["scan_halves_hold_a"] = bool(np.array_equal(rows["c_lo"][0] + rows["c_hi"][0], rows["a"][0]))
        # ---- gets
        keys = mixes(info, a.keys)["spread"]
        kb, ko = (torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev) for x in runtime.keys_columnar(keys))
        kt = (kb, ko, len(keys))
        first = runtime.lsm_get_filtered_device(tree, None, kt, stream=s)
        s.synchronize()
        gkw = dict(stream=s, workspace=first["_ws"])
        calls = {"a": lambda: runtime.lsm_get_filtered_device(tree, None, kt, **gkw)}
        if other:
            calls["a_other"] = through(other, calls["a"])
        for name, p in proj.items():
            calls[name] = (lambda p=p: runtime.lsm_get_projected_device(tree, None, p, kt, **gkw))
        got = timed(s, calls, reps)
        line["keys"] = len(keys)
        cols = {}
        for name, (ev, r) in got.items():
            smr = dict(zip(runtime.GET_SUMMARY, (int(x) for x in r["summary"].cpu().numpy())))
            line["get_" + name] = {"device": stats(ev), "blocks_checked": smr["blocks_checked"], "num_found": smr["num_found"],
                                   "status": smr["status"] & 0xFFFFFFFF}
            cols[name] = [r[f].cpu().numpy() for f, _ in runtime.GET_FIELDS]
        line["get_b_same_as_a"] = all(np.array_equal(x, y) for x, y in zip(cols["a"], cols["b"]))
        if other:
            line["get_a_other_same_as_a"] = all(np.array_equal(x, y) for x, y in zip(cols["a"], cols["a_other"]))
        line["get_halves_hold_a"] = line["get_c_lo"]["num_found"] + line["get_c_hi"]["num_found"] == line["get_a"]["num_found"]
    for kind in ("scan", "get"):
        am = line[kind + "_a"]["device"]["median_ms"]
        line[kind + "_b_minus_a_ms"] = round(line[kind + "_b"]["device"]["median_ms"] - am, 4)
        if other:
            line[kind + "_a_minus_a_other_ms"] = round(am - line[kind + "_a_other"]["device"]["median_ms"], 4)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
