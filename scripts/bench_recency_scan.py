"""Batched Db::scan_prefix_by_recency (sdb_lsm_scan_recency) over the tree, the tables and the ranges of
scripts/bench_mem_scan.py, mix "spread" (the tables' keys interleave with the tree's): workload (a) 4,096 narrow
ranges, (b) 64 wide ranges.  Every key has one version here, so limit 0 returns the rows sdb_lsm_scan_mem returns, in
another order: the same inputs, the same candidates, and the two calls differ only behind staging (k_lr_* in place of
k_ls_rank).

  python scripts/bench_recency_scan.py [--reps R] [--sst-entries N] [--table-entries N] [--workload a|b|all]
                                       [--out FILE] [--one-call SETTING] [--kernel-trace CSV]

Three settings per workload:
  limit0      limit = 0: every source is drained;
  first       limit[r] = the rows of range r in its first source with a row of it: the walk stops there;
  last_run    limit[r] = one more than the rows before the range's last source: the walk ends in it.
Per (workload, setting) one JSON line: the device time between two events of sdb_lsm_scan_recency, of sdb_lsm_scan_mem
over the same inputs before and after it, medians of R with min .. max, the summary, the sources read, and whether
the rows are the model's: per range the rows of sdb_lsm_scan_mem regrouped by source in walk order, truncated.
--one-call SETTING runs warm-up calls and then one call of that setting, for `rocprofv3 --kernel-trace`; --kernel-trace
CSV reads such a trace and prints the kernels of its last call (everything from the last k_ls_mreset on).  A record,
not a gate.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import bench_get as BG  # noqa: E402
import bench_mem_scan as BM  # noqa: E402
from slatedb_amd import datasets, runtime  # noqa: E402

SETTINGS = ("limit0", "first", "last_run")


def last_call_kernels(path):
    """The kernels of the last call in a rocprofv3 kernel trace: name -> microseconds, in launch order."""
    rows = list(csv.DictReader(open(path)))
    col = lambda *names: next(c for c in rows[0] if c.lower() in names)  # noqa: E731
    name, start, end = col("kernel_name", "name"), col("start_timestamp", "start"), col("end_timestamp", "end")
    rows.sort(key=lambda r: int(r[start]))
    at = max(i for i, r in enumerate(rows) if "k_ls_mreset" in r[name])
    out = {}
    for r in rows[at:]:
        k = r[name].split("(")[0].replace("sdb::", "").replace("void ", "")
        out[k] = round(out.get(k, 0.0) + (int(r[end]) - int(r[start])) / 1e3, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sst-entries", type=int, default=datasets.D1_N)
    ap.add_argument("--table-entries", type=int, default=datasets.D1_N)
    ap.add_argument("--workload", default="all")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-call", default=None, choices=SETTINGS)
    ap.add_argument("--kernel-trace", default=None)
    a = ap.parse_args()
    if a.kernel_trace:
        print(json.dumps({"what": "kernels of the last call, microseconds", "trace": os.path.basename(a.kernel_trace),
                          "kernels": last_call_kernels(a.kernel_trace)}))
        return
    reps = max(5, a.reps)
    runtime.require_device()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    t0 = time.perf_counter()
    views, runs, info = BG.build_tree(a.sst_entries, dev)
    tree = runtime.lsm_tree_device(views, runs)
    tree_c = np.unique(np.concatenate([x["counters"] for x in info]))
    total = sum(x["counters"].size for x in info)
    druns, tabs = BM.build_tables(a.table_entries, dev, tree_c, 0, BM.TOP, 31)
    mem = runtime.mem_tables_device(druns)
    T = BM.TABLES
    run_of_sst = np.repeat(np.arange(len(runs)), runs)
    nsrc = T + len(runs)  # the walk's sources: the tables, then the runs
    lines = [{"what": "tree and tables", "ssts": len(views), "runs": len(runs), "total_blocks": tree["total_blocks"],
              "entries_per_sst": a.sst_entries, "tables": T, "rows_per_table": [int(t.size) for t in tabs],
              "build_s": round(time.perf_counter() - t0, 1)}]
    print(json.dumps(lines[0]), flush=True)
    rng = np.random.default_rng(33)
    for wname, count, width in (("a", 4096, 100), ("b", 64, 50000)):
        if a.workload not in ("all", wname):
            continue
        ranges, _, _ = BM.ranges_of(rng, 0, BM.TOP, BM.TOP / (total + sum(t.size for t in tabs)), count, width)
        n = len(ranges)
        rt = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev)
              for k, v in runtime.scan_ranges_columnar(ranges).items()}
        rt["n"] = n
        with torch.cuda.stream(s):
            sized = runtime.lsm_scan_mem_device(mem, tree, rt, stream=s)  # the sizing calls of rule 6
            s.synchronize()
            sm = [int(x) for x in sized["summary"].cpu().numpy()]
            cand, cap, ws = (sm[2], sm[3]), (sm[2], sm[3]), sized["_ws"]
            rsized = runtime.lsm_scan_recency_device(mem, tree, rt, stream=s, cand=cand, cap=cap)
            s.synchronize()
            rws = rsized["_ws"]
            # the model: sdb_lsm_scan_mem's rows (one version per key: the same set) regrouped by source in walk order
            ne = sm[0]
            starts = sized["range_entry_start"].cpu().numpy()[:n + 1]
            keys = sized["key_arena"].cpu().numpy()[:16 * ne].reshape(-1, 16).view("S16").ravel()
            tab, sst = sized["table"].cpu().numpy()[:ne], sized["sst"].cpu().numpy()[:ne]
            src = np.where(tab >= 0, tab.astype(np.int64), T + run_of_sst[np.maximum(sst, 0)])
            rid = np.repeat(np.arange(n), np.diff(starts))
            order = np.lexsort((np.arange(ne), src, rid))  # (a run's SSTs hold disjoint ascending key ranges)
            m_keys, m_src, m_rid = keys[order], src[order], rid[order]
            per = np.zeros((n, nsrc), np.int64)
            np.add.at(per, (rid, src), 1)
            nz = per > 0
            first_src, last_src = nz.argmax(1), nsrc - 1 - nz[:, ::-1].argmax(1)
            lim = {"limit0": np.zeros(n, np.int64),
                   "first": np.where(nz.any(1), per[np.arange(n), first_src], 1),
                   "last_run": np.where(nz.any(1), per.sum(1) - per[np.arange(n), last_src] + 1, 1)}
            res = {}

            def mem_scan():
                res["m"] = runtime.lsm_scan_mem_device(mem, tree, rt, stream=s, workspace=ws, cand=cand, cap=cap)

            def device(fn):
                ev = []
                for _ in range(reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    fn()
                    e1.record(s)
                    torch.cuda.synchronize()
                    ev.append(e0.elapsed_time(e1))
                return BG.stats(ev)

            for setting in SETTINGS:
                if a.one_call and a.one_call != setting:
                    continue
                d_lim = torch.from_numpy(lim[setting]).to(dev)

                def recency():
                    res["r"] = runtime.lsm_scan_recency_device(mem, tree, rt, limit=d_lim, stream=s, workspace=rws, cand=cand, cap=cap)

                for _ in range(2):
                    recency()
                    mem_scan()
                torch.cuda.synchronize()
                if a.one_call:
                    recency()  # the call to read from the kernel trace
                    torch.cuda.synchronize()
                    continue
                d_mem = device(mem_scan)
                d_rec = device(recency)
                d_mem2 = device(mem_scan)  # again after, so a drift of the machine shows beside the difference
                r = res["r"]
                smr = [int(x) for x in r["summary"].cpu().numpy()]
                got_starts = r["range_entry_start"].cpu().numpy()[:n + 1]
                got_keys = r["key_arena"].cpu().numpy()[:16 * smr[0]].reshape(-1, 16).view("S16").ravel()
                L = lim[setting]
                within = np.arange(ne) - np.concatenate([[0], np.cumsum(np.bincount(m_rid, minlength=n))])[m_rid]
                keep = (L[m_rid] == 0) | (within < L[m_rid])
                want_starts = np.concatenate([[0], np.cumsum(np.bincount(m_rid[keep], minlength=n))])
                same = bool(np.array_equal(got_starts, want_starts) and np.array_equal(got_keys, m_keys[keep]))
                read = r["range_sources_read"].cpu().numpy()[:n]
                line = {"what": "sdb_lsm_scan_recency, workload (%s), %s" % (wname, setting), "ranges": n, "tables": T,
                        "scan_recency_device": d_rec, "scan_mem_device": d_mem, "scan_mem_device_after": d_mem2,
                        "recency_over_scan_mem": round(d_rec["median_ms"] / d_mem["median_ms"], 3),
                        "summary": {k: v for k, v in zip(runtime.LSM_SCAN_SUMMARY, smr)},
                        "sources_read_mean": round(float(read.mean()), 2), "sources": nsrc,
                        "visible": int(r["range_visible"].cpu().numpy()[:n].sum()), "same_rows": same}
                line["summary"]["status"] &= 0xFFFFFFFF
                lines.append(line)
                print(json.dumps(line), flush=True)
    if a.out and not a.one_call:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
