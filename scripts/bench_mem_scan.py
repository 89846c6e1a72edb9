"""Batched Db::scan over device memtables and the tree (sdb_lsm_scan_mem): the tree of scripts/bench_get.py (8 L0
SSTs plus 3 sorted runs of 8 SSTs of the configs[1] shape), in front of it one active and three immutable
memtables of the same row shape (16-byte keys, 100-byte values), and the two workloads of scripts/bench_lsm_scan.py:
(a) 4,096 narrow ranges, (b) 64 wide ranges, start included, end excluded.

  python scripts/bench_mem_scan.py [--reps R] [--sst-entries N] [--table-entries N] [--workload a|b|all] [--mix NAME]
                                   [--out FILE] [--one-call MIX]

Mixes: "mem_only" ranges whose rows are all in tables (the tree's key space ends below the ranges: no SST takes
part); "spread" the tables' keys interleave with the tree's, rows come from both; "tree_only" the tables hold no key
of any range; "zero_tables" the same ranges with no tables at all (mem NULL).

Two yardsticks, neither of them the code under test (both exist at the parent commit):
  1. what a caller had to do before: sdb_lsm_scan_projected over the tree, a synchronise, its key / seq / sst
     columns copied back, the tables' key / seq / flag columns copied back, and the deduplicating merge on the
     host (numpy: the tables' stretches by searchsorted, one lexsort over range, key, -seq, source);
  2. sdb_lsm_scan_projected alone on the same ranges, as device time, before and after the call under test: for
     zero_tables the same kernel sequence.

Per (workload, mix) one JSON line: the device time of sdb_lsm_scan_mem between two events and of yardstick 2, the
wall-clock per call of sdb_lsm_scan_mem (columns copied back) and of yardstick 1, medians of R with min .. max, the
summary, and the agreement on every row (range, key, seq, source) with yardstick 1.  --one-call runs a single call
of one mix after the warm-up, for `rocprofv3 --kernel-trace --stats`.  A record, not a gate.
"""
import argparse
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
from slatedb_amd import _abi, datasets, runtime  # noqa: E402
from slatedb_amd.batch import Run  # noqa: E402

TABLES = 4
TOP = 1 << 62  # the tree's counters are uniform below this


def build_tables(n_per_table, dev, taken, lo, hi, seed):
    """-> (DeviceRuns in search order, per table the sorted counters in [lo, hi)).  One version per key, seqs above
    the tree's, keys disjoint from the tree's and from one another."""
    rng = np.random.default_rng(seed)
    druns, counters = [], []
    for t in range(TABLES):
        c = np.unique(rng.integers(lo, hi, n_per_table, dtype=np.uint64))
        c = c[~np.isin(c, taken)]
        taken = np.concatenate([taken, c])
        druns.append(runtime.DeviceRun.from_host(Run.from_batch(BG.make_batch(c, 2000 - t, 500 + t)), dev))
        counters.append(c)
    return druns, counters


def ranges_of(rng, lo, hi, per_key, count, width):
    span = int(width * per_key)
    starts = rng.integers(lo, hi - span, count, dtype=np.uint64)
    return [(BG.key_of(s), _abi.BOUND_INCLUDED, BG.key_of(int(s) + span), _abi.BOUND_EXCLUDED) for s in starts], starts, span


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sst-entries", type=int, default=datasets.D1_N)
    ap.add_argument("--table-entries", type=int, default=datasets.D1_N)
    ap.add_argument("--workload", default="all")
    ap.add_argument("--mix", default="all")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-call", default=None)
    a = ap.parse_args()
    reps = max(5, a.reps)
    runtime.require_device()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    t0 = time.perf_counter()
    views, runs, info = BG.build_tree(a.sst_entries, dev)
    tree = runtime.lsm_tree_device(views, runs)
    ns = len(views)
    tree_c = np.unique(np.concatenate([x["counters"] for x in info]))
    total = sum(x["counters"].size for x in info)
    # "spread": tables inside the tree's key space; "mem_only": tables above it (counters in [2^62, 2^63))
    inside, inside_c = build_tables(a.table_entries, dev, tree_c, 0, TOP, 31)
    above, above_c = build_tables(a.table_entries, dev, tree_c, TOP, 2 * TOP, 37)
    mems = {"spread": (runtime.mem_tables_device(inside), inside, inside_c),
            "mem_only": (runtime.mem_tables_device(above), above, above_c)}
    lines = [{"what": "tree and tables", "ssts": ns, "runs": len(runs), "total_blocks": tree["total_blocks"],
              "entries_per_sst": a.sst_entries, "tables": TABLES, "rows_per_table": [int(t.size) for t in inside_c],
              "build_s": round(time.perf_counter() - t0, 1)}]
    print(json.dumps(lines[0]), flush=True)
    rng = np.random.default_rng(33)
    for wname, count, width in (("a", 4096, 100), ("b", 64, 50000)):
        if a.workload not in ("all", wname):
            continue
        for mix in ("mem_only", "spread", "tree_only", "zero_tables"):
            if a.mix not in ("all", mix) or (a.one_call and a.one_call != mix):
                continue
            if mix == "mem_only":  # about `width` rows per range, all from the four tables
                mem, druns, tabs = mems["mem_only"]
                ranges, _, _ = ranges_of(rng, TOP, 2 * TOP, TOP / sum(t.size for t in tabs), count, width)
            elif mix == "spread":  # about `width` rows per range from the tree and the tables together
                mem, druns, tabs = mems["spread"]
                ranges, _, _ = ranges_of(rng, 0, TOP, TOP / (total + sum(t.size for t in tabs)), count, width)
            else:  # the tree's ranges; tables that hold none of their keys, or no tables
                mem, druns, tabs = mems["mem_only"] if mix == "tree_only" else (None, [], [])
                ranges, _, _ = ranges_of(rng, 0, TOP, TOP / total, count, width)
            n = len(ranges)
            rt = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev)
                  for k, v in runtime.scan_ranges_columnar(ranges).items()}
            rt["n"] = n
            host_lo = np.array([r[0] for r in ranges], dtype="S16")
            host_hi = np.array([r[2] for r in ranges], dtype="S16")
            with torch.cuda.stream(s):
                sized = runtime.lsm_scan_mem_device(mem, tree, rt, stream=s)  # the sizing calls of rule 6
                s.synchronize()
                sm = [int(x) for x in sized["summary"].cpu().numpy()]
                cand, cap = (sm[2], sm[3]), (sm[0], sm[1])
                ws = sized["_ws"]
                psized = runtime.lsm_scan_projected_device(tree, None, rt, stream=s)
                s.synchronize()
                pm = [int(x) for x in psized["summary"].cpu().numpy()]
                pcand, pcap, pws = (pm[2], pm[3]), (pm[0], pm[1]), psized["_ws"]
                res = {}

                def new_path():
                    res["r"] = runtime.lsm_scan_mem_device(mem, tree, rt, stream=s, workspace=ws, cand=cand, cap=cap)

                def projected():
                    res["p"] = runtime.lsm_scan_projected_device(tree, None, rt, stream=s, workspace=pws, cand=pcand, cap=pcap)

                def rows_of(r, ne):
                    keys = r["key_arena"].cpu().numpy()[:16 * ne].reshape(-1, 16)  # every key is 16 bytes
                    return r["range_entry_start"].cpu().numpy()[:n + 1], keys, r["seq"].cpu().numpy()[:ne], r["sst"].cpu().numpy()[:ne]

                def new_host():
                    new_path()
                    s.synchronize()
                    r = res["r"]
                    ne = int(r["summary"][0].item())
                    return rows_of(r, ne) + (r["table"].cpu().numpy()[:ne],)

                def old_host():
                    """Yardstick 1: the projected scan, a synchronise, the columns and the tables' columns copied back, the merge."""
                    projected()
                    s.synchronize()
                    r = res["p"]
                    ne = int(r["summary"][0].item())
                    starts, keys, seq, sst = rows_of(r, ne)
                    rid = [np.repeat(np.arange(n), np.diff(starts))]
                    keys, seq, src = [keys], [seq.astype(np.int64)], [sst.astype(np.int64) + TABLES]
                    flags = [np.zeros(ne, np.uint8)]  # the projected scan has dropped the tree's tombstones; no table row can revive one
                    for t, d in enumerate(druns):
                        tk = d.t[0].cpu().numpy()[:16 * d.n].reshape(-1, 16)
                        tseq = d.t[5].cpu().numpy().view(np.int64)[:d.n]
                        tfl = d.t[6].cpu().numpy()[:d.n]
                        flat = tk.view("S16").ravel()
                        g0, g1 = np.searchsorted(flat, host_lo, "left"), np.searchsorted(flat, host_hi, "left")
                        idx = np.concatenate([np.arange(x, y) for x, y in zip(g0, g1)]) if n else np.zeros(0, np.int64)
                        rid.append(np.repeat(np.arange(n), np.maximum(g1 - g0, 0)))
                        keys.append(tk[idx])
                        seq.append(tseq[idx])
                        flags.append(tfl[idx])
                        src.append(np.full(idx.size, t, np.int64))
                    rid, keys, seq, flags, src = (np.concatenate(x) for x in (rid, keys, seq, flags, src))
                    hi, lo = keys[:, :8].copy().view(">u8").ravel(), keys[:, 8:].copy().view(">u8").ravel()
                    order = np.lexsort((src, -seq, lo, hi, rid))
                    rid, hi, lo, seq, flags, src, keys = rid[order], hi[order], lo[order], seq[order], flags[order], src[order], keys[order]
                    first = np.ones(rid.size, bool)
                    first[1:] = (rid[1:] != rid[:-1]) | (hi[1:] != hi[:-1]) | (lo[1:] != lo[:-1])
                    keep = first & ((flags & _abi.FLAG_TOMBSTONE) == 0)
                    starts = np.concatenate([[0], np.cumsum(np.bincount(rid[keep], minlength=n))])
                    return starts, keys[keep], seq[keep], src[keep]

                def wall(fn):
                    for _ in range(2):
                        fn()
                    ms = []
                    for _ in range(reps):
                        torch.cuda.synchronize()
                        t = time.perf_counter()
                        fn()
                        ms.append((time.perf_counter() - t) * 1e3)
                    return BG.stats(ms)

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

                if a.one_call:
                    new_host()
                    new_host()
                    torch.cuda.synchronize()
                    new_path()  # the call to read from the kernel trace: the last of its kernels' three
                    torch.cuda.synchronize()
                    continue
                t_new = wall(new_host)
                d_proj = device(projected)
                d_new = device(new_path)
                d_proj2 = device(projected)  # again after, so a drift of the machine shows beside the difference
                got = new_host()
                smr = res["r"]["summary"].cpu().numpy()
                t_old = wall(old_host)
                want = old_host()
                src_new = np.where(got[4] >= 0, got[4].astype(np.int64), got[3].astype(np.int64) + TABLES)
                same = (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and
                        np.array_equal(got[2].astype(np.int64), want[2]) and np.array_equal(src_new, want[3]))
                line = {"what": "sdb_lsm_scan_mem, workload (%s), mix %s" % (wname, mix), "ranges": n,
                        "tables": TABLES if mem else 0, "scan_mem_device": d_new, "scan_projected_device": d_proj,
                        "scan_projected_device_after": d_proj2, "scan_mem_wall": t_new,
                        "projected_scan_plus_host_merge_wall": t_old,
                        "new_over_old_wall": round(t_new["median_ms"] / t_old["median_ms"], 3),
                        "summary": {k: int(v) for k, v in zip(runtime.LSM_SCAN_SUMMARY, smr)},
                        "rows_from_tables": int((got[4] >= 0).sum()), "same_rows": bool(same)}
                line["summary"]["status"] &= 0xFFFFFFFF
                lines.append(line)
                print(json.dumps(line), flush=True)
    if a.out and not a.one_call:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
