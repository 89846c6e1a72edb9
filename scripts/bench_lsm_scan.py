"""Batched Db::scan measurements (sdb_lsm_scan) on the device-resident tree of scripts/bench_get.py: 8 L0 SSTs
plus 3 sorted runs of 8 SSTs, every SST of the configs[1] shape (578,524 entries, 16-byte keys, 100-byte
values, 4 KiB blocks).

  python scripts/bench_lsm_scan.py [--reps R] [--sst-entries N] [--workload a|b|all] [--skip-baseline]

Workloads: (a) 4,096 ranges of about 100 keys; (b) 64 wide ranges of about 50,000 keys.  Every range is
start included, end excluded, as Db::scan builds it.

The yardstick is what a caller had to do before the call existed: one sdb_sst_scan per SST of the tree with all
ranges (its columns sized exactly, so one call each), a synchronise, the key, seq and flag columns copied back and
the merge on the host: per range the newest version per key over all SSTs, tombstones dropped.

Per workload one JSON line: wall-clock per call of both paths (host time included, the stream synchronised and the
result columns copied back), the device time of sdb_lsm_scan between two events, medians of R with min .. max,
the summary, and whether both paths agree on every row (key, seq, SST).  A record, not a gate.
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
from bench_get import build_tree, key_of, stats  # noqa: E402
from slatedb_amd import _abi, datasets, runtime  # noqa: E402


def workloads(info):
    """name -> [(start, INCLUDED, end, EXCLUDED)]: ranges of about `width` keys of the tree's key space."""
    rng = np.random.default_rng(33)
    total = sum(x["counters"].size for x in info)
    per_key = (1 << 62) / total  # the counters are uniform in [0, 2^62)
    out = {}
    for name, count, width in (("a", 4096, 100), ("b", 64, 50000)):
        span = int(width * per_key)
        starts = rng.integers(0, (1 << 62) - span, count, dtype=np.uint64)
        out[name] = [(key_of(s), _abi.BOUND_INCLUDED, key_of(int(s) + span), _abi.BOUND_EXCLUDED) for s in starts]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sst-entries", type=int, default=datasets.D1_N)
    ap.add_argument("--workload", default="all")
    ap.add_argument("--skip-baseline", action="store_true")
    a = ap.parse_args()
    reps = max(5, a.reps)
    runtime.require_device()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    t0 = time.perf_counter()
    views, runs, info = build_tree(a.sst_entries, dev)
    tree = runtime.lsm_tree_device(views, runs)
    ns = len(views)
    print(json.dumps({"what": "tree", "ssts": ns, "runs": len(runs), "total_blocks": tree["total_blocks"],
                      "entries_per_sst": a.sst_entries, "build_s": round(time.perf_counter() - t0, 1)}), flush=True)
    for name, ranges in workloads(info).items():
        if a.workload not in ("all", name):
            continue
        n = len(ranges)
        rt = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev)
              for k, v in runtime.scan_ranges_columnar(ranges).items()}
        rt["n"] = n
        with torch.cuda.stream(s):
            sized = runtime.lsm_scan_device(tree, rt, stream=s)  # the sizing calls of rule 6
            s.synchronize()
            sm = [int(x) for x in sized["summary"].cpu().numpy()]
            cand, cap = (sm[2], sm[3]), (sm[0], sm[1])
            ws = sized["_ws"]
            res = {}

            def new_path():
                res["r"] = runtime.lsm_scan_device(tree, rt, stream=s, workspace=ws, cand=cand, cap=cap)

            def new_host():
                new_path()
                s.synchronize()
                r = res["r"]
                return (r["range_entry_start"].cpu().numpy(), r["key_arena"].cpu().numpy(), r["key_off"].cpu().numpy(),
                        r["seq"].cpu().numpy(), r["sst"].cpu().numpy())

            # the baseline's exact column sizes, found once outside the timed region
            caps = []
            if not a.skip_baseline:
                for v in views:
                    o = runtime.sst_scan_device(v, rt, stream=s)
                    m = o["summary"].cpu().numpy()
                    caps.append((int(m[0]), int(m[1])))

            def old_host():
                """sdb_sst_scan per SST, a synchronise, the columns copied back, the merge on the host."""
                outs = [runtime.sst_scan_device(v, rt, stream=s, cap_entries=c[0], key_cap=c[1]) for v, c in zip(views, caps)]
                s.synchronize()
                rid, keys, seq, flags, sst = [], [], [], [], []
                for i, (o, c) in enumerate(zip(outs, caps)):
                    res_ = o["range_entry_start"].cpu().numpy()
                    rid.append(np.repeat(np.arange(n), np.diff(res_)))
                    keys.append(o["key_arena"].cpu().numpy()[:c[1]].reshape(-1, 16))  # the tree's keys are 16 bytes
                    seq.append(o["seq"].cpu().numpy()[:c[0]])
                    flags.append(o["flags"].cpu().numpy()[:c[0]])
                    sst.append(np.full(c[0], i, np.int32))
                rid, keys, seq = np.concatenate(rid), np.concatenate(keys), np.concatenate(seq)
                flags, sst = np.concatenate(flags), np.concatenate(sst)
                hi, lo = keys[:, :8].copy().view(">u8").ravel(), keys[:, 8:].copy().view(">u8").ravel()
                order = np.lexsort((sst, -seq, lo, hi, rid))  # range, key ascending, seq descending, search order
                rid, hi, lo, seq, flags, sst, keys = rid[order], hi[order], lo[order], seq[order], flags[order], sst[order], keys[order]
                first = np.ones(rid.size, bool)
                first[1:] = (rid[1:] != rid[:-1]) | (hi[1:] != hi[:-1]) | (lo[1:] != lo[:-1])
                keep = first & ((flags & _abi.FLAG_TOMBSTONE) == 0)
                starts = np.concatenate([[0], np.cumsum(np.bincount(rid[keep], minlength=n))])
                return starts, keys[keep].reshape(-1), None, seq[keep], sst[keep]

            def wall(fn):
                for _ in range(2):
                    fn()
                ms = []
                for _ in range(reps):
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    fn()
                    ms.append((time.perf_counter() - t) * 1e3)
                return stats(ms)

            t_new = wall(new_host)
            ev = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                new_path()
                e1.record(s)
                torch.cuda.synchronize()
                ev.append(e0.elapsed_time(e1))
            got = new_host()
            smr = res["r"]["summary"].cpu().numpy()
            line = {"what": "sdb_lsm_scan, workload (%s)" % name, "ranges": n, "lsm_scan_wall": t_new,
                    "lsm_scan_device": stats(ev), "summary": {k: int(v) for k, v in zip(runtime.LSM_SCAN_SUMMARY, smr)}}
            line["summary"]["status"] &= 0xFFFFFFFF
            if not a.skip_baseline:
                t_old = wall(old_host)
                want = old_host()
                ne = int(got[0][n])
                same = (np.array_equal(got[0][:n + 1], want[0]) and np.array_equal(got[1][:16 * ne], want[1]) and
                        np.array_equal(got[3][:ne], want[3]) and np.array_equal(got[4][:ne], want[4]))
                line.update(scan_per_sst_wall=t_old, new_over_old=round(t_new["median_ms"] / t_old["median_ms"], 3),
                            same_rows=bool(same))
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
