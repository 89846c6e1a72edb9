"""Db::scan_prefix measurements: sdb_lsm_scan_filtered next to sdb_lsm_scan on a device-resident tree of the shape
scripts/bench_lsm_scan.py scans (8 L0 SSTs plus 3 sorted runs of 8 SSTs, 16-byte keys, 100-byte values, 4 KiB
blocks, 10 filter bits per key), with keys that carry a 4-byte tenant prefix and filters built with the
fixed-length extractor (prefix_kind = SDB_PREFIX_FIXED, prefix_arg = 4, whole keys too).

  python scripts/bench_prefix_scan.py [--reps R] [--sst-entries N] [--tenants T] [--ranges K]

Every SST holds a subset of the T tenants: an L0 SST a random quarter of them, a sorted run a random half, dealt
to its 8 SSTs in key order, so an SST's key interval spans tenants it does not hold.  The batch is K scan_prefix
ranges: a tenant's prefix and about 100 of its keys, start included, end excluded.

One JSON line: per path the device time of a call between two events and the wall-clock with the stream
synchronised (medians of R with min .. max), blocks_checked, num_candidates and, for the filtered call,
num_filtered; and whether both paths return the same rows.  A record, not a gate.
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
from bench_get import L0, PER_RUN, RUNS, stats  # noqa: E402
from oracle import oracle as O  # noqa: E402
from slatedb_amd import _abi, datasets, runtime  # noqa: E402
from slatedb_amd.batch import Batch  # noqa: E402

POLICY = (_abi.PREFIX_FIXED, 4, 0)


def key_of(tenant, counter):
    return int(tenant).to_bytes(4, "big") + int(counter).to_bytes(8, "big") + b"\0\0\0\0"


def make_batch(tenants, counters, seq, seed):
    """(tenant, counter) pairs sorted by key -> 16-byte keys: the tenant and the counter big-endian, 4 zero bytes."""
    n = counters.size
    keys = np.zeros((n, 16), np.uint8)
    keys[:, :4] = tenants.astype(">u4").view(np.uint8).reshape(-1, 4)
    keys[:, 4:12] = counters.astype(">u8").view(np.uint8).reshape(-1, 8)
    vals = datasets.random_bytes(seed, 2, n * 104).reshape(n, 104)[:, :100]
    return Batch(keys.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(16), np.ascontiguousarray(vals).reshape(-1),
                 np.arange(n + 1, dtype=np.uint64) * np.uint64(100), np.zeros(n, np.uint8), np.full(n, seq, np.uint64),
                 None, None, None)


def build_tree(n_per_sst, ntenants, dev):
    """-> (views, runs): the views carry the filter and its policy."""
    rng = np.random.default_rng(7)
    views, runs = [], []
    prm = O.params(block_size=4096, sst_version=2, bloom_bits_per_key=10, prefix_kind=POLICY[0], prefix_arg=POLICY[1])
    probes = O.optimal_num_probes(10)
    dv = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).to(dev)  # noqa: E731

    def pairs(held, n):
        t = rng.choice(held, n).astype(np.uint64)
        c = rng.integers(0, 1 << 62, n, dtype=np.uint64)
        order = np.lexsort((c, t))
        return t[order], c[order]

    def add(t, c, seq):
        b = make_batch(t, c, seq, 100 + len(views))
        enc = O.encode_sst(b, prm)
        assert enc.status == 0
        ik, iko = O.sst_index_keys(b, enc)
        views.append({"data": dv(np.concatenate([enc.data, np.zeros(64, np.uint8)])), "block_off": dv(enc.block_off),
                      "num_blocks": len(enc.block_off) - 1, "index_keys": dv(ik), "index_key_off": dv(iko), "sst_version": 2,
                      "bloom": dv(enc.bloom), "bloom_len": len(enc.bloom), "num_probes": probes, "policy": POLICY,
                      "first_key": b.key(0), "last_key": b.key(b.n - 1)})

    level = 0
    for _ in range(L0):
        t, c = pairs(rng.choice(ntenants, max(1, ntenants // 4), replace=False), n_per_sst)
        add(t, c, 1000 - level)
        runs.append(1)
        level += 1
    for _ in range(RUNS):
        t, c = pairs(rng.choice(ntenants, max(PER_RUN, ntenants // 2), replace=False), n_per_sst * PER_RUN)
        for part in np.array_split(np.arange(t.size), PER_RUN):
            add(t[part], c[part], 1000 - level)
        runs.append(PER_RUN)
        level += 1
    return views, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sst-entries", type=int, default=datasets.D1_N)
    ap.add_argument("--tenants", type=int, default=64)
    ap.add_argument("--ranges", type=int, default=4096)
    a = ap.parse_args()
    reps = max(5, a.reps)
    runtime.require_device()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    t0 = time.perf_counter()
    views, runs = build_tree(a.sst_entries, a.tenants, dev)
    tree = runtime.lsm_tree_device(views, runs)
    build_s = round(time.perf_counter() - t0, 1)
    # a tenant's keys in an SST that holds it: sst_entries / (tenants / 4); about 100 of them per range
    rng = np.random.default_rng(33)
    span = int(100 * (1 << 62) / (a.sst_entries / max(1, a.tenants // 4)))
    ten = rng.integers(0, a.tenants, a.ranges)
    start = rng.integers(0, (1 << 62) - span, a.ranges, dtype=np.uint64)
    ranges = [(key_of(t, c), _abi.BOUND_INCLUDED, key_of(t, int(c) + span), _abi.BOUND_EXCLUDED) for t, c in zip(ten, start)]
    n = len(ranges)
    to_dev = lambda d: {k: None if v is None else torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev)  # noqa: E731
                        for k, v in d.items()}
    rt = to_dev(runtime.scan_ranges_columnar(ranges))
    rt["n"] = n
    px = to_dev(runtime.scan_prefixes_columnar([int(t).to_bytes(4, "big") for t in ten]))
    line = {"what": "scan_prefix: sdb_lsm_scan_filtered next to sdb_lsm_scan", "ssts": len(views), "tenants": a.tenants,
            "entries_per_sst": a.sst_entries, "total_blocks": tree["total_blocks"], "ranges": n, "build_s": build_s}
    rows = {}
    with torch.cuda.stream(s):
        for name in ("sdb_lsm_scan", "sdb_lsm_scan_filtered"):
            if name == "sdb_lsm_scan":
                run = lambda **kw: runtime.lsm_scan_device(tree, rt, stream=s, **kw)  # noqa: E731
            else:
                run = lambda **kw: runtime.lsm_scan_filtered_device(tree, rt, px, stream=s, **kw)  # noqa: E731
            sized = run()  # the sizing calls of rule 6
            s.synchronize()
            sm = [int(x) for x in sized["summary"].cpu().numpy()]
            kw = dict(workspace=sized["_ws"], cand=(sm[2], sm[3]), cap=(sm[0], sm[1]))
            wall, ev = [], []
            for i in range(reps + 2):
                torch.cuda.synchronize()
                t = time.perf_counter()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                r = run(**kw)
                e1.record(s)
                s.synchronize()
                if i >= 2:  # two warm-up calls
                    wall.append((time.perf_counter() - t) * 1e3)
                    ev.append(e0.elapsed_time(e1))
            smr = dict(zip(runtime.LSM_SCAN_SUMMARY, (int(x) for x in r["summary"].cpu().numpy())))
            line[name] = {"device": stats(ev), "wall": stats(wall), "blocks_checked": smr["blocks_checked"],
                          "num_candidates": smr["num_candidates"], "num_entries": smr["num_entries"],
                          "status": smr["status"] & 0xFFFFFFFF}
            if name == "sdb_lsm_scan_filtered":
                line[name]["num_filtered"] = int(r["num_filtered"].cpu().numpy()[0])
                line[name]["range_ssts_mean"] = round(float(r["range_ssts"].float().mean()), 2)
            rows[name] = [r[k].cpu().numpy()[:(n + 1 if k == "range_entry_start" else smr["num_entries"])]
                          for k in ("range_entry_start", "seq", "sst", "val_off")]
    line["same_rows"] = all(np.array_equal(x, y) for x, y in zip(rows["sdb_lsm_scan"], rows["sdb_lsm_scan_filtered"]))
    a_, b_ = line["sdb_lsm_scan"]["device"]["median_ms"], line["sdb_lsm_scan_filtered"]["device"]["median_ms"]
    line["filtered_over_unfiltered"] = round(b_ / a_, 3)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
