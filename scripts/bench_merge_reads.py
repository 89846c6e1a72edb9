"""Merging-read measurements (sdb_lsm_get_merge, sdb_lsm_scan_merge) on the device-resident tree of
scripts/bench_get.py: 8 L0 SSTs plus 3 sorted runs of 8 SSTs, every SST of the configs[1] shape (578,524 entries,
16-byte keys, 100-byte values, 4 KiB blocks, 10 filter bits per key).

  python scripts/bench_merge_reads.py [--reps R] [--sst-entries N] [--keys K] [--chain 0|4|64] [--share S]

--chain 0 is that tree as it stands: no operand anywhere, every chain is one link, so the difference between
sdb_lsm_get_merge and sdb_lsm_get (and between the scans) is the cost of the count, scan and emit passes.  With
--chain C, keys / S extra keys (S = --share, default 8) are written as C merge operands each and nothing else,
spread round-robin over the 11 levels (C = 4: the newest and the fourth L0 SST, the newest and the oldest sorted
run), newer levels holding higher seqs; their chains run through every level and end without a base.

Gets: the "spread" mix of bench_get.py, every S-th key replaced by a chain key.  Scans: 4,096 ranges of about 100
keys, start included, end excluded (workload (a) of bench_lsm_scan.py), every S-th range starting on a chain key.

Per call one JSON line: device time between two events and wall-clock (host time, a stream synchronise), medians
of R with min .. max, and the summaries.  On a tree with chains the plain calls report their operands
(SDB_MERGE_OPERATOR_MISSING) and are timed only as the same walk without the chain passes.  A record, not a gate.
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
from bench_get import L0, PER_RUN, RUNS, key_of, mixes, stats  # noqa: E402
from oracle import oracle as O  # noqa: E402
from slatedb_amd import _abi, datasets, runtime  # noqa: E402
from slatedb_amd.batch import Batch  # noqa: E402

LEVELS = L0 + RUNS


def make_batch(counters, kind, seq, seed):
    """Rows sorted by (counter, seq descending) -> 16-byte keys as bench_get.make_batch builds them."""
    n = counters.size
    keys = np.zeros((n, 16), np.uint8)
    keys[:, 4:12] = counters.astype(">u8").view(np.uint8).reshape(-1, 8)
    vals = datasets.random_bytes(seed, 2, n * 104).reshape(n, 104)[:, :100]
    return Batch(keys.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(16), np.ascontiguousarray(vals).reshape(-1),
                 np.arange(n + 1, dtype=np.uint64) * np.uint64(100), kind, seq, None, None, None)


def build_tree(n_per_sst, dev, chain, chain_keys):
    """bench_get.build_tree (the same draws), plus `chain` operand versions of every chain key: version v in level
    v % 11 when chain >= 11, else in the levels spread evenly from the newest to the oldest."""
    rng = np.random.default_rng(7)
    views, info, runs = [], [], []
    prm = O.params(block_size=4096, sst_version=2, bloom_bits_per_key=10)
    probes = O.optimal_num_probes(10)
    dv = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).to(dev)  # noqa: E731
    if chain >= LEVELS:
        per_level = [chain // LEVELS + (1 if j < chain % LEVELS else 0) for j in range(LEVELS)]
    else:
        per_level = [0] * LEVELS
        for v in range(chain):
            per_level[round(v * (LEVELS - 1) / max(chain - 1, 1))] += 1

    def rows(counters, level):
        """The level's own values and its share of the chain keys' operands, sorted as an SST holds them."""
        m = per_level[level]
        base_seq = (1000 - level) * 1000
        c = np.concatenate([counters] + [chain_keys] * m)
        kind = np.concatenate([np.zeros(counters.size, np.uint8)] + [np.ones(chain_keys.size, np.uint8)] * m)
        seq = np.concatenate([np.full(counters.size, base_seq, np.uint64)] +
                             [np.full(chain_keys.size, base_seq - x, np.uint64) for x in range(m)])
        order = np.lexsort((np.uint64(1 << 63) - seq, c))
        return c[order], kind[order], seq[order]

    def add(c, kind, seq):
        b = make_batch(c, kind, seq, 100 + len(views))
        enc = O.encode_sst(b, prm)
        assert enc.status == 0
        ik, iko = O.sst_index_keys(b, enc)
        nb = len(enc.block_off) - 1
        views.append({"data": dv(np.concatenate([enc.data, np.zeros(64, np.uint8)])), "block_off": dv(enc.block_off),
                      "num_blocks": nb, "index_keys": dv(ik if ik.size else np.zeros(16, np.uint8)), "index_key_off": dv(iko),
                      "sst_version": 2, "bloom": dv(enc.bloom), "bloom_len": len(enc.bloom), "num_probes": probes,
                      "first_key": b.key(0), "last_key": b.key(b.n - 1)})
        info.append({"counters": np.unique(c[kind == 0])})

    level = 0
    for _ in range(L0):
        add(*rows(np.unique(rng.integers(0, 1 << 62, n_per_sst, dtype=np.uint64)), level))
        runs.append(1)
        level += 1
    for _ in range(RUNS):
        c, kind, seq = rows(np.unique(rng.integers(0, 1 << 62, n_per_sst * PER_RUN, dtype=np.uint64)), level)
        for part in np.array_split(np.arange(c.size), PER_RUN):
            add(c[part], kind[part], seq[part])
        runs.append(PER_RUN)
        level += 1
    return views, runs, info


def timed(fn, s, reps):
    """fn() enqueues one call on stream s -> (device time between two events, wall-clock with a synchronise)."""
    for _ in range(2):
        fn()
    s.synchronize()
    wall, ev = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        s.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        torch.cuda.synchronize()
        ev.append(e0.elapsed_time(e1))
    return {"device": stats(ev), "wall": stats(wall)}


def words(t, names):
    d = {k: int(v) for k, v in zip(names, t.cpu().numpy())}
    d["status"] &= 0xFFFFFFFF
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sst-entries", type=int, default=datasets.D1_N)
    ap.add_argument("--keys", type=int, default=65536)
    ap.add_argument("--chain", type=int, default=0)
    ap.add_argument("--share", type=int, default=8)
    a = ap.parse_args()
    reps = max(5, a.reps)
    runtime.require_device()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    t0 = time.perf_counter()
    crng = np.random.default_rng(77)
    # uniform over the tree's key space; 2^62 counters make a collision with a value key a non-event
    chain_keys = np.unique(crng.integers(0, 1 << 62, a.keys // a.share if a.chain else 0, dtype=np.uint64))
    views, runs, info = build_tree(a.sst_entries, dev, a.chain, chain_keys)
    tree = runtime.lsm_tree_device(views, runs)
    ns, nr = len(views), len(runs)
    print(json.dumps({"what": "tree", "ssts": ns, "runs": nr, "total_blocks": tree["total_blocks"], "chain": a.chain,
                      "chain_keys": int(chain_keys.size), "build_s": round(time.perf_counter() - t0, 1)}), flush=True)
    lib = runtime.lib()
    with torch.cuda.stream(s):
        # ---- gets
        keys = mixes(info, a.keys)["spread"]
        for j in range(chain_keys.size):
            keys[j * a.share] = key_of(chain_keys[j])
        n = len(keys)
        hb, ho = runtime.keys_columnar(keys)
        kb, ko = torch.from_numpy(hb).to(dev), torch.from_numpy(ho.view(np.int64)).to(dev)
        ws = torch.empty(lib.sdb_lsm_get_merge_workspace_bytes(tree["total_blocks"], ns, nr, n), dtype=torch.uint8, device=dev)
        res = {}
        sized = runtime.lsm_get_merge_device(tree, None, (kb, ko, n), stream=s, workspace=ws)
        s.synchronize()
        cap_links = int(sized["chain_summary"][0])

        def get_plain():
            res["g"] = runtime.lsm_get_device(tree, None, (kb, ko, n), stream=s, workspace=ws)

        def get_merge():
            res["m"] = runtime.lsm_get_merge_device(tree, None, (kb, ko, n), stream=s, workspace=ws, cap_links=cap_links)

        line = {"what": "gets, spread mix", "keys": n, "chain": a.chain, "sdb_lsm_get": timed(get_plain, s, reps),
                "sdb_lsm_get_merge": timed(get_merge, s, reps)}
        line["get_summary"] = words(res["g"]["summary"], runtime.GET_SUMMARY)
        line["get_merge_summary"] = words(res["m"]["summary"], runtime.GET_SUMMARY)
        line["chains"] = words(res["m"]["chain_summary"], runtime.CHAIN_SUMMARY)
        print(json.dumps(line), flush=True)
        del ws, sized
        # ---- scans
        rng = np.random.default_rng(33)
        total = sum(x["counters"].size for x in info)
        span = int(100 * (1 << 62) / total)
        starts = rng.integers(0, (1 << 62) - span, 4096, dtype=np.uint64)
        for j in range(min(chain_keys.size, 4096 // a.share)):
            starts[j * a.share] = min(int(chain_keys[j]), (1 << 62) - span - 1)
        ranges = [(key_of(x), _abi.BOUND_INCLUDED, key_of(int(x) + span), _abi.BOUND_EXCLUDED) for x in starts]
        rt = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev)
              for k, v in runtime.scan_ranges_columnar(ranges).items()}
        rt["n"] = len(ranges)
        sized = runtime.lsm_scan_merge_device(tree, rt, stream=s)  # the sizing calls of rule 6
        s.synchronize()
        sm = [int(x) for x in sized["summary"].cpu().numpy()]
        cand, cap, cl = (sm[2], sm[3]), (max(sm[0], 1), max(sm[1], 1)), int(sized["chain_summary"][0])
        wss = sized["_ws"]

        def scan_plain():
            res["s"] = runtime.lsm_scan_device(tree, rt, stream=s, workspace=wss, cand=cand, cap=cap)

        def scan_merge():
            res["sm"] = runtime.lsm_scan_merge_device(tree, rt, stream=s, workspace=wss, cand=cand, cap=cap, cap_links=cl)

        line = {"what": "scans, 4096 ranges of ~100 keys", "chain": a.chain, "sdb_lsm_scan": timed(scan_plain, s, reps),
                "sdb_lsm_scan_merge": timed(scan_merge, s, reps)}
        line["scan_summary"] = words(res["s"]["summary"], runtime.LSM_SCAN_SUMMARY)
        line["scan_merge_summary"] = words(res["sm"]["summary"], runtime.LSM_SCAN_SUMMARY)
        line["chains"] = words(res["sm"]["chain_summary"], runtime.CHAIN_SUMMARY)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
