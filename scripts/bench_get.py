"""Batched Db::get measurements (sdb_lsm_get) on a device-resident tree: 8 L0 SSTs plus 3 sorted runs of 8
SSTs, every SST of the configs[1] shape (578,524 entries, 16-byte keys, 100-byte values, 4 KiB blocks,
10 filter bits per key), 64 Ki keys per call.

  python scripts/bench_get.py [--reps R] [--sst-entries N] [--keys K] [--mix NAME] [--skip-baseline]

The yardstick is what a caller had to do before the call existed: one sdb_sst_lookup per SST of the tree
with all keys, a synchronise, the columns copied back and the chain resolved on the host (newest SST that
holds the key and covers it wins).  That path has no max_seq; the mixes use none.

Mixes: "newest" every key answered by the newest L0 SST; "spread" keys drawn evenly from the 11 levels;
"absent" no key present, so the filters carry the call.

Per mix one JSON line: wall-clock per call of both paths (host time included, the stream synchronised), the
device time of sdb_lsm_get between two events, medians of R with min .. max, blocks_checked next to the
distinct blocks the lazy walk of the reference needs, and whether both paths agree on every key.
A record, not a gate.
"""
import argparse
import bisect
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
from slatedb_amd import _abi, datasets, runtime  # noqa: E402
from slatedb_amd.batch import Batch  # noqa: E402

L0, RUNS, PER_RUN = 8, 3, 8


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
            "spread_ms": round(ms[-1] - ms[0], 4), "reps": len(ms)}


def make_batch(counters, seq, seed):
    """Sorted unique u64 counters -> 16-byte keys (4 zero bytes, the counter big-endian, 4 zero bytes)."""
    n = counters.size
    keys = np.zeros((n, 16), np.uint8)
    keys[:, 4:12] = counters.astype(">u8").view(np.uint8).reshape(-1, 8)
    vals = datasets.random_bytes(seed, 2, n * 104).reshape(n, 104)[:, :100]
    return Batch(keys.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(16), np.ascontiguousarray(vals).reshape(-1),
                 np.arange(n + 1, dtype=np.uint64) * np.uint64(100), np.zeros(n, np.uint8), np.full(n, seq, np.uint64),
                 None, None, None)


def build_tree(n_per_sst, dev):
    """-> (views, runs, per-SST host info).  L0 SSTs sample the whole key space; a run partitions it."""
    rng = np.random.default_rng(7)
    views, info, runs = [], [], []
    prm = O.params(block_size=4096, sst_version=2, bloom_bits_per_key=10)
    probes = O.optimal_num_probes(10)
    dv = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else np.ascontiguousarray(a)).to(dev)  # noqa: E731

    def add(counters, seq):
        b = make_batch(counters, seq, 100 + len(views))
        enc = O.encode_sst(b, prm)
        assert enc.status == 0
        ik, iko = O.sst_index_keys(b, enc)
        nb = len(enc.block_off) - 1
        ikb = ik.tobytes()
        views.append({"data": dv(np.concatenate([enc.data, np.zeros(64, np.uint8)])), "block_off": dv(enc.block_off),
                      "num_blocks": nb, "index_keys": dv(ik if ik.size else np.zeros(16, np.uint8)), "index_key_off": dv(iko),
                      "sst_version": 2, "bloom": dv(enc.bloom), "bloom_len": len(enc.bloom), "num_probes": probes,
                      "first_key": b.key(0), "last_key": b.key(b.n - 1)})
        info.append({"counters": counters, "first": b.key(0), "last": b.key(b.n - 1), "nb": nb,
                     "index_keys": [ikb[int(iko[k]):int(iko[k + 1])] for k in range(nb)]})

    level = 0
    for _ in range(L0):
        add(np.unique(rng.integers(0, 1 << 62, n_per_sst, dtype=np.uint64)), 1000 - level)
        runs.append(1)
        level += 1
    for _ in range(RUNS):
        c = np.unique(rng.integers(0, 1 << 62, n_per_sst * PER_RUN, dtype=np.uint64))
        for part in np.array_split(c, PER_RUN):
            add(part, 1000 - level)
        runs.append(PER_RUN)
        level += 1
    return views, runs, info


def key_of(counter):
    return b"\0\0\0\0" + int(counter).to_bytes(8, "big") + b"\0\0\0\0"


def mixes(info, nkeys):
    rng = np.random.default_rng(21)
    pick = lambda i, m: rng.choice(info[i]["counters"], m, replace=False)  # noqa: E731
    levels = [[i] for i in range(L0)] + [list(range(L0 + r * PER_RUN, L0 + (r + 1) * PER_RUN)) for r in range(RUNS)]
    spread = []
    for j, ssts in enumerate(levels):
        m = nkeys // len(levels) + (1 if j < nkeys % len(levels) else 0)
        per = [m // len(ssts) + (1 if x < m % len(ssts) else 0) for x in range(len(ssts))]
        spread += [pick(i, p) for i, p in zip(ssts, per)]
    present = np.unique(np.concatenate([x["counters"] for x in info]))
    absent = rng.integers(0, 1 << 62, nkeys + 1024, dtype=np.uint64)
    absent = absent[~np.isin(absent, present)][:nkeys]
    out = {"newest": pick(0, nkeys), "spread": rng.permutation(np.concatenate(spread)), "absent": absent}
    return {k: [key_of(c) for c in v] for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sst-entries", type=int, default=datasets.D1_N)
    ap.add_argument("--keys", type=int, default=65536)
    ap.add_argument("--mix", default="all")
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
                      "entries_per_sst": a.sst_entries, "encoded_bytes": int(sum(v["data"].numel() for v in views)),
                      "build_s": round(time.perf_counter() - t0, 1)}), flush=True)
    for name, keys in mixes(info, a.keys).items():
        if a.mix not in ("all", name):
            continue
        n = len(keys)
        hb, ho = runtime.keys_columnar(keys)
        kb, ko = torch.from_numpy(hb).to(dev), torch.from_numpy(ho.view(np.int64)).to(dev)
        ws = torch.empty(runtime.lib().sdb_lsm_get_workspace_bytes(tree["total_blocks"], ns, len(runs), n),
                         dtype=torch.uint8, device=dev)
        res = {}

        def new_path():
            res["r"] = runtime.lsm_get_device(tree, None, (kb, ko, n), stream=s, workspace=ws)

        def new_host():
            new_path()
            s.synchronize()
            return res["r"]["state"].cpu().numpy(), res["r"]["sst"].cpu().numpy()

        def old_host():
            """sdb_sst_lookup per SST, a synchronise, the resolve on the host."""
            outs = [runtime.sst_lookup_device(v, kb, ko, n, stream=s) for v in views]
            s.synchronize()
            state = np.stack([o["state"].cpu().numpy()[:n] for o in outs])
            flags = np.stack([o["flags"].cpu().numpy()[:n] for o in outs])
            found = state == _abi.LOOKUP_FOUND  # in a sorted run only the SST that holds the key reports FOUND
            first = np.where(found.any(0), found.argmax(0), -1)
            fl = flags[np.maximum(first, 0), np.arange(n)]
            st = np.where(first < 0, _abi.GET_NOT_FOUND,
                          np.where(fl & _abi.FLAG_TOMBSTONE, _abi.GET_DELETED,
                                   np.where(fl & _abi.FLAG_MERGE_OPERAND, _abi.GET_MERGE_OPERAND, _abi.GET_FOUND)))
            return st.astype(np.uint8), first.astype(np.int32), state

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

        with torch.cuda.stream(s):
            t_new = wall(new_host)
            ev = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                new_path()
                e1.record(s)
                torch.cuda.synchronize()
                ev.append(e0.elapsed_time(e1))
            st_new, sst_new = new_host()
            sm = res["r"]["summary"].cpu().numpy()
            line = {"what": "sdb_lsm_get, mix " + name, "keys": n, "lsm_get_wall": t_new, "lsm_get_device": stats(ev),
                    "states": {k: int(v) for k, v in zip(runtime.GET_SUMMARY, sm)}}
            line["states"]["status"] &= 0xFFFFFFFF
            if not a.skip_baseline:
                t_old = wall(lambda: old_host())
                st_old, sst_old, state = old_host()
                line.update(lookup_per_sst_wall=t_old, new_over_old=round(t_new["median_ms"] / t_old["median_ms"], 3),
                            same_answers=bool(np.array_equal(st_new[:n], st_old) and np.array_equal(sst_new[:n], sst_old)))
                # the distinct blocks the lazy chain needs: per key the covering SSTs in order, the filtered ones
                # skipped (the lookups' own verdict), up to the SST that holds the key
                need = set()
                for q, k in enumerate(keys):
                    for i in range(ns):
                        x = info[i]
                        if not (x["first"] <= k <= x["last"]):
                            continue
                        if state[i, q] == _abi.LOOKUP_FILTERED:
                            continue
                        lt, le = bisect.bisect_left(x["index_keys"], k), bisect.bisect_right(x["index_keys"], k)
                        b0 = lt - 1 if lt else 0
                        need.update((i, b) for b in range(b0, le if le else b0))
                        if state[i, q] == _abi.LOOKUP_FOUND:
                            break
                line["blocks_lazy_walk_needs"] = len(need)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
