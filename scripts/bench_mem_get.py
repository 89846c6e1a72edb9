"""Batched Db::get over device memtables and the tree (sdb_lsm_get_mem): the tree of scripts/bench_get.py (8 L0
SSTs plus 3 sorted runs of 8 SSTs of the configs[1] shape), in front of it one active and three immutable
memtables of the same row shape (16-byte keys, 100-byte values), 64 Ki keys per call.

  python scripts/bench_mem_get.py [--reps R] [--sst-entries N] [--table-entries N] [--keys K] [--mix NAME]
                                  [--out FILE] [--one-call MIX]

Mixes: "mem_hot" every key in the active table; "mem_spread" keys drawn evenly from the four tables and the 11
tree levels; "tree_only" no key in any table; "zero_tables" the same keys with no tables at all (mem NULL).

Two yardsticks, neither of them the code under test (both exist at the parent commit):
  1. what a caller had to do before: sdb_lsm_get over the tree for all keys, a synchronise, the columns copied
     back, the tables' key columns probed on the host (numpy searchsorted over host copies, the fastest bisect a
     caller has: one vectorised pass per table) and the shadowed answers overwritten;
  2. sdb_lsm_get_projected alone on the same keys: for zero_tables the same kernel sequence, for tree_only the
     difference is the cost of the table probe.

Per mix one JSON line: the device time of sdb_lsm_get_mem between two events and of yardstick 2, the wall-clock
per call of sdb_lsm_get_mem and of yardstick 1 (host time included, the stream synchronised), medians of R with
min .. max, blocks_checked, and the agreement on every key with yardstick 1 and with the layer each key was drawn
from.  --one-call runs a single call of one mix after the warm-up, for `rocprofv3 --kernel-trace --stats`.
A record, not a gate.
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
NO_TABLE = 0xFFFFFFFF


def build_tables(n_per_table, dev, taken):
    """-> (DeviceRuns in search order, per table the sorted counters).  One version per key, seqs above the tree's."""
    rng = np.random.default_rng(31)
    druns, counters = [], []
    for t in range(TABLES):  # disjoint from the tree and from one another: a key's layer is the one it was drawn from
        c = np.unique(rng.integers(0, 1 << 62, n_per_table, dtype=np.uint64))
        c = c[~np.isin(c, taken)]
        taken = np.concatenate([taken, c])
        druns.append(runtime.DeviceRun.from_host(Run.from_batch(BG.make_batch(c, 2000 - t, 500 + t)), dev))
        counters.append(c)
    return druns, counters


def mixes(info, tabs, nkeys):
    """name -> (keys, the layer each was drawn from: a table index, or NO_TABLE for the tree)."""
    rng = np.random.default_rng(23)
    levels = [[i] for i in range(BG.L0)] + [list(range(BG.L0 + r * BG.PER_RUN, BG.L0 + (r + 1) * BG.PER_RUN))
                                            for r in range(BG.RUNS)]
    in_tables = np.unique(np.concatenate(tabs))

    def from_tree(m):
        out = []
        for j, ssts in enumerate(levels):
            mj = m // len(levels) + (1 if j < m % len(levels) else 0)
            per = [mj // len(ssts) + (1 if x < mj % len(ssts) else 0) for x in range(len(ssts))]
            for i, p in zip(ssts, per):
                c = info[i]["counters"]
                out.append(rng.choice(c[~np.isin(c, in_tables)], p, replace=False))
        return np.concatenate(out)

    parts = TABLES + len(levels)
    m_tab = nkeys // parts
    spread_c = [rng.choice(tabs[t], m_tab, replace=False) for t in range(TABLES)]
    spread_l = [np.full(m_tab, t, np.uint32) for t in range(TABLES)]
    tree_part = from_tree(nkeys - TABLES * m_tab)
    spread = np.concatenate(spread_c + [tree_part])
    layer = np.concatenate(spread_l + [np.full(tree_part.size, NO_TABLE, np.uint32)])
    order = rng.permutation(spread.size)
    tree_keys = from_tree(nkeys)
    out = {"mem_hot": (rng.choice(tabs[0], nkeys, replace=False), np.zeros(nkeys, np.uint32)),
           "mem_spread": (spread[order], layer[order]),
           "tree_only": (tree_keys, np.full(nkeys, NO_TABLE, np.uint32)),
           "zero_tables": (tree_keys, np.full(nkeys, NO_TABLE, np.uint32))}
    return {k: ([BG.key_of(c) for c in v], l) for k, (v, l) in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sst-entries", type=int, default=datasets.D1_N)
    ap.add_argument("--table-entries", type=int, default=datasets.D1_N)
    ap.add_argument("--keys", type=int, default=65536)
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
    druns, tabs = build_tables(a.table_entries, dev, np.unique(np.concatenate([x["counters"] for x in info])))
    mem = runtime.mem_tables_device(druns)
    tab_keys = [np.array([BG.key_of(c) for c in t], dtype="S16") for t in tabs]  # the host copies yardstick 1 probes
    ns = len(views)
    lines = [{"what": "tree and tables", "ssts": ns, "runs": len(runs), "total_blocks": tree["total_blocks"],
              "entries_per_sst": a.sst_entries, "tables": TABLES, "rows_per_table": [int(t.size) for t in tabs],
              "build_s": round(time.perf_counter() - t0, 1)}]
    print(json.dumps(lines[0]), flush=True)
    for name, (keys, layer) in mixes(info, tabs, a.keys).items():
        if a.mix not in ("all", name) or (a.one_call and a.one_call != name):
            continue
        n = len(keys)
        hb, ho = runtime.keys_columnar(keys)
        kb, ko = torch.from_numpy(hb).to(dev), torch.from_numpy(ho.view(np.int64)).to(dev)
        use = None if name == "zero_tables" else mem
        wsb = runtime.lib().sdb_lsm_get_mem_workspace_bytes(TABLES if use else 0, tree["total_blocks"], ns, len(runs), n, 0)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        host_q = np.array(keys, dtype="S16")
        res = {}

        def new_path():
            res["r"] = runtime.lsm_get_mem_device(use, tree, None, (kb, ko, n), stream=s, workspace=ws)

        def projected():
            res["p"] = runtime.lsm_get_projected_device(tree, None, None, (kb, ko, n), stream=s, workspace=ws)

        def new_host():
            new_path()
            s.synchronize()
            r = res["r"]
            return r["state"].cpu().numpy()[:n], r["sst"].cpu().numpy()[:n], r["table"].cpu().numpy()[:n].view(np.uint32)

        def old_host():
            """Yardstick 1: the tree get for all keys, a synchronise, the host probe of the tables, the overwrite."""
            r = runtime.lsm_get_device(tree, None, (kb, ko, n), stream=s, workspace=ws)
            s.synchronize()
            state, sst = r["state"].cpu().numpy()[:n].copy(), r["sst"].cpu().numpy()[:n].copy()
            table = np.full(n, NO_TABLE, np.uint32)
            for t in (range(TABLES - 1, -1, -1) if use else ()):  # the front table overwrites last: it shadows the rest
                at = np.minimum(np.searchsorted(tab_keys[t], host_q), tab_keys[t].size - 1)
                hit = tab_keys[t][at] == host_q
                table[hit] = t
            state[table != NO_TABLE] = _abi.GET_FOUND
            sst[table != NO_TABLE] = -1
            return state, sst, table

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

        with torch.cuda.stream(s):
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
            st_new, sst_new, tab_new = new_host()
            sm = res["r"]["summary"].cpu().numpy()
            t_old = wall(old_host)
            st_old, sst_old, tab_old = old_host()
            line = {"what": "sdb_lsm_get_mem, mix " + name, "keys": n, "tables": TABLES if use else 0,
                    "get_mem_device": d_new, "get_projected_device": d_proj, "get_projected_device_after": d_proj2,
                    "get_mem_wall": t_new, "tree_get_plus_host_probe_wall": t_old,
                    "new_over_old_wall": round(t_new["median_ms"] / t_old["median_ms"], 3),
                    "states": {k: int(v) for k, v in zip(runtime.GET_SUMMARY, sm)},
                    "same_answers": bool(np.array_equal(st_new, st_old) and np.array_equal(sst_new, sst_old) and
                                         np.array_equal(tab_new, tab_old)),
                    "layers_as_drawn": bool(np.array_equal(tab_new, layer))}
            line["states"]["status"] &= 0xFFFFFFFF
            lines.append(line)
            print(json.dumps(line), flush=True)
    if a.out and not a.one_call:
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
