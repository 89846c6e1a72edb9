"""WAL replay on the device (sdb_wal_replay_sort + sdb_wal_replay_emit) at the D1 shape: 578,524 rows of 16-byte
keys and 100-byte values (about 64 MiB), as 16 batches in shuffled key order with ascending seqs.

  python scripts/bench_wal_replay.py [--reps R] [--rows N] [--kernel-stats FILE]

JSON lines on stdout:
  replay      device time of _sort and of _emit (hip events around each call, medians of R with min .. max), the
              HBM bytes the kernels ask for against the bytes a replay must move (both computed from the shape)
  merge       the yardstick, existing code on the same rows: the rows pre-sorted on the host into 32 runs and merged
              by sdb_merge_runs with a retention that keeps everything.  It does strictly less work (its input is
              sorted within runs), so the replay is expected to be slower.
  cpu         numpy.lexsort over the fixed-width keys and seqs, for scale only (host wall-clock)
Per-kernel times are not visible from the host: run the script once more under `rocprofv3 --kernel-trace --stats`
and pass the kernel statistics CSV as --kernel-stats for the `kernels` line (profile runs slow the host: take the
other lines from a run without the profiler).  A record, not a gate.
"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NBATCHES, NRUNS = 16, 32


def kernel_stats_line(path):
    rows = list(csv.DictReader(open(path)))
    name = next(k for k in rows[0] if k.lower() == "name")
    total = next(k for k in rows[0] if k.lower().startswith("totalduration"))
    calls = next(k for k in rows[0] if k.lower() == "calls")
    out = {}
    for r in rows:
        m = re.search(r"::(k_(?:rp|mg)_\w+)", r[name])
        if m:
            out[m.group(1)] = {"calls": int(r[calls]), "us_per_call": round(int(r[total]) / int(r[calls]) / 1e3, 1),
                               "total_ms": round(int(r[total]) / 1e6, 3)}
    return {"what": "kernel statistics of the profiled run (rocprofv3 --kernel-trace --stats); k_rp_merge runs once "
                    "per merge pass, the other k_rp_* once per call", "kernels": out}


def shuffled_rows(n, seed=5):
    """-> host Run of the D1 rows in shuffled key order, seq = arrival index + 1."""
    from slatedb_amd import datasets
    from slatedb_amd.batch import Run
    b = datasets.d1(n=n)
    order = np.random.default_rng(seed).permutation(n)
    keys = b.key_bytes.reshape(n, 16)[order]
    vlen = int(b.val_off[1])
    vals = b.val_bytes.reshape(n, vlen)[order]
    z = np.zeros(n, np.int64)
    return Run(keys.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(16), vals.reshape(-1),
               np.arange(n, dtype=np.uint64) * np.uint64(vlen), np.full(n, vlen, np.uint32),
               np.arange(1, n + 1, dtype=np.uint64), np.zeros(n, np.uint8), z, z), vlen


def key_order(run, lo, hi):
    """argsort of rows [lo, hi) by (key asc, seq desc) over fixed 16-byte keys."""
    k = run.key_arena.reshape(-1, 16)[lo:hi]
    w = k.view(">u8").astype(np.uint64)
    return np.lexsort((np.uint64(0xFFFFFFFFFFFFFFFF) - run.seq[lo:hi], w[:, 1], w[:, 0]))


def presorted_runs(run, vlen):
    from slatedb_amd.batch import Run
    n, out = run.n, []
    for r in range(NRUNS):
        lo, hi = n * r // NRUNS, n * (r + 1) // NRUNS
        o = key_order(run, lo, hi) + lo
        m = hi - lo
        z = np.zeros(m, np.int64)
        out.append(Run(run.key_arena.reshape(-1, 16)[o].reshape(-1), np.arange(m + 1, dtype=np.uint64) * np.uint64(16),
                       run.val_base.reshape(-1, vlen)[o].reshape(-1), np.arange(m, dtype=np.uint64) * np.uint64(vlen),
                       np.full(m, vlen, np.uint32), run.seq[o], np.zeros(m, np.uint8), z, z))
    return out


def traffic(n, klen, vlen, tile):
    """HBM bytes per replay from the shape: what the kernels ask for (gathers counted at their element size; the
    hardware fetches whole sectors for them) and what any replay must move (read every row once, write it once)."""
    passes, run = 0, tile
    while run < n:
        passes, run = passes + 1, run * 2
    meta_in = 8 + 8 + 4 + 8 + 1                      # key_off, val_off, val_len, seq, flags
    meta_out = 8 + 8 + 1 + 8 + 8 + 8 + 1             # key_off, val_off, kind, seq, create_ts, expire_ts, ts_mask
    sort = {"k_rp_facts": 8 + 8 + 1 + klen + 4 + 1, "k_rp_tile_sort": 8 + klen + 8 + 1 + 8 + 4,
            "k_rp_merge": passes * (4 + 8 + 8 + 4), "k_rp_mark": 2 * (4 + 8 + 8), "k_rp_count": 4 + 1 + 1 + 8 + 4}
    emit = {"k_rp_tcount": 4 + 1 + 4 + 4, "k_rp_tscatter": 4 + 1 + 4 + 4 + 4, "k_rp_sizes": 4 + 8 + 1 + 4,
            "k_rp_gather": 4 + meta_in + klen + vlen + meta_out + klen + vlen}
    return {"merge_passes": passes, "sort_bytes": n * sum(sort.values()), "emit_bytes": n * sum(emit.values()),
            "must_move_bytes": n * (meta_in + meta_out + 2 * (klen + vlen)),
            "per_row": {**sort, **emit}}


def med(xs):
    return {"median_ms": round(float(np.median(xs)), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", type=int, default=578524)
    ap.add_argument("--kernel-stats")
    args = ap.parse_args()
    if args.kernel_stats:
        print(json.dumps(kernel_stats_line(args.kernel_stats)))
        return
    import torch
    from slatedb_amd import _abi, replay, runtime as rt
    rt.require_device()
    lib = rt.lib()
    n = args.rows
    run, vlen = shuffled_rows(n)
    start = [n * b // NBATCHES for b in range(NBATCHES + 1)]

    # ---- the replay ----
    drun = rt.DeviceRun.from_host(run)
    w = rt.WalReplay(drun, start)
    facts, sm = w.sort(None)
    assert sm.status == 0 and sm.rows_out == n, (sm.status, sm.rows_out)
    cuts = replay.split_tables(facts, rt.params(), 1 << 62)
    o, esm = w.emit(cuts)
    assert esm.status == 0
    koff = o["key_off"][:n + 1].cpu().numpy()
    keys = o["key_bytes"][:16 * n].cpu().numpy().reshape(n, 16)
    want = run.key_arena.reshape(n, 16)[key_order(run, 0, n)]
    assert np.array_equal(keys, want) and int(koff[-1]) == 16 * n, "the replay's order differs from numpy's"
    tbs = torch.tensor(cuts, dtype=torch.int64, device="cuda")
    out = _abi.WalTablesOut(o["key_bytes"].data_ptr(), drun.key_bytes, o["key_off"].data_ptr(), o["val_bytes"].data_ptr(),
                            drun.val_bytes, o["val_off"].data_ptr(), o["kind"].data_ptr(), o["seq"].data_ptr(),
                            o["create_ts"].data_ptr(), o["expire_ts"].data_ptr(), o["ts_mask"].data_ptr(), n,
                            o["table_row_start"].data_ptr(), o["summary"].data_ptr())
    ev = lambda: torch.cuda.Event(enable_timing=True)
    ts, te = [], []
    for rep in range(args.reps + 3):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        st = lib.sdb_wal_replay_sort(C.byref(w.run), w.bs.data_ptr(), w.nb, 0, 0, w.facts_t.data_ptr(), w.summary_t.data_ptr(),
                                     w.ws.data_ptr(), w.ws.numel(), None)
        e1.record()
        st |= lib.sdb_wal_replay_emit(C.byref(w.run), w.bs.data_ptr(), w.nb, tbs.data_ptr(), len(cuts) - 1, C.byref(out),
                                      w.ws.data_ptr(), w.ws.numel(), None)
        e2.record()
        torch.cuda.synchronize()
        assert st == 0
        if rep >= 3:
            ts.append(e0.elapsed_time(e1))
            te.append(e1.elapsed_time(e2))
    tr = traffic(n, 16, vlen, lib.sdb_diag_replay_tile())
    print(json.dumps({"job": "replay", "rows": n, "batches": NBATCHES, "bytes": int(n * (16 + vlen)), "reps": args.reps,
                      "sort": med(ts), "emit": med(te), "total": med([a + b for a, b in zip(ts, te)]), "traffic": tr}))

    # ---- the yardstick: sdb_merge_runs over the same rows, pre-sorted into 32 runs ----
    druns = [rt.DeviceRun.from_host(r) for r in presorted_runs(run, vlen)]
    ret = _abi.Retention()
    mo, msm = rt.merge_runs_device(druns, ret)
    assert msm.status == 0 and msm.num_out == n
    assert np.array_equal(mo["key_bytes"][:16 * n].cpu().numpy().reshape(n, 16), want)
    cr = (_abi.Run * NRUNS)(*[r.to_ctypes() for r in druns])
    mout = _abi.MergedOut(mo["key_bytes"].data_ptr(), 16 * n, mo["key_off"].data_ptr(), mo["val_bytes"].data_ptr(), vlen * n,
                          mo["val_off"].data_ptr(), mo["kind"].data_ptr(), mo["seq"].data_ptr(), mo["create_ts"].data_ptr(),
                          mo["expire_ts"].data_ptr(), mo["ts_mask"].data_ptr(), n, mo["summary"].data_ptr())
    ws = mo["_ws"]
    tm = []
    for rep in range(args.reps + 3):
        e0, e1 = ev(), ev()
        e0.record()
        st = lib.sdb_merge_runs(cr, NRUNS, C.byref(ret), C.byref(mout), ws.data_ptr(), ws.numel(), None)
        e1.record()
        torch.cuda.synchronize()
        assert st == 0
        if rep >= 3:
            tm.append(e0.elapsed_time(e1))
    print(json.dumps({"job": "merge", "what": "sdb_merge_runs, 32 host-sorted runs of the same rows, retention keeps all",
                      "rows": n, "runs": NRUNS, "reps": args.reps, "total": med(tm)}))

    # ---- numpy, for scale ----
    tc = []
    for _ in range(3):
        t0 = time.perf_counter()
        key_order(run, 0, n)
        tc.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"job": "cpu", "what": "numpy.lexsort over two big-endian u64 key words and the seq (one host "
                                            "thread; the order only, no row is moved)", "rows": n, "sort": med(tc)}))


if __name__ == "__main__":
    main()
