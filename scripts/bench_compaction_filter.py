"""What a compaction filter and a resume cursor cost on the device compactor (sdb_compactor_run_filtered), over the
inputs of scripts/bench_compact_merge.py: 4 runs of 578,524 entries, 16-byte keys, 100-byte values, 4 KiB blocks, 10
filter bits per key, max_sst_size 256 MiB, operands passed on unmerged (retention_min_seq Some(0)).

  python scripts/bench_compaction_filter.py [--reps R] [--run-entries N]

One JSON line per job: wall-clock of the whole job (the call returns after its last synchronisation), medians of R with
min .. max, the time spent inside the Python callback, and filter_stats().  The jobs:
  the unfiltered job (sdb_compactor_run);
  keep-all with want_values 0 and with want_values 1 (F7: what the gather alone costs);
  a numpy batch filter that tombstones a tenth of the keys by a range of 10-byte key prefixes;
  one that rewrites every tenth row's value (the replacements handed over as one packed arena);
  a job resumed at the stream's midpoint, without a filter.
A record, not a gate."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_compact_merge import make_runs, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--run-entries", type=int, default=578524)
    a = ap.parse_args()
    import torch
    from slatedb_amd import _abi, runtime
    from slatedb_amd import compaction_filter as CF
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
    ret = _abi.Retention(0, 0, 0, 1, 0, 0, 1, 0)

    class Timed(CF.BatchFilter):
        def __init__(self, fn, want_values=False):
            self.fn, self.want_values, self.s = fn, want_values, 0.0

        def filter_batch(self, rows):
            t = time.perf_counter()
            r = self.fn(rows)
            self.s += time.perf_counter() - t
            return r

    # keys are 4 zero bytes, a big-endian counter (2^40 + 977 k for key k), 4 zero bytes: the tenth of the keys with the
    # lowest counters is a range of 10-byte key prefixes
    tenth = (nkeys * 977 // 10) >> 16

    def tombstone_prefix(rows):
        at = rows.key_off[:-1].astype(np.int64)
        p10 = (rows.key_bytes[at + 8].astype(np.uint32) << 8) | rows.key_bytes[at + 9]
        return np.where(p10 < tenth, CF.TOMBSTONE, CF.KEEP).astype(np.uint8)

    def rewrite_tenth(rows):
        hit = np.nonzero(rows.seq % np.uint64(10) == 0)[0]
        dec = np.zeros(rows.n, np.uint8)
        dec[hit] = CF.VALUE
        return dec, (np.full(100 * hit.size, 114, np.uint8), np.arange(hit.size + 1, dtype=np.uint64) * np.uint64(100))

    def job(what, call, flt=None):
        walls, inside = [], []
        for i in range(a.reps + 1):
            f = flt() if flt else None
            torch.cuda.synchronize()
            t = time.perf_counter()
            st, ns = call(f)
            torch.cuda.synchronize()
            assert st == 0, st
            if i:
                walls.append((time.perf_counter() - t) * 1e3)
                inside.append(f.s * 1e3 if f else 0.0)
        fs = comp.filter_stats()
        line = {"what": what, "ms_wall": spread(walls), "output_ssts": ns,
                "GiB_per_s_logical": round(logical / (np.median(walls) * 1e-3) / 2**30, 2)}
        if flt:
            line["ms_inside_callback"] = spread(inside)
        line["filter_stats"] = {f: int(getattr(fs, f)) for f, _ in _abi.FilterStats._fields_}
        print(json.dumps(line), flush=True)

    filtered = lambda f, cur=None: comp.run_filtered(druns, ret, prm, max_sst, f, cur)  # noqa: E731
    job("sdb_compactor_run (unfiltered)", lambda f: comp.run(druns, ret, prm, max_sst))
    job("run_filtered, no filter and no cursor (F6)", lambda f: filtered(None))
    job("keep-all, want_values 0", filtered, lambda: Timed(lambda rows: None, False))
    job("keep-all, want_values 1", filtered, lambda: Timed(lambda rows: None, True))
    job("numpy filter: tombstone the keys of a prefix range", filtered, lambda: Timed(tombstone_prefix))
    job("numpy filter: rewrite every tenth value", filtered, lambda: Timed(rewrite_tenth))
    # the cursor: the middle row of the full stream
    st, ns = comp.run(druns, ret, prm, max_sst)
    torch.cuda.synchronize()
    full, _ = comp.merged()
    mid = full.n // 2
    cur = (full.key(mid), int(full.seq[mid]))
    del full
    job("resumed at the stream's midpoint, no filter", lambda f: filtered(None, cur))
    comp.close()


if __name__ == "__main__":
    main()
