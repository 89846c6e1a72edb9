"""The ranged compaction (sdb_compactor_run_ssts_ranged) next to sdb_compactor_run_ssts on the compaction job of
scripts/bench_configs.py: 4 L0 SSTs of the configs[1] shape (578,524 x 16-byte key / 100-byte value each, key ranges
interleaved, 4 KiB blocks, 10 filter bits per key), encoded on the device and resident.

  python scripts/bench_ranged_compaction.py [--reps R] [--sst-entries N] [--out FILE]

The job runs whole through sdb_compactor_run_ssts, then as 1, 2, 4 and 8 key ranges through the ranged call, each
range a job of its own on one handle.  The ranges are the planner's (slatedb_amd/subcompaction.py select_boundaries
over the inputs' anchors) with the floor of one input SST lifted, so that 8 ranges exist for 4 inputs.  Per job: the
time on the stream between two events around the call and its wall-clock (the call synchronises inside), median of R
with min .. max; per range count these are summed over the ranges.  Beside them blocks_checked / blocks_total summed
over the ranges (with N ranks and whole-input decodes this would be N), the host synchronisations per job (the header's
count: run_ssts 2, ranged 4) and whether the ranges' merged streams concatenate to the whole job's.

One JSON line per job kind, appended to --out when given.  A record, not a gate."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
from slatedb_amd import _abi, datasets, runtime  # noqa: E402
from slatedb_amd import subcompaction as S  # noqa: E402

SYNCS = {"sdb_compactor_run_ssts": 2, "sdb_compactor_run_ssts_ranged": 4}  # include/slatedb_amd.h, R8


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sst-entries", type=int, default=datasets.D1_N)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    runtime.require_device()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    prm = runtime.params(block_size=4096, sst_version=2, bloom_bits_per_key=10)
    ret = _abi.Retention(0, 0, 0, 1, 0, 0, 0, 0)  # retention_min_seq Some(0), as bench_configs.py --compact
    max_sst = 256 << 20
    to_dev = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)  # noqa: E731
    inputs, metas = [], []
    for j in range(4):
        h = datasets.d1(n=a.sst_entries, sst_index=j)
        out = runtime.DeviceSstOutput(h.n, h.logical_bytes(), h.logical_bytes(), prm, device=dev)
        runtime.encode_sst_device(h.to_device(dev), out)
        torch.cuda.synchronize()
        enc = types.SimpleNamespace(**out.to_host())
        sm, nb = enc.summary, int(enc.summary.num_blocks)
        ikb, iko = O.sst_index_keys(h, enc)
        inputs.append(types.SimpleNamespace(data=out.data, block_off=out.block_off[:nb + 1], num_entries=int(sm.num_entries),
                                            key_bytes=int(sm.raw_key_size), val_bytes=int(sm.raw_val_size),
                                            index_keys=to_dev(np.concatenate([ikb, np.zeros(1, np.uint8)])),
                                            index_key_off=to_dev(iko), keep=out))
        metas.append(S.SstMeta.from_encoded(h, enc))
    anchors = [x for m in metas for x in S.sample_anchors(m.first_keys, m.offsets, m.data_len)]
    comp = runtime.Compactor()
    lines = []

    def timed(call):
        """One job on s: (stream ms between two events, wall ms, its result)."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(s)
        r = call()
        e1.record(s)
        s.synchronize()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3, r

    def merged_keys():
        m, sm = comp.merged()
        return sm.num_out, m.key_bytes.tobytes(), m.seq.tobytes()

    with torch.cuda.stream(s):
        whole = lambda: comp.run_ssts(inputs, ret, prm, max_sst, stream=s)  # noqa: E731
        for _ in range(2):
            whole()
        ev, wall = [], []
        for _ in range(a.reps):
            d, w, (st, ns) = timed(whole)
            assert st == 0
            ev.append(d)
            wall.append(w)
        n_whole, keys_whole, seq_whole = merged_keys()
        lines.append({"what": "sdb_compactor_run_ssts, the whole job (the yardstick)", "inputs": 4, "entries_per_sst": a.sst_entries,
                      "host_syncs_per_job": SYNCS["sdb_compactor_run_ssts"], "stream": stats(ev), "wall": stats(wall),
                      "output_ssts": ns, "entries_out": int(n_whole)})
        base = lines[0]["stream"]["median_ms"]
        for k in (1, 2, 4, 8):
            ranges = S.select_boundaries(anchors, k, 0)
            # the range arrays uploaded once, as a compactor that plans ahead would hold them
            dr = [{f: to_dev(x) for f, x in runtime.scan_ranges_columnar([S.range_bounds(r)]).items()} for r in ranges]
            jobs = [(lambda d=d: comp.run_ssts_ranged(inputs, ret, prm, max_sst, job_range=d, stream=s)) for d in dr]
            for j in jobs:
                j()
            ev, wall, frac = [], [], None
            for rep in range(a.reps):
                de, wa, checked, total, rows, keys, seqs = 0.0, 0.0, 0, 0, 0, b"", b""
                for j in jobs:
                    d, w, (st, ns) = timed(j)
                    assert st == 0, st
                    de += d
                    wa += w
                    rs = comp.range_stats()
                    checked += rs.blocks_checked
                    total = rs.blocks_total
                    if rep == 0:
                        n, kb, sq = merged_keys()
                        rows, keys, seqs = rows + n, keys + kb, seqs + sq
                ev.append(de)
                wall.append(wa)
                if rep == 0:
                    frac = (checked, total, rows == n_whole and keys == keys_whole and seqs == seq_whole)
            st_ = stats(ev)
            lines.append({"what": "sdb_compactor_run_ssts_ranged, the job as %d planner range(s), summed over the ranges" % len(ranges),
                          "ranges": len(ranges), "host_syncs_per_job": SYNCS["sdb_compactor_run_ssts_ranged"], "stream": st_,
                          "wall": stats(wall), "blocks_checked": frac[0], "blocks_total": frac[1],
                          "blocks_checked_over_total": round(frac[0] / frac[1], 4), "ranges_concatenate_to_whole": bool(frac[2]),
                          "stream_minus_whole_ms": round(st_["median_ms"] - base, 4)})
    comp.close()
    for line in lines:
        print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
