"""Range-scan measurements (sdb_sst_scan) on one oracle-encoded D1 SST (datasets.d1 at its default size,
the SST shape scripts/bench_configs.py decodes), device-resident, timed per call with HIP events.

  python scripts/bench_scan.py [--reps R]

  (a) whole-SST scan: one range, both bounds unbounded, against sdb_decode_blocks of the same SST in the
      same process.  Both read the same blocks and write the same columns.
  (b) many short ranges: 4096 ranges of ~100 entries, against what a caller could do before:
      sdb_sst_lookup for the start keys, then one sdb_decode_blocks_at over every range's covering blocks.
      The host round trip between those two calls (the block list is built from the lookup's answer) and
      the CPU clip of each range's first and last block are NOT in the old path's time.
Each line: the median of R timings and their spread (min .. max).  A record, not a gate.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle as O  # noqa: E402
from slatedb_amd import _abi, datasets, runtime  # noqa: E402


def timings(fn, reps, stream):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
            "spread_ms": round(ms[-1] - ms[0], 4), "reps": reps}


def dev_t(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)


class Columns:
    def __init__(self, n, kbytes, dev):
        o = lambda m, dt: torch.empty(max(m, 1), dtype=dt, device=dev)  # noqa: E731
        self.ka, self.ko = o(kbytes + 16, torch.uint8), o(n + 1, torch.int64)
        self.vo, self.vl, self.sq = o(n, torch.int64), o(n, torch.int32), o(n, torch.int64)
        self.fl, self.ct, self.et = o(n, torch.uint8), o(n, torch.int64), o(n, torch.int64)
        self.n, self.kbytes = n, kbytes

    def ptrs(self):
        return [t.data_ptr() for t in (self.vo, self.vl, self.sq, self.fl, self.ct, self.et)]


def scan_call(lib, view, ranges, dev, stream, n_entries, kbytes):
    """A prepared sdb_sst_scan call (everything allocated up front) -> (run(), outputs)."""
    cols = {k: dev_t(v, dev) for k, v in runtime.scan_ranges_columnar(ranges).items()}
    n = len(ranges)
    rg = _abi.ScanRanges(n, cols["start_bytes"].data_ptr(), cols["start_off"].data_ptr(), cols["start_kind"].data_ptr(),
                         cols["end_bytes"].data_ptr(), cols["end_off"].data_ptr(), cols["end_kind"].data_ptr())
    c = Columns(n_entries, kbytes, dev)
    res, rb = torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.zeros(2 * n, dtype=torch.int32, device=dev)
    rs, sm = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(5, dtype=torch.int64, device=dev)
    out = _abi.ScanOut(res.data_ptr(), rb.data_ptr(), rs.data_ptr(), c.ka.data_ptr(), kbytes, c.ko.data_ptr(), *c.ptrs(),
                       n_entries, sm.data_ptr())
    wsb = lib.sdb_sst_scan_workspace_bytes(view.num_blocks, n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def run():
        st = lib.sdb_sst_scan(C.byref(view), C.byref(rg), 0, C.byref(out), ws.data_ptr(), wsb, stream.cuda_stream)
        assert st == 0, st

    return run, {"cols": c, "res": res, "rb": rb, "rs": rs, "sm": sm, "_keep": (cols, ws, rg, out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    reps = max(5, a.reps)
    runtime.require_device()
    lib = runtime.lib()
    dev = torch.device("cuda", 0)
    s = torch.cuda.Stream(device=dev)
    h = datasets.d1()
    enc = O.encode_sst(h, O.params(block_size=4096, sst_version=2, bloom_bits_per_key=0))
    assert enc.status == 0
    ik, iko = O.sst_index_keys(h, enc)
    nb = len(enc.block_off) - 1
    kbytes = int(h.key_off[h.n] - h.key_off[0])
    data = dev_t(np.concatenate([enc.data, np.zeros(64, np.uint8)]), dev)
    boff, dik, diko = dev_t(enc.block_off, dev), dev_t(ik if ik.size else np.zeros(16, np.uint8), dev), dev_t(iko, dev)
    view = _abi.SstView(data.data_ptr(), boff.data_ptr(), nb, dik.data_ptr(), diko.data_ptr(), None, 0, 0, 2, 0)
    shape = {"entries": int(h.n), "blocks": nb, "encoded_bytes": int(enc.data.size), "key_bytes": kbytes}

    # ---- (a) whole-SST scan against sdb_decode_blocks -------------------------------------------------
    dc = Columns(h.n, kbytes, dev)
    bes, bad = torch.empty(nb + 1, dtype=torch.int64, device=dev), torch.empty(nb + 1, dtype=torch.int32, device=dev)
    dsm = torch.zeros(64, dtype=torch.uint8, device=dev)
    dout = _abi.DecodedOut(bes.data_ptr(), dc.ka.data_ptr(), kbytes + 16, dc.ko.data_ptr(), *dc.ptrs(), h.n, bad.data_ptr(),
                           nb + 1, dsm.data_ptr())
    dwsb = lib.sdb_decode_workspace_bytes(nb)
    dws = torch.empty(dwsb, dtype=torch.uint8, device=dev)

    def run_decode():
        st = lib.sdb_decode_blocks(data.data_ptr(), boff.data_ptr(), nb, 2, C.byref(dout), dws.data_ptr(), dwsb, s.cuda_stream)
        assert st == 0, st

    run_scan, so = scan_call(lib, view, [(None, 0, None, 0)], dev, s, h.n, kbytes)
    with torch.cuda.stream(s):
        t_dec = timings(run_decode, reps, s)
        t_scan = timings(run_scan, reps, s)
    sm = so["sm"].cpu().numpy()
    same = (int(sm[0]), int(sm[1]), int(sm[4]) & 0xFFFFFFFF) == (h.n, kbytes, 0)
    for x, y in ((so["cols"].ka[:kbytes], dc.ka[:kbytes]), (so["cols"].ko[:h.n + 1], dc.ko[:h.n + 1]),
                 (so["cols"].vo[:h.n], dc.vo[:h.n]), (so["cols"].sq[:h.n], dc.sq[:h.n]), (so["cols"].fl[:h.n], dc.fl[:h.n])):
        same = same and bool(torch.equal(x, y))
    print(json.dumps({"what": "(a) whole-SST scan (one unbounded range) vs sdb_decode_blocks, one D1 SST", **shape,
                      "scan": t_scan, "decode": t_dec, "scan_over_decode": round(t_scan["median_ms"] / t_dec["median_ms"], 3),
                      "same_columns": same}), flush=True)

    # ---- (b) 4096 short ranges against lookup + decode_blocks_at -----------------------------------------
    rng = np.random.default_rng(11)
    nr, span = 4096, 100
    first = np.sort(rng.integers(0, h.n - span, nr))
    ranges = [(h.key(int(i)), _abi.BOUND_INCLUDED, h.key(int(i) + span - 1), _abi.BOUND_INCLUDED) for i in first]
    run0, s0 = scan_call(lib, view, ranges, dev, s, 0, 0)  # sizing call
    with torch.cuda.stream(s):
        run0()
    torch.cuda.synchronize()
    need = s0["sm"].cpu().numpy()
    run_b, sb = scan_call(lib, view, ranges, dev, s, int(need[0]), int(need[1]))
    rblk = s0["rb"].cpu().numpy().reshape(-1, 2).astype(np.int64)
    blist = np.concatenate([np.arange(x, y) for x, y in rblk])  # every range's covering blocks, in range order
    bo = enc.block_off.astype(np.int64)
    bstart, bend = dev_t(bo[blist], dev), dev_t(bo[blist + 1], dev)
    nbl = int(blist.size)
    per_block = np.diff(np.asarray(enc.block_first_entry[:nb + 1]).astype(np.int64))
    cap_e = int(per_block[blist].sum())
    oc = Columns(cap_e, cap_e * 16 + 4096, dev)
    obes, obad = torch.empty(nbl + 1, dtype=torch.int64, device=dev), torch.empty(nbl + 1, dtype=torch.int32, device=dev)
    osm = torch.zeros(64, dtype=torch.uint8, device=dev)
    oout = _abi.DecodedOut(obes.data_ptr(), oc.ka.data_ptr(), oc.kbytes, oc.ko.data_ptr(), *oc.ptrs(), cap_e, obad.data_ptr(),
                           nbl + 1, osm.data_ptr())
    owsb = lib.sdb_decode_workspace_bytes(nbl)
    ows = torch.empty(owsb, dtype=torch.uint8, device=dev)
    skeys = b"".join(r[0] for r in ranges)
    skoff = np.zeros(nr + 1, np.uint64)
    skoff[1:] = np.cumsum([len(r[0]) for r in ranges])
    dk, dko = dev_t(np.frombuffer(skeys, np.uint8).copy(), dev), dev_t(skoff, dev)
    vt = {"data": data, "block_off": boff, "num_blocks": nb, "index_keys": dik, "index_key_off": diko, "sst_version": 2}

    def run_old():
        runtime.sst_lookup_device(vt, dk, dko, nr, stream=s)
        st = lib.sdb_decode_blocks_at(data.data_ptr(), bstart.data_ptr(), bend.data_ptr(), nbl, 2, C.byref(oout),
                                      ows.data_ptr(), owsb, s.cuda_stream)
        assert st == 0, st

    with torch.cuda.stream(s):
        t_old = timings(run_old, reps, s)
        t_new = timings(run_b, reps, s)
    smb = sb["sm"].cpu().numpy()
    print(json.dumps({"what": "(b) %d ranges of %d entries: sdb_sst_scan vs sdb_sst_lookup + sdb_decode_blocks_at" % (nr, span),
                      "scan": t_new, "lookup_plus_decode_at": t_old,
                      "scan_over_old": round(t_new["median_ms"] / t_old["median_ms"], 3),
                      "scan_entries": int(smb[0]), "scan_status": int(smb[4]) & 0xFFFFFFFF, "blocks_read": int(smb[3]),
                      "old_blocks_decoded": nbl, "old_entries_decoded": cap_e,
                      "not_in_old_path": "host round trip for the block list, CPU clip"}), flush=True)


if __name__ == "__main__":
    main()
