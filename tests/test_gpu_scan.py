"""GPU parity of the batched range scans (sdb_sst_scan, slatedb_amd/csrc/sdb_scan.hip) against the
expectations of tests/scan_cases.py: block ranges, entry ranges, statuses and every column of every range,
ascending and descending, V1 and V2, small and large blocks; corruption, capacity, an oversize row,
degenerate inputs and HIP graph capture."""
import numpy as np
import pytest

from slatedb_amd import _abi, datasets
from slatedb_amd.batch import Batch

from .scan_cases import EXC, INC, U, Sst, empty_as_set, range_list
from .test_descending import irregular_v2
from .test_lookup_oracle import dup_batch

pytestmark = pytest.mark.gpu

COLS = ("val_off", "val_len", "seq", "flags")


@pytest.fixture(scope="module")
def rt():
    from slatedb_amd import runtime
    runtime.require_device()
    return runtime


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if not a.size:
        a = np.zeros(16, a.dtype)
    return torch.from_numpy(a).cuda()


def view_of(sst, data=None):
    return {"data": _dev(np.concatenate([sst.data if data is None else data, np.zeros(64, np.uint8)])),
            "block_off": _dev(sst.block_off), "num_blocks": sst.nb, "index_keys": _dev(sst.ik_bytes),
            "index_key_off": _dev(sst.ik_off), "sst_version": sst.version}


def host(res):
    import torch
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in res.items() if not k.startswith("_")}
    sm = h["summary"]
    h["num_entries"], h["key_bytes"], h["num_failed"], h["blocks_read"] = (int(x) for x in sm[:4])
    h["status"] = int(sm[4]) & 0xFFFFFFFF
    return h


def check(sst, ranges, h, desc, failing=None):
    """Every range of `ranges` in full against the expectation; `failing`: {range: status}."""
    n, failing = len(ranges), failing or {}
    exp = [sst.expect_idx(r, desc) for r in ranges]
    want_blocks = np.array([b for (b, _) in exp], np.int64).reshape(-1)
    assert np.array_equal(h["range_block"][:2 * n].astype(np.int64), want_blocks)
    want_status = np.array([failing.get(r, 0) for r in range(n)], np.int64)
    assert np.array_equal(h["range_status"][:n].astype(np.int64), want_status)
    lens = [0 if r in failing else len(i) for r, (_, i) in enumerate(exp)]
    res = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert np.array_equal(h["range_entry_start"][:n + 1], res)
    N = int(res[-1])
    idx = np.concatenate([i for r, (_, i) in enumerate(exp) if r not in failing] + [np.zeros(0, np.int64)])
    d = sst.dec
    assert h["num_entries"] == N
    for f in COLS:
        assert np.array_equal(h[f][:N].astype(np.int64), np.asarray(getattr(d, f)).astype(np.int64)[idx]), f
    fl = np.asarray(d.flags).astype(np.int64)[idx]
    for f, bit in (("create_ts", _abi.FLAG_HAS_CREATE_TS), ("expire_ts", _abi.FLAG_HAS_EXPIRE_TS)):
        m = (fl & bit) != 0
        assert np.array_equal(h[f][:N][m], np.asarray(getattr(d, f)).astype(np.int64)[idx][m]), f
    ko = h["key_off"][:N + 1].astype(np.int64)
    klen = np.diff(np.asarray(d.key_off).astype(np.int64))[idx]
    assert ko[0] == 0 and np.array_equal(np.diff(ko), klen)
    assert h["key_bytes"] == int(klen.sum()) == int(ko[-1])
    ka, kol = h["key_arena"].tobytes(), ko.tolist()
    got_keys = [ka[kol[i]:kol[i + 1]] for i in range(N)]
    assert got_keys == [sst.keys[i] for i in idx.tolist()]
    first_bad = min(failing) if failing else None
    assert h["status"] == (failing[first_bad] if failing else 0)
    assert h["num_failed"] == len(failing)


_cases = {}


def case(name, version, bs):
    """The SST, its device view and its range list, built once per (dataset, version, block size)."""
    key = (name, version, bs)
    if key not in _cases:
        b = dup_batch() if name == "dup" else datasets.d3(n=3000)
        sst = Sst(b, version, bs)
        _cases[key] = (sst, view_of(sst), range_list(sst, seed=bs + version))
    return _cases[key]


@pytest.mark.parametrize("name", ["dup", "d3"])
@pytest.mark.parametrize("version,bs", [(2, 256), (2, 4096), (1, 512), (2, 16384)])
@pytest.mark.parametrize("desc", [False, True])
def test_scan_ranges(rt, name, version, bs, desc):
    sst, view, ranges = case(name, version, bs)
    if name == "dup" and bs <= 512:
        assert sst.straddling_key() is not None
    h = host(rt.sst_scan_device(view, ranges, descending=desc))
    check(sst, ranges, h, desc)
    marked = np.zeros(sst.nb, bool)
    for r in ranges:
        (s, e), idx = sst.expect_idx(r)
        s_, sk, e_, ek = r
        if not empty_as_set(s_ or b"", sk, e_ or b"", ek):
            marked[s:e] = True
    assert h["blocks_read"] == int(marked.sum())


@pytest.mark.parametrize("desc", [False, True])
def test_scan_corrupt_block(rt, desc):
    sst, _, ranges = case("d3", 2, 512)
    bad = sst.nb // 3
    data = sst.data.copy()
    data[int(sst.block_off[bad]) + 9] ^= 0x20
    h = host(rt.sst_scan_device(view_of(sst, data), ranges, descending=desc))
    failing = {}
    for r, rg in enumerate(ranges):
        (s, e), idx = sst.expect_idx(rg)
        if s <= bad < e and not empty_as_set(rg[0] or b"", rg[1], rg[2] or b"", rg[3]):
            failing[r] = _abi.SDB_CHECKSUM_MISMATCH
    assert 5 < len(failing) < len(ranges) - 5
    check(sst, ranges, h, desc, failing)


def test_scan_irregular_restarts(rt):
    b = datasets.d3(n=2000)
    data, off, k = irregular_v2(b)
    sst = Sst(b, 2, 512, restart_interval=2)
    assert np.array_equal(off, sst.block_off)
    ranges = [(None, U, None, U), (sst.keys[sst.bes[k]], INC, sst.keys[sst.bes[k + 1] - 1], INC),
              (sst.keys[sst.bes[k + 2]], INC, None, U), (None, U, sst.keys[0], INC)]
    view = view_of(sst, data)
    check(sst, ranges, host(rt.sst_scan_device(view, ranges)), False)
    failing = {r: _abi.SDB_CORRUPT_BLOCK for r, rg in enumerate(ranges)
               if sst.expect_idx(rg)[0][0] <= k < sst.expect_idx(rg)[0][1]}
    assert set(failing) == {0, 1}
    check(sst, ranges, host(rt.sst_scan_device(view, ranges, descending=True)), True, failing)


@pytest.mark.parametrize("desc", [False, True])
def test_scan_capacity(rt, desc):
    import torch
    sst, view, ranges = case("dup", 2, 256)
    ranges = ranges[:40]
    full = host(rt.sst_scan_device(view, ranges, descending=desc))
    N, KB = full["num_entries"], full["key_bytes"]
    assert N > 1000
    for ce, kc in ((N - 1, KB), (N, KB - 1)):
        res = rt.sst_scan_device(view, ranges, descending=desc, cap_entries=ce, key_cap=kc)
        h = host(res)
        assert h["status"] == _abi.SDB_LIMIT_EXCEEDED
        assert (h["num_entries"], h["key_bytes"]) == (N, KB)
        for f in COLS + ("create_ts", "expire_ts", "key_off", "key_arena"):
            assert not h[f].any(), f  # the zero-filled columns are untouched
        for f in ("range_entry_start", "range_block", "range_status"):
            assert np.array_equal(h[f], full[f]), f
    again = host(rt.sst_scan_device(view, ranges, descending=desc, cap_entries=N, key_cap=KB))
    check(sst, ranges, again, desc)
    torch.cuda.synchronize()


def test_scan_capacity_canaries(rt):
    """The same with 0xA5-filled columns handed to the C ABI directly: not one byte changes."""
    import ctypes as C
    import torch
    sst, view, ranges = case("dup", 2, 256)
    ranges = ranges[:40]
    full = host(rt.sst_scan_device(view, ranges))
    N, KB = full["num_entries"], full["key_bytes"]
    cols = rt.scan_ranges_columnar(ranges)
    dr = {k: _dev(v) for k, v in cols.items()}
    n = len(ranges)
    for ce, kc in ((N - 1, KB), (N, KB - 1)):
        t = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")  # noqa: E731
        bufs = {"key_arena": t(KB), "key_off": t(8 * (N + 1)), "val_off": t(8 * N), "val_len": t(4 * N), "seq": t(8 * N),
                "flags": t(N), "create_ts": t(8 * N), "expire_ts": t(8 * N)}
        res_, rb, rs, sm = (torch.zeros(n + 1, dtype=torch.int64, device="cuda"),
                            torch.zeros(2 * n, dtype=torch.int32, device="cuda"),
                            torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(5, dtype=torch.int64, device="cuda"))
        v = _abi.SstView(view["data"].data_ptr(), view["block_off"].data_ptr(), sst.nb, view["index_keys"].data_ptr(),
                         view["index_key_off"].data_ptr(), None, 0, 0, 2, 0)
        rg = _abi.ScanRanges(n, dr["start_bytes"].data_ptr(), dr["start_off"].data_ptr(), dr["start_kind"].data_ptr(),
                             dr["end_bytes"].data_ptr(), dr["end_off"].data_ptr(), dr["end_kind"].data_ptr())
        out = _abi.ScanOut(res_.data_ptr(), rb.data_ptr(), rs.data_ptr(), bufs["key_arena"].data_ptr(), kc,
                           bufs["key_off"].data_ptr(), bufs["val_off"].data_ptr(), bufs["val_len"].data_ptr(),
                           bufs["seq"].data_ptr(), bufs["flags"].data_ptr(), bufs["create_ts"].data_ptr(),
                           bufs["expire_ts"].data_ptr(), ce, sm.data_ptr())
        wsb = rt.lib().sdb_sst_scan_workspace_bytes(sst.nb, n)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        assert rt.lib().sdb_sst_scan(C.byref(v), C.byref(rg), 0, C.byref(out), ws.data_ptr(), wsb, None) == 0
        torch.cuda.synchronize()
        smh = sm.cpu().numpy()
        assert (int(smh[0]), int(smh[1]), int(smh[4]) & 0xFFFFFFFF) == (N, KB, _abi.SDB_LIMIT_EXCEEDED)
        for f, b in bufs.items():
            assert bool((b == 0xA5).all()), f
        assert np.array_equal(res_.cpu().numpy(), full["range_entry_start"])
        assert np.array_equal(rb.cpu().numpy(), full["range_block"][:2 * n])


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("desc", [False, True])
def test_scan_oversize_row(rt, version, desc):
    es = [(b"key%04d" % i, 0, b"v" * (9000 if i == 37 else 20), 1000 - i, None, None) for i in range(80)]
    sst = Sst(Batch.from_entries(es), version, 256)
    assert int(np.diff(sst.block_off.astype(np.int64)).max()) > 9000
    ranges = [(b"key0030", INC, b"key0045", INC), (b"key0037", INC, b"key0037", INC), (None, U, None, U),
              (b"key0037", EXC, None, U), (None, U, b"key0037", EXC)]
    check(sst, ranges, host(rt.sst_scan_device(view_of(sst), ranges, descending=desc)), desc)


def test_scan_degenerate(rt):
    sst, view, _ = case("dup", 2, 256)
    h = host(rt.sst_scan_device(view, []))
    assert h["status"] == 0 and h["num_entries"] == 0 and not h["range_entry_start"].any()
    empty = dict(view, num_blocks=0)
    ranges = [(None, U, None, U), (b"a", INC, b"z", EXC)]
    h = host(rt.sst_scan_device(empty, ranges, cap_entries=4, key_cap=16))
    assert h["status"] == 0 and h["num_entries"] == 0 and h["blocks_read"] == 0
    assert not h["range_entry_start"].any() and not h["range_block"].any() and not h["range_status"].any()


def test_scan_bad_kind_on_device(rt):
    """Bound kinds live in device memory: a kind above 2 fails that range, not the call."""
    sst, view, _ = case("dup", 2, 256)
    ranges = [(None, U, None, U), (sst.keys[5], 3, None, U), (sst.keys[10], INC, sst.keys[20], INC)]
    h = host(rt.sst_scan_device(view, ranges))
    assert h["range_status"].tolist() == [0, _abi.SDB_INVALID_ARGUMENT, 0]
    assert h["status"] == _abi.SDB_INVALID_ARGUMENT and h["num_failed"] == 1
    good = [ranges[0], ranges[2]]
    g = host(rt.sst_scan_device(view, good))
    assert h["num_entries"] == g["num_entries"] and np.array_equal(h["seq"], g["seq"])


@pytest.mark.parametrize("desc", [False, True])
def test_scan_graph_capture(rt, desc):
    import torch
    sst, view, ranges = case("dup", 2, 256)
    ranges = ranges[:60]
    eager = host(rt.sst_scan_device(view, ranges, descending=desc))
    N, KB = eager["num_entries"], eager["key_bytes"]
    dr = {k: _dev(v) for k, v in rt.scan_ranges_columnar(ranges).items()}
    dr["n"] = len(ranges)
    ranges = dr
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # allocations and the first launch (function attributes) outside the capture
        warm = rt.sst_scan_device(view, ranges, descending=desc, stream=s, cap_entries=N, key_cap=KB)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    holder = {}
    with torch.cuda.graph(g, stream=s):
        holder["res"] = rt.sst_scan_device(view, ranges, descending=desc, stream=s, cap_entries=N, key_cap=KB)
    for _ in range(2):
        for k, t in holder["res"].items():
            if not k.startswith("_"):
                t.zero_()
        torch.cuda.synchronize()
        g.replay()
        h = host(holder["res"])
        for k in eager:
            assert np.array_equal(np.asarray(h[k]), np.asarray(eager[k])), k
    del warm
