"""CPU checks of sdb_lsm_scan_recency's interface: the exports, the struct layout against the header, the rules the
header states, the workspace sizes, and the host-side argument checks (R7) in their order, SDB_DEVICE_ERROR after them."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from slatedb_amd import _abi

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slatedb_amd.h")


@pytest.fixture(scope="module")
def lib():
    from slatedb_amd import runtime
    return runtime.lib()


def test_exports(lib):
    assert lib.sdb_lsm_scan_recency is not None and lib.sdb_lsm_scan_recency_workspace_bytes is not None
    assert "sdb_lsm_scan_recency" in _abi.SIGNATURES and "sdb_lsm_scan_recency_workspace_bytes" in _abi.SIGNATURES
    from slatedb_amd import runtime
    assert callable(runtime.lsm_scan_recency_device)
    entry, sizer = runtime.RECENCY_CALLS["sdb_lsm_scan_recency"]
    assert len(entry) + 3 == len(_abi.SIGNATURES["sdb_lsm_scan_recency"][1])
    assert len(sizer) == len(_abi.SIGNATURES["sdb_lsm_scan_recency_workspace_bytes"][1])


def test_struct_layout_matches_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, "int main(void){",
             'printf("size %zu\\n", sizeof(sdb_recency_out));']
    for f, _ in _abi.RecencyOut._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(sdb_recency_out, %s));' % (f, f))
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-o", exe, src])
        out = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    assert int(out["size"]) == C.sizeof(_abi.RecencyOut)
    for f, _ in _abi.RecencyOut._fields_:
        assert int(out[f]) == getattr(_abi.RecencyOut, f).offset, f
    assert [f for f, _ in _abi.RecencyOut._fields_] == ["range_sources_read", "range_visible"]


def test_header_carries_the_rules():
    text = open(HDR).read()
    for rule in ["R%d." % i for i in range(1, 8)]:
        assert " %s " % rule in text, rule
    for words in ("sdb_lsm_scan_recency(", "segment_iterator.rs:44-45", "db_iter.rs:413-440", "RecencyScanPrefixSpansMultipleSegments",
                  "SDB_MERGE_OPERATOR_MISSING cannot come out of this call"):
        assert words in text, words


def test_workspace_bytes(lib):
    f, g = lib.sdb_lsm_scan_recency_workspace_bytes, lib.sdb_lsm_scan_mem_workspace_bytes
    base = (2, 100, 8, 4, 50, 1000, 16000)  # num_tables, total_blocks, num_ssts, num_runs, nranges, cand_entries, cand_key_bytes
    grids = {0: (0, 1, 2, 3, 8, 64), 1: (0, 1, 7, 100, 1025, 1 << 20), 2: (0, 1, 5, 8, 40, 1000), 3: (0, 1, 3, 4, 9),
             4: (0, 1, 2, 63, 64, 65, 1000, 100000), 5: (0, 1, 255, 256, 257, 4096, 1 << 20), 6: (0, 1, 255, 256, 16000, 1 << 24)}
    for axis, values in grids.items():  # monotone in each argument
        sizes = [f(*(base[:axis] + (x,) + base[axis + 1:])) for x in values]
        assert sizes == sorted(sizes), (axis, sizes)
        if axis != 3:  # (runs only fix the walk order: no state per run)
            assert sizes[-1] > sizes[0], axis
    for shape in (base, (0, 0, 0, 0, 0, 0, 0), (0, 5, 1, 1, 1, 0, 0), (3, 3000, 40, 9, 4096, 1 << 20, 1 << 24)):
        assert f(*shape) > g(*shape, 0)  # the flags, their scans and the plan, beside what the merging scan carves
        # per candidate: two flags, two scans and the group starts
        assert f(*shape) - g(*shape, 0) >= 5 * 8 * shape[5]


def _arrs():
    keep = []

    def arr(count, dt):
        a = np.zeros(max(count, 1), dt)
        keep.append(a)
        return a.ctypes.data
    return keep, arr


def _call(lib, n=2, cap=4, ntab=2, num_ssts=1, cand=(8, 64), nranges=None, limit=True, **nulls):
    """sdb_lsm_scan_recency over host arrays (never dereferenced: the call stops at its argument / device checks)."""
    keep, arr = _arrs()
    view = (_abi.SstView * 1)()
    lsm = _abi.LsmView(C.addressof(view), num_ssts, 1, arr(2, np.uint32), arr(8, np.uint8), arr(2, np.uint64),
                       arr(8, np.uint8), arr(2, np.uint64), arr(2, np.uint64), 3)
    rg = _abi.ScanRanges(n if nranges is None else nranges, arr(8, np.uint8), arr(n + 1, np.uint64), arr(n, np.uint8),
                         arr(8, np.uint8), arr(n + 1, np.uint64), arr(n, np.uint8))
    px = _abi.ScanPrefixes(arr(8, np.uint8), arr(n + 1, np.uint64), arr(n, np.uint8), None)
    sm = _abi.LsmScanSummary()
    out = _abi.LsmScanOut(arr(n + 1, np.uint64), arr(n, np.int32), arr(n, np.uint32), arr(64, np.uint8), 64,
                          arr(cap + 1, np.uint64), arr(cap, np.uint32), arr(cap, np.uint64), arr(cap, np.uint32),
                          arr(cap, np.uint64), arr(cap, np.uint8), arr(cap, np.int64), arr(cap, np.int64), cap,
                          C.addressof(sm))
    mout = _abi.MemScanOut(arr(cap, np.uint32), arr(cap, np.uint64), arr(n, np.uint32))
    fout = _abi.ScanFilterOut(arr(n, np.uint32), arr(1, np.uint64))
    rout = _abi.RecencyOut(arr(n, np.uint32), arr(n, np.uint64))
    runs = (_abi.Run * max(ntab, 1))()
    mem = _abi.MemView(C.addressof(runs), ntab, 0)
    wsb = lib.sdb_lsm_scan_recency_workspace_bytes(ntab, 3, num_ssts, 1, n, cand[0], cand[1])
    ws = arr(wsb, np.uint8)
    for name in nulls:
        for prefix, obj in (("mem.", mem), ("mout.", mout), ("out.", out), ("lsm.", lsm), ("fout.", fout), ("rout.", rout),
                            ("ranges.", rg), ("prefixes.", px)):
            if name.startswith(prefix):
                setattr(obj, name[len(prefix):], None)
    ref = lambda name, obj: None if name in nulls else C.byref(obj)  # noqa: E731
    return lib.sdb_lsm_scan_recency(ref("mem", mem), ref("lsm", lsm), None, None, ref("ranges", rg), ref("prefixes", px), None,
                                    arr(n, np.uint64) if limit else None, 0, cand[0], cand[1], ref("out", out),
                                    ref("mout", mout), ref("fout", fout), ref("rout", rout),
                                    None if "ws" in nulls else ws, wsb - 1 if "short_ws" in nulls else wsb, None)


@pytest.mark.parametrize("null", ["lsm", "out", "mout", "fout", "rout", "ranges", "mem.tables", "ws", "short_ws", "mout.table",
                                  "mout.row", "mout.range_tables", "out.summary", "out.range_status", "out.sst", "lsm.ssts",
                                  "fout.range_filtered", "rout.range_sources_read", "rout.range_visible", "ranges.start_kind",
                                  "prefixes.has_prefix"])
def test_null_arguments_and_short_workspace(lib, null):
    assert _call(lib, **{null: True}) == _abi.SDB_INVALID_ARGUMENT


def test_short_workspace_counts_the_recency_arrays(lib):
    """A workspace that holds sdb_lsm_scan_mem's call over the same shape is short."""
    need = lib.sdb_lsm_scan_recency_workspace_bytes(2, 3, 1, 1, 2, 8, 64)
    assert need > lib.sdb_lsm_scan_mem_workspace_bytes(2, 3, 1, 1, 2, 8, 64, 0)
    assert _call(lib, short_ws=True) == _abi.SDB_INVALID_ARGUMENT


def test_pair_limit(lib):
    n = (1 << 40) // 3 + 1  # over the limit only with the two tables beside the one SST
    for ntab, want in ((2, _abi.SDB_LIMIT_EXCEEDED), (0, _abi.SDB_INVALID_ARGUMENT)):  # without tables: the short workspace
        assert _call(lib, ntab=ntab, nranges=n) == want, ntab


def test_valid_arguments_need_a_device(lib):
    if lib.sdb_device_count() > 0:  # with a device the call would go on to launch over these host arrays
        return
    for kw in ({}, {"limit": False}, {"n": 0}, {"n": 0, "rout.range_visible": True}, {"ntab": 0}, {"mem": True}, {"num_ssts": 0},
               {"prefixes": True}, {"cap": 0, "mout.table": True, "mout.row": True}):
        assert _call(lib, **kw) == _abi.SDB_DEVICE_ERROR, kw
    # every host check comes first: a valid call but for one argument never reports the device
    for null in ("rout", "rout.range_visible", "short_ws", "mem.tables"):
        assert _call(lib, **{null: True}) == _abi.SDB_INVALID_ARGUMENT
