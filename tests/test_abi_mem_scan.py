"""CPU checks of sdb_lsm_scan_mem's interface: the struct layout against the header, the workspace sizes, and the
host-side argument checks (S9) in their order, SDB_DEVICE_ERROR after them."""
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
    assert lib.sdb_lsm_scan_mem is not None and lib.sdb_lsm_scan_mem_workspace_bytes is not None
    assert "sdb_lsm_scan_mem" in _abi.SIGNATURES and "sdb_lsm_scan_mem_workspace_bytes" in _abi.SIGNATURES
    from slatedb_amd import runtime
    assert callable(runtime.lsm_scan_mem_device)


def test_struct_layouts_match_header():
    structs = {"sdb_mem_scan_out": _abi.MemScanOut, "sdb_mem_view": _abi.MemView, "sdb_mem_chain_out": _abi.MemChainOut}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, "int main(void){"]
    for cname, py in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in py._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-o", exe, src])
        out = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    for cname, py in structs.items():
        assert int(out[cname]) == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out["%s.%s" % (cname, f)]) == getattr(py, f).offset, (cname, f)
    assert [f for f, _ in _abi.MemScanOut._fields_] == ["table", "row", "range_tables"]


def test_header_carries_the_rules():
    text = open(HDR).read()
    for rule in ["S%d." % i for i in range(1, 11)]:
        assert " %s " % rule in text, rule
    assert "sdb_lsm_scan_mem(" in text and "DIFFERS FROM M5" in text


def test_workspace_bytes(lib):
    f, g = lib.sdb_lsm_scan_mem_workspace_bytes, lib.sdb_lsm_scan_projected_workspace_bytes
    # (total_blocks, num_ssts, num_runs, nranges, cand_entries, cand_key_bytes)
    for shape in ((100, 8, 4, 1000, 5000, 80000), (0, 0, 0, 0, 0, 0), (0, 0, 0, 77, 10, 100), (5, 1, 1, 1, 0, 0),
                  (3000, 40, 9, 4096, 1 << 20, 1 << 24)):
        for merge in (0, 1):
            assert f(0, *shape, merge) == g(*shape, merge), (shape, merge)  # S7: no tables: the projected call's
            sizes = [f(t, *shape, merge) for t in (0, 1, 2, 3, 8, 64)]
            assert sizes == sorted(sizes), (shape, merge)  # monotone in num_tables
            if shape[3] >= 77:
                assert sizes[1] > sizes[0] and sizes[-1] > sizes[1]
                # the per-pair state of a (range, table) pair: over 80 bytes
                assert sizes[-1] - sizes[0] >= 64 * shape[3] * 80
    for t in (0, 1, 4):
        for merge in (0, 1):
            sizes = [f(t, 100, 8, 4, n, 1000, 16000, merge) for n in (0, 1, 2, 63, 64, 65, 1000, 100000)]
            assert sizes == sorted(sizes) and sizes[-1] > sizes[0], (t, merge)  # monotone in the ranges
            sizes = [f(t, 100, 8, 4, 50, ce, 16 * ce, merge) for ce in (0, 1, 255, 256, 257, 4096, 1 << 20)]
            assert sizes == sorted(sizes) and sizes[-1] > sizes[0], (t, merge)  # monotone in the candidates
            assert f(t, 100, 8, 4, 50, 1000, 16000, 1) > f(t, 100, 8, 4, 50, 1000, 16000, 0)


def _arrs():
    keep = []

    def arr(count, dt):
        a = np.zeros(max(count, 1), dt)
        keep.append(a)
        return a.ctypes.data
    return keep, arr


def _call(lib, n=2, cap=4, capl=4, ntab=2, with_chain=True, num_ssts=1, cand=(8, 64), nranges=None, **nulls):
    """sdb_lsm_scan_mem over host arrays (never dereferenced: the call stops at its argument / device checks)."""
    keep, arr = _arrs()
    view = (_abi.SstView * 1)()
    lsm = _abi.LsmView(C.addressof(view), num_ssts, 1, arr(2, np.uint32), arr(8, np.uint8), arr(2, np.uint64),
                       arr(8, np.uint8), arr(2, np.uint64), arr(2, np.uint64), 3)
    rg = _abi.ScanRanges(n if nranges is None else nranges, arr(8, np.uint8), arr(n + 1, np.uint64), arr(n, np.uint8),
                         arr(8, np.uint8), arr(n + 1, np.uint64), arr(n, np.uint8))
    sm = _abi.LsmScanSummary()
    out = _abi.LsmScanOut(arr(n + 1, np.uint64), arr(n, np.int32), arr(n, np.uint32), arr(64, np.uint8), 64,
                          arr(cap + 1, np.uint64), arr(cap, np.uint32), arr(cap, np.uint64), arr(cap, np.uint32),
                          arr(cap, np.uint64), arr(cap, np.uint8), arr(cap, np.int64), arr(cap, np.int64), cap,
                          C.addressof(sm))
    mout = _abi.MemScanOut(arr(cap, np.uint32), arr(cap, np.uint64), arr(n, np.uint32))
    csm = _abi.ChainSummary()
    ch = _abi.ChainOut(arr(cap + 1, np.uint64), arr(capl, np.uint32), arr(capl, np.uint32), arr(capl, np.uint64),
                       arr(capl, np.uint32), arr(capl, np.uint64), arr(capl, np.uint8), arr(capl, np.int64),
                       arr(capl, np.int64), capl, C.addressof(csm))
    mch = _abi.MemChainOut(arr(capl, np.uint32), arr(capl, np.uint64))
    fout = _abi.ScanFilterOut(arr(n, np.uint32), arr(1, np.uint64))
    runs = (_abi.Run * max(ntab, 1))()
    mem = _abi.MemView(C.addressof(runs), ntab, 0)
    wsb = lib.sdb_lsm_scan_mem_workspace_bytes(ntab, 3, num_ssts, 1, n, cand[0], cand[1], int(with_chain))
    ws = arr(wsb, np.uint8)
    for name in nulls:
        for prefix, obj in (("mem.", mem), ("mout.", mout), ("mchain.", mch), ("out.", out), ("chain.", ch), ("lsm.", lsm),
                            ("fout.", fout), ("ranges.", rg)):
            if name.startswith(prefix):
                setattr(obj, name[len(prefix):], None)
    want_chain = with_chain and "chain" not in nulls
    want_mchain = (with_chain and "mchain" not in nulls) or "extra_mchain" in nulls
    return lib.sdb_lsm_scan_mem(None if "mem" in nulls else C.byref(mem), None if "lsm" in nulls else C.byref(lsm), None, None,
                                None if "ranges" in nulls else C.byref(rg), None, None, 0, cand[0], cand[1],
                                None if "out" in nulls else C.byref(out), None if "mout" in nulls else C.byref(mout),
                                C.byref(ch) if want_chain else None, C.byref(mch) if want_mchain else None,
                                None if "fout" in nulls else C.byref(fout), None if "ws" in nulls else ws,
                                wsb - 1 if "short_ws" in nulls else wsb, None)


@pytest.mark.parametrize("null", ["lsm", "out", "mout", "chain", "mchain", "mem.tables", "ws", "short_ws", "mout.table",
                                  "mout.row", "mout.range_tables", "mchain.table", "mchain.row", "out.summary",
                                  "out.range_status", "out.sst", "chain.chain_start", "chain.seq", "lsm.ssts", "fout",
                                  "fout.range_filtered", "ranges", "ranges.start_kind"])
def test_null_arguments_and_short_workspace(lib, null):
    assert _call(lib, **{null: True}) == _abi.SDB_INVALID_ARGUMENT


def test_chain_and_mchain_go_together(lib):
    assert _call(lib, with_chain=False, extra_mchain=True) == _abi.SDB_INVALID_ARGUMENT  # mchain without chain
    assert _call(lib, mchain=True) == _abi.SDB_INVALID_ARGUMENT                      # chain without mchain


def test_short_workspace_counts_the_tables(lib):
    """A workspace that holds the projected call but not the table pairs is short."""
    f = lib.sdb_lsm_scan_mem_workspace_bytes
    assert f(40, 3, 1, 1, 64, 8, 64, 1) > f(0, 3, 1, 1, 64, 8, 64, 1)
    assert _call(lib, ntab=2, short_ws=True) == _abi.SDB_INVALID_ARGUMENT


def test_pair_limit(lib):
    """n * (num_ssts + num_tables) over 2^40 is SDB_LIMIT_EXCEEDED; the tables count."""
    n = (1 << 40) // 3 + 1  # over the limit only with the two tables beside the one SST
    for ntab, want in ((2, _abi.SDB_LIMIT_EXCEEDED), (0, _abi.SDB_INVALID_ARGUMENT)):  # without tables: the short workspace
        assert _call(lib, ntab=ntab, nranges=n) == want, ntab


def test_valid_arguments_need_a_device(lib):
    if lib.sdb_device_count() > 0:  # with a device the call would go on to launch over these host arrays
        return
    for kw in ({}, {"with_chain": False}, {"n": 0}, {"ntab": 0}, {"mem": True}, {"num_ssts": 0},
               {"capl": 0, "mchain.table": True, "mchain.row": True}, {"cap": 0, "mout.table": True, "mout.row": True}):
        assert _call(lib, **kw) == _abi.SDB_DEVICE_ERROR, kw
    # every host check comes first: a valid call but for one argument never reports the device
    for null in ("mout", "mchain", "short_ws", "mem.tables"):
        assert _call(lib, **{null: True}) == _abi.SDB_INVALID_ARGUMENT
