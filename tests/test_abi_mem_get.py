"""CPU checks of sdb_lsm_get_mem's interface: the struct layouts against the header, the workspace sizes, and the
host-side argument checks (M8) in their order, SDB_DEVICE_ERROR after them."""
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
    assert lib.sdb_lsm_get_mem is not None and lib.sdb_lsm_get_mem_workspace_bytes is not None
    assert "sdb_lsm_get_mem" in _abi.SIGNATURES and "sdb_lsm_get_mem_workspace_bytes" in _abi.SIGNATURES


def test_struct_layouts_match_header():
    structs = {"sdb_mem_view": _abi.MemView, "sdb_mem_get_out": _abi.MemGetOut, "sdb_mem_chain_out": _abi.MemChainOut}
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
    from slatedb_amd import runtime
    assert [f for f, _ in _abi.MemGetOut._fields_] == [f for f, _ in runtime.MEM_FIELDS]
    assert [f for f, _ in _abi.MemChainOut._fields_] == [f for f, _ in runtime.MEM_FIELDS]


def test_workspace_bytes(lib):
    f, g = lib.sdb_lsm_get_mem_workspace_bytes, lib.sdb_lsm_get_projected_workspace_bytes
    for shape in ((100, 8, 4, 1000), (0, 0, 0, 0), (0, 0, 0, 77), (5, 1, 1, 1), (3000, 40, 9, 65536)):
        for merge in (0, 1):
            assert f(0, *shape, merge) == g(*shape, merge), (shape, merge)  # no tables: the projected call's
            sizes = [f(t, *shape, merge) for t in (0, 1, 2, 3, 8, 64)]
            assert sizes == sorted(sizes), (shape, merge)  # monotone in num_tables
            if shape[3]:
                assert sizes[1] > sizes[0] and sizes[-1] > sizes[1]
                # a record per (query, table): 20 bytes, 72 with a chain
                assert sizes[-1] - sizes[0] >= 64 * shape[3] * (72 if merge else 20)
    for t in (0, 1, 4):
        for merge in (0, 1):
            sizes = [f(t, 100, 8, 4, n, merge) for n in (0, 1, 2, 63, 64, 65, 1000, 100000)]
            assert sizes == sorted(sizes) and sizes[-1] > sizes[0], (t, merge)  # monotone in nkeys


def _arrs():
    keep = []

    def arr(count, dt):
        a = np.zeros(max(count, 1), dt)
        keep.append(a)
        return a.ctypes.data
    return keep, arr


def _call(lib, n=2, cap=4, ntab=2, with_chain=True, num_runs=1, **nulls):
    """sdb_lsm_get_mem over host arrays (never dereferenced: the call stops at its argument / device checks)."""
    keep, arr = _arrs()
    view = (_abi.SstView * 1)()
    lsm = _abi.LsmView(C.addressof(view), 1, num_runs, arr(2, np.uint32), arr(8, np.uint8), arr(2, np.uint64),
                       arr(8, np.uint8), arr(2, np.uint64), arr(2, np.uint64), 3)
    gs = _abi.GetSummary()
    out = _abi.GetOut(arr(n, np.uint8), arr(n, np.int32), arr(n, np.uint32), arr(n, np.uint32), arr(n, np.uint64),
                      arr(n, np.uint32), arr(n, np.uint64), arr(n, np.uint8), arr(n, np.int64), arr(n, np.int64),
                      arr(n, np.uint32), arr(n, np.uint32), C.addressof(gs))
    mout = _abi.MemGetOut(arr(n, np.uint32), arr(n, np.uint64))
    sm = _abi.ChainSummary()
    ch = _abi.ChainOut(arr(n + 1, np.uint64), arr(cap, np.uint32), arr(cap, np.uint32), arr(cap, np.uint64),
                       arr(cap, np.uint32), arr(cap, np.uint64), arr(cap, np.uint8), arr(cap, np.int64),
                       arr(cap, np.int64), cap, C.addressof(sm))
    mch = _abi.MemChainOut(arr(cap, np.uint32), arr(cap, np.uint64))
    runs = (_abi.Run * max(ntab, 1))()
    mem = _abi.MemView(C.addressof(runs), ntab, 0)
    wsb = lib.sdb_lsm_get_mem_workspace_bytes(ntab, 3, 1, num_runs, n, int(with_chain))
    ws = arr(wsb, np.uint8)
    kb, ko = arr(8, np.uint8), arr(n + 1, np.uint64)
    for name in nulls:
        for prefix, obj in (("mem.", mem), ("mout.", mout), ("mchain.", mch), ("out.", out), ("chain.", ch), ("lsm.", lsm)):
            if name.startswith(prefix):
                setattr(obj, name[len(prefix):], None)
    want_chain = with_chain and "chain" not in nulls
    want_mchain = (with_chain and "mchain" not in nulls) or "extra_mchain" in nulls
    return lib.sdb_lsm_get_mem(None if "mem" in nulls else C.byref(mem), None if "lsm" in nulls else C.byref(lsm), None, None,
                               kb, ko, n, None, None, None if "out" in nulls else C.byref(out),
                               None if "mout" in nulls else C.byref(mout), C.byref(ch) if want_chain else None,
                               C.byref(mch) if want_mchain else None, None if "ws" in nulls else ws,
                               wsb - 1 if "short_ws" in nulls else wsb, None)


@pytest.mark.parametrize("null", ["lsm", "out", "mout", "chain", "mchain", "mem.tables", "ws", "short_ws", "mout.table",
                                  "mout.row", "mchain.table", "mchain.row", "out.summary", "out.state", "chain.chain_start",
                                  "lsm.ssts"])
def test_null_arguments_and_short_workspace(lib, null):
    assert _call(lib, **{null: True}) == _abi.SDB_INVALID_ARGUMENT


def test_chain_and_mchain_go_together(lib):
    assert _call(lib, with_chain=False, extra_mchain=True) == _abi.SDB_INVALID_ARGUMENT  # mchain without chain
    assert _call(lib, mchain=True) == _abi.SDB_INVALID_ARGUMENT                      # chain without mchain


def test_short_workspace_counts_the_tables(lib):
    """A workspace that holds the projected call but not the table pairs is short."""
    f = lib.sdb_lsm_get_mem_workspace_bytes
    assert f(2, 3, 1, 1, 2, 1) > f(0, 3, 1, 1, 2, 1)
    assert _call(lib, ntab=2, short_ws=True) == _abi.SDB_INVALID_ARGUMENT


def test_pair_limit(lib):
    """nkeys * (num_runs + num_tables) over 2^40 is SDB_LIMIT_EXCEEDED; the tables count."""
    n = (1 << 40) // 3 + 1  # over the limit only with the two tables beside the one run
    f = lib.sdb_lsm_get_mem
    gs = _abi.GetSummary()
    out = _abi.GetOut(*([1] * 12), C.addressof(gs))
    mout = _abi.MemGetOut(1, 1)
    runs = (_abi.Run * 2)()
    view = (_abi.SstView * 1)()
    one = np.zeros(4, np.uint64)
    lsm = _abi.LsmView(C.addressof(view), 1, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, one.ctypes.data,
                       one.ctypes.data, one.ctypes.data, 3)
    for ntab, want in ((2, _abi.SDB_LIMIT_EXCEEDED), (0, _abi.SDB_INVALID_ARGUMENT)):  # without tables: the NULL workspace
        mem = _abi.MemView(C.addressof(runs), ntab, 0)
        st = f(C.byref(mem), C.byref(lsm), None, None, one.ctypes.data, one.ctypes.data, n, None, None, C.byref(out),
               C.byref(mout), None, None, None, 0, None)
        assert st == want, ntab


def test_valid_arguments_need_a_device(lib):
    if lib.sdb_device_count() > 0:  # with a device the call would go on to launch over these host arrays
        return
    for kw in ({}, {"with_chain": False}, {"n": 0}, {"ntab": 0}, {"mem": True}, {"cap": 0, "mchain.table": True, "mchain.row": True}):
        assert _call(lib, **kw) == _abi.SDB_DEVICE_ERROR, kw
