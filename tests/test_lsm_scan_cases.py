"""CPU checks of the batched Db::scan (sdb_lsm_scan): the model of tests/lsm_scan_cases.py reproduces the
reference's own ScanTestCase table and an independent brute force, agrees with the get model on point ranges,
the trees the device tests scan are not vacuous, and the call's struct layouts and host-side argument checks
hold.  No kernel runs here."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from slatedb_amd import _abi

from . import get_cases as G
from . import lsm_scan_cases as L
from .scan_cases import INC, U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "slatedb_amd.h")


@pytest.fixture(scope="module")
def plain():
    return L.plain_tree()


@pytest.fixture(scope="module")
def mainm():
    return G.main_tree()


@pytest.mark.parametrize("version", [1, 2])
def test_model_reproduces_the_reference_table(version):
    cases = L.golden_cases()
    assert len(cases) == L.KEPT_CASES
    for c in cases:
        tree = L.golden_tree(c, version)
        assert all(len(r) == 1 for r in tree.runs) and len(tree.runs) == len(c["layer_order"])
        got = L.scan(tree, L.golden_range(c), c["max_seq"])
        assert got.status == 0, c["description"]
        have = []
        for row in got.rows:
            col = L.columns(tree, row)
            data = tree.leaves[col["sst"]].sst.data
            have.append([row[0].decode(), data[col["val_off"]:col["val_off"] + col["val_len"]].tobytes().decode()])
        assert have == c["expected"], c["description"]
        assert [r[0] for r in L.scan(tree, L.golden_range(c), c["max_seq"], True).rows] == [r[0] for r in got.rows][::-1]


def _against_brute(tree, rngs, bounds):
    for q, r in enumerate(rngs):
        b = None if bounds is None else bounds[q]
        got = L.scan(tree, r, b)
        if r[1] > 2 or r[3] > 2:
            continue
        rows, status = L.brute(tree, r, b)
        assert got.status == status and got.rows == rows, (r, b)
        assert L.scan(tree, r, b, True).rows == rows[::-1]
        assert len(got.rows) <= got.candidates and len(got.ssts) <= len(tree.leaves)


def test_model_equals_brute_force(plain, mainm):
    for tree, straddler in (plain, mainm):
        rngs = L.ranges(tree, straddler)
        assert 350 <= len(rngs) <= 450
        _against_brute(tree, rngs, None)
        rb, bounds = L.bounds_for(tree, rngs[:150], straddler)
        _against_brute(tree, rb, bounds)


def test_point_ranges_agree_with_get(mainm):
    tree, straddler = mainm
    keys, bounds = G.bounded_queries(tree, G.main_queries(tree, straddler), straddler)
    seen = set()
    for k, b in list(zip(keys, [None] * len(keys))) + list(zip(keys, bounds)):
        g = tree.get(k, b)
        s = L.scan(tree, (k, INC, k, INC), b)
        seen.add(g.state)
        if g.state == _abi.GET_FOUND:
            assert s.status == 0 and s.rows == [(k, g.sst, g.row)], k
        elif g.state == _abi.GET_MERGE_OPERAND:
            assert s.status == _abi.SDB_MERGE_OPERATOR_MISSING and not s.rows, k
        else:
            assert s.status == 0 and not s.rows, k
    assert seen == {_abi.GET_FOUND, _abi.GET_DELETED, _abi.GET_NOT_FOUND, _abi.GET_MERGE_OPERAND}


def test_device_cases_are_not_vacuous(plain, mainm):
    tree, _ = plain
    assert [len(r) for r in tree.runs] == [1, 1, 1, 1, 1, 3, 3] and tree.leaves[1].sst.nb == 0
    assert sorted({l.version for l in tree.leaves}) == [1, 2]
    assert not any(r[4] & _abi.FLAG_MERGE_OPERAND for l in tree.leaves for r in l.sst.rows)
    full = L.scan(tree, (None, U, None, U))
    total = sum(len(l.sst.rows) for l in tree.leaves)
    print("plain_tree: rows", len(full.rows), "candidates", full.candidates, "blocks", len(full.blocks))
    assert full.status == 0 and len(full.rows) >= 150 and full.candidates == total >= 2000
    assert len(full.blocks) == int(tree.block_base[-1]) and len(full.ssts) == 10
    hidden = len(L.all_keys(tree)) - len(full.rows)  # keys whose newest version is a tombstone
    assert hidden >= 40
    assert {r[1] for r in full.rows} == {i for i, l in enumerate(tree.leaves) if l.sst.nb}  # every SST wins a key
    mtree, _ = mainm
    assert L.scan(mtree, (None, U, None, U)).status == _abi.SDB_MERGE_OPERATOR_MISSING
    st = [L.scan(mtree, r).status for r in L.narrow_ranges(mtree)]
    assert st.count(_abi.SDB_MERGE_OPERATOR_MISSING) >= 30 and st.count(0) >= 30 and len(st) == 300


# ------------------------------------------------------------------------------------------------
# Layouts and host-only behaviour
# ------------------------------------------------------------------------------------------------
STRUCTS = {"sdb_lsm_scan_out": _abi.LsmScanOut, "sdb_lsm_scan_summary": _abi.LsmScanSummary}


def test_struct_layouts_match_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, "int main(void){"]
    for cname, py in STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in py._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-o", exe, src])
        out = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    for cname, py in STRUCTS.items():
        assert int(out[cname]) == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out["%s.%s" % (cname, f)]) == getattr(py, f).offset, (cname, f)
    from slatedb_amd import runtime
    assert len(runtime.LSM_SCAN_SUMMARY) * 8 == C.sizeof(_abi.LsmScanSummary)
    assert [f for f, _ in _abi.LsmScanSummary._fields_][:7] == list(runtime.LSM_SCAN_SUMMARY)


@pytest.fixture(scope="module")
def lib():
    from slatedb_amd import runtime
    return runtime.lib()


def test_workspace_bytes_grows(lib):
    f = lib.sdb_lsm_scan_workspace_bytes
    base = f(100, 8, 4, 1000, 5000, 60000)
    assert f(0, 0, 0, 0, 0, 0) > 0
    assert base > 100 * 5 + 8 * 1000 + 5000 * 40 + 60000  # marks and statuses, a byte per pair, the staged columns, keys
    for args in ((10000, 8, 4, 1000, 5000, 60000), (100, 800, 4, 1000, 5000, 60000), (100, 8, 4, 100000, 5000, 60000),
                 (100, 8, 4, 1000, 500000, 60000), (100, 8, 4, 1000, 5000, 6000000)):
        assert f(*args) > base, args
    # runs only fix the search order (rule 1): the state is per (range, SST), so more runs never need less
    assert f(100, 8, 400, 1000, 5000, 60000) >= base
    for lo, hi in ((50, 100), (100, 101), (0, 1)):
        for pos in range(6):
            a, b = [100, 8, 4, 1000, 5000, 60000], [100, 8, 4, 1000, 5000, 60000]
            a[pos], b[pos] = lo, hi
            assert f(*a) <= f(*b), (pos, lo, hi)


def _host_call(lib, n=2, num_ssts=1, total_blocks=3, cap=4, **nulls):
    """sdb_lsm_scan over host arrays (never dereferenced: the call stops at its argument / device checks)."""
    keep = []

    def arr(count, dt):
        a = np.zeros(max(count, 1), dt)
        keep.append(a)
        return a.ctypes.data

    view = (_abi.SstView * 1)()
    lsm = _abi.LsmView(C.addressof(view), num_ssts, 1, arr(2, np.uint32), arr(8, np.uint8), arr(2, np.uint64),
                       arr(8, np.uint8), arr(2, np.uint64), arr(2, np.uint64), total_blocks)
    rg = _abi.ScanRanges(n, arr(8, np.uint8), arr(n + 1, np.uint64), arr(n, np.uint8), arr(8, np.uint8),
                         arr(n + 1, np.uint64), arr(n, np.uint8))
    sm = _abi.LsmScanSummary()
    out = _abi.LsmScanOut(arr(n + 1, np.uint64), arr(n, np.int32), arr(n, np.uint32), arr(64, np.uint8), 64,
                          arr(cap + 1, np.uint64), arr(cap, np.uint32), arr(cap, np.uint64), arr(cap, np.uint32),
                          arr(cap, np.uint64), arr(cap, np.uint8), arr(cap, np.int64), arr(cap, np.int64), cap,
                          C.addressof(sm))
    wsb = lib.sdb_lsm_scan_workspace_bytes(min(total_blocks, 3), min(num_ssts, 1), 1, n, 16, 256)  # limits come first
    ws = arr(wsb, np.uint8)
    for name in nulls:
        if name in ("ws", "lsm", "out", "ranges", "short_ws"):
            continue
        setattr([o for o in (out, rg, lsm) if hasattr(o, name)][0], name, None)
    return lib.sdb_lsm_scan(None if "lsm" in nulls else C.byref(lsm), None if "ranges" in nulls else C.byref(rg), None, 0,
                            16, 256, None if "out" in nulls else C.byref(out), None if "ws" in nulls else ws,
                            wsb - 1 if "short_ws" in nulls else wsb, None)


@pytest.mark.parametrize("null", ["lsm", "ranges", "out", "ws", "short_ws", "ssts", "run_start", "first_key_off",
                                  "last_key_off", "block_base", "start_bytes", "start_off", "start_kind", "end_bytes",
                                  "end_off", "end_kind", "range_entry_start", "range_status", "range_ssts", "key_arena",
                                  "key_off", "sst", "val_off", "val_len", "seq", "flags", "create_ts", "expire_ts",
                                  "summary"])
def test_null_arguments_and_short_workspace(lib, null):
    assert _host_call(lib, **{null: True}) == _abi.SDB_INVALID_ARGUMENT


def test_limits(lib):
    assert _host_call(lib, total_blocks=0xFFFFFFFF) == _abi.SDB_LIMIT_EXCEEDED
    assert _host_call(lib, num_ssts=0xFFFFFFFF) == _abi.SDB_LIMIT_EXCEEDED


def test_valid_arguments_need_a_device(lib):
    if lib.sdb_device_count() > 0:
        pytest.skip("a HIP device is visible")
    assert _host_call(lib) == _abi.SDB_DEVICE_ERROR
    assert _host_call(lib, n=0) == _abi.SDB_DEVICE_ERROR
