"""CPU checks of the merging reads (sdb_lsm_get_merge, sdb_lsm_scan_merge): the model of tests/merge_read_cases.py
plus slatedb_amd.merge.fold against the reference's recorded expectations, the batch shapes fold hands the
operator, the exports, the struct layouts, the workspace sizes and the host-side argument checks."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from slatedb_amd import _abi, merge

from . import get_cases as G
from . import merge_read_cases as M
from .scan_cases import INC, U

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slatedb_amd.h")


# ------------------------------------------------------------------------------------------------
# The model and fold against the reference's expectations
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [2, 1])
def test_model_reproduces_golden_gets(version):
    cases = M.golden()["get_cases"]
    assert len(cases) == M.KEPT_GET
    states = set()
    for c in cases:
        tree = G.golden_tree(c, version)
        key = c["query_key"].encode()
        g = M.get_merge(tree, key, c["max_seq"])
        states.add(g.state)
        assert g.status == 0, c["description"]
        got = M.folded(tree, key, g.links, g.base) if g.links else None
        assert got == (None if c["expected"] is None else c["expected"].encode()), c["description"]
    assert states == {_abi.GET_MERGE_OPERAND}  # every recorded query begins on an operand


@pytest.mark.parametrize("split", [1, 2, 3])
@pytest.mark.parametrize("descending", [False, True])
def test_model_reproduces_golden_iterator_cases(split, descending):
    cases = M.golden()["iter_cases"]
    assert [c["name"] for c in cases] == ["different_expire_ts_read_path", "merge_with_tombstone", "multiple_values"]
    for c in cases:
        tree = M.iter_tree(c, 2, split=split)
        s = M.scan_merge(tree, (None, U, None, U), None, descending)
        assert s.status == 0
        got = []
        for row in s.rows:
            col = M.scan_columns(tree, row)
            kind = 1 if col["flags"] & _abi.FLAG_MERGE_OPERAND else 0
            got.append((row[0], kind, M.folded(tree, row[0], row[1], row[2]), col["seq"], col["expire_ts"]))
        want = M.iter_expected(c)
        assert got == (want[::-1] if descending else want), c["name"]


def test_point_get_does_not_fold_a_tombstone_base_but_a_scan_does():
    es = [(b"k", 1, b"b", 9, 5, None), (b"k", 1, b"a", 8, None, 70), (b"k", 2, b"", 7, 90, 30), (b"k", 0, b"old", 6, None, None)]
    for version in (1, 2):
        tree = G.Tree([[G.leaf_of(es, version, 4096)]])
        g = M.get_merge(tree, b"k")
        assert g.state == _abi.GET_MERGE_OPERAND and len(g.links) == 2 and not g.base and (g.cts, g.ets) == (5, 70)
        assert M.get_columns(tree, g)["flags"] == _abi.FLAG_MERGE_OPERAND | _abi.FLAG_HAS_CREATE_TS | _abi.FLAG_HAS_EXPIRE_TS
        (row,) = M.scan_merge(tree, (b"k", INC, b"k", INC)).rows
        # a V1 tombstone carries no expire_ts (row.rs:223-231)
        assert len(row[1]) == 2 and row[2] and row[3:] == (90, 30 if version == 2 else 70)
        assert M.folded(tree, b"k", row[1], row[2]) == b"ab"


def test_chain_tree_covers_the_chain_shapes():
    tree, straddler = M.chain_tree()
    keys = M.chain_queries(tree, straddler)
    assert 200 <= len(keys) <= 300
    got = [M.get_merge(tree, k) for k in keys]
    run_of = [j for j, r in enumerate(tree.runs) for _ in r]
    ops = [g for g in got if g.state == _abi.GET_MERGE_OPERAND]
    assert len(ops) >= 40 and sum(1 for g in got if g.state == _abi.GET_FOUND) >= 20
    assert sum(1 for g in got if g.state == _abi.GET_DELETED) >= 5 and sum(1 for g in got if g.state == 0) >= 50
    assert any(len(g.links) == 1 for g in ops) and max(len(g.links) for g in ops) >= 12
    assert any(g.base for g in ops) and any(not g.base for g in ops)
    same_sst = lambda g: [b for i, _, b in g.links if i == g.links[0][0]]  # noqa: E731
    assert sum(1 for g in ops if len(set(same_sst(g))) >= 3) >= 3  # one key's links over three blocks of an SST
    assert any({3, 4} <= {i for i, _, _ in g.links} for g in ops)  # across the cut of the sorted run
    assert any(len({run_of[i] for i, _, _ in g.links}) >= 3 for g in ops)  # across L0 SSTs and runs
    assert any(g.ssts_filtered and g.links and min(i for i, _, _ in g.links) == 0 and max(i for i, _, _ in g.links) >= 2
               and not any(i == 1 for i, _, _ in g.links) for g in ops)  # a filtered SST in the middle
    g = M.get_merge(tree, straddler, None)
    assert 3 in tree.chain(straddler) and 4 in tree.chain(straddler)


# ------------------------------------------------------------------------------------------------
# fold: the reference's batch shapes (merge_operator.rs:341-435)
# ------------------------------------------------------------------------------------------------
class Recorder:
    def __init__(self):
        self.calls = []

    def merge_batch(self, key, existing, operands):
        self.calls.append((key, existing, list(operands)))
        return (existing or b"") + b"".join(operands)


@pytest.mark.parametrize("n", [1, 100, 101, 250])
@pytest.mark.parametrize("base", [None, b"B"])
def test_fold_batch_shapes(n, base):
    ops = [b"%03d," % i for i in range(n)]  # oldest first: operand i was written i-th
    rec = Recorder()
    out = merge.fold(b"key", ops[::-1], base, rec)
    assert out == (base or b"") + b"".join(ops)
    nb = (n + 99) // 100
    assert len(rec.calls) == nb + 1
    newest_first = ops[::-1]
    for j, (key, existing, operands) in enumerate(rec.calls[:nb]):
        assert key == b"key" and existing is None
        assert operands == newest_first[100 * j:100 * (j + 1)][::-1]  # a batch from the newest link, oldest first
    key, existing, operands = rec.calls[nb]
    assert existing == base and len(operands) == nb
    assert operands == [b"".join(c[2]) for c in rec.calls[:nb]][::-1]  # the batch results, oldest first


def test_fold_of_nothing():
    rec = Recorder()
    assert merge.fold(b"k", [], None, rec) is None and not rec.calls
    assert merge.fold(b"k", [], b"v", rec) == b"v" and rec.calls == [(b"k", b"v", [])]
    assert merge.MERGE_BATCH_SIZE == 100


# ------------------------------------------------------------------------------------------------
# Exports, layouts, sizes, argument checks
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from slatedb_amd import runtime
    return runtime.lib()


def test_exports_and_status_name(lib):
    for name in ("sdb_lsm_get_merge", "sdb_lsm_get_merge_workspace_bytes", "sdb_lsm_scan_merge",
                 "sdb_lsm_scan_merge_workspace_bytes"):
        assert getattr(lib, name) is not None
    assert _abi.SDB_INVALID_SEQUENCE_ORDER == 12 and _abi.STATUS_NAMES[12] == "INVALID_SEQUENCE_ORDER"
    lib.sdb_status_name.restype = C.c_char_p
    assert lib.sdb_status_name(12) == b"INVALID_SEQUENCE_ORDER"
    assert lib.sdb_abi_version() == 2


def test_struct_layouts_match_header():
    structs = {"sdb_chain_out": _abi.ChainOut, "sdb_chain_summary": _abi.ChainSummary}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, "int main(void){"]
    for cname, py in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in py._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append('printf("seqorder %d\\n", (int)SDB_INVALID_SEQUENCE_ORDER);')
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
    assert int(out["seqorder"]) == _abi.SDB_INVALID_SEQUENCE_ORDER
    from slatedb_amd import runtime
    assert len(runtime.CHAIN_SUMMARY) * 8 == C.sizeof(_abi.ChainSummary)
    assert [f for f, _ in _abi.ChainSummary._fields_][:3] == list(runtime.CHAIN_SUMMARY)
    assert [f for f, _ in _abi.ChainOut._fields_][1:9] == [f for f, _ in runtime.CHAIN_COLUMNS]


def test_workspace_bytes_grow(lib):
    f = lib.sdb_lsm_get_merge_workspace_bytes
    base = [100, 8, 4, 1000]
    assert f(0, 0, 0, 0) > 0
    assert f(*base) > lib.sdb_lsm_get_workspace_bytes(*base) + 64 * 4 * 1000  # a record per (query, run) on top
    for pos in range(4):
        for lo, hi in ((50, 100), (100, 101), (0, 1), (1000, 100000)):
            a, b = list(base), list(base)
            a[pos], b[pos] = lo, hi
            assert f(*a) <= f(*b), (pos, lo, hi)
        big = list(base)
        big[pos] *= 100
        assert f(*big) >= f(*base) and (pos == 1 or f(*big) > f(*base)), pos
    f = lib.sdb_lsm_scan_merge_workspace_bytes
    base = [100, 8, 4, 1000, 5000, 60000]
    assert f(*base) >= lib.sdb_lsm_scan_workspace_bytes(*base) + 3 * 8 * 5000  # three words per candidate on top
    for pos in range(6):
        for lo, hi in ((50, 100), (100, 101), (0, 1)):
            a, b = list(base), list(base)
            a[pos], b[pos] = lo, hi
            assert f(*a) <= f(*b), (pos, lo, hi)
        big = list(base)
        big[pos] *= 100
        assert f(*big) >= f(*base) and (pos == 2 or f(*big) > f(*base)), pos


def _arrs():
    keep = []

    def arr(count, dt):
        a = np.zeros(max(count, 1), dt)
        keep.append(a)
        return a.ctypes.data
    return keep, arr


def _chain(arr, items, cap):
    sm = _abi.ChainSummary()
    return sm, _abi.ChainOut(arr(items + 1, np.uint64), arr(cap, np.uint32), arr(cap, np.uint32), arr(cap, np.uint64),
                             arr(cap, np.uint32), arr(cap, np.uint64), arr(cap, np.uint8), arr(cap, np.int64),
                             arr(cap, np.int64), cap, C.addressof(sm))


def _lsm(arr, num_ssts=1, total_blocks=3):
    view = (_abi.SstView * 1)()
    return view, _abi.LsmView(C.addressof(view), num_ssts, 1, arr(2, np.uint32), arr(8, np.uint8), arr(2, np.uint64),
                              arr(8, np.uint8), arr(2, np.uint64), arr(2, np.uint64), total_blocks)


def _get_call(lib, n=2, cap=4, **nulls):
    """sdb_lsm_get_merge over host arrays (never dereferenced: the call stops at its argument / device checks)."""
    keep, arr = _arrs()
    view, lsm = _lsm(arr)
    gs = _abi.GetSummary()
    out = _abi.GetOut(arr(n, np.uint8), arr(n, np.int32), arr(n, np.uint32), arr(n, np.uint32), arr(n, np.uint64),
                      arr(n, np.uint32), arr(n, np.uint64), arr(n, np.uint8), arr(n, np.int64), arr(n, np.int64),
                      arr(n, np.uint32), arr(n, np.uint32), C.addressof(gs))
    sm, chain = _chain(arr, n, cap)
    wsb = lib.sdb_lsm_get_merge_workspace_bytes(3, 1, 1, n)
    ws = arr(wsb, np.uint8)
    kb, ko = arr(8, np.uint8), arr(n + 1, np.uint64)
    for name in nulls:
        if name.startswith("chain."):
            setattr(chain, name[6:], None)
        elif name.startswith("out."):
            setattr(out, name[4:], None)
        elif name.startswith("lsm."):
            setattr(lsm, name[4:], None)
    return lib.sdb_lsm_get_merge(None if "lsm" in nulls else C.byref(lsm), None if "keys" in nulls else kb,
                                 None if "key_off" in nulls else ko, n, None, None if "out" in nulls else C.byref(out),
                                 None if "chain" in nulls else C.byref(chain), None if "ws" in nulls else ws,
                                 wsb - 1 if "short_ws" in nulls else wsb, None)


def _scan_call(lib, n=2, cap=4, lcap=4, **nulls):
    """sdb_lsm_scan_merge over host arrays."""
    keep, arr = _arrs()
    view, lsm = _lsm(arr)
    rg = _abi.ScanRanges(n, arr(8, np.uint8), arr(n + 1, np.uint64), arr(n, np.uint8), arr(8, np.uint8),
                         arr(n + 1, np.uint64), arr(n, np.uint8))
    ss = _abi.LsmScanSummary()
    out = _abi.LsmScanOut(arr(n + 1, np.uint64), arr(n, np.int32), arr(n, np.uint32), arr(64, np.uint8), 64,
                          arr(cap + 1, np.uint64), arr(cap, np.uint32), arr(cap, np.uint64), arr(cap, np.uint32),
                          arr(cap, np.uint64), arr(cap, np.uint8), arr(cap, np.int64), arr(cap, np.int64), cap,
                          C.addressof(ss))
    sm, chain = _chain(arr, cap, lcap)
    wsb = lib.sdb_lsm_scan_merge_workspace_bytes(3, 1, 1, n, 16, 256)
    ws = arr(wsb, np.uint8)
    for name in nulls:
        if name.startswith("chain."):
            setattr(chain, name[6:], None)
        elif name.startswith("out."):
            setattr(out, name[4:], None)
        elif name.startswith("ranges."):
            setattr(rg, name[7:], None)
    return lib.sdb_lsm_scan_merge(None if "lsm" in nulls else C.byref(lsm), None if "ranges" in nulls else C.byref(rg),
                                  None, 0, 16, 256, None if "out" in nulls else C.byref(out),
                                  None if "chain" in nulls else C.byref(chain), None if "ws" in nulls else ws,
                                  wsb - 1 if "short_ws" in nulls else wsb, None)


CHAIN_NULLS = ["chain", "chain.chain_start", "chain.summary", "chain.sst", "chain.block", "chain.val_off", "chain.val_len",
               "chain.seq", "chain.flags", "chain.create_ts", "chain.expire_ts"]


@pytest.mark.parametrize("null", ["lsm", "out", "ws", "short_ws", "keys", "key_off", "out.summary", "out.state",
                                  "out.ssts_filtered", "lsm.ssts", "lsm.block_base"] + CHAIN_NULLS)
def test_get_merge_null_arguments_and_short_workspace(lib, null):
    assert _get_call(lib, **{null: True}) == _abi.SDB_INVALID_ARGUMENT


@pytest.mark.parametrize("null", ["lsm", "ranges", "out", "ws", "short_ws", "out.summary", "out.range_entry_start",
                                  "out.key_off", "out.sst", "ranges.start_off", "ranges.end_kind"] + CHAIN_NULLS)
def test_scan_merge_null_arguments_and_short_workspace(lib, null):
    assert _scan_call(lib, **{null: True}) == _abi.SDB_INVALID_ARGUMENT


def test_link_columns_may_be_null_without_room(lib):
    """cap_links == 0: only chain_start and the summary are needed, so the call gets past the argument checks."""
    nulls = {n: True for n in CHAIN_NULLS[3:]}
    assert _get_call(lib, cap=4, **nulls) == _abi.SDB_INVALID_ARGUMENT
    assert _scan_call(lib, lcap=4, **nulls) == _abi.SDB_INVALID_ARGUMENT
    if lib.sdb_device_count() == 0:  # with a device the call would go on to launch over these host arrays
        assert _get_call(lib, cap=0, **nulls) == _abi.SDB_DEVICE_ERROR
        assert _scan_call(lib, lcap=0, **nulls) == _abi.SDB_DEVICE_ERROR


def test_valid_arguments_need_a_device(lib):
    if lib.sdb_device_count() > 0:
        pytest.skip("a HIP device is visible")
    assert _get_call(lib) == _abi.SDB_DEVICE_ERROR and _get_call(lib, n=0) == _abi.SDB_DEVICE_ERROR
    assert _scan_call(lib) == _abi.SDB_DEVICE_ERROR and _scan_call(lib, n=0) == _abi.SDB_DEVICE_ERROR
