"""CPU checks of the batched Db::get (sdb_lsm_get): the model of tests/get_cases.py reproduces the reference's
own LayerPriorityTestCase table (tests/golden/get_cases.json), and the C ABI's host side: sizing, argument
checks, the no-device error path and the struct layouts.  The device runs are in tests/test_gpu_get.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from slatedb_amd import _abi

from . import get_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "slatedb_amd.h")


def test_golden_fixture_shape():
    cases = G.golden_cases()
    assert len(cases) == G.KEPT_CASES
    for c in cases:
        assert all(e["layer"] != "wb" and e["kind"] in (0, 2) for e in c["entries"])
        assert sorted(c["layer_order"]) == sorted({e["layer"] for e in c["entries"]})
    assert sum(c["max_seq"] is not None for c in cases) >= 8
    assert sum(c["expected"] is None for c in cases) >= 8


@pytest.mark.parametrize("version", [2, 1])
@pytest.mark.parametrize("bloom", [False, True])
def test_model_reproduces_reference_table(version, bloom):
    for c in G.golden_cases():
        tree = G.golden_tree(c, version, bloom=bloom)
        g = tree.get(c["query_key"].encode(), c["max_seq"])
        assert g.status == 0, c["description"]
        if c["expected"] is None:
            assert g.state in (_abi.GET_NOT_FOUND, _abi.GET_DELETED), c["description"]
        else:
            assert g.state == _abi.GET_FOUND, c["description"]
            s = tree.leaves[g.sst].sst
            col = tree.columns(g)
            val = s.data[col["val_off"]:col["val_off"] + col["val_len"]].tobytes()
            assert val == c["expected"].encode(), c["description"]
            assert s.bes[g.block] <= g.row < s.bes[g.block + 1]


def test_model_tombstone_above_bound_hides_nothing():
    """A tombstone above max_seq is dropped before the walk; at the bound it decides (rule 2 / 3)."""
    tree = G.Tree([[G.leaf_of([(b"k", 2, b"", 90, None, None), (b"k", 0, b"mid", 60, None, None)], 2, 4096)],
                   [G.leaf_of([(b"k", 0, b"old", 30, None, None)], 2, 4096)]])
    assert tree.get(b"k").state == _abi.GET_DELETED
    assert tree.get(b"k", 90).state == _abi.GET_DELETED
    g = tree.get(b"k", 89)
    assert (g.state, g.sst, g.ssts_read) == (_abi.GET_FOUND, 0, 1)
    g = tree.get(b"k", 59)
    assert (g.state, g.sst, g.ssts_read) == (_abi.GET_FOUND, 1, 2)
    assert tree.get(b"k", 29).state == _abi.GET_NOT_FOUND


@pytest.fixture(scope="module")
def lib():
    from slatedb_amd import runtime
    return runtime.lib()


def test_workspace_bytes_monotone(lib):
    f = lib.sdb_lsm_get_workspace_bytes
    base = f(100, 8, 4, 1000)
    assert f(0, 0, 0, 0) > 0 and base > 100 + 4 * 100 + 4 * 8 + 4 * 1000  # marks, block and SST status, run states
    for args in ((10000, 8, 4, 1000), (100, 8, 4, 100000), (100, 800, 4, 1000), (100, 8, 400, 1000)):
        assert f(*args) > base, args
    for lo, hi in ((50, 100), (100, 101), (0, 1)):
        assert f(lo, 8, 4, 1000) <= f(hi, 8, 4, 1000) and f(100, 8, 4, lo) <= f(100, 8, 4, hi)
        assert f(100, lo, 4, 1000) <= f(100, hi, 4, 1000) and f(100, 8, lo, 1000) <= f(100, 8, hi, 1000)


def _host_call(lib, nkeys=2, num_ssts=1, total_blocks=3, **nulls):
    """sdb_lsm_get over host arrays (never dereferenced: the call stops at its argument / device checks)."""
    keep = []

    def arr(n, dt):
        a = np.zeros(max(n, 1), dt)
        keep.append(a)
        return a.ctypes.data

    view = (_abi.SstView * 1)()
    lsm = _abi.LsmView(C.addressof(view), num_ssts, 1, arr(2, np.uint32), arr(8, np.uint8), arr(2, np.uint64),
                       arr(8, np.uint8), arr(2, np.uint64), arr(2, np.uint64), total_blocks)
    sm = _abi.GetSummary()
    out = _abi.GetOut(arr(nkeys, np.uint8), arr(nkeys, np.int32), arr(nkeys, np.uint32), arr(nkeys, np.uint32),
                      arr(nkeys, np.uint64), arr(nkeys, np.uint32), arr(nkeys, np.uint64), arr(nkeys, np.uint8),
                      arr(nkeys, np.int64), arr(nkeys, np.int64), arr(nkeys, np.uint32), arr(nkeys, np.uint32),
                      C.addressof(sm))
    kb, ko = arr(8, np.uint8), arr(nkeys + 1, np.uint64)
    wsb = lib.sdb_lsm_get_workspace_bytes(total_blocks, num_ssts, 1, nkeys)
    ws = arr(wsb, np.uint8)
    for name in nulls:
        if name in ("kb", "ko", "ws", "lsm", "out", "short_ws"):
            continue
        setattr(out if hasattr(out, name) else lsm, name, None)  # the two structs share no field name
    return lib.sdb_lsm_get(None if "lsm" in nulls else C.byref(lsm), None if "kb" in nulls else kb,
                           None if "ko" in nulls else ko, nkeys, None, None if "out" in nulls else C.byref(out),
                           None if "ws" in nulls else ws, wsb - 1 if "short_ws" in nulls else wsb, None)


@pytest.mark.parametrize("null", ["lsm", "out", "kb", "ko", "ws", "short_ws", "ssts", "run_start", "first_key_off",
                                  "last_key_off", "block_base", "state", "status", "sst", "block", "val_off", "val_len",
                                  "seq", "flags", "create_ts", "expire_ts", "ssts_read", "ssts_filtered", "summary"])
def test_null_arguments_and_short_workspace(lib, null):
    assert _host_call(lib, **{null: True}) == _abi.SDB_INVALID_ARGUMENT


def test_valid_arguments_need_a_device(lib):
    if lib.sdb_device_count() > 0:
        pytest.skip("a HIP device is visible")
    assert _host_call(lib) == _abi.SDB_DEVICE_ERROR
    assert _host_call(lib, nkeys=0) == _abi.SDB_DEVICE_ERROR
    assert _host_call(lib, total_blocks=0xFFFFFFFF) == _abi.SDB_LIMIT_EXCEEDED


STRUCTS = {"sdb_lsm_view": _abi.LsmView, "sdb_get_out": _abi.GetOut, "sdb_get_summary": _abi.GetSummary}


def test_struct_layouts_match_header():
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, "int main(void){"]
    for cname, py in STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in py._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append('printf("states %d\\n", SDB_GET_NOT_FOUND + 10 * SDB_GET_FOUND + 100 * SDB_GET_DELETED + '
                 '1000 * SDB_GET_MERGE_OPERAND);')
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
    assert int(out["states"]) == (_abi.GET_NOT_FOUND + 10 * _abi.GET_FOUND + 100 * _abi.GET_DELETED +
                                  1000 * _abi.GET_MERGE_OPERAND)
