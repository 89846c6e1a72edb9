"""Every output of a tree read comes from the allocator (slatedb_amd.runtime._read_output, the wrappers' alloc=): for
each entry of READ_CALLS and RECENCY_CALLS one well-formed call over a one-SST tree of CPU tensors, with every
capacity given so that exactly one C call is made, and an allocator that records what it is asked for.  Without a
device the call ends in SDB_DEVICE_ERROR, after every output was allocated; with one it would be launched over host
memory, so the module runs only without (as the well-formed calls of tests/test_read_call_args.py do)."""
import pytest
import torch

from slatedb_amd import _abi, runtime

from . import get_cases as G
from . import mem_get_cases as MG
from .read_harness import view_of
from .scan_cases import INC, U


@pytest.fixture(scope="module", autouse=True)
def no_device():
    if runtime.device_count() > 0:
        pytest.skip("a well-formed call over host memory would be launched")


N, CAND, CAP, CAPL, FILL = 2, (8, 64), (4, 32), 5, 0x5A
i64, i32, u8 = torch.int64, torch.int32, torch.uint8
KEYS = [b"a", b"k"]
RANGES = [(b"a", INC, b"k", INC), (None, U, None, U)]
VISIBLE = [(b"a", INC, None, U)]

# (name, count, dtype, fill) in the order the call asks for them; "_ws" (its count is what the sizer answers) is named
# where the call allocates its workspace
GET = [("state", N, u8, 0), ("status", N, i32, 0), ("sst", N, i32, 0), ("block", N, i32, 0), ("val_off", N, i64, 0),
       ("val_len", N, i32, 0), ("seq", N, i64, 0), ("flags", N, u8, 0), ("create_ts", N, i64, 0), ("expire_ts", N, i64, 0),
       ("ssts_read", N, i32, 0), ("ssts_filtered", N, i32, 0), ("summary", 7, i64, 0)]
GET_MEM = [("table", N, i32, None), ("row", N, i64, None)]
RANGE = [("range_entry_start", N + 1, i64, 0), ("range_status", N, i32, 0), ("range_ssts", N, i32, 0), ("summary", 7, i64, 0)]
FOUT = [("range_filtered", N, i32, 0), ("num_filtered", 1, i64, 0)]
MOUT = [("range_tables", N, i32, 0)]
ROUT = [("range_sources_read", N, i32, 0), ("range_visible", N, i64, 0)]
ROWS = [("key_arena", CAP[1], u8, 0), ("key_off", CAP[0] + 1, i64, 0), ("sst", CAP[0], i32, 0), ("val_off", CAP[0], i64, 0),
        ("val_len", CAP[0], i32, 0), ("seq", CAP[0], i64, 0), ("flags", CAP[0], u8, 0), ("create_ts", CAP[0], i64, 0),
        ("expire_ts", CAP[0], i64, 0)]
SCAN_MEM = [("table", CAP[0], i32, 0xFF), ("row", CAP[0], i64, 0)]
MCHAIN = [("chain_table", CAPL, i32, FILL), ("chain_row", CAPL, i64, FILL)]


def chain(items):
    return [("chain_start", items + 1, i64, 0), ("chain_sst", CAPL, i32, FILL), ("chain_block", CAPL, i32, FILL),
            ("chain_val_off", CAPL, i64, FILL), ("chain_val_len", CAPL, i32, FILL), ("chain_seq", CAPL, i64, FILL),
            ("chain_flags", CAPL, u8, FILL), ("chain_create_ts", CAPL, i64, FILL), ("chain_expire_ts", CAPL, i64, FILL),
            ("chain_summary", 3, i64, 0)]


WS = [("_ws", None, u8, None)]
LINKS = dict(merge=True, cap_links=CAPL, fill=FILL)
SIZES = dict(cand=CAND, cap=CAP)
# entry -> (the wrapper's call over (tree, tables, alloc), the outputs, the call has a chain, the call has tables, what its
# sizer takes before and behind (total_blocks, num_ssts, num_runs, n))
CALLS = {
    "sdb_lsm_get": (lambda t, m, a: runtime.lsm_get_device(t, None, KEYS, alloc=a), GET + WS, False, False, (), ()),
    "sdb_lsm_get_merge": (lambda t, m, a: runtime.lsm_get_merge_device(t, None, KEYS, cap_links=CAPL, fill=FILL, alloc=a),
                          GET + WS + chain(N), True, False, (), ()),
    "sdb_lsm_get_filtered": (lambda t, m, a: runtime.lsm_get_filtered_device(t, None, KEYS, alloc=a, **LINKS),
                             GET + WS + chain(N), True, False, (), (1,)),
    "sdb_lsm_get_projected": (lambda t, m, a: runtime.lsm_get_projected_device(t, None, VISIBLE, KEYS, alloc=a), GET + WS, False,
                              False, (), (0,)),
    "sdb_lsm_get_mem": (lambda t, m, a: runtime.lsm_get_mem_device(m, t, None, KEYS, alloc=a, **LINKS),
                        GET + GET_MEM + WS + chain(N) + MCHAIN, True, True, (1,), (1,)),
    "sdb_lsm_scan": (lambda t, m, a: runtime.lsm_scan_device(t, RANGES, alloc=a, **SIZES), RANGE + WS + ROWS, False, False, (), CAND),
    "sdb_lsm_scan_merge": (lambda t, m, a: runtime.lsm_scan_merge_device(t, RANGES, cap_links=CAPL, fill=FILL, alloc=a, **SIZES),
                           RANGE + WS + ROWS + chain(CAP[0]), True, False, (), CAND),
    "sdb_lsm_scan_filtered": (lambda t, m, a: runtime.lsm_scan_filtered_device(t, RANGES, [b"a", None], alloc=a, **SIZES),
                              RANGE + FOUT + WS + ROWS, False, False, (), CAND + (0,)),
    "sdb_lsm_scan_projected": (lambda t, m, a: runtime.lsm_scan_projected_device(t, VISIBLE, RANGES, alloc=a, **SIZES, **LINKS),
                               RANGE + FOUT + WS + ROWS + chain(CAP[0]), True, False, (), CAND + (1,)),
    "sdb_lsm_scan_mem": (lambda t, m, a: runtime.lsm_scan_mem_device(m, t, RANGES, alloc=a, **SIZES, **LINKS),
                         RANGE + FOUT + MOUT + WS + ROWS + chain(CAP[0]) + SCAN_MEM + MCHAIN, True, True, (1,), CAND + (1,)),
    "sdb_lsm_scan_recency": (lambda t, m, a: runtime.lsm_scan_recency_device(m, t, RANGES, limit=[0, 3], alloc=a, **SIZES),
                             RANGE + FOUT + MOUT + ROUT + WS + ROWS + SCAN_MEM, False, True, (1,), CAND),
}


def test_every_entry_point_has_a_case():
    assert sorted(CALLS) == sorted(list(runtime.READ_CALLS) + list(runtime.RECENCY_CALLS))


@pytest.mark.parametrize("entry", sorted(CALLS))
def test_outputs_come_from_the_allocator(entry):
    call, outputs, merge, has_tables, before, behind = CALLS[entry]
    leaf = G.leaf_of([(b"a", 0, b"x", 9, None, None), (b"k", 0, b"y", 8, None, 77)], 2, 4096)
    tree = runtime.lsm_tree_device([view_of(leaf, device="cpu")], [1])
    assert tree["device"].type == "cpu" and tree["num_ssts"] == 1
    table = MG.Table([(b"k", 0, b"mem", 20, None, None)])
    mem = runtime.mem_tables_device([runtime.DeviceRun.from_host(table.run, "cpu")]) if has_tables else None
    wsb = runtime.read_workspace_bytes(entry, tree, N, CAND if "_scan" in entry else (0, 0), merge, mem)
    assert wsb == getattr(runtime.lib(), entry + "_workspace_bytes")(*before, tree["total_blocks"], 1, 1, N, *behind) > 0
    asked = []

    def record(name, count, dtype, fill):
        asked.append((name, count, dtype, fill))
        return runtime._read_output("cpu", name, count, dtype, fill)

    with pytest.raises(runtime.SdbError) as err:
        call(tree, mem, record)
    assert err.value.status == _abi.SDB_DEVICE_ERROR
    assert asked == [(name, wsb if name == "_ws" else count, dtype, fill) for name, count, dtype, fill in outputs]
