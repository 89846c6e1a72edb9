"""CPU checks of compaction with a merge operator: the model (tests/compaction_merge_cases.py) against the
reference's own write-path cases and against merge.fold's batching, and the ABI the feature adds."""
import ctypes as C
import os
import re
import subprocess

import pytest

from slatedb_amd import _abi, merge
from slatedb_amd.batch import Run

from . import compaction_merge_cases as CM
from .compaction_merge_cases import M, T, V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", CM.FIXTURE, ids=[c["name"] for c in CM.FIXTURE])
def test_collapse_reproduces_reference_cases(case):
    got = CM.collapse([CM.fixture_run(case)], case["barrier"], merge.StringConcat)
    assert got == CM.fixture_entries(case["expected"])


def test_fixture_holds_the_four_write_path_cases():
    assert sorted(c["name"] for c in CM.FIXTURE) == ["different_expire_ts_write_path", "merge_with_snapshot_barrier",
                                                    "merge_with_tombstone", "multiple_values"]
    assert {c["name"]: c["barrier"] for c in CM.FIXTURE}["merge_with_snapshot_barrier"] == 3


@pytest.mark.parametrize("base", [None, V, T])
@pytest.mark.parametrize("links", [1, 99, 100, 101, 200, 201])
def test_model_batches_like_fold(links, base):
    run = [(b"k", M, b"%d" % s, s, None, None) for s in range(links + 1, 1, -1)]
    if base is not None:
        run.append((b"k", base, b"B" if base == V else b"", 1, None, None))
    stats = {}
    got = CM.collapse([run], None, CM.Bracket, stats)
    want = merge.fold(b"k", [e[2] for e in run if e[1] == M], b"B" if base == V else None, CM.Bracket)
    assert got == [(b"k", M if base is None else V, want, links + 1, None, None)]
    assert stats["operator_calls"] == -(-links // 100) + 1
    assert stats["links"] == links + (base is not None) and stats["groups"] == 1
    # the call structure is visible: one bracket per batch, newest batch last inside the final call
    assert want.count(b"(") == -(-links // 100) + 1


def test_model_partition_rules():
    c = lambda run, barrier=None: CM.collapse([run], barrier, merge.StringConcat)
    # None / Some(5) / Some(7) interleaved: every change of expire_ts ends a chain, nothing is a base
    run = [(b"k", M, b"a", 9, None, None), (b"k", M, b"b", 8, None, 5), (b"k", M, b"c", 7, None, 5),
           (b"k", M, b"d", 6, None, 7), (b"k", M, b"e", 5, None, None), (b"k", V, b"f", 4, None, 7)]
    assert c(run) == [(b"k", M, b"a", 9, None, None), (b"k", M, b"cb", 8, None, 5), (b"k", M, b"d", 6, None, 7),
                      (b"k", M, b"e", 5, None, None), (b"k", V, b"f", 4, None, 7)]
    # a tombstone base with a create_ts: kind Value, timestamps folded
    run = [(b"k", M, b"x", 3, 10, None), (b"k", T, b"", 2, 30, None), (b"k", V, b"old", 1, None, None)]
    assert c(run) == [(b"k", V, b"x", 3, 30, None), (b"k", V, b"old", 1, None, None)]
    # the barrier is strict
    run = [(b"k", M, b"3", 3, None, None), (b"k", M, b"2", 2, None, None), (b"k", M, b"1", 1, None, None)]
    assert c(run, 3) == [(b"k", M, b"123", 3, None, None)]
    assert c(run, 2) == [(b"k", M, b"3", 3, None, None), (b"k", M, b"12", 2, None, None)]


def test_expected_runs_the_oracle_over_the_collapsed_stream():
    from oracle import oracle as O
    run = [(b"a", M, b"2", 5, None, None), (b"a", V, b"1", 4, None, None), (b"a", V, b"0", 3, None, None),
           (b"b", M, b"z", 2, None, 7)]
    merged, sm, cuts, ssts = CM.expected([run], O.retention(compaction_start_ts=10), O.params(), 1 << 20, merge.StringConcat)
    assert sm.status == 0 and sm.expired_merges == 1 and merged.n == 1
    assert (merged.key(0), merged.value(0), int(merged.kind[0])) == (b"a", b"12", V)
    assert Run.from_entries(run).n == 4 and len(ssts) == 1


def test_new_symbols_and_abi():
    from slatedb_amd import runtime
    lib = runtime.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "slatedb_amd", "libslatedb_amd.so")]).decode()
    exported = set(re.findall(r" T (sdb_\w+)", out))
    assert {"sdb_compactor_run_merge", "sdb_compactor_run_ssts_merge", "sdb_compactor_merge_stats"} <= exported
    assert lib.sdb_abi_version() == 2
    assert _abi.SDB_MERGE_OPERATOR_ERROR == 13 and lib.sdb_status_name(13) == b"MERGE_OPERATOR_ERROR"
    assert C.sizeof(_abi.MergeOpStats) == 40
    assert all(t is C.c_uint64 for _, t in _abi.MergeOpStats._fields_)
    for name in ("run_merge", "run_ssts_merge", "merge_stats"):
        assert hasattr(runtime.Compactor, name)
    # argument checks that need no device: a NULL handle, a NULL operator
    ns = C.c_uint32(7)
    ret, prm = _abi.Retention(), _abi.SstParams(4096, 2, 16, 10, 0)
    null_op = C.cast(None, _abi.MERGE_BATCH_FN)
    assert lib.sdb_compactor_run_merge(None, None, 0, C.byref(ret), null_op, None, C.byref(prm), 1, None,
                                       C.byref(ns)) == _abi.SDB_INVALID_ARGUMENT
    assert lib.sdb_compactor_merge_stats(None, None) == _abi.SDB_INVALID_ARGUMENT
