"""Shared inputs and checks of the WAL replay tests (tests/test_replay_cases.py on the CPU,
tests/test_gpu_wal_replay.py on the device).  Rows are Batch.from_entries tuples:
(key, kind, value, seq, create_ts | None, expire_ts | None)."""
import random

import numpy as np

from slatedb_amd import _abi, replay
from slatedb_amd.batch import Batch, Run

V, M, T = _abi.KIND_VALUE, _abi.KIND_MERGE, _abi.KIND_TOMBSTONE
BIG = 1 << 63


def value_row(key, value, seq, cts=None, ets=None):
    """RowEntry::new_value"""
    return (bytes(key), V, bytes(value), seq, cts, ets)


def rand_key(rng, lo=1, hi=24):
    return bytes(rng.randrange(256) for _ in range(rng.randint(lo, hi)))


def rand_row(rng, key, seq):
    kind = rng.choice([V, V, V, M, T])
    value = b"" if kind == T else bytes(rng.randrange(256) for _ in range(rng.choice([0, 1, 5, 17, 70])))
    cts = rng.choice([None, rng.randrange(-50, 1000)])
    ets = rng.choice([None, None, rng.randrange(0, 5000)])
    return (key, kind, value, seq, cts, ets)


def rand_rows(rng, n, seq0=1, lo=1, hi=24):
    """n rows with distinct ascending seqs in arrival order and random keys."""
    return [rand_row(rng, rand_key(rng, lo, hi), seq0 + i) for i in range(n)]


def small_alphabet_batches(rng, nbatches):
    """Short keys over two letters, few seqs per batch: duplicates, keys that are prefixes of one another and
    (key, seq) repeats are common.  Batches respect W2; some are empty."""
    out, seq = [], rng.randrange(1, 4)
    for _ in range(nbatches):
        rows = []
        width = rng.randint(1, 3)
        for _ in range(rng.choice([0, 1, 3, 8, 20])):
            key = bytes(rng.choice(b"ab") for _ in range(rng.randint(1, 3)))
            rows.append(rand_row(rng, key, seq + rng.randrange(width)))
        out.append(rows)
        if rows:
            seq += width
    return out


def brute_force(batches, min_seq, prm, max_memtable_bytes):
    """The second model: KVTable::put as a literal insert into a list kept sorted by (key asc, seq desc), one row
    at a time (mem_table.rs:524-557), inside the loop of WalReplayIterator::next (wal_replay.rs:119-184).
    Returns the tables: (rows, entry_num, entries_size_in_bytes, first_seq, last_seq, last_tick)."""
    tables, cur, applied = [], None, False

    def fresh():
        return {"rows": [], "size": 0, "first": replay.U64_MAX, "last": 0, "tick": replay.I64_MIN}

    def close():
        tables.append((cur["rows"], len(cur["rows"]), cur["size"], cur["first"], cur["last"], cur["tick"]))

    cur = fresh()
    for rows in batches:
        applied = True
        for r in rows:
            if min_seq is not None and r[3] <= min_seq:
                continue
            if r[4] is not None:
                cur["tick"] = max(cur["tick"], r[4])
            cur["last"], cur["first"] = max(cur["last"], r[3]), min(cur["first"], r[3])
            at = 0
            while at < len(cur["rows"]):
                o = cur["rows"][at]
                if (o[0], -o[3]) >= (r[0], -r[3]):
                    break
                at += 1
            if at < len(cur["rows"]) and cur["rows"][at][0] == r[0] and cur["rows"][at][3] == r[3]:
                cur["size"] -= replay.row_estimated_size(cur["rows"][at])
                cur["rows"][at] = r
            else:
                cur["rows"].insert(at, r)
            cur["size"] += replay.row_estimated_size(r)
        if cur["rows"] and replay.estimate_encoded_size_compacted(prm, len(cur["rows"]), cur["size"]) >= max_memtable_bytes:
            close()
            cur, applied = fresh(), False
    if applied:
        close()
    return tables


def as_run(batches):
    """(Run of every row in arrival order, batch_start)"""
    rows = [r for b in batches for r in b]
    start = [0]
    for b in batches:
        start.append(start[-1] + len(b))
    return Run.from_entries(rows), start


def expected_stream(model):
    """The model's tables as the one output stream: (Batch, table_row_start)."""
    rows = [r for t in model["tables"] for r in t["rows"]]
    trs = [0]
    for t in model["tables"]:
        trs.append(trs[-1] + len(t["rows"]))
    return Batch.from_entries(rows), trs


FACT_FIELDS = ("rows", "bytes", "replaced", "min_seq", "max_seq", "max_create_ts", "any_create_ts")
SUMMARY_FIELDS = ("rows_in", "rows_skipped", "rows_replaced", "rows_out", "key_bytes", "val_bytes")


def check_device(rt, batches, min_seq, prm, max_memtable_bytes, workspace=None, fill=None):
    """Both device calls against replay_model, every output compared exactly.  Returns (model, outputs)."""
    import torch
    model = replay.replay_model(batches, min_seq, prm, max_memtable_bytes)
    run, start = as_run(batches)
    drun = rt.DeviceRun.from_host(run)
    w = rt.WalReplay(drun, start, workspace=workspace, fill=fill)
    facts, sm = w.sort(min_seq)
    torch.cuda.synchronize()
    assert sm.status == model["status"], (sm.status, model["status"])
    assert sm.first_error_entry == model["first_error_entry"]
    assert sm.rows_in == model["summary"]["rows_in"]
    if model["status"]:
        return model, (w, facts, sm, None)
    for f in SUMMARY_FIELDS:
        assert getattr(sm, f) == model["summary"][f], f
    for b, (got, want) in enumerate(zip(facts, model["facts"])):
        for f in FACT_FIELDS:
            assert getattr(got, f) == want[f], (b, f, getattr(got, f), want[f])
    cuts = replay.split_tables(facts, prm, max_memtable_bytes)
    assert cuts == model["cuts"]
    if len(cuts) < 2:
        return model, (w, facts, sm, None)
    o, esm = w.emit(cuts)
    torch.cuda.synchronize()
    assert esm.status == 0, esm.status
    for f in SUMMARY_FIELDS:
        assert getattr(esm, f) == model["summary"][f], f
    want, trs = expected_stream(model)
    n = want.n
    assert [int(x) for x in o["table_row_start"][:len(trs)].cpu().numpy()] == trs
    v = lambda k, m, dt: o[k][:m].cpu().numpy().view(dt)
    assert np.array_equal(v("key_off", n + 1, np.uint64), want.key_off)
    assert np.array_equal(v("val_off", n + 1, np.uint64), want.val_off)
    assert np.array_equal(v("key_bytes", int(want.key_off[-1]), np.uint8), want.key_bytes)
    assert np.array_equal(v("val_bytes", int(want.val_off[-1]), np.uint8), want.val_bytes)
    for f, dt in (("kind", np.uint8), ("seq", np.uint64), ("create_ts", np.int64), ("expire_ts", np.int64),
                  ("ts_mask", np.uint8)):
        assert np.array_equal(v(f, n, dt), getattr(want, f)), f
    return model, (w, facts, sm, o)
