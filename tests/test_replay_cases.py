"""CPU checks of the WAL replay's host half: replay_model against a brute-force model, wal_replay.rs's own
scripted tests restated by hand, estimate_encoded_size_compacted against hand arithmetic, and the argument
checks of sdb_wal_replay_sort / sdb_wal_replay_emit.  No compute call runs here."""
import ctypes as C
import random

import pytest

from slatedb_amd import _abi, replay, runtime

from .replay_cases import brute_force, small_alphabet_batches, value_row

X128 = b"x" * 128
PRM = runtime.params()  # SsTableFormat::default(): 4096-byte blocks, "_bf" at 10 bits per key, min_filter_keys 0


@pytest.mark.parametrize("seed", range(8))
def test_model_matches_brute_force(seed):
    """A few hundred random batches per seed over a two-letter alphabet: the tables, rows and KVTableMetadata of
    replay_model equal the literal one-row-at-a-time insertion."""
    rng = random.Random(1000 + seed)
    batches = small_alphabet_batches(rng, 300)
    top = max((r[3] for b in batches for r in b), default=0)
    for min_seq in (None, 0, top // 3):
        for limit in (1 << 62, 700, 1):
            m = replay.replay_model(batches, min_seq, PRM, limit)
            assert m["status"] == 0
            want = brute_force(batches, min_seq, PRM, limit)
            assert len(m["tables"]) == len(want)
            for got, (rows, num, size, first, last, tick) in zip(m["tables"], want):
                assert got["rows"] == rows
                assert (got["entry_num"], got["entries_size_in_bytes"]) == (num, size)
                assert (got["first_seq"], got["last_seq"], got["last_tick"]) == (first, last, tick)
            assert m["summary"]["rows_replaced"] + m["summary"]["rows_skipped"] + m["summary"]["rows_out"] == m["summary"]["rows_in"]


def test_model_rejects_batches_out_of_order():
    """W2 (iterator.rs:394-419): equal seqs across batches fail, an empty batch in between does not reset the
    running maximum, equal seqs inside a batch are fine."""
    a, b = [value_row(b"k", b"v", 5), value_row(b"j", b"v", 7)], [value_row(b"k", b"v", 7)]
    assert replay.replay_model([a, b], None, PRM, 1 << 62)["first_error_entry"] == 1
    m = replay.replay_model([a, [], b], None, PRM, 1 << 62)
    assert (m["status"], m["first_error_entry"], m["tables"]) == (_abi.SDB_INVALID_ARGUMENT, 2, [])
    assert replay.replay_model([a + [value_row(b"i", b"", 7)], [], [value_row(b"k", b"v", 8)]], None, PRM, 1 << 62)["status"] == 0


def test_watermark_follows_last_consumed_wal_file_id():
    """wal_replay.rs:320-359: two one-row batches, max_memtable_bytes = the estimate of one row, so each batch
    closes a table; the tables carry their last batch's last_consumed_wal_file_id (0, then 1)."""
    first, second = value_row(b"key_001", X128, 1), value_row(b"key_002", X128, 2)
    limit = replay.estimate_encoded_size_compacted(PRM, 1, replay.row_estimated_size(first))
    m = replay.replay_model([[first], [second]], 0, PRM, limit, wal_ids=[0, 1])
    assert [(t["last_wal_id"], t["replay_last_seq"]) for t in m["tables"]] == [(0, 1), (1, 2)]


def test_max_memtable_bytes_applies_at_batch_boundaries():
    """wal_replay.rs:531-588: three one-row WALs, the limit one byte over a one-row table: the first table takes
    two WALs and exceeds the target, the last WAL gets its own; seqs come out 1, 2, 3."""
    wals = [[value_row(b"key_00%d" % i, X128, i)] for i in (1, 2, 3)]
    limit = replay.estimate_encoded_size_compacted(PRM, 1, replay.row_estimated_size(wals[0][0])) + 1
    m = replay.replay_model(wals, 0, PRM, limit, wal_ids=[1, 2, 3])
    assert [t["last_wal_id"] for t in m["tables"]] == [2, 3]
    t0 = m["tables"][0]
    assert replay.estimate_encoded_size_compacted(PRM, t0["entry_num"], t0["entries_size_in_bytes"]) > limit
    assert [r[3] for t in m["tables"] for r in t["rows"]] == [1, 2, 3]


def test_one_commit_seq_stays_in_one_table():
    """wal_replay.rs:591-647: eight rows of one commit seq in one batch, the limit at one row: one table with
    first_seq == last_seq == the commit seq (tables split only between batches)."""
    rows = [value_row(b"key_%03d" % i, X128, 42) for i in range(8)]
    limit = replay.estimate_encoded_size_compacted(PRM, 1, replay.row_estimated_size(rows[0]))
    m = replay.replay_model([rows], 0, PRM, limit)
    assert [(t["first_seq"], t["last_seq"], t["entry_num"]) for t in m["tables"]] == [(42, 42, 8)]


def test_enforced_limit_every_table_but_the_last_reaches_it():
    """wal_replay.rs:474-528 with its shape scaled down: 500 rows in WALs of up to 20, max_memtable_bytes 1024:
    every table but the last estimates at or over the limit, and the tables together hold every row once."""
    rng = random.Random(7)
    keys = sorted({b"k%05d" % rng.randrange(100000) for _ in range(500)})
    wals, seq = [], 1
    at = 0
    while at < len(keys):
        k = min(len(keys) - at, rng.randrange(0, 20))
        wals.append([value_row(keys[at + i], b"v" * 10, seq + i) for i in range(k)])
        at, seq = at + k, seq + k
    m = replay.replay_model(wals, 0, PRM, 1024)
    assert len(m["tables"]) > 3
    for t in m["tables"][:-1]:
        assert replay.estimate_encoded_size_compacted(PRM, t["entry_num"], t["entries_size_in_bytes"]) >= 1024
    assert sorted(r[0] for t in m["tables"] for r in t["rows"]) == keys


def test_min_seq_skips_rows_at_or_under_it():
    """wal_replay.rs:767-804: 1000 rows with seqs 1..1000, last_l0_seq 500: the one table holds the 500 rows
    with seq > 500 (the compare at :146 is strict)."""
    wals = [[value_row(b"k%04d" % (s * 7919 % 1000), b"v", s) for s in range(lo, lo + 100)] for lo in range(1, 1001, 100)]
    m = replay.replay_model(wals, 500, PRM, 1 << 62, last_l0_seq=500, last_l0_clock_tick=0)
    (t,) = m["tables"]
    assert t["entry_num"] == 500 and min(r[3] for r in t["rows"]) == 501
    assert (t["replay_last_seq"], t["replay_last_tick"]) == (1000, 0)
    assert m["summary"]["rows_skipped"] == 500


def test_empty_trailing_table_carries_the_wal_id():
    """wal_replay.rs:361-382 (applied_any, :168-177): a WAL that yields no row still returns one empty table
    with its WAL id, last_seq 0 and last_tick i64::MIN; and a closed table followed by an all-skipped batch
    leaves an empty last table.  No batch at all: no table."""
    m = replay.replay_model([[]], 0, PRM, 1 << 62, wal_ids=[1])
    (t,) = m["tables"]
    assert (t["entry_num"], t["last_wal_id"], t["replay_last_seq"], t["replay_last_tick"]) == (0, 1, 0, replay.I64_MIN)
    m = replay.replay_model([[value_row(b"a", X128, 9)], [value_row(b"b", b"", 10)]], 9, PRM, 1, wal_ids=[4, 5])
    assert [t["entry_num"] for t in m["tables"]] == [1]  # seq 9 is skipped: the open table takes both batches
    m = replay.replay_model([[value_row(b"a", X128, 9)], []], 0, PRM, 1, wal_ids=[4, 5])
    assert [(t["entry_num"], t["last_wal_id"]) for t in m["tables"]] == [(1, 4), (0, 5)]
    assert replay.replay_model([], 0, PRM, 1)["tables"] == []


def test_estimate_encoded_size_compacted():
    assert replay.estimate_encoded_size_compacted(PRM, 0, 12345) == 0  # format/sst.rs:1046-1048
    # by hand, 100 entries of 3000 bytes, 4096-byte blocks, "_bf" at 10 bits per key:
    #   rows     3000 + (2 + 2 + 4 + 1) * 100                      = 3900, one block
    #   blocks   3900 + 2 * 100 + 4 * 1                            = 4104
    #   index    1 * (12 + 2) + 4                                  = 18
    #   info     12 + 16 + 16 + 1 + 1 + 12 + 16 + 1 + 4            = 79
    #   tail     8 + 2                                             = 10
    #   filter   2 + (2 + 3 + 8) + (ceil(1000 / 8) + 2) + 4        = 146
    #   stats    24 + 16 + 1 * 6 + 4                               = 50
    assert replay.estimate_encoded_size_compacted(PRM, 100, 3000) == 4104 + 18 + 79 + 10 + 146 + 50 == 4407
    none = runtime.params(bloom_bits_per_key=0)
    assert replay.estimate_encoded_size_compacted(none, 100, 3000) == 4407 - 146
    few = runtime.params(min_filter_keys=101)
    assert replay.estimate_encoded_size_compacted(few, 100, 3000) == 4407 - 146  # below min_filter_keys: no filter
    assert replay.estimate_encoded_size_compacted(few, 101, 3000) > 4407
    # two blocks: one more checksum, index entry and stats row
    assert replay.estimate_encoded_size_compacted(none, 100, 3000 + 197) == 4261 + 197 + 4 + 14 + 6
    named = runtime.params(prefix_kind=1, prefix_arg=3)  # "_bf:p=fixed3": nine more name bytes
    assert replay.estimate_encoded_size_compacted(named, 100, 3000) == 4407 + 9


def test_split_tables_walk():
    F = lambda rows, size: {"rows": rows, "bytes": size}
    one = replay.estimate_encoded_size_compacted(PRM, 1, 143)
    assert replay.split_tables([], PRM, 1) == [0]
    assert replay.split_tables([F(0, 0)], PRM, 1) == [0, 1]
    assert replay.split_tables([F(1, 143), F(1, 143)], PRM, one) == [0, 1, 2]
    assert replay.split_tables([F(1, 143), F(1, 143), F(1, 143)], PRM, one + 1) == [0, 2, 3]
    assert replay.split_tables([F(0, 0), F(1, 143), F(0, 0)], PRM, one) == [0, 2, 3]  # an empty table never closes


# ------------------------------------------------------------------------------------------------
# the two calls' argument checks (no device needed: they come before the device check)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return runtime.lib()


def _args(lib, n=4, nb=2, nt=1):
    run = _abi.Run(n, 8, 8, 8, 8, 8, 8, 8, 8, 8)  # non-NULL device pointers that no check dereferences
    ws = lib.sdb_wal_replay_workspace_bytes(n, nb)
    out = _abi.WalTablesOut(8, 64, 8, 8, 64, 8, 8, 8, 8, 8, 8, n, 8, 8)
    return run, ws, out


def test_workspace_bytes(lib):
    assert lib.sdb_diag_replay_tile() >= 128 and lib.sdb_diag_replay_tile() & (lib.sdb_diag_replay_tile() - 1) == 0
    sizes = [lib.sdb_wal_replay_workspace_bytes(n, 3) for n in (0, 1, 1000, 578524)]
    assert sizes == sorted(sizes) and sizes[0] >= 256
    assert sizes[-1] >= 578524 * (8 + 4 + 4 + 4 + 1 + 4)  # prefixes, two permutations, batch, state, destination
    assert lib.sdb_wal_replay_workspace_bytes(1000, 500) > lib.sdb_wal_replay_workspace_bytes(1000, 1)


def test_sort_argument_checks(lib):
    run, ws, _ = _args(lib)
    bad = _abi.SDB_INVALID_ARGUMENT
    call = lambda r=C.byref(run), bs=8, nb=2, facts=8, sm=8, w=8, wb=ws: lib.sdb_wal_replay_sort(r, bs, nb, 0, 0, facts, sm, w, wb, None)
    assert call(r=None) == bad
    assert call(bs=None) == bad
    assert call(facts=None) == bad
    assert call(sm=None) == bad
    assert call(w=None) == bad
    assert call(wb=ws - 1) == bad
    holes = _abi.Run(4, 8, None, 8, 8, 8, 8, 8, 8, 8)
    assert call(r=C.byref(holes)) == bad
    huge = _abi.Run(1 << 31, 8, 8, 8, 8, 8, 8, 8, 8, 8)
    assert lib.sdb_wal_replay_sort(C.byref(huge), 8, 1, 0, 0, 8, 8, 8, 1 << 62, None) == _abi.SDB_LIMIT_EXCEEDED


def test_emit_argument_checks(lib):
    run, ws, out = _args(lib)
    bad = _abi.SDB_INVALID_ARGUMENT
    call = lambda r=C.byref(run), bs=8, nb=2, tbs=8, nt=1, o=C.byref(out), w=8, wb=ws: lib.sdb_wal_replay_emit(r, bs, nb, tbs, nt, o, w, wb, None)
    assert call(r=None) == bad
    assert call(bs=None) == bad
    assert call(tbs=None) == bad
    assert call(o=None) == bad
    assert call(w=None) == bad
    assert call(wb=ws - 1) == bad
    assert call(nt=3) == bad  # more tables than batches
    for f in ("key_off", "val_bytes", "ts_mask", "table_row_start", "summary"):
        o2 = _abi.WalTablesOut.from_buffer_copy(bytes(out))
        setattr(o2, f, None)
        assert call(o=C.byref(o2)) == bad, f


def test_no_device_fails_loudly(lib):
    """Arguments that pass the checks reach the device check: without a GPU both calls report DEVICE_ERROR."""
    if lib.sdb_device_count() > 0:
        pytest.skip("a HIP device is visible")
    run, ws, out = _args(lib)
    assert lib.sdb_wal_replay_sort(C.byref(run), 8, 2, 0, 0, 8, 8, 8, ws, None) == _abi.SDB_DEVICE_ERROR
    assert lib.sdb_wal_replay_emit(C.byref(run), 8, 2, 8, 1, C.byref(out), 8, ws, None) == _abi.SDB_DEVICE_ERROR
    empty = _abi.Run(0)
    assert lib.sdb_wal_replay_sort(C.byref(empty), None, 0, 0, 0, None, 8, 8, ws, None) == _abi.SDB_DEVICE_ERROR
