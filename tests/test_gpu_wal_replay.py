"""sdb_wal_replay_sort / sdb_wal_replay_emit on the device against slatedb_amd.replay.replay_model: every output
column, table_row_start, the per-batch facts and the summaries, exactly (tests/replay_cases.py check_device)."""
import ctypes as C
import random

import numpy as np
import pytest

from oracle import oracle as O
from slatedb_amd import _abi, replay
from slatedb_amd.batch import Batch, Run

from .replay_cases import BIG, M, T, V, as_run, check_device, rand_key, rand_row, rand_rows, value_row

pytestmark = pytest.mark.gpu
CANARY = 0xA5


@pytest.fixture(scope="module")
def rt():
    from slatedb_amd import runtime
    runtime.require_device()
    return runtime


@pytest.fixture(scope="module")
def tile(rt):
    return rt.lib().sdb_diag_replay_tile()


@pytest.fixture(scope="module")
def prm(rt):
    return rt.params()


def untouched(t):
    return bool((t.view(__import__("torch").uint8) == CANARY).all().item())


SHAPES = {"0": lambda t: 0, "1": lambda t: 1, "2": lambda t: 2, "T-1": lambda t: t - 1, "T": lambda t: t, "T+1": lambda t: t + 1,
          "2T+1": lambda t: 2 * t + 1, "5T+3": lambda t: 5 * t + 3}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_row_counts(rt, tile, prm, shape):
    """One batch of random keys of 1..24 bytes around the tile size; 5T + 3 takes three merge passes over an odd
    number of tiles."""
    n = SHAPES[shape](tile)
    rng = random.Random(n)
    check_device(rt, [rand_rows(rng, n)], None, prm, BIG)


def shared_prefix(keys):
    """L0 as the kernels find it: the bytes every key shares with the first."""
    n = 0
    while all(len(k) > n and k[n] == keys[0][n] for k in keys):
        n += 1
    return n


def tie8_keys(rng, tile):
    """Two bytes shared by every key, so L0 = 2; then groups of keys equal in bytes [2, 10) whose tails of 0..12
    bytes over a two-letter alphabet differ only behind them: some differ in a later byte, some are prefixes of one
    another there.  A few keys outside the groups keep the shared prefix short."""
    keys = [b"u/a", b"u/", b"u/zzzzzzzzzzzz", b"u/\x00"]
    for head in (b"u/ABCDEFGH", b"u/ABCDEFGI", b"u/\x00\x00\x00\x00\x00\x00\x00\x00"):
        keys += [head + bytes(rng.choice(b"xy") for _ in range(rng.randint(0, 12))) for _ in range(tile // 2)]
    return keys


@pytest.mark.parametrize("case", ["shared40", "tie8", "prefixes"])
def test_prefix_ties(rt, tile, prm, case):
    rng = random.Random({"shared40": 40, "tie8": 8, "prefixes": 26}[case])
    if case == "shared40":  # every key shares 40 bytes: the 8-byte prefixes start behind them
        head = bytes(rng.randrange(256) for _ in range(40))
        keys = [head + rand_key(rng, 1, 12) for _ in range(tile + 50)]
    elif case == "tie8":  # equal in the 8 bytes behind the shared prefix: those compares read the key bytes
        keys = tie8_keys(rng, tile)
        L0 = shared_prefix(keys)
        assert L0 == 2 and len(keys) > tile
        groups = {}
        for k in set(keys):
            groups.setdefault(k[L0:L0 + 8].ljust(8, b"\x00"), []).append(k)
        tied = [g for g in groups.values() if len(g) > 100]  # many keys on one comparison prefix
        assert len(tied) == 3 and all(any(len(k) > L0 + 8 for k in g) for g in tied)
        assert any(x != y and not x.startswith(y) and not y.startswith(x) for g in tied for x in g[:40] for y in g[:40])
        assert any(x != y and x.startswith(y) for g in tied for x in g[:40] for y in g[:40])
    else:  # a, ab, abc, ...: a key sorts before its extensions, zero padding included
        keys = [b"abcdefghijklmnopqrstuvwxyz"[:k] for k in range(1, 27)] + [b"ab" + b"\x00" * k for k in range(0, 12)]
        keys = keys * 3
    rng.shuffle(keys)
    rows = [rand_row(rng, k, 10 + i) for i, k in enumerate(keys)]
    if case == "tie8":  # equal (key, seq) pairs among the tied keys, near and more than a tile apart: W4's compare
        long = [i for i, r in enumerate(rows) if len(r[0]) > 12]
        for src, dst in ((long[0], long[1]), (long[2], long[-1]), (long[3], long[len(long) // 2])):
            rows[dst] = rand_row(rng, rows[src][0], rows[src][3])
        model = replay.replay_model([rows], None, prm, BIG)
        assert model["summary"]["rows_replaced"] >= 3
    check_device(rt, [rows], None, prm, BIG)


def test_one_key_many_versions(rt, tile, prm):
    """3T versions of one key, distinct seqs in shuffled arrival order: seq descending across tile boundaries."""
    rng = random.Random(3)
    seqs = list(range(100, 100 + 3 * tile))
    rng.shuffle(seqs)
    model, _ = check_device(rt, [[rand_row(rng, b"the-one-key", s) for s in seqs]], None, prm, BIG)
    assert [r[3] for r in model["tables"][0]["rows"]] == sorted(seqs, reverse=True)


def test_replacement(rt, tile, prm):
    """(key, seq) written twice and three times in one batch with different values, kinds and timestamps: the
    last arrival wins, bytes counts only the survivor, max_create_ts sees a replaced row; one pair lies more
    than a tile apart."""
    rng = random.Random(4)
    rows = [(b"twice", V, b"first-long-value", 7, 5000, None), (b"other", V, b"x", 7, None, None),
            (b"twice", T, b"", 7, None, 50), (b"thrice", M, b"m1", 8, 5, 6), (b"thrice", V, b"", 8, None, None),
            (b"thrice", M, b"the last one", 8, 1, None), (b"far", V, b"early", 9, 700, 800)]
    rows += rand_rows(rng, 2 * tile, seq0=20)
    rows.append((b"far", T, b"", 9, None, None))
    model, _ = check_device(rt, [rows], None, prm, BIG)
    (f,) = model["facts"]
    assert f["replaced"] == 4 and f["max_create_ts"] == 5000
    out = {(r[0], r[3]): r for r in model["tables"][0]["rows"]}
    assert out[(b"twice", 7)][1] == T and out[(b"thrice", 8)][2] == b"the last one" and out[(b"far", 9)][1] == T
    assert f["bytes"] == sum(replay.row_estimated_size(r) for r in model["tables"][0]["rows"])


def test_w1_min_seq(rt, tile, prm):
    rng = random.Random(5)
    batches = [rand_rows(rng, 300, seq0=1), rand_rows(rng, 300, seq0=301)]
    for min_seq in (150, 149, 300, 0):  # a row's own seq is skipped; one below keeps it; a whole batch skipped
        model, _ = check_device(rt, batches, min_seq, prm, BIG)
        assert model["summary"]["rows_skipped"] == min_seq
    model, _ = check_device(rt, batches, 600, prm, BIG)  # every row skipped: one empty table
    assert [t["entry_num"] for t in model["tables"]] == [0] and model["summary"]["rows_out"] == 0
    # the flag itself: a row with seq 0 is kept when has_min_seq = 0 and skipped by has_min_seq = 1, min_seq = 0
    zero = [[value_row(b"seq-zero", b"v", 0)] + batches[0], batches[1]]
    model, _ = check_device(rt, zero, None, prm, BIG)
    assert model["summary"]["rows_skipped"] == 0 and model["tables"][0]["first_seq"] == 0
    assert any(r[0] == b"seq-zero" for r in model["tables"][0]["rows"])
    model, _ = check_device(rt, zero, 0, prm, BIG)
    assert model["summary"]["rows_skipped"] == 1 and model["tables"][0]["first_seq"] == 1


def test_w2_batch_order(rt, tile, prm):
    """A batch whose smallest seq equals the largest seq before it fails the call with that batch's index; empty
    batches in between do not reset the running maximum; nothing is emitted."""
    import torch
    rng = random.Random(6)
    a, c = rand_rows(rng, 40, seq0=10), rand_rows(rng, 40, seq0=49)  # 49 = a's largest
    for batches, bad in (([a, c], 1), ([a, [], [], c], 3), ([[], a, rand_rows(rng, 5, seq0=100), [], c], 4)):
        run, start = as_run(batches)
        w = rt.WalReplay(rt.DeviceRun.from_host(run), start, fill=CANARY)
        _, sm = w.sort(None)
        assert (sm.status, sm.first_error_entry, sm.rows_in) == (_abi.SDB_INVALID_ARGUMENT, bad, run.n)
        assert untouched(w.facts_t)
        o, esm = w.emit([0, len(batches)])
        torch.cuda.synchronize()
        assert (esm.status, esm.first_error_entry) == (_abi.SDB_INVALID_ARGUMENT, bad)
        assert all(untouched(o[k]) for k in o if k != "summary")
    check_device(rt, [a, [], rand_rows(rng, 40, seq0=50)], None, prm, BIG)  # one above: fine


def test_split(rt, tile, prm):
    """Tables split where the host's walk says (W6): after batches 2 and 5 of 6; a trailing empty batch joins the
    last table; 2^63 gives one table; a limit of 1 gives a table per batch."""
    rng = random.Random(7)
    sizes, seq, batches = [10, 10, 5, 5, 10, 10], 1, []
    for k in sizes:
        batches.append([value_row(rand_key(rng, 8, 8), b"v" * 20, seq + i) for i in range(k)])
        seq += k
    limit = replay.estimate_encoded_size_compacted(prm, 20, 20 * replay.row_estimated_size(batches[0][0]))
    model, _ = check_device(rt, batches, None, prm, limit)
    assert model["cuts"] == [0, 2, 5, 6]
    model, _ = check_device(rt, batches + [[]], None, prm, limit)
    assert model["cuts"] == [0, 2, 5, 7]
    model, _ = check_device(rt, batches, None, prm, BIG)
    assert model["cuts"] == [0, 6]
    model, _ = check_device(rt, batches, None, prm, 1)
    assert model["cuts"] == list(range(7))


def test_more_tables_than_one_partition_pass(rt, tile, prm):
    """150 one-row-or-more batches, each its own table: the partition runs three passes of 64 tables."""
    rng = random.Random(8)
    batches, seq = [], 1
    for _ in range(150):
        k = rng.randint(1, 9)
        batches.append(rand_rows(rng, k, seq0=seq, lo=1, hi=3))
        seq += k
    model, _ = check_device(rt, batches, None, prm, 1)
    assert len(model["tables"]) == 150


def test_metadata_columns(rt, tile, prm):
    """All four create_ts / expire_ts combinations on values, merge operands and tombstones, zero-length values
    among them."""
    shapes = [(kind, value, cts, ets) for cts in (None, -7, 1234) for ets in (None, 99)
              for kind, value in ((V, b"value"), (V, b""), (M, b"operand"), (M, b""), (T, b""))]
    random.Random(9).shuffle(shapes)
    rows = [(b"key-%02d" % (i * 37 % 100), kind, value, i + 1, cts, ets) for i, (kind, value, cts, ets) in enumerate(shapes)]
    model, _ = check_device(rt, [rows[:11], rows[11:]], None, prm, BIG)
    assert model["summary"]["val_bytes"] == sum(len(r[2]) for r in rows)


def test_long_rows(rt, tile, prm):
    """Keys past 64 bytes and values past 128: the gather's tail copies, next to rows that end inside its first step."""
    rng = random.Random(14)
    rows = []
    for i in range(300):
        key = rand_key(rng, *rng.choice([(1, 8), (60, 70), (64, 64), (65, 200)]))
        value = bytes(rng.randrange(256) for _ in range(rng.choice([0, 63, 64, 65, 127, 128, 129, 192, 193, 700])))
        rows.append((key, rng.choice([V, M]), value, 1 + i, rng.choice([None, i]), None))
    check_device(rt, [rows[:100], rows[100:]], None, prm, BIG)


def test_malformed_device_arrays(rt, tile, prm):
    """A descending batch_start and a table_batch_start that does not end at nbatches give the status through the
    summary, and nothing else is written."""
    import torch
    rng = random.Random(10)
    batches = [rand_rows(rng, 30, seq0=1), rand_rows(rng, 30, seq0=31), rand_rows(rng, 30, seq0=61)]
    run, start = as_run(batches)
    drun = rt.DeviceRun.from_host(run)
    w = rt.WalReplay(drun, [0, 60, 30, 90], fill=CANARY)
    _, sm = w.sort(None)
    assert (sm.status, sm.first_error_entry) == (_abi.SDB_INVALID_ARGUMENT, 1)
    assert untouched(w.facts_t)
    o, esm = w.emit([0, 3])
    assert esm.status == _abi.SDB_INVALID_ARGUMENT and all(untouched(o[k]) for k in o if k != "summary")
    w = rt.WalReplay(drun, [0, 30, 60, 89], fill=CANARY)  # does not end at n
    _, sm = w.sort(None)
    assert (sm.status, sm.first_error_entry) == (_abi.SDB_INVALID_ARGUMENT, 3)
    empty = rt.DeviceRun.from_host(as_run([])[0])  # no rows: every element of batch_start has to be 0
    w = rt.WalReplay(empty, [0, 0, 1], fill=CANARY)
    _, sm = w.sort(None)
    assert (sm.status, sm.first_error_entry) == (_abi.SDB_INVALID_ARGUMENT, 2) and untouched(w.facts_t)
    o, esm = w.emit([0, 2])
    assert esm.status == _abi.SDB_INVALID_ARGUMENT and untouched(o["table_row_start"])
    facts, sm = rt.WalReplay(empty, [0, 0, 0], fill=CANARY).sort(None)
    assert sm.status == 0 and [f.rows for f in facts] == [0, 0]
    w = rt.WalReplay(drun, start, fill=CANARY)
    _, sm = w.sort(None)
    assert sm.status == 0
    for cuts, bad in (([0, 1, 2], 2), ([1, 3], 0), ([0, 2, 1, 3], 1)):
        o, esm = w.emit(cuts)
        torch.cuda.synchronize()
        assert (esm.status, esm.first_error_entry) == (_abi.SDB_INVALID_ARGUMENT, bad), cuts
        assert all(untouched(o[k]) for k in o if k != "summary")
    o, esm = w.emit([0, 1, 3])  # and the workspace is still good for a well-formed call
    assert esm.status == 0 and [int(x) for x in o["table_row_start"].cpu().numpy()] == [0, 30, 90]


def test_short_capacities(rt, tile, prm):
    rng = random.Random(11)
    batches = [rand_rows(rng, 200, seq0=1)]
    run, start = as_run(batches)
    drun = rt.DeviceRun.from_host(run)
    w = rt.WalReplay(drun, start, fill=CANARY)
    _, sm = w.sort(None)
    assert sm.status == 0 and sm.rows_out == 200
    for kw in (dict(cap_entries=199), dict(val_cap=sm.val_bytes - 1), dict(key_cap=sm.key_bytes - 1)):
        o, esm = w.emit([0, 1], extra=64, **kw)
        assert esm.status == _abi.SDB_LIMIT_EXCEEDED, kw
        assert (esm.rows_out, esm.key_bytes, esm.val_bytes) == (200, sm.key_bytes, sm.val_bytes)  # the sizes needed
        assert all(untouched(o[k]) for k in o if k != "summary"), kw
    o, esm = w.emit([0, 1], cap_entries=200, key_cap=sm.key_bytes, val_cap=sm.val_bytes, extra=64)  # exact: fits
    assert esm.status == 0
    assert untouched(o["key_bytes"][sm.key_bytes:]) and untouched(o["val_bytes"][sm.val_bytes:])
    assert untouched(o["key_off"][201:]) and untouched(o["val_off"][201:]) and untouched(o["seq"][200:])
    assert untouched(o["kind"][200:]) and untouched(o["ts_mask"][200:]) and untouched(o["create_ts"][200:])


def test_workspace_canaries(rt, tile, prm):
    """A workspace of exactly sdb_wal_replay_workspace_bytes between guard bytes: the guards survive both calls,
    and a second pair of calls on the dirty workspace gives the same outputs."""
    import torch
    rng = random.Random(12)
    batches = [rand_rows(rng, tile + 7, seq0=1), [], rand_rows(rng, 2 * tile + 1, seq0=5000)]
    batches[2][900] = (batches[2][5][0], V, b"the later arrival", batches[2][5][3], None, None)  # a replaced pair
    run, start = as_run(batches)
    drun = rt.DeviceRun.from_host(run)
    need = rt.lib().sdb_wal_replay_workspace_bytes(run.n, 3)
    guard = 1024
    buf = torch.full((need + 2 * guard,), CANARY, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    w = rt.WalReplay(drun, start, workspace=buf)
    outs = []
    for _ in range(2):
        facts, sm = w.sort(10, ws_ptr=buf.data_ptr() + guard, ws_bytes=need)
        assert sm.status == 0
        cuts = replay.split_tables(facts, prm, 1)
        o, esm = w.emit(cuts, ws_ptr=buf.data_ptr() + guard, ws_bytes=need)
        torch.cuda.synchronize()
        assert esm.status == 0
        assert untouched(buf[:guard]) and untouched(buf[guard + need:])
        outs.append((bytes(w.facts_t.cpu().numpy()), bytes(w.summary_t.cpu().numpy()),
                     {k: o[k].cpu().numpy().tobytes() for k in o}))
    assert outs[0] == outs[1]
    st = rt.lib().sdb_wal_replay_sort(C.byref(w.run), w.bs.data_ptr(), 3, 0, 0, w.facts_t.data_ptr(), w.summary_t.data_ptr(),
                                      buf.data_ptr() + guard, need - 1, None)
    assert st == _abi.SDB_INVALID_ARGUMENT
    model = replay.replay_model(batches, 10, prm, 1)
    assert model["summary"]["rows_replaced"] == 1
    check_device(rt, batches, 10, prm, 1)


def test_end_to_end_wal_ssts_to_l0(rt, tile, prm):
    """Three WAL SSTs from the device encoder, decoded by sdb_decode_blocks_at into one run, replayed, and each
    table flushed by Compactor.run with one run and the retention flush.rs:223-232 builds: every L0 SST equals
    the oracle's compaction of the model's table byte for byte."""
    import torch
    from .test_gpu_compaction import sst_view
    from .test_gpu_parity import assert_same
    rng = random.Random(13)
    keys = [b"user%05d" % rng.randrange(3000) for _ in range(900)]
    batches, seq = [], 1
    for b in range(3):
        rows = []
        for k in keys[300 * b:300 * b + 300]:
            kind = rng.choice([V, V, V, T])
            rows.append((k, kind, b"" if kind == T else bytes(rng.randrange(256) for _ in range(rng.randint(0, 60))), seq,
                         rng.choice([None, 1000 + seq]), rng.choice([None, None, 10 ** 6 + seq])))
            seq += 1
        batches.append(rows)
    wal_prm = rt.params(block_size=1024, sst_type=_abi.SST_WAL, bloom_bits_per_key=0)
    enc = rt.Encoder(wal_prm)
    datas, bstart, bend, base = [], [], [], 0
    for rows in batches:
        e = enc.encode(Batch.from_entries(rows))
        assert e.status == 0
        datas.append(e.data)
        bstart += [base + int(x) for x in e.block_off[:-1]]
        bend += [base + int(x) for x in e.block_off[1:]]
        base += len(e.data)
    enc.close()
    arena = torch.from_numpy(np.concatenate(datas + [np.zeros(64, np.uint8)])).cuda()
    nblocks = len(bstart)
    dout = rt.DeviceDecodeOutput(nblocks, 900 + 16, sum(len(k) for k in keys) + 64)
    rt.decode_blocks_at_device(arena, torch.tensor(bstart, dtype=torch.int64, device="cuda"),
                               torch.tensor(bend, dtype=torch.int64, device="cuda"), nblocks, dout, 2)
    torch.cuda.synchronize()
    assert dout.summary_host().status == 0 and dout.summary_host().num_entries == 900
    drun = rt.DeviceRun.from_decoded(dout, arena, 900)
    size = replay.row_estimated_size
    limit = replay.estimate_encoded_size_compacted(prm, 300, sum(size(r) for r in batches[0]))
    model = replay.replay_model(batches, 100, prm, limit, wal_ids=[7, 8, 9])
    assert len(model["tables"]) >= 2
    tables = rt.wal_replay_device(drun, [0, 300, 600, 900], 100, prm, limit, wal_ids=[7, 8, 9])
    assert len(tables) == len(model["tables"])
    comp = rt.Compactor()
    sst_kw = dict(block_size=4096, bloom_bits_per_key=10)
    for got, want in zip(tables, model["tables"]):
        for f in ("entry_num", "entries_size_in_bytes", "first_seq", "last_seq", "last_tick", "replay_last_seq",
                  "replay_last_tick", "last_wal_id", "batches"):
            assert got.meta[f] == want[f], f
        ret = O.retention(min_seq=450, compaction_start_ts=want["last_tick"], filter_tombstone=False)
        st, ns = comp.run([got.as_run()], ret, rt.params(**sst_kw), 1 << 40)
        torch.cuda.synchronize()
        _, msum, _, ssts = O.compact([Run.from_entries(want["rows"])], ret, O.params(**sst_kw), 1 << 40)
        assert st == msum.status == 0 and ns == len(ssts) == 1
        assert_same(ssts[0], sst_view(comp.sst(0)), "L0 of table %s" % (want["batches"],))
    comp.close()
