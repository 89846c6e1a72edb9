"""GPU parity of the compaction filter and the resume cursor (sdb_compactor_run_filtered, _run_ssts_filtered; k_cf_size,
k_cf_scan, k_cf_emit, k_cf_seek and k_cf_drain in sdb_compact_filter.hip, filter_step and seek_runs in
sdb_compactor.cpp, the cursor's bound in k_rx_cover) against rules F1-F10 and S1-S3 of include/slatedb_amd.h as
tests/compaction_filter_cases.py restates them in front of the pinned C oracle: the final stream field by field, every
output SST byte for byte, filter_stats() word for word and the recorded filter calls, for both entry points."""
import copy
import ctypes as C
import struct

import numpy as np
import pytest

from oracle import oracle as O
from slatedb_amd import _abi
from slatedb_amd import compaction_filter as CF
from slatedb_amd.batch import Run

from . import compaction_filter_cases as F
from . import ranged_compaction_cases as R
from .compaction_merge_cases import Bracket
from .test_gpu_compaction import sst_view
from .test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu
V, M, T = F.V, F.M, F.T
OUT = dict(block_size=512, bloom_bits_per_key=10)
MAX_SST = 32 << 10
SUMMARY = ("num_out", "key_bytes", "val_bytes", "expired_values", "expired_merges")
LENS = [0, 1, 15, 16, 17, 127, 128, 129, 300]  # the chunk copy's edges: 16 bytes per lane, 128 per step
PATHS = ("runs", "ssts")
SST_FIELDS = ("data", "block_off", "block_first_entry", "index_key_len", "block_stats", "bloom")


@pytest.fixture(scope="module")
def rt():
    from slatedb_amd import runtime
    runtime.require_device()
    return runtime


@pytest.fixture(scope="module")
def comp(rt):
    c = rt.Compactor()
    yield c
    c.close()


def keep_all_versions():
    return O.retention(min_seq=0)  # every seq lies above it: retention passes every version on


def make_rows(n):
    """n rows in stream order: one 1-byte key, then keys and values whose lengths walk LENS next to each other; every
    50th key has three versions; some rows are tombstones, some carry a create_ts, an expire_ts (never expired) or
    both."""
    rows = [(b"\x00", V, b"v", 1, None, None)] if n else []
    i = 1
    while len(rows) < n:
        key = struct.pack(">I", i) + bytes([i * 7 & 255]) * (max(4, LENS[i % 9]) - 4)
        for v in range(3 if i % 50 == 10 else 1):
            if len(rows) < n:
                tomb = i % 19 == 7
                val = b"" if tomb else (bytes([i & 255, (i >> 8) & 255, v]) * 100)[:LENS[(2 * i + v + 3) % 9]]
                rows.append((key, T if tomb else V, val, 3 * i + 3 - v, i if i % 3 == 0 else None,
                             10 ** 6 + i if i % 5 == 0 and not tomb else None))
        i += 1
    return rows


def split_runs(rows, k=2):
    runs = [[] for _ in range(k)]
    for j, e in enumerate(rows):
        runs[(j // 3) % k].append(e)
    return [r for r in runs if r]


_JOBS = {}


def inputs_of(runs, key):
    """The runs as encoded input SSTs on the device (built once per `key`)."""
    if key not in _JOBS:
        job = R.build_job([Run.from_entries(r) for r in runs], dict(block_size=256))
        _JOBS[key] = (job, R.upload(job))
    return _JOBS[key]


class ByIndex:
    """A stateful per-entry filter: rule(i, entry) for the i-th row it is shown."""

    def __init__(self, rule, end_error=False):
        self.rule, self.i, self.ended, self.end_error = rule, 0, 0, end_error

    def __call__(self, e):
        d = self.rule(self.i, e)
        self.i += 1
        return d

    filter = __call__

    def on_compaction_end(self):
        self.ended += 1
        if self.end_error:
            raise F.FilterError("end")


class Recording(CF.BatchFilter):
    """The device side of a per-entry filter: what every call showed it."""

    def __init__(self, fn, batch_rows=0, want_values=False):
        self.fn, self.batch_rows, self.want_values = fn, batch_rows, want_values
        self.calls, self.seen, self.had_values = [], [], []

    def filter_batch(self, rows):
        self.calls.append((rows.first, rows.n))
        self.had_values.append(rows.val_bytes is not None)
        dec, vals = np.zeros(rows.n, np.uint8), {}
        for i in range(rows.n):
            e = rows.entry(i)
            self.seen.append(tuple(e))
            r = self.fn(e)
            if isinstance(r, tuple):
                dec[i], vals[i] = r
            else:
                dec[i] = r
        return dec, vals

    def on_compaction_end(self):
        self.fn.on_compaction_end()


def mixed(i, e):
    if i % 7 == 3:
        return (CF.VALUE, bytes([i & 255]) * LENS[(i // 7) % 9])
    if i % 11 == 5:
        return CF.DROP
    if i % 13 == 2 or (e[5] is not None and i % 4 == 1):  # (rows that carry an expire_ts among them)
        return CF.TOMBSTONE
    if i % 17 == 1:
        return (CF.MERGE, b"m%d" % i)
    return CF.KEEP


def device_job(rt, comp, runs, path, ret, flt=None, cursor=None, op=None, key=None, inputs=None, job_range=None):
    import torch
    prm = rt.params(**OUT)
    if path == "runs":
        druns = [rt.DeviceRun.from_host(Run.from_entries(r)) for r in runs]
        res = comp.run_filtered(druns, ret, prm, MAX_SST, flt, cursor, operator=op)
    else:
        job, ins = inputs_of(runs, key)
        res = comp.run_ssts_filtered(inputs or ins, ret, prm, MAX_SST, flt, cursor, job_range=job_range, operator=op,
                                     input_version=job.version, run_start=job.run_start)
    torch.cuda.synchronize()
    return res


def check(rt, comp, runs, path, mk=None, batch_rows=0, want_values=False, cursor=None, op=None, ret=None, key=None,
          what=""):
    """One job on the device against the model; returns (model result, device filter, final stream entries)."""
    ret = ret or keep_all_versions()
    what = "%s %s" % (what, path)
    if path == "ssts":  # the model reads what the inputs decode to
        job, _ = inputs_of(runs, key)
        runs = [sum((R.run_entries(job.inputs[i].ref) for i in range(job.run_start[r], job.run_start[r + 1])), [])
                for r in range(len(job.run_start) - 1)]
    want = F.expected(runs, ret, O.params(**OUT), MAX_SST, mk() if mk else None, batch_rows, want_values, cursor, op)
    dev = Recording(mk(), batch_rows, want_values) if mk else None
    st, ns = device_job(rt, comp, runs, path, ret, dev, cursor, op, key)
    assert st == want["status"], (what, st, want["status"])
    gm, gsm = comp.merged()
    assert gsm.status == st, what
    fs = comp.filter_stats()
    got_stats = {f: getattr(fs, f) for f in F.STATS}
    if dev:  # F8: the calls and the rows they showed
        assert dev.calls == want["calls"], (what, dev.calls[:5], want["calls"][:5])
        seen = [e if want_values else e[:2] + (None,) + e[3:] for e in want["seen"]]
        assert dev.seen == seen, what
        assert all(h == bool(want_values) for h in dev.had_values), what
    if st:
        assert ns == 0 and gsm.first_error_entry == want["first_error_entry"], (what, gsm.first_error_entry)
        return want, dev, None
    assert got_stats == want["stats"], (what, got_stats, want["stats"])
    for f in SUMMARY:  # F10: the summary stays retention's
        assert getattr(gsm, f) == getattr(want["sm"], f), (what, f)
    if op is None:
        assert gsm.num_in == want["sm"].num_in, what
    got = F.batch_entries(gm)
    assert len(got) == len(want["stream"]), (what, len(got), len(want["stream"]))
    for i, (a, b) in enumerate(zip(got, want["stream"])):
        assert a == b, (what, i, a[:2], b[:2], a[3:], b[3:], len(a[2]), len(b[2]))
    assert ns == len(want["ssts"]), (what, ns, len(want["ssts"]))
    for i, ref in enumerate(want["ssts"]):
        d = comp.sst(i)
        assert (d["entry_start"], d["entry_end"]) == (want["cuts"][i], want["cuts"][i + 1]), what
        assert_same(ref, sst_view(d), "%s sst %d" % (what, i))
    if dev:
        assert dev.fn.ended == 1, what  # F8: `end` once
    return want, dev, got


def raw_ssts(comp, ns):
    return [comp.sst(i) for i in range(ns)]


def assert_ssts_identical(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert (x["entry_start"], x["entry_end"]) == (y["entry_start"], y["entry_end"])
        for f in SST_FIELDS:
            assert np.array_equal(x[f], y[f]), f
        assert bytes(x["summary"]) == bytes(y["summary"])


# ---- 1. row counts and copy lengths ------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2100])
def test_row_counts(rt, comp, n, path):
    """kMergeTile edges and three tiles, under a filter that drops, tombstones and rewrites (a replacement every 7th
    row, so the replacement ranks cross the tile edges), keys and values of every chunk-copy edge length."""
    rows = make_rows(n)
    want, dev, got = check(rt, comp, split_runs(rows), path, lambda: ByIndex(mixed), key=("rows", n), what="n=%d" % n)
    st = want["stats"]
    assert st["rows_in"] == n and st["calls"] == 1
    if n >= 1023:
        assert st["applied"] == 1 and st["new_values"] >= n // 7 and st["new_merges"] and st["dropped"] and st["tombstoned"]
        assert {len(e[0]) for e in got} >= {1, 4, 15, 16, 17, 127, 128, 129, 300}
        assert {len(e[2]) for e in got} >= set(LENS)
        # F3 on rows that carried both timestamps: the create_ts stays, the expire_ts goes
        was = {(e[0], e[3]): e for e in want["seen"]}
        tomb = [e for e in got if e[1] == T and was[(e[0], e[3])][1] == V and was[(e[0], e[3])][5] is not None]
        assert tomb and all(e[5] is None and e[4] == was[(e[0], e[3])][4] for e in tomb) and any(e[4] is not None for e in tomb)
        assert any(e[1] == M for e in got)  # F4: a Merge written in a job without an operator


@pytest.mark.parametrize("path", PATHS)
def test_no_rows(rt, comp, path):
    """A stream of no rows: no call, `end` still runs (F5), no SST."""
    rows = make_rows(40)
    if path == "runs":
        want, dev, got = check(rt, comp, [], path, lambda: ByIndex(mixed), what="empty")
    else:  # an empty job range over real inputs
        dev = Recording(ByIndex(mixed))
        st, ns = device_job(rt, comp, split_runs(rows), path, keep_all_versions(), dev, key=("rows", 40),
                            job_range=(b"\x09", 1, b"\x01", 1))
        assert (st, ns) == (0, 0) and dev.fn.ended == 1
        want, got = None, F.batch_entries(comp.merged()[0])
    fs = comp.filter_stats()
    assert got == [] and dev.calls == [] and dev.fn.ended == 1
    assert all(getattr(fs, f) == 0 for f in F.STATS)


# ---- 2. decisions ------------------------------------------------------------------------------------------------
N3 = 2100
DECISIONS = {
    "drop the first row": lambda i, e: CF.DROP if i == 0 else CF.KEEP,
    "drop the last row": lambda i, e: CF.DROP if i == N3 - 1 else CF.KEEP,
    "drop a whole tile": lambda i, e: CF.DROP if 1024 <= i < 2048 else CF.KEEP,
    "drop everything": lambda i, e: CF.DROP,
    "drop every row but one": lambda i, e: CF.KEEP if i == 1500 else CF.DROP,
    "modified rows at the tile edges": lambda i, e: (CF.VALUE, b"edge%d" % i * (i % 5)) if i in (1023, 1024, 2047, 2048) else CF.KEEP,
}


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(DECISIONS))
def test_decisions(rt, comp, name, path):
    rows = make_rows(N3)
    want, dev, got = check(rt, comp, split_runs(rows), path, lambda: ByIndex(DECISIONS[name]), key=("rows", N3), what=name)
    if name == "drop everything":  # F10: like an empty merge
        assert got == [] and want["stats"]["applied"] == 0 and want["stats"]["dropped"] == N3
    elif name == "drop every row but one":
        assert len(got) == 1 and got[0][:4] == rows[1500][:4]
    else:
        assert want["stats"]["applied"] == 1 and len(got) >= N3 - 1024


@pytest.mark.parametrize("path", PATHS)
def test_value_rewrites(rt, comp, path):
    """F4: an empty replacement, a shorter one (300 -> 1), a longer one (1 -> 300), one on a tombstone (which keeps its
    'no expire_ts'), and a MERGE; F3 next to them."""
    rows = [(b"a", V, b"A" * 300, 9, 5, 10 ** 6), (b"b", V, b"B", 8, None, 10 ** 6 + 1), (b"c", V, b"C" * 50, 7, 3, None),
            (b"d", T, b"", 6, 4, None), (b"e", V, b"E" * 17, 5, None, None), (b"f", V, b"F" * 16, 4, 2, 10 ** 6 + 2),
            (b"g", V, b"G" * 129, 3, None, None)]
    by_key = {b"a": (CF.VALUE, b"x"), b"b": (CF.VALUE, b"y" * 300), b"c": (CF.VALUE, b""), b"d": (CF.VALUE, b"revived"),
              b"e": (CF.MERGE, b"operand"), b"f": CF.TOMBSTONE, b"g": CF.KEEP}
    want, dev, got = check(rt, comp, [rows[::2], rows[1::2]], path, lambda: ByIndex(lambda i, e: by_key[e[0]]),
                           want_values=True, key="rewrites", what="rewrites")
    assert got == [(b"a", V, b"x", 9, 5, 10 ** 6), (b"b", V, b"y" * 300, 8, None, 10 ** 6 + 1), (b"c", V, b"", 7, 3, None),
                   (b"d", V, b"revived", 6, 4, None), (b"e", M, b"operand", 5, None, None), (b"f", T, b"", 4, 2, None),
                   (b"g", V, b"G" * 129, 3, None, None)]


# ---- 3. batching and keep-all ------------------------------------------------------------------------------------
def test_batching(rt, comp):
    """batch_rows 1, 7, 1024 and 0 under a stateful filter (it drops every third row it is shown): identical results,
    ascending contiguous calls, `end` once."""
    rows = make_rows(N3)
    streams = []
    for path, batch in (("runs", 1), ("runs", 7), ("runs", 1024), ("runs", 0), ("ssts", 7), ("ssts", 0)):
        mk = lambda: ByIndex(lambda i, e: CF.DROP if i % 3 == 2 else CF.KEEP)  # noqa: E731
        want, dev, got = check(rt, comp, split_runs(rows), path, mk, batch_rows=batch, key=("rows", N3), what="batch %d" % batch)
        step = batch or N3
        assert dev.calls == [(f, min(step, N3 - f)) for f in range(0, N3, step)]
        streams.append(got)
    assert all(s == streams[0] for s in streams) and len(streams[0]) == N3 - N3 // 3


@pytest.mark.parametrize("path", PATHS)
def test_keep_all(rt, comp, path):
    """F7: nothing uploaded, no apply kernel, and the bytes of the job without a filter; want_values decides whether
    the value bytes travel."""
    import torch
    rows = make_rows(1500)
    runs = split_runs(rows)
    ret, prm = keep_all_versions(), rt.params(**OUT)
    if path == "runs":
        st, ns = comp.run([rt.DeviceRun.from_host(Run.from_entries(r)) for r in runs], ret, prm, MAX_SST)
    else:
        job, ins = inputs_of(runs, ("rows", 1500))
        st, ns = comp.run_ssts_ranged(ins, ret, prm, MAX_SST, run_start=job.run_start)
    torch.cuda.synchronize()
    assert st == 0 and ns >= 2
    plain, plain_ssts = comp.merged(), raw_ssts(comp, ns)
    d2h = []
    for wv in (False, True):
        want, dev, got = check(rt, comp, runs, path, lambda: ByIndex(lambda i, e: CF.KEEP), want_values=wv,
                               key=("rows", 1500), what="keep-all")
        fs = comp.filter_stats()
        assert (fs.h2d_bytes, fs.applied, fs.kept, fs.rows_in) == (0, 0, 1500, 1500)
        gm, gsm = comp.merged()
        for f in ("key_bytes", "key_off", "val_bytes", "val_off", "kind", "seq", "create_ts", "expire_ts", "ts_mask"):
            assert np.array_equal(getattr(gm, f), getattr(plain[0], f)), f
        assert bytes(gsm) == bytes(plain[1])
        assert_ssts_identical(raw_ssts(comp, ns), plain_ssts)
        d2h.append(fs.d2h_bytes)
    assert d2h[1] - d2h[0] == plain[1].val_bytes > 0


# ---- 4. retention and operator interplay -------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_filter_tombstone_survives_last_run(rt, comp, path):
    """F3 with filter_tombstone = 1: retention has already dropped the stored tombstones; the filter's stay."""
    rows = make_rows(300)
    ret = O.retention(min_seq=0, filter_tombstone=True)
    want, dev, got = check(rt, comp, split_runs(rows), path, lambda: ByIndex(lambda i, e: CF.TOMBSTONE if i % 4 == 0 else CF.KEEP),
                           ret=ret, key=("rows", 300), what="last run")
    assert all(e[1] != T for e in want["seen"]) and sum(e[1] == T for e in got) == (len(want["seen"]) + 3) // 4


@pytest.mark.parametrize("path", PATHS)
def test_filter_sees_the_collapsed_units(rt, comp, path):
    import random
    from .test_compaction_oracle import rand_runs
    runs = [r for r in rand_runs(random.Random(5), 3, 400, 4, tomb=0.1, merge=0.5, expire=0.0) if r]
    ret = O.retention(min_seq=900, filter_tombstone=False)
    mk = lambda: ByIndex(lambda i, e: (CF.VALUE, b"<" + e[2] + b">") if e[1] == V and i % 3 == 0 else (CF.DROP if i % 10 == 9 else CF.KEEP))  # noqa: E731
    want, dev, got = check(rt, comp, runs, path, mk, want_values=True, op=Bracket, ret=ret, key="operator", what="operator")
    assert comp.merge_stats().groups > 10
    assert any(e[2].startswith(b"<(") for e in got)  # a rewritten value that the operator had merged
    assert len(want["seen"]) < sum(len(r) for r in runs)


# ---- 5. failures (F9) --------------------------------------------------------------------------------------------
def raw_filter(decide):
    """An sdb_compaction_filter whose callback is `decide(n, decision, new_val, new_len)`, and an `end` counter."""
    state = {"ended": 0}

    def call(ctx, rows, first, decision, new_val, new_len):
        return decide(int(rows.contents.n), decision, new_val, new_len) or 0

    def end(ctx):
        state["ended"] += 1
        return 0
    return _abi.CompactionFilter(_abi.COMPACTION_FILTER_FN(call), _abi.COMPACTION_END_FN(end), None, 0, 0, 0), state


@pytest.mark.parametrize("path", PATHS)
def test_failures(rt, comp, path):
    rows = make_rows(300)
    runs, key = split_runs(rows), ("rows", 300)

    def fail_at(k):
        def rule(i, e):
            if i == k:
                raise F.FilterError("row %d" % k)
            return CF.DROP if i % 2 else CF.KEEP
        return rule
    # a failing call: first_error_entry = `first` of that call, no SST, no `end`
    want, dev, _ = check(rt, comp, runs, path, lambda: ByIndex(fail_at(100)), batch_rows=7, key=key, what="filter error")
    assert want["status"] == _abi.SDB_COMPACTION_FILTER_ERROR and want["first_error_entry"] == 98 and dev.fn.ended == 0
    assert isinstance(comp.filter_state["error"], F.FilterError)
    check(rt, comp, runs, path, lambda: ByIndex(mixed), key=key, what="after a filter error")
    # a failing `end`: first_error_entry = rows_in
    want, dev, _ = check(rt, comp, runs, path, lambda: ByIndex(mixed, end_error=True), key=key, what="end error")
    assert want["status"] == _abi.SDB_COMPACTION_FILTER_ERROR and want["first_error_entry"] == 300 and dev.fn.ended == 1
    check(rt, comp, runs, path, lambda: ByIndex(mixed), key=key, what="after an end error")

    # what a callback may not return: found on the host, nothing uploaded, no `end`
    def bad_decision(n, decision, new_val, new_len):
        decision[n // 2] = 5

    def null_value(n, decision, new_val, new_len):
        decision[3] = CF.VALUE
        new_len[3] = 4
    for decide, row in ((bad_decision, 150), (null_value, 3)):
        cf, state = raw_filter(decide)
        st, ns = device_job(rt, comp, runs, path, keep_all_versions(), cf, key=key)
        sm, fs = comp.merged()[1], comp.filter_stats()
        assert (st, ns, sm.status, sm.first_error_entry) == (_abi.SDB_INVALID_ARGUMENT, 0, _abi.SDB_INVALID_ARGUMENT, row)
        assert (fs.h2d_bytes, fs.applied, state["ended"]) == (0, 0, 0)
        check(rt, comp, runs, path, lambda: ByIndex(mixed), key=key, what="after a bad return")
    # an empty replacement with a NULL pointer is legal
    def null_empty(n, decision, new_val, new_len):
        decision[3] = CF.VALUE
    cf, state = raw_filter(null_empty)
    assert device_job(rt, comp, runs, path, keep_all_versions(), cf, key=key)[0] == 0 and state["ended"] == 1
    assert F.batch_entries(comp.merged()[0])[3][:3] == (rows[3][0], V, b"")
    # F9 from the call: a filter without a callback, a cursor whose key is NULL with key_len > 0; alone and together
    good = lambda: Recording(ByIndex(mixed))  # noqa: E731
    for flt, cur in ((_abi.CompactionFilter(), None), (None, _abi.ResumeCursor(None, 3, 0)),
                     (good(), _abi.ResumeCursor(None, 1, 7)), (_abi.CompactionFilter(), (rows[5][0], 0))):
        assert device_job(rt, comp, runs, path, keep_all_versions(), flt, cur, key=key) == (_abi.SDB_INVALID_ARGUMENT, 0)
        assert flt is None or isinstance(flt, _abi.CompactionFilter) or (flt.calls == [] and flt.fn.ended == 0)
        check(rt, comp, runs, path, lambda: ByIndex(mixed), cursor=(rows[5][0], 0), key=key, what="after a bad argument")


class NullColumn:
    """A device run whose sdb_run lacks one column."""

    def __init__(self, drun, field):
        self.d, self.field = drun, field

    def to_ctypes(self):
        r = self.d.to_ctypes()
        setattr(r, self.field, None)
        return r


@pytest.mark.parametrize("field", ["key_arena", "key_off", "val_off", "val_len", "seq", "flags"])
def test_resumed_job_checks_its_runs_first(rt, comp, field):
    """A run with n > 0 and a NULL column is SDB_INVALID_ARGUMENT from the host, with a cursor as without one: the
    cursor's seek over the runs' keys is not launched."""
    rows = make_rows(300)
    runs = split_runs(rows)
    druns = [rt.DeviceRun.from_host(Run.from_entries(r)) for r in runs]
    bad = [druns[0], NullColumn(druns[1], field)]
    ret, prm = keep_all_versions(), rt.params(**OUT)
    for cur in (None, (rows[100][0], 0)):
        assert comp.run_filtered(bad, ret, prm, MAX_SST, None, cur) == (_abi.SDB_INVALID_ARGUMENT, 0)
        assert comp.run_filtered(bad, ret, prm, MAX_SST, Recording(ByIndex(mixed)), cur) == (_abi.SDB_INVALID_ARGUMENT, 0)
    check(rt, comp, runs, "runs", lambda: ByIndex(mixed), cursor=(rows[100][0], 0), what="after a NULL column")


def test_packed_replacements(rt, comp):
    """The packed form of a batch filter's replacements (one arena and m + 1 offsets per call) against the per-row
    form: the same stream and the same filter_stats, across several calls."""
    rows = make_rows(1100)
    runs = split_runs(rows)

    def rule(i, e):
        return (CF.VALUE if i % 2 else CF.MERGE, bytes([i & 255]) * LENS[(i // 7) % 9]) if i % 7 == 3 else (CF.DROP if i % 11 == 5 else CF.KEEP)

    class Packed(CF.BatchFilter):
        batch_rows = 256

        def filter_batch(self, rows_):
            out = [rule(rows_.first + i, None) for i in range(rows_.n)]
            dec = np.array([d[0] if isinstance(d, tuple) else d for d in out], np.uint8)
            vals = [d[1] for d in out if isinstance(d, tuple)]
            off = np.concatenate([[0], np.cumsum([len(v) for v in vals])]).astype(np.uint64)
            return dec, (np.frombuffer(b"".join(vals), np.uint8), off)
    want, dev, got = check(rt, comp, runs, "runs", lambda: ByIndex(rule), batch_rows=256, what="per-row form")
    st, ns = device_job(rt, comp, runs, "runs", keep_all_versions(), Packed())
    assert (st, ns) == (0, len(want["ssts"])) and comp.filter_state["error"] is None
    fs = comp.filter_stats()
    assert {f: getattr(fs, f) for f in F.STATS} == want["stats"] and fs.new_values and fs.new_merges
    assert F.batch_entries(comp.merged()[0]) == got


# ---- 6. cursors --------------------------------------------------------------------------------------------------
def cursor_rows():
    rows = make_rows(300)
    keys = [e[0] for e in rows]
    k3 = next(k for k in keys if keys.count(k) == 3 and keys.index(k) > 100)  # a key with three versions
    seqs = [e[3] for e in rows if e[0] == k3]
    assert len(seqs) == 3 and seqs == sorted(seqs, reverse=True)
    return rows, k3, seqs


def cursors():
    rows, k3, seqs = cursor_rows()
    between = rows[150][0] + b"\x00"
    assert rows[150][0] < between < rows[151][0]
    return {
        "K below every key": (b"", 0),
        "K the first row's key": (rows[0][0], rows[0][3]),
        "three versions, S above all": (k3, seqs[0] + 1),
        "three versions, S the middle": (k3, seqs[1]),
        "three versions, S 0": (k3, 0),
        "K absent between two keys": (between, 5),
        "K above every key": (b"\xff" * 9, 0),
    }


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", list(cursors()))
def test_cursor(rt, comp, name, path):
    rows, k3, seqs = cursor_rows()
    cur = cursors()[name]
    want, _, got = check(rt, comp, split_runs(rows), path, cursor=cur, key=("rows", 300), what=name)
    drained = {"K below every key": 0, "K the first row's key": 1, "three versions, S above all": 0,
               "three versions, S the middle": 2, "three versions, S 0": 3, "K absent between two keys": 0,
               "K above every key": 0}[name]
    assert want["stats"]["resume_drained"] == drained
    first = {"K below every key": 0, "K the first row's key": 1, "K absent between two keys": 151}.get(name)
    if name == "K above every key":
        assert got == [] and want["sm"].num_in == 0
    elif first is not None:
        assert got[0][:4] == rows[first][:4] and len(got) == 300 - first
    else:
        i3 = [e[0] for e in rows].index(k3)
        assert got[0][:4] == rows[i3 + drained][:4] and want["sm"].num_in == 300 - i3  # S1: nothing below K is read


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", F.FIXTURE["resume_cases"], ids=lambda c: c["name"])
def test_reference_resume_case(rt, comp, case, path):
    runs, ret, op, cursor, want_rows = F.resume_case(case)
    want, _, got = check(rt, comp, runs, path, cursor=cursor, op=op, ret=ret, key=("ref", case["name"]), what=case["name"])
    assert [(e[0], e[1], e[2], e[3], e[5]) for e in got or []] == [(e[0], e[1], e[2], e[3], e[5]) for e in want_rows]


@pytest.mark.parametrize("path", PATHS)
def test_resume_matches_full(rt, comp, path):
    """Cursors at five positions of a full job's stream give exactly its tail."""
    rows, k3, seqs = cursor_rows()
    runs = split_runs(rows)
    assert device_job(rt, comp, runs, path, keep_all_versions(), key=("rows", 300))[0] == 0
    full = F.batch_entries(comp.merged()[0])
    assert [e[:4] for e in full] == [e[:4] for e in rows]
    i3 = [e[0] for e in rows].index(k3)
    for pos in (0, i3, i3 + 2, len(full) - 2, len(full) - 1):
        st, ns = device_job(rt, comp, runs, path, keep_all_versions(), cursor=(full[pos][0], full[pos][3]), key=("rows", 300))
        assert st == 0 and (ns == 0) == (pos == len(full) - 1)
        assert F.batch_entries(comp.merged()[0]) == full[pos + 1:], pos


def test_laziness(rt, comp):
    """S1 in the ssts job: an input whose first block is corrupt, K inside its third block: the resumed job never
    reads that block; the unresumed one fails on it."""
    import torch
    job = R.small_job()
    inputs = [copy.copy(x) for x in R.upload(job)]
    inputs[0].data = inputs[0].data.clone()
    inputs[0].data[int(inputs[0].block_off[0].item()) + 10] ^= 0x5A
    x = job.inputs[0]
    lo, hi = int(x.first_row[2]), int(x.first_row[3])
    K = next(x.keys[j] for j in range(lo + 1, hi) if x.keys[j] != x.keys[lo])  # inside the third block, not its first key
    assert x.ikeys[2] < K
    ret, prm = O.retention(min_seq=3000, compaction_start_ts=1000, filter_tombstone=True), rt.params(**OUT)
    st, ns = comp.run_ssts_filtered(inputs, ret, prm, R.MAX_SST, None, None, run_start=job.run_start)
    assert (st, ns) == (_abi.SDB_CHECKSUM_MISMATCH, 0) and comp.merged()[1].first_error_entry == 0
    st, ns = comp.run_ssts_filtered(inputs, ret, prm, R.MAX_SST, None, (K, 1 << 62), run_start=job.run_start)
    torch.cuda.synchronize()
    assert st == 0 and ns >= 1
    runs = [sum((R.run_entries(job.inputs[i].ref) for i in range(job.run_start[r], job.run_start[r + 1])), [])
            for r in range(len(job.run_start) - 1)]
    want = F.expected(runs, ret, O.params(**OUT), R.MAX_SST, cursor=(K, 1 << 62))
    assert F.batch_entries(comp.merged()[0]) == want["stream"] and ns == len(want["ssts"])
    rs = comp.range_stats()
    assert rs.blocks_checked < rs.blocks_total and rs.entries_in == want["sm"].num_in
    for i, ref in enumerate(want["ssts"]):
        assert_same(ref, sst_view(comp.sst(i)), "lazy sst %d" % i)


@pytest.mark.parametrize("path", PATHS)
def test_filter_with_cursor(rt, comp, path):
    """The rows shown are exactly the retained rows with key >= K, the drained ones included; a drained row's
    replacement is not applied to anything."""
    rows, k3, seqs = cursor_rows()
    i3 = [e[0] for e in rows].index(k3)

    def rule(i, e):  # the first row shown is rewritten, the second dropped: the drain passes over both
        return (CF.VALUE, b"drained") if i == 0 else (CF.DROP if i == 1 else mixed(i, e))
    want, dev, got = check(rt, comp, split_runs(rows), path, lambda: ByIndex(rule), batch_rows=64, cursor=(k3, seqs[2]),
                           key=("rows", 300), what="filter and cursor")
    assert [e[:2] + e[3:] for e in dev.seen] == [e[:2] + e[3:] for e in rows[i3:]]
    assert want["stats"]["resume_drained"] == 2 and want["stats"]["rows_in"] == 300 - i3
    assert got[0][0] > k3 and all(e[2] != b"drained" for e in got)
    # keep-all with a cursor: F7 holds and the stream starts behind the drained rows
    want, dev, got = check(rt, comp, split_runs(rows), path, lambda: ByIndex(lambda i, e: CF.KEEP), cursor=(k3, seqs[1]),
                           key=("rows", 300), what="keep-all and cursor")
    assert (want["stats"]["applied"], want["stats"]["resume_drained"]) == (0, 2) and got[0][:4] == rows[i3 + 2][:4]


# ---- 7. identity (F6) --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", [None, Bracket])
def test_identity(rt, comp, op):
    """Both entry points with NULL, NULL against the existing calls on the same inputs."""
    import random
    import torch
    from .test_compaction_oracle import rand_runs
    runs = [r for r in rand_runs(random.Random(9), 3, 500, 4, tomb=0.1, merge=0.4 if op else 0.0, expire=0.1) if r]
    ret, prm = O.retention(min_seq=700, compaction_start_ts=900, filter_tombstone=True), rt.params(**OUT)
    druns = [rt.DeviceRun.from_host(Run.from_entries(r)) for r in runs]
    job, ins = inputs_of(runs, ("identity", op is None))
    kw = dict(run_start=job.run_start)
    pairs = [(lambda: comp.run_merge(druns, ret, op, prm, MAX_SST) if op else comp.run(druns, ret, prm, MAX_SST),
              lambda: comp.run_filtered(druns, ret, prm, MAX_SST, operator=op)),
             (lambda: comp.run_ssts_ranged(ins, ret, prm, MAX_SST, operator=op, **kw),
              lambda: comp.run_ssts_filtered(ins, ret, prm, MAX_SST, operator=op, **kw))]
    for old, new in pairs:
        res = []
        for call in (old, new):
            st, ns = call()
            torch.cuda.synchronize()
            assert st == 0 and ns >= 1
            fs = comp.filter_stats()
            assert all(getattr(fs, f) == 0 for f in F.STATS)
            res.append((ns, comp.merged(), raw_ssts(comp, ns), bytes(comp.merge_stats()), bytes(comp.range_stats())))
        a, b = res
        assert a[0] == b[0] and bytes(a[1][1]) == bytes(b[1][1]) and a[3:] == b[3:]
        for f in ("key_bytes", "key_off", "val_bytes", "val_off", "kind", "seq", "create_ts", "expire_ts", "ts_mask"):
            assert np.array_equal(getattr(a[1][0], f), getattr(b[1][0], f)), f
        assert_ssts_identical(a[2], b[2])
