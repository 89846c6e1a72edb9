"""The model of a compaction with a compaction filter and / or a resume cursor: rules F1-F5, F7-F10 and S1-S3 of
include/slatedb_amd.h restated literally over the stream the pinned C oracle's merge yields (O.merge_runs; with an
operator the stream of compaction_merge_cases.collapse through it), in front of O.sst_cuts and O.encode_sst, which
still cut and encode the final stream.

Entries are (key, kind, value, seq, create_ts, expire_ts) as everywhere in the tests; a run is a list of them, key
ascending and seq descending.  A filter is a callable entry -> KEEP | DROP | TOMBSTONE | (VALUE, b) | (MERGE, b) that
may raise FilterError; it may carry an on_compaction_end().  A cursor is (key, seq)."""
import json
import os

from oracle import oracle as O
from slatedb_amd import _abi
from slatedb_amd.batch import Batch, Run
from slatedb_amd.compaction_filter import DROP, KEEP, MERGE, TOMBSTONE, VALUE

from . import compaction_merge_cases as CM

V, M, T = _abi.KIND_VALUE, _abi.KIND_MERGE, _abi.KIND_TOMBSTONE
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "compaction_filter_cases.json")))
STATS = [f for f, _ in _abi.FilterStats._fields_]


class FilterError(Exception):
    pass


def batch_entries(b):
    """A Batch's rows as entries (a timestamp the mask lacks: None)."""
    out = []
    for i in range(b.n):
        m = int(b.ts_mask[i])
        out.append((b.key(i), int(b.kind[i]), b.value(i) if b.kind[i] != T else b"", int(b.seq[i]),
                    int(b.create_ts[i]) if m & _abi.TS_CREATE else None, int(b.expire_ts[i]) if m & _abi.TS_EXPIRE else None))
    return out


def retained(runs, ret, op=None, cursor=None, mstats=None):
    """What retention yields -> (entries, MergeSummary).  S1: only the rows with key >= K are read."""
    if cursor is not None:
        runs = [[e for e in r if e[0] >= cursor[0]] for r in runs]
    if op is None:
        merged, sm = O.merge_runs([Run.from_entries(r) for r in runs], ret)
    else:
        r = _abi.Retention.from_buffer_copy(ret)
        r.merge_operands = 1
        merged, sm = O.merge_runs([Run.from_entries(CM.collapse(runs, CM.barrier_of(ret), op, mstats))], r)
    return batch_entries(merged), sm


def apply_decision(e, d):
    """F1-F4 for one row -> the row that passes, or None."""
    key, kind, val, seq, cts, ets = e
    if d == KEEP:                    # F1
        return e
    if d == DROP:                    # F2
        return None
    if d == TOMBSTONE:               # F3: the expire_ts goes, create_ts, seq and key stay
        return (key, T, b"", seq, cts, None)
    code, b = d                      # F4: the kind and the value change, both timestamps stay
    assert code in (VALUE, MERGE)
    return (key, V if code == VALUE else M, bytes(b), seq, cts, ets)


def filter_stream(rows, flt, batch_rows=0):
    """F8 / F5 over the retained rows -> dict(decisions, calls [(first, n)], seen, error_at, end_calls).  A raised
    FilterError: error_at = `first` of the failing call (F9), no on_compaction_end."""
    n = len(rows)
    step = batch_rows or n
    out = dict(decisions=[], calls=[], seen=[], error_at=None, end_error=False)
    first = 0
    while first < n:
        cnt = min(step, n - first)
        out["calls"].append((first, cnt))
        for e in rows[first:first + cnt]:
            out["seen"].append(e)
            try:
                out["decisions"].append(flt(e))
            except FilterError:
                out["error_at"] = first
                return out
        first += cnt
    end = getattr(flt, "on_compaction_end", None)
    if end is not None:
        try:
            end()
        except FilterError:
            out["end_error"] = True
    return out


def drain(rows, cursor):
    """S2: how many leading rows have key == K && seq >= S (a literal prefix)."""
    d = 0
    while d < len(rows) and rows[d][0] == cursor[0] and rows[d][3] >= cursor[1]:
        d += 1
    return d


def expected(runs, ret, prm, max_sst_size, flt=None, batch_rows=0, want_values=False, cursor=None, op=None):
    """What the filtered job must give -> dict: status, first_error_entry, sm (retention's summary), stream (the final
    entries), cuts, ssts ([SstResult]), calls, seen, stats (the sdb_filter_stats words)."""
    rows, sm = retained(runs, ret, op, cursor)
    res = dict(status=sm.status, first_error_entry=sm.first_error_entry, sm=sm, stream=[], cuts=[], ssts=[], calls=[],
               seen=[], stats=dict.fromkeys(STATS, 0))
    if sm.status:
        return res
    st = res["stats"]
    n = len(rows)
    final, mods = rows, []
    if flt is not None:
        f = filter_stream(rows, flt, batch_rows)
        res["calls"], res["seen"] = f["calls"], f["seen"]
        st["calls"], st["rows_in"] = len(f["calls"]), len(f["seen"])
        kb, vb = sum(len(e[0]) for e in rows), sum(len(e[2]) for e in rows)
        st["d2h_bytes"] = n * 26 + 16 * (n + 1) + kb + (vb if want_values else 0) if n else 0
        if f["error_at"] is not None:
            res["status"], res["first_error_entry"] = _abi.SDB_COMPACTION_FILTER_ERROR, f["error_at"]
            return res
        for d in f["decisions"]:
            name = {KEEP: "kept", DROP: "dropped", TOMBSTONE: "tombstoned"}.get(d) if not isinstance(d, tuple) else \
                ("new_values" if d[0] == VALUE else "new_merges")
            st[name] += 1
        if f["end_error"]:
            res["status"], res["first_error_entry"] = _abi.SDB_COMPACTION_FILTER_ERROR, st["rows_in"]
            return res
        passed = [(apply_decision(e, d), d) for e, d in zip(rows, f["decisions"])]
        passed = [(e, d) for e, d in passed if e is not None]
        final = [e for e, _ in passed]
        mods = [isinstance(d, tuple) for _, d in passed]
    if cursor is not None:  # S2, over what the filter passed
        k = drain(final, cursor)
        st["resume_drained"] = k
        final, mods = final[k:], mods[k:]
    if flt is not None and st["kept"] != n and final:  # F7: a keep-all filter uploads and applies nothing
        st["applied"] = 1
        st["h2d_bytes"] = n + 8 * (sum(mods) + 1) + sum(len(e[2]) for e, m in zip(final, mods) if m)
    res["stream"] = final
    if final:  # S3: the writer starts at the first surviving row
        b = Batch.from_entries(final)
        code, res["cuts"] = O.sst_cuts(b, prm, max_sst_size)
        assert code == 0, code
        res["ssts"] = [O.encode_sst(b.slice(res["cuts"][i], res["cuts"][i + 1]), prm) for i in range(len(res["cuts"]) - 1)]
    return res


# ---- the fixture's cases as the model takes them ----
def fixture_rows(rows):
    """(key, kind, value, seq, expire_ts) -> entries."""
    return [(k.encode(), kind, v.encode() if kind != T else b"", seq, None, x) for k, kind, v, seq, x in rows]


class FixtureFilter:
    """The filter a fixture's filter case names, by the decisions the fixture recorded for its rows (keyed by the
    row's key and seq)."""

    def __init__(self, case):
        self.by_row = {}
        for r, d in zip(case["entries"], case["decisions"]):
            self.by_row[(r[0].encode(), r[3])] = d
        self.ended = 0

    def __call__(self, e):
        d = self.by_row[(e[0], e[3])]
        if d == "error":
            raise FilterError(e[0])
        return (d[0], d[1].encode()) if isinstance(d, list) else d

    def on_compaction_end(self):
        self.ended += 1


def resume_case(case):
    """A fixture resume case -> (runs, retention, operator or None, cursor or None, expected entries)."""
    from slatedb_amd.merge import StringConcat
    runs = [fixture_rows(s) for s in case["l0"]] + [sum((fixture_rows(t) for t in s), []) for s in case["sr"]]
    op = StringConcat if case["operator"] else None
    ret = O.retention(min_seq=None if case["operator"] else 0)  # as the reference's test sets retention_min_seq
    cursor = None
    if case["resume_index"] is not None:
        every = sorted((e for r in runs for e in r), key=lambda e: (e[0], -e[3]))
        cursor = (every[case["resume_index"]][0], every[case["resume_index"]][3])
    return runs, ret, op, cursor, fixture_rows(case["expected"])
