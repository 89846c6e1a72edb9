"""The model of tests/compaction_filter_cases.py against the reference's own cases (tests/golden/
compaction_filter_cases.json): the nine tests of CompactionFilterIterator and the ten cases of the resumed
load_iterators.  No device is needed."""
import pytest

from oracle import oracle as O
from slatedb_amd import _abi
from slatedb_amd import compaction_filter as CF

from . import compaction_filter_cases as F

FILTER_CASES = F.FIXTURE["filter_cases"]
RESUME_CASES = F.FIXTURE["resume_cases"]


def test_fixture_shape():
    assert len(FILTER_CASES) == 9 and len(RESUME_CASES) == 10
    assert sum(c["operator"] for c in RESUME_CASES) == 2 and sum(c["resume_index"] is None for c in RESUME_CASES) == 1


@pytest.mark.parametrize("case", FILTER_CASES, ids=lambda c: c["name"])
def test_filter_case(case):
    """The filter stage alone, over the rows in the order the reference's mock iterator yields them."""
    rows = F.fixture_rows(case["entries"])
    flt = F.FixtureFilter(case)
    f = F.filter_stream(rows, flt, batch_rows=1)  # one row per call: the reference's granularity
    if case["error_at"] is not None:
        assert f["error_at"] == case["error_at"] and flt.ended == 0  # F9: no on_compaction_end after a failure
        rows = rows[:case["error_at"]]
    else:
        assert f["error_at"] is None and flt.ended == 1              # F5: once, after the last row
        assert f["calls"] == [(i, 1) for i in range(len(rows))] and f["seen"] == rows
    got = [F.apply_decision(e, d) for e, d in zip(rows, f["decisions"])]
    got = [e for e in got if e is not None]
    assert got == F.fixture_rows(case["expected"])
    for j, a in enumerate(case["asserted"]):  # what the reference's test itself asserts of every next()
        if a.get("none") or a.get("error"):
            assert j == len(got)
            continue
        key, kind, val, seq, _, ets = got[j]
        if "entry" in a:
            assert got[j] == F.fixture_rows([case["entries"][a["entry"]]])[0]
        if "key" in a:
            assert key == a["key"].encode()
        if "value" in a:
            assert (kind, val) == (F.V, a["value"].encode())
        if "tombstone" in a:
            assert (kind == F.T) == a["tombstone"]
        if "seq" in a:
            assert seq == a["seq"]
        if "expire_ts" in a:
            assert ets == a["expire_ts"]


@pytest.mark.parametrize("batch_rows", [0, 1, 2])
def test_batching_does_not_change_the_decisions(batch_rows):
    case = FILTER_CASES[1]
    rows = F.fixture_rows(case["entries"])
    f = F.filter_stream(rows, F.FixtureFilter(case), batch_rows)
    assert f["decisions"] == case["decisions"] and sum(n for _, n in f["calls"]) == len(rows)
    assert [a for a, _ in f["calls"]] == sorted({a for a, _ in f["calls"]}) and f["calls"][0][0] == 0


@pytest.mark.parametrize("case", RESUME_CASES, ids=lambda c: c["name"])
def test_resume_case(case):
    """S1-S3 over the oracle's merge: the rows the resumed load_iterators yields."""
    runs, ret, op, cursor, want = F.resume_case(case)
    res = F.expected(runs, ret, O.params(block_size=case["block_size"]), case["max_sst_size"], cursor=cursor, op=op)
    assert res["status"] == 0
    assert [(e[0], e[1], e[2], e[3], e[5]) for e in res["stream"]] == [(e[0], e[1], e[2], e[3], e[5]) for e in want]
    assert (len(res["ssts"]) == 0) == (len(want) == 0)
    if res["cuts"]:
        assert res["cuts"][0] == 0 and res["cuts"][-1] == len(want)  # S3: the cuts count from the first surviving row
    if cursor is None:
        assert res["stats"]["resume_drained"] == 0
    # S1: the rows below K are never read (with an operator the model's merge runs over the collapsed units)
    assert op is not None or res["sm"].num_in ==sum(e[0] >= (cursor[0] if cursor else b"") for r in runs for e in r)


@pytest.mark.parametrize("case", [c for c in RESUME_CASES if c["resume_index"] is not None], ids=lambda c: c["name"])
def test_resumed_stream_is_the_tail_of_the_full_one(case):
    runs, ret, op, cursor, _ = F.resume_case(case)
    prm = O.params(block_size=case["block_size"])
    full = F.expected(runs, ret, prm, case["max_sst_size"], op=op)["stream"]
    part = F.expected(runs, ret, prm, case["max_sst_size"], cursor=cursor, op=op)["stream"]
    assert part == full[len(full) - len(part):]
    assert all((e[0], -e[3]) > (cursor[0], -cursor[1]) for e in part)


def test_filter_is_called_for_the_drained_rows():
    """S2 / F8: a cursor in the middle of a key's versions; the filter sees every retained row with key >= K."""
    runs = [[(b"a", F.V, b"1", 9, None, None), (b"b", F.V, b"2", 8, None, None), (b"b", F.V, b"3", 5, None, None),
             (b"b", F.V, b"4", 2, None, None), (b"c", F.V, b"5", 7, None, None)]]
    seen = []

    def flt(e):
        seen.append(e)
        return CF.TOMBSTONE if e[3] == 5 else CF.KEEP
    res = F.expected(runs, O.retention(min_seq=0), O.params(), 1 << 20, flt=flt, cursor=(b"b", 5))
    assert [e[3] for e in seen] == [8, 5, 2, 7] and res["seen"] == seen
    assert [(e[0], e[1], e[3]) for e in res["stream"]] == [(b"b", F.V, 2), (b"c", F.V, 7)]  # the tombstoned (b, 5) drains too
    assert res["stats"]["resume_drained"] == 2 and res["stats"]["tombstoned"] == 1 and res["stats"]["applied"] == 1


def test_context_and_example_filter():
    ctx = CF.CompactionJobContext.from_retention(O.retention(min_seq=7, compaction_start_ts=5, filter_tombstone=True), 3)
    assert ctx == (3, True, 5, 7) and CF.CompactionJobContext.from_retention(O.retention()).retention_min_seq is None
    f = CF.PrefixTombstoneFilter(b"delete:")
    e = CF.Entry(b"delete:k", 0, b"v", 1, None, 9)
    assert f.filter(e) == CF.TOMBSTONE and f.filter(e._replace(key=b"keep:k")) == CF.KEEP and f.tombstone_count == 1
    assert (CF.KEEP, CF.DROP, CF.TOMBSTONE, CF.VALUE, CF.MERGE) == (0, 1, 2, 3, 4)
    assert _abi.STATUS_NAMES[_abi.SDB_COMPACTION_FILTER_ERROR] == "COMPACTION_FILTER_ERROR"
