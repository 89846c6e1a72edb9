"""Generate tests/golden/compaction_filter_cases.json from the reference's own tests of CompactionFilterIterator and
of the resumed load_iterators.

Run where the reference tree is present (SDB_REFERENCE names it, as for make_retention_cases.py); the tests read only
the committed JSON:

    python tests/golden/make_compaction_filter_cases.py          # writes the fixture
    python tests/golden/make_compaction_filter_cases.py --check  # compares with the committed fixture

Source, data only:
  filter_cases   the nine #[tokio::test]s of slatedb/src/compaction_filter_iterator.rs:243-537.  Per test: the rows of
                 its `entries` vector, the filter it boxes (its struct name and its prefix / suffix literal), and what
                 the test asserts of every next(): `asserted`, one item per call, either {"none": true}, {"error":
                 true}, or the fields it checks ({"entry": i} = equal to entries[i]; key, value, tombstone, seq,
                 expire_ts).  `decisions` and `expected` restate the boxed filter's rule over the rows (0 keep, 1 drop,
                 2 tombstone, [3, value]) and are checked here against every asserted field, so a reference test that
                 changes fails the generation.
  resume_cases   the ten #[case::name(...)] of test_load_iterators_resume, slatedb/src/compactor_executor.rs:1086-1446:
                 the L0 entry sets, the sorted runs' SST entry sets, block_size, output_max_sst_size, resume_index
                 (the cursor is row resume_index of all entries sorted by key ascending, seq descending; null: no
                 cursor), whether the case runs StringConcatMergeOperator, and the expected rows.  The test runs with
                 retention_min_seq = Some(0) without an operator and None with one, is_dest_last_run = false and
                 compaction_clock_tick = 0.
Rows are (key, kind, value, seq, expire_ts); kind: 0 value, 1 merge, 2 tombstone.
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_merge_read_cases import rows  # noqa: E402
from make_retention_cases import REF, bstr, opt_int, split_top, strip_comments  # noqa: E402

FILTER_SRC = os.path.join(REF, "slatedb", "src", "compaction_filter_iterator.rs")
EXEC_SRC = os.path.join(REF, "slatedb", "src", "compactor_executor.rs")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "compaction_filter_cases.json")
SOURCE_NOTE = __doc__.split("Source, data only:")[1].strip()
FILTER_TESTS = ("test_keep_all_filter", "test_drop_prefix_filter", "test_modify_value_filter", "test_tombstone_decision",
                "test_tombstone_on_merge_operand_converts_to_tombstone", "test_on_compaction_end_called_on_completion",
                "test_tombstone_clears_expire_ts", "test_modify_value_preserves_expire_ts",
                "test_filter_error_aborts_iteration")
RESUME_CASES = ("l0_only", "l0_only_multi_block", "sr_only", "l0_and_sr", "l0_and_sr_overlap", "tombstones_resume",
                "no_output_ssts", "resume_at_end", "merge_operator_resume", "merge_operator_resume_skip_merged_operands")
KEEP, DROP, TOMBSTONE, VALUE = 0, 1, 2, 3


def made_row(expr):
    m = re.fullmatch(r"(make_entry|make_tombstone|make_merge|make_entry_with_expire_ts)\((.*)\)", expr.strip(), re.S)
    if not m:
        raise ValueError("unparsed row: " + expr)
    a = split_top(m.group(2))
    if m.group(1) == "make_tombstone":
        return [bstr(a[0]), 2, "", int(a[1]), None]
    return [bstr(a[0]), 1 if m.group(1) == "make_merge" else 0, bstr(a[1]), int(a[2]),
            int(a[3]) if m.group(1) == "make_entry_with_expire_ts" else None]


def boxed_filter(body):
    """(struct name, its byte-string field or None) of the filter the test hands the iterator."""
    m = re.search(r"let filter = (\w+) \{\s*(\w+): (b\"[^\"]*\")\.to_vec\(\),?\s*\}", body)
    if m:
        return m.group(1), bstr(m.group(3))
    if "let filter = TrackingFilter" in body:
        return "TrackingFilter", None
    m = re.search(r"CompactionFilterIterator::new\(mock_iter, Box::new\((\w+)\)\)", body)
    return m.group(1), None


def decide(name, arg, row):
    """The rule of the test's filter struct over one row (compaction_filter_iterator.rs:114-200, :494-514)."""
    key, kind, val = row[0], row[1], row[2]
    if name in ("KeepAllFilter", "TrackingFilter"):
        return KEEP
    if name == "DropPrefixFilter":
        return DROP if key.startswith(arg) else KEEP
    if name == "TombstoneFilter":
        return TOMBSTONE if key.startswith(arg) else KEEP
    if name == "ModifyValueFilter":  # value.as_bytes(): Some for a value and for a merge operand
        return [VALUE, val + arg] if kind != 2 else KEEP
    if name == "FailingFilter":
        return "error" if key.startswith("fail:") else KEEP
    raise ValueError(name)


def asserted(body):
    """What the test asserts of each next(), in call order."""
    calls, by_name = [], {}
    for stmt in split_top(body, ";"):
        s = " ".join(stmt.split())
        m = re.match(r"let (result\d*) = iter\.next\(\)\.await(\.unwrap\(\))?(\.unwrap\(\))?$", s)
        if m:
            by_name[m.group(1)] = {}
            calls.append(by_name[m.group(1)])
            continue
        m = re.match(r"assert!\(iter\.next\(\)\.await\.unwrap\(\)\.is_(some|none)\(\)\)$", s)
        if m:
            calls.append({"none": True} if m.group(1) == "none" else {})
            continue
        m = re.match(r"assert_eq!\((result\d*), (?:Some\()?entries\[(\d+)\](?:\.clone\(\)\))?\)$", s)
        if m:
            by_name[m.group(1)]["entry"] = int(m.group(2))
            continue
        m = re.match(r"assert_eq!\((result\d*), None\)$", s)
        if m:
            by_name[m.group(1)]["none"] = True
            continue
        m = re.match(r"assert!\((result\d*)\.is_err\(\)\)$", s)
        if m:
            by_name[m.group(1)]["error"] = True
            continue
        m = re.match(r"assert!\((!?)(result\d*)\.value\.is_tombstone\(\)\)$", s)
        if m:
            by_name[m.group(2)]["tombstone"] = m.group(1) == ""
            continue
        m = re.match(r"assert_eq!\((result\d*)\.key, Bytes::from_static\((b\"[^\"]*\")\)\)$", s)
        if m:
            by_name[m.group(1)]["key"] = bstr(m.group(2))
            continue
        m = re.match(r"assert_eq!\( ?(result\d*)\.value, ValueDeletable::Value\(Bytes::from_static\((b\"[^\"]*\")\)\) ?\)$", s)
        if m:
            by_name[m.group(1)]["value"] = bstr(m.group(2))
            continue
        m = re.match(r"assert_eq!\((result\d*)\.seq, (\d+)\)$", s)
        if m:
            by_name[m.group(1)]["seq"] = int(m.group(2))
            continue
        m = re.match(r"assert_eq!\((result\d*)\.expire_ts, (None|Some\(\d+\))\)$", s)
        if m:
            by_name[m.group(1)]["expire_ts"] = opt_int(m.group(2))
            by_name[m.group(1)]["expire_ts_checked"] = True
            continue
        if s.startswith(("assert", "let result")) and "end_called" not in s and "err" not in s:
            raise ValueError("unparsed assertion: " + s)
    return calls


def apply(row, d):
    if d == TOMBSTONE:
        return [row[0], 2, "", row[3], None]
    if isinstance(d, list):
        return [row[0], 0, d[1], row[3], row[4]]
    return list(row)


def filter_cases():
    src = strip_comments(open(FILTER_SRC, encoding="utf-8").read())
    out = []
    for name, body in re.findall(r"async fn (test_\w+)\(\) \{(.*?)\n    \}\n", src, re.S):
        if name not in FILTER_TESTS:
            continue
        es = [made_row(e) for e in split_top(re.search(r"let entries = vec!\[(.*?)\];", body, re.S).group(1)) if e.strip()]
        fname, arg = boxed_filter(body)
        decisions = [decide(fname, arg, r) for r in es]
        expected, error_at = [], None
        for i, (r, d) in enumerate(zip(es, decisions)):
            if d == "error":
                error_at = i
                break
            if d != DROP:
                expected.append(apply(r, d))
        calls = asserted(body[body.index("iter.init()"):])
        # every asserted field holds for the restated rule
        for j, c in enumerate(calls):
            if c.get("none"):
                assert j == len(expected) and error_at is None, (name, j)
            elif c.get("error"):
                assert j == len(expected) and error_at is not None, (name, j)
            else:
                row = expected[j]
                if "entry" in c:
                    assert row == es[c["entry"]], (name, j)
                if "key" in c:
                    assert row[0] == c["key"], (name, j)
                if "value" in c:
                    assert (row[1], row[2]) == (0, c["value"]), (name, j)
                if "tombstone" in c:
                    assert (row[1] == 2) == c["tombstone"], (name, j)
                if "seq" in c:
                    assert row[3] == c["seq"], (name, j)
                if c.get("expire_ts_checked"):
                    assert row[4] == c["expire_ts"], (name, j)
        for c in calls:
            c.pop("expire_ts_checked", None) and c.setdefault("expire_ts", None)
        out.append({"name": name, "entries": es, "filter": [fname, arg],
                    "decisions": decisions[:error_at + 1] if error_at is not None else decisions, "expected": expected,
                    "error_at": error_at, "asserted": calls})
    if sorted(c["name"] for c in out) != sorted(FILTER_TESTS):
        sys.exit("compaction_filter_iterator.rs tests changed: %s" % [c["name"] for c in out])
    return out


def resume_cases():
    src = strip_comments(open(EXEC_SRC, encoding="utf-8").read())
    end = src.index("async fn test_load_iterators_resume(")
    start = src.rindex("#[rstest]", 0, end)
    out = []
    for name, body in re.findall(r"#\[case::(\w+)\((.*?)\n    \)\]", src[start:end], re.S):
        l0, sr, block_size, max_sst, resume_index, op, expected = [a.strip() for a in split_top(body) if a.strip()]
        sets = lambda e: [] if e == "Vec::new()" else split_top(re.fullmatch(r"vec!\[(.*)\]", e, re.S).group(1))  # noqa: E731
        out.append({"name": name,
                    "l0": [rows(s) for s in sets(l0) if s.strip()],
                    "sr": [[rows(t) for t in sets(s.strip()) if t.strip()] for s in sets(sr) if s.strip()],
                    "block_size": int(block_size.replace("_", "")), "max_sst_size": int(max_sst.replace("_", "")),
                    "resume_index": opt_int(resume_index), "operator": op != "None",
                    "expected": rows(expected) if expected != "vec![]" else []})
        if op != "None" and "StringConcatMergeOperator" not in op:
            sys.exit("case %s: another operator" % name)
    if [c["name"] for c in out] != list(RESUME_CASES):
        sys.exit("test_load_iterators_resume cases changed: %s" % [c["name"] for c in out])
    return out


def main():
    if not os.path.exists(FILTER_SRC):
        sys.exit("reference not found at %s" % FILTER_SRC)
    data = {"source": SOURCE_NOTE, "filter_cases": filter_cases(), "resume_cases": resume_cases()}
    if "--check" in sys.argv:
        have = json.load(open(OUT))
        if have["filter_cases"] != data["filter_cases"] or have["resume_cases"] != data["resume_cases"]:
            sys.exit("compaction_filter_cases.json differs from the reference")
        print("compaction_filter_cases.json matches the reference (%d + %d cases)" %
              (len(data["filter_cases"]), len(data["resume_cases"])))
        return
    json.dump(data, open(OUT, "w"), indent=1)
    print("wrote %s (%d + %d cases)" % (OUT, len(data["filter_cases"]), len(data["resume_cases"])))


if __name__ == "__main__":
    main()
