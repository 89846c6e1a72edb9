"""Generate tests/golden/merge_read_cases.json from the reference's own tests of reads with a merge operator.

Run where the reference tree is present (SDB_REFERENCE names it, as for make_retention_cases.py); the tests
read only the committed JSON:

    python tests/golden/make_merge_read_cases.py          # writes the fixture
    python tests/golden/make_merge_read_cases.py --check  # compares with the committed fixture

Sources, data only:
  get_cases   the #[case(LayerPriorityTestCase { ... })] attributes of slatedb/src/reader.rs:1086-1253 whose
              description carries [MERGE] (the harness then configures StringConcatMergeOperator, :489,
              :1275-1280), parsed as make_get_cases.py parses the others: entries with their layer, the query key,
              the resolved max_seq, the order in which the layers are searched, the expected bytes (null: none).
              Kept: the 11 of 16 without a write-batch entry; the write batch stays on the host in this project.
  iter_cases  the #[case::name(TestCase { ... })] attributes of slatedb/src/merge_operator.rs:723-806 that run
              with TestCase's defaults (merge_different_expire_ts = true, no snapshot barrier: the read path of
              db_iter.rs:234-243): different_expire_ts_read_path, merge_with_tombstone, multiple_values; entries
              and expected rows as (key, kind, value, seq, expire_ts).  Left out: different_expire_ts_write_path
              (merge_different_expire_ts = false) and merge_with_snapshot_barrier, both write-path variants.
              The iterator under test has no deduplicating merge below it, so `expected` may hold several rows
              of one key; a scan sees the first of them (merge_iterator.rs:193-206 drops what follows a key's
              first value or tombstone).

Kinds: 0 value, 1 merge, 2 tombstone.
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_get_cases import effective_max_seq, entry, layer_order, opt  # noqa: E402
from make_retention_cases import REF, bstr, split_top, strip_comments  # noqa: E402

READER = os.path.join(REF, "slatedb", "src", "reader.rs")
MERGE_OP = os.path.join(REF, "slatedb", "src", "merge_operator.rs")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "merge_read_cases.json")
MERGE_CASES, KEPT_GET = 16, 11
ITER_KEPT = ("different_expire_ts_read_path", "merge_with_tombstone", "multiple_values")
ITER_LEFT_OUT = ("different_expire_ts_write_path", "merge_with_snapshot_barrier")
SOURCE_NOTE = ("get_cases: slatedb/src/reader.rs:1086-1253, the [MERGE] rows of the LayerPriorityTestCase table "
               "(StringConcatMergeOperator, :489); kept 11 of 16, the 5 left out hold a write-batch entry, which stays "
               "on the host. iter_cases: slatedb/src/merge_operator.rs:723-806, the 3 of 5 TestCase rows that run with "
               "the defaults (merge_different_expire_ts = true, no snapshot barrier); the 2 left out are write-path "
               "variants. Rows are (key, kind, value, seq, expire_ts); kind: 0 value, 1 merge, 2 tombstone")


def get_cases():
    src = strip_comments(open(READER, encoding="utf-8").read())
    cases, merge = [], 0
    for body in re.findall(r"#\[case\(LayerPriorityTestCase \{(.*?)\}\)\]", src, re.S):
        fields = {}
        for f in split_top(body):
            k, v = f.split(":", 1)
            fields[k.strip()] = v.strip()
        desc = json.loads(fields["description"])
        if "[MERGE]" not in desc:
            continue
        merge += 1
        es = [entry(e) for e in split_top(re.fullmatch(r"vec!\[(.*)\]", fields["entries"], re.S).group(1))]
        if any(e["layer"] == "wb" for e in es):
            continue
        cases.append({"description": desc, "entries": es, "layer_order": layer_order({e["layer"] for e in es}),
                      "query_key": bstr(fields["query_key"]),
                      "max_seq": effective_max_seq(fields["dirty"] == "true", opt(fields["last_committed_seq"], int),
                                                   opt(fields["max_seq"], int)),
                      "expected": opt(fields["expected"], bstr)})
    if merge != MERGE_CASES or len(cases) != KEPT_GET:
        sys.exit("parsed %d [MERGE] cases and kept %d; expected %d and %d" % (merge, len(cases), MERGE_CASES, KEPT_GET))
    return cases


def row(expr):
    m = re.match(r"RowEntry::new_(value|merge|tombstone)\((.*?)\)\s*(?:\.with_expire_ts\((-?\d+)\))?\s*$", expr.strip(), re.S)
    if not m:
        raise ValueError("unparsed row: " + expr)
    args = split_top(m.group(2))
    if m.group(1) == "tombstone":
        key, kind, val, seq = bstr(args[0]), 2, "", int(args[1])
    else:
        key, kind, val, seq = bstr(args[0]), 0 if m.group(1) == "value" else 1, bstr(args[1]), int(args[2])
    return [key, kind, val, seq, int(m.group(3)) if m.group(3) else None]


def rows(expr):
    body = re.fullmatch(r"vec!\[(.*)\]", expr.strip(), re.S).group(1)
    return [row(e) for e in split_top(body) if e.strip()]


def iter_cases():
    src = strip_comments(open(MERGE_OP, encoding="utf-8").read())
    found, cases = [], []
    for name, body in re.findall(r"#\[case::(\w+)\(TestCase \{(.*?)\.\.TestCase::default\(\)\s*\}\)\]", src, re.S):
        found.append(name)
        fields = {}
        for f in split_top(body):
            if f.strip():
                k, v = f.split(":", 1)
                fields[k.strip()] = v.strip()
        defaults = set(fields) <= {"unsorted_data", "expected"}
        if (name in ITER_KEPT) != defaults:
            sys.exit("case %s: kept list and defaults disagree" % name)
        if defaults:
            cases.append({"name": name, "entries": rows(fields["unsorted_data"]), "expected": rows(fields["expected"])})
    if sorted(found) != sorted(ITER_KEPT + ITER_LEFT_OUT):
        sys.exit("merge_operator.rs cases changed: %s" % found)
    return cases


def main():
    if not os.path.exists(READER):
        sys.exit("reference not found at %s" % READER)
    data = {"source": SOURCE_NOTE, "get_cases": get_cases(), "iter_cases": iter_cases()}
    if "--check" in sys.argv:
        have = json.load(open(OUT))
        if have["get_cases"] != data["get_cases"] or have["iter_cases"] != data["iter_cases"]:
            sys.exit("merge_read_cases.json differs from the reference")
        print("merge_read_cases.json matches the reference (%d + %d cases)" % (len(data["get_cases"]), len(data["iter_cases"])))
        return
    json.dump(data, open(OUT, "w"), indent=1)
    print("wrote %s (%d + %d cases)" % (OUT, len(data["get_cases"]), len(data["iter_cases"])))


if __name__ == "__main__":
    main()
