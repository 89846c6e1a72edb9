"""Generate tests/golden/compaction_merge_cases.json from the reference's own tests of MergeOperatorIterator as
compaction and memtable flush configure it (merge_different_expire_ts = false, a snapshot barrier).

Run where the reference tree is present (SDB_REFERENCE names it, as for make_retention_cases.py); the tests
read only the committed JSON:

    python tests/golden/make_compaction_merge_cases.py          # writes the fixture
    python tests/golden/make_compaction_merge_cases.py --check  # compares with the committed fixture

Source, data only: the #[case::name(TestCase { ... })] attributes of slatedb/src/merge_operator.rs:741-806:
  different_expire_ts_write_path   merge_different_expire_ts = false, no barrier
  merge_with_snapshot_barrier      snapshot_barrier_seq = Some(3) (merge_different_expire_ts at its default, true:
                                   no row carries an expire_ts, so the flag cannot matter)
  merge_with_tombstone, multiple_values   TestCase's defaults; neither carries an expire_ts, so they hold for
                                   merge_different_expire_ts = false as well
Per case: the entries, the expected rows, both as (key, kind, value, seq, expire_ts), and the barrier (null: none).
The operator is MockMergeOperator (:504): existing ++ operands in order.

Kinds: 0 value, 1 merge, 2 tombstone.
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_merge_read_cases import MERGE_OP, rows  # noqa: E402
from make_retention_cases import split_top, strip_comments  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "compaction_merge_cases.json")
KEPT = ("different_expire_ts_write_path", "merge_with_snapshot_barrier", "merge_with_tombstone", "multiple_values")
SOURCE_NOTE = ("slatedb/src/merge_operator.rs:741-806, the TestCase rows that hold on the write path "
               "(merge_different_expire_ts = false, snapshot_barrier_seq = retention_min_seq): "
               "different_expire_ts_write_path and merge_with_snapshot_barrier set those fields; merge_with_tombstone "
               "and multiple_values run with the defaults and carry no expire_ts, so merge_different_expire_ts cannot "
               "matter for them. Rows are (key, kind, value, seq, expire_ts); kind: 0 value, 1 merge, 2 tombstone; "
               "barrier: snapshot_barrier_seq, null = none; operator: existing ++ operands (MockMergeOperator, :504)")


def cases():
    src = strip_comments(open(MERGE_OP, encoding="utf-8").read())
    out = []
    for name, body in re.findall(r"#\[case::(\w+)\(TestCase \{(.*?)\.\.TestCase::default\(\)\s*\}\)\]", src, re.S):
        if name not in KEPT:
            continue
        fields = {}
        for f in split_top(body):
            if f.strip():
                k, v = f.split(":", 1)
                fields[k.strip()] = v.strip()
        es = rows(fields["unsorted_data"])
        mdet = fields.get("merge_different_expire_ts", "true")
        if mdet != "false" and any(e[4] is not None for e in es):
            sys.exit("case %s: merge_different_expire_ts = true over rows with an expire_ts" % name)
        m = re.fullmatch(r"Some\((\d+)\)", fields.get("snapshot_barrier_seq", "None"))
        out.append({"name": name, "entries": es, "expected": rows(fields["expected"]),
                    "barrier": int(m.group(1)) if m else None})
    if sorted(c["name"] for c in out) != sorted(KEPT):
        sys.exit("merge_operator.rs cases changed: %s" % [c["name"] for c in out])
    return out


def main():
    if not os.path.exists(MERGE_OP):
        sys.exit("reference not found at %s" % MERGE_OP)
    data = {"source": SOURCE_NOTE, "cases": cases()}
    if "--check" in sys.argv:
        if json.load(open(OUT))["cases"] != data["cases"]:
            sys.exit("compaction_merge_cases.json differs from the reference")
        print("compaction_merge_cases.json matches the reference (%d cases)" % len(data["cases"]))
        return
    json.dump(data, open(OUT, "w"), indent=1)
    print("wrote %s (%d cases)" % (OUT, len(data["cases"])))


if __name__ == "__main__":
    main()
