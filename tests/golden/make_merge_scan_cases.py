"""Generate tests/golden/merge_scan_cases.json from the [MERGE SCAN] cases of the reference's table-driven test of
the scan path.

Run where the reference tree is present (SDB_REFERENCE names it, as for make_get_cases.py); the tests read
only the committed JSON:

    python tests/golden/make_merge_scan_cases.py          # writes the fixture
    python tests/golden/make_merge_scan_cases.py --check  # compares with the committed fixture

Source: the #[case(ScanTestCase { ... })] attributes of slatedb/src/reader.rs:1350-1683 whose description starts
with "[MERGE SCAN]", in the format of lsm_scan_cases.json (make_lsm_scan_cases.py).  Data only: per case the entries
(key, kind, value, seq, expire_ts, layer), the range (start included, end excluded), the effective max_seq, the
order in which the layers are merged (newest first) and the expected (key, value) list under the test's
string-concatenating merge operator (StringConcatMergeOperator, reader.rs:489).

Kept: the cases none of whose entries names the write batch: 7 of the table's 13 [MERGE SCAN] cases.  Every one of
them has memtable rows, so they run through sdb_lsm_scan_mem with their mem / imm layers as device tables.
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_get_cases import effective_max_seq, entry, layer_order, opt  # noqa: E402
from make_retention_cases import REF, bstr, split_top, strip_comments  # noqa: E402

SRC = os.path.join(REF, "slatedb", "src", "reader.rs")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "merge_scan_cases.json")
TOTAL, KEPT = 13, 7
SOURCE_NOTE = ("slatedb/src/reader.rs:1350-1683 (ScanTestCase table, the cases marked [MERGE SCAN]), layer order from "
               "populate_db_state (:689-771) and TestDbState (:507-601); max_seq resolved as prepare_max_seq (:103-131); "
               "the range is start included, end excluded; expected values under the string-concatenating operator "
               "(:489). Cases with a write-batch entry are left out. kind: 0 value, 1 merge, 2 tombstone")


def extract():
    src = strip_comments(open(SRC, encoding="utf-8").read())
    cases, total = [], 0
    for body in re.findall(r"#\[case\(ScanTestCase \{(.*?)\}\)\]", src, re.S):
        fields = {}
        for f in split_top(body):
            k, v = f.split(":", 1)
            fields[k.strip()] = v.strip()
        desc = json.loads(fields["description"])
        if not desc.startswith("[MERGE SCAN]"):
            continue
        total += 1
        es = [entry(e) for e in split_top(re.fullmatch(r"vec!\[(.*)\]", fields["entries"], re.S).group(1))]
        if any(e["layer"] == "wb" for e in es):
            continue
        if not any(e["layer"] == "mem" or e["layer"].startswith("imm") for e in es):
            sys.exit("a kept [MERGE SCAN] case has no memtable row: " + desc)
        expected = []
        for pair in split_top(re.fullmatch(r"vec!\[(.*)\]", fields["expected"], re.S).group(1)):
            k, v = split_top(re.fullmatch(r"\((.*)\)", pair.strip(), re.S).group(1))
            expected.append([bstr(k), bstr(v)])
        cases.append({"description": desc, "entries": es, "layer_order": layer_order({e["layer"] for e in es}),
                      "range_start": bstr(fields["range_start"]), "range_end": bstr(fields["range_end"]),
                      "max_seq": effective_max_seq(fields["dirty"] == "true", opt(fields["last_committed_seq"], int),
                                                   opt(fields["max_seq"], int)),
                      "expected": expected})
    if total != TOTAL or len(cases) != KEPT:
        sys.exit("parsed %d [MERGE SCAN] cases and kept %d; expected %d and %d" % (total, len(cases), TOTAL, KEPT))
    return {"source": SOURCE_NOTE, "cases": cases}


def main():
    if not os.path.exists(SRC):
        sys.exit("reference not found at %s" % SRC)
    data = extract()
    if "--check" in sys.argv:
        have = json.load(open(OUT))
        if have["cases"] != data["cases"]:
            sys.exit("merge_scan_cases.json differs from the reference table")
        print("merge_scan_cases.json matches the reference (%d kept cases)" % len(data["cases"]))
        return
    json.dump(data, open(OUT, "w"), indent=1)
    print("wrote %s (%d kept cases)" % (OUT, len(data["cases"])))


if __name__ == "__main__":
    main()
