"""Generate tests/golden/lsm_scan_cases.json from the reference's own table-driven test of the scan path.

Run where the reference tree is present (SDB_REFERENCE names it, as for make_get_cases.py); the tests read
only the committed JSON:

    python tests/golden/make_lsm_scan_cases.py          # writes the fixture
    python tests/golden/make_lsm_scan_cases.py --check  # compares with the committed fixture

Source: the #[case(ScanTestCase { ... })] attributes of slatedb/src/reader.rs:1350-1683 and the layer order of
populate_db_state / TestDbState (:507-601, 689-771).  Data only: per case the entries (key, kind, value, seq,
expire_ts, layer), the range (start included, end excluded: BytesRange::from_slice(start..end), :1721), the
effective max_seq as prepare_max_seq (:103-131) resolves it, the order in which the layers are merged (newest
first) and the expected (key, value) list.

Kept: the cases that are not marked [MERGE and have no write-batch entry: 13 of the table's 26 (Tests 1-5 and
8-15; none of them names the write batch, and none holds a merge operand).  The write batch and the memtables
stay on the host in this project; a memtable layer is kept as a layer of its own, newest first.

Layers and kinds as in make_get_cases.py.
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_get_cases import effective_max_seq, entry, layer_order, opt  # noqa: E402
from make_retention_cases import REF, bstr, split_top, strip_comments  # noqa: E402

SRC = os.path.join(REF, "slatedb", "src", "reader.rs")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lsm_scan_cases.json")
TOTAL, KEPT = 26, 13
SOURCE_NOTE = ("slatedb/src/reader.rs:1350-1683 (ScanTestCase table), layer order from populate_db_state (:689-771) "
               "and TestDbState (:507-601); max_seq resolved as prepare_max_seq (:103-131); the range is start "
               "included, end excluded. Cases marked [MERGE or with a write-batch entry are left out. kind: 0 value, "
               "1 merge, 2 tombstone")


def extract():
    src = strip_comments(open(SRC, encoding="utf-8").read())
    cases, total = [], 0
    for body in re.findall(r"#\[case\(ScanTestCase \{(.*?)\}\)\]", src, re.S):
        fields = {}
        for f in split_top(body):
            k, v = f.split(":", 1)
            fields[k.strip()] = v.strip()
        total += 1
        desc = json.loads(fields["description"])
        if "[MERGE" in desc:
            continue
        es = [entry(e) for e in split_top(re.fullmatch(r"vec!\[(.*)\]", fields["entries"], re.S).group(1))]
        if any(e["layer"] == "wb" for e in es):
            sys.exit("a case that is not [MERGE names the write batch: " + desc)
        if any(e["kind"] == 1 for e in es):
            sys.exit("a case that is not [MERGE holds a merge operand: " + desc)
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
        sys.exit("parsed %d cases and kept %d; expected %d and %d" % (total, len(cases), TOTAL, KEPT))
    return {"source": SOURCE_NOTE, "cases": cases}


def main():
    if not os.path.exists(SRC):
        sys.exit("reference not found at %s" % SRC)
    data = extract()
    if "--check" in sys.argv:
        have = json.load(open(OUT))
        if have["cases"] != data["cases"]:
            sys.exit("lsm_scan_cases.json differs from the reference table")
        print("lsm_scan_cases.json matches the reference (%d kept cases)" % len(data["cases"]))
        return
    json.dump(data, open(OUT, "w"), indent=1)
    print("wrote %s (%d kept cases)" % (OUT, len(data["cases"])))


if __name__ == "__main__":
    main()
