"""Generate tests/golden/get_cases.json from the reference's own table-driven test of the read path.

Run where the reference tree is present (SDB_REFERENCE names it, as for make_retention_cases.py); the tests
read only the committed JSON:

    python tests/golden/make_get_cases.py          # writes the fixture
    python tests/golden/make_get_cases.py --check  # compares with the committed fixture

Source: the #[case(LayerPriorityTestCase { ... })] attributes of slatedb/src/reader.rs:790-1290 and the
layer order of populate_db_state / TestDbState (:507-601, 689-771).  Data only: per case the entries (key,
kind, value, seq, expire_ts, layer), the query key, the effective max_seq as prepare_max_seq (:103-131)
resolves it from dirty / last_committed_seq / max_seq (the durability filter of the harness is not Remote),
the order in which the layers are searched, and the expected value (null: none).

Kept: the cases without a write-batch entry and without a merge operand, 23 of the 27 that are not marked
[MERGE] (four of those name LayerLocation::WriteBatch).  The write batch and the memtables stay on the host
in this project; a memtable layer is kept as a layer because a filtered leaf means the same there.

Layers: "mem", "imm<i>" (i = index in the queue, front first), "l0_<i>" (higher = newer: add_to_l0 pushes
to the front), "sr<id>" (higher id = newer, added first).  Kinds: 0 value, 1 merge, 2 tombstone.
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_retention_cases import REF, bstr, split_top, strip_comments  # noqa: E402

SRC = os.path.join(REF, "slatedb", "src", "reader.rs")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "get_cases.json")
NOT_MERGE, KEPT = 27, 23
U64_MAX = (1 << 64) - 1
SOURCE_NOTE = ("slatedb/src/reader.rs:790-1290 (LayerPriorityTestCase table), layer order from populate_db_state "
               "(:689-771) and TestDbState (:507-601); max_seq resolved as prepare_max_seq (:103-131). Cases with a "
               "write-batch entry or a merge operand are left out. kind: 0 value, 1 merge, 2 tombstone")


def opt(expr, conv):
    e = expr.strip()
    if e == "None":
        return None
    return conv(re.fullmatch(r"Some\((.*)\)", e, re.S).group(1))


def seq_of(tok):
    return U64_MAX if tok.strip() == "u64::MAX" else int(tok)


def layer_of(chain):
    m = re.search(r"\.with_location\(LayerLocation::(\w+)(?:\((\d+)\))?\)", chain)
    if not m:
        return "mem"  # TestEntry's constructors default to the memtable
    name, arg = m.group(1), m.group(2)
    return {"WriteBatch": "wb", "Memtable": "mem", "ImmutableMemtable": "imm%s" % arg, "L0Sst": "l0_%s" % arg,
            "SortedRun": "sr%s" % arg}[name]


def entry(expr):
    m = re.match(r"TestEntry::(value|tombstone|merge)\((.*?)\)((?:\s*\.with_\w+\((?:[^()]|\([^()]*\))*\))*)\s*$",
                 expr.strip(), re.S)
    if not m:
        raise ValueError("unparsed entry: " + expr)
    ctor, args, chain = m.group(1), split_top(m.group(2)), m.group(3)
    if ctor == "tombstone":
        key, kind, val, seq = bstr(args[0]), 2, "", seq_of(args[1])
    else:
        key, kind, val, seq = bstr(args[0]), 0 if ctor == "value" else 1, bstr(args[1]), seq_of(args[2])
    ets = re.search(r"\.with_expire_ts\((-?\d+)\)", chain)
    return {"key": key, "kind": kind, "value": val, "seq": seq, "expire_ts": int(ets.group(1)) if ets else None,
            "layer": layer_of(chain)}


def layer_order(layers):
    """The order GetIterator searches them: memtable, immutable memtables front first, L0 newest first
    (highest index), sorted runs newest first (highest id)."""
    num = lambda s: int(re.search(r"\d+$", s).group(0))  # noqa: E731
    imm = sorted((l for l in layers if l.startswith("imm")), key=num)
    l0 = sorted((l for l in layers if l.startswith("l0_")), key=num, reverse=True)
    sr = sorted((l for l in layers if l.startswith("sr")), key=num, reverse=True)
    return (["mem"] if "mem" in layers else []) + imm + l0 + sr


def effective_max_seq(dirty, last_committed, user):
    """prepare_max_seq (reader.rs:103-131); last_committed_seq None is u64::MAX in the harness."""
    max_seq = None
    if not dirty:
        max_seq = U64_MAX if last_committed is None else last_committed
    if user is not None:
        max_seq = user if max_seq is None else min(max_seq, user)
    return max_seq


def extract():
    src = strip_comments(open(SRC, encoding="utf-8").read())
    cases, not_merge = [], 0
    for body in re.findall(r"#\[case\(LayerPriorityTestCase \{(.*?)\}\)\]", src, re.S):
        fields = {}
        for f in split_top(body):
            k, v = f.split(":", 1)
            fields[k.strip()] = v.strip()
        desc = json.loads(fields["description"])
        if "[MERGE]" in desc:
            continue
        not_merge += 1
        es = [entry(e) for e in split_top(re.fullmatch(r"vec!\[(.*)\]", fields["entries"], re.S).group(1))]
        if any(e["layer"] == "wb" or e["kind"] == 1 for e in es):
            continue
        cases.append({"description": desc, "entries": es, "layer_order": layer_order({e["layer"] for e in es}),
                      "query_key": bstr(fields["query_key"]),
                      "max_seq": effective_max_seq(fields["dirty"] == "true", opt(fields["last_committed_seq"], int),
                                                   opt(fields["max_seq"], int)),
                      "expected": opt(fields["expected"], bstr)})
    if not_merge != NOT_MERGE or len(cases) != KEPT:
        sys.exit("parsed %d cases that are not [MERGE] and kept %d; expected %d and %d" %
                 (not_merge, len(cases), NOT_MERGE, KEPT))
    return {"source": SOURCE_NOTE, "cases": cases}


def main():
    if not os.path.exists(SRC):
        sys.exit("reference not found at %s" % SRC)
    data = extract()
    if "--check" in sys.argv:
        have = json.load(open(OUT))
        if have["cases"] != data["cases"]:
            sys.exit("get_cases.json differs from the reference table")
        print("get_cases.json matches the reference (%d kept cases)" % len(data["cases"]))
        return
    json.dump(data, open(OUT, "w"), indent=1)
    print("wrote %s (%d kept cases)" % (OUT, len(data["cases"])))


if __name__ == "__main__":
    main()
