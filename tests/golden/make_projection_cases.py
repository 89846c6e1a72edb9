"""Generate tests/golden/projection_cases.json from the reference's own tests of projected SST views.

Run where the reference tree is present (SDB_REFERENCE names it, as for make_get_cases.py); the tests read only the
committed JSON:

    python tests/golden/make_projection_cases.py          # writes the fixture
    python tests/golden/make_projection_cases.py --check  # compares with the committed fixture

Data only, with the source lines: the keys, the visible ranges and the expected results that four of the reference's
tests pin.
  sst_iter       slatedb/src/sst_builder.rs:1210-1280 (test_sst_handle_with_visible_ranges): keys 'a'..='z', visible
                 "c"..="f"; a full scan yields c, d, e, f; the range "m".."p" yields no iterator
  sorted_run     slatedb/src/sorted_run_iterator.rs:393-464 (test_sr_iter_respects_visible_range): key1-4 and key5-8,
                 visible "key2".."key4" and "key5".."key7"; a full scan yields key2, key3, key5, key6
  overlap        slatedb/src/db_state.rs:1364-1438 (max_l0_overlap_*): views given by first / last entry and a visible
                 range, and the largest number of views whose effective ranges share a key
  key_gap        slatedb/src/manifest/mod.rs:4928-4992: a run of [a, c] and [m, p]; projected to "e".."g" both SSTs
                 are dropped, projected to "b".."f" one stays
A bound is [key, kind] with kind 0 unbounded, 1 included, 2 excluded (SDB_BOUND_*); a range is [start, end].
"""
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_retention_cases import REF, strip_comments  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "projection_cases.json")
U, INC, EXC = 0, 1, 2
OPEN = [["", U], ["", U]]


def source(*path):
    p = os.path.join(REF, "slatedb", "src", *path)
    if not os.path.exists(p):
        sys.exit("reference not found at %s" % p)
    return strip_comments(open(p, encoding="utf-8").read())


def body(src, name):
    """The text of fn `name` up to the next fn."""
    m = re.search(r"fn %s\b(.*?)(?=\n    (?:#\[|async fn |fn ))" % re.escape(name), src, re.S)
    if not m:
        sys.exit("fn %s not found" % name)
    return m.group(1)


def from_ref(tok):
    """BytesRange::from_ref("a".."b") / ("a"..="b") -> a range."""
    m = re.fullmatch(r'"([^"]*)"\.\.(=?)"([^"]*)"', tok.strip())
    if not m:
        sys.exit("not a from_ref range: " + tok)
    return [[m.group(1), INC], [m.group(3), INC if m.group(2) else EXC]]


def sst_iter():
    b = body(source("sst_builder.rs"), "test_sst_handle_with_visible_ranges")
    lo, hi = re.search(r"for key in '(.)'\.\.='(.)'", b).groups()
    vis = from_ref(re.search(r"with_visible_range\(BytesRange::from_ref\((.*?)\)\)", b).group(1))
    expected = re.findall(r'RowEntry::new_value\(b"([^"]*)"', b)
    m = re.search(r'Bytes::from_static\(b"([^"]*)"\)\.\.Bytes::from_static\(b"([^"]*)"\)', b)
    return {"source": "slatedb/src/sst_builder.rs:1210-1280", "keys": [chr(c) for c in range(ord(lo), ord(hi) + 1)],
            "visible": vis, "full_scan": expected, "no_iterator_range": [[m.group(1), INC], [m.group(2), EXC]]}


def sorted_run():
    b = body(source("sorted_run_iterator.rs"), "test_sr_iter_respects_visible_range")
    loops = re.findall(r"for i in (\d+)\.\.=(\d+)", b)
    vis = re.findall(r"Some\(BytesRange::from_ref\((.*?)\)\)", b)
    exp = re.search(r"for i in \[([\d, ]+)\]", b).group(1)
    if len(loops) != 2 or len(vis) != 2:
        sys.exit("sorted_run: expected two SSTs")
    return {"source": "slatedb/src/sorted_run_iterator.rs:393-464",
            "ssts": [{"keys": ["key%d" % i for i in range(int(a), int(z) + 1)], "visible": from_ref(v)}
                     for (a, z), v in zip(loops, vis)],
            "full_scan": ["key%d" % int(x) for x in exp.split(",")]}


OVERLAP_TESTS = ("max_l0_overlap_edge_touching_exclusive_end_is_disjoint", "max_l0_overlap_unbounded_end_via_visible_range",
                 "max_l0_overlap_respects_visible_range")


def overlap():
    src = source("db_state.rs")
    cases = []
    for name in OVERLAP_TESTS:
        b = body(src, name).replace(".clone()", "")
        names = dict(re.findall(r'let (\w+) = Bytes::copy_from_slice\(b"([^"]*)"\);', b))

        def bound(tok):
            tok = tok.strip()
            if tok == "Unbounded":
                return ["", U]
            kind, var = re.fullmatch(r"(Included|Excluded)\((\w+)\)", tok).groups()
            return [names[var], INC if kind == "Included" else EXC]

        views = []
        pat = (r'create_compacted_sst_view_with_bounds\(b"([^"]*)", (None|Some\(b"([^"]*)"\))\)'
               r'(\s*\.with_visible_range\(BytesRange::new\(((?:[^()]|\([^()]*\))*)\)\))?')
        for first, last_tok, last, has_vis, vis in re.findall(pat, b):
            v = OPEN
            if has_vis:
                s, e = [t for t in re.split(r",\s*(?![^()]*\))", vis) if t.strip()]
                v = [bound(s), bound(e)]
            views.append({"first": first, "last": None if last_tok == "None" else last, "visible": v})
        peak = int(re.search(r"max_l0_overlap\(&l0\), (\d+)\)", b).group(1))
        cases.append({"name": name, "views": views, "max_overlap": peak})
    return {"source": "slatedb/src/db_state.rs:1364-1438", "cases": cases}


def key_gap():
    src = source("manifest", "mod.rs")
    b = body(src, "manifest_with_two_sst_sorted_run_gap")
    run = [{"first": f, "last": l, "visible": from_ref(v)}
           for f, l, v in re.findall(r'make\(sst\d, b"([^"]*)", b"([^"]*)", BytesRange::from_ref\((.*?)\)\)', b)]
    if len(run) != 2:
        sys.exit("key_gap: expected a run of two SSTs")
    cases = []
    for name in ("test_projected_drops_sorted_run_sst_when_range_falls_in_key_gap",
                 "test_projected_keeps_sorted_run_sst_overlapping_physical_keys"):
        t = body(src, name)
        rng = from_ref(re.search(r"from_global_range\(BytesRange::from_ref\((.*?)\)\)", t).group(1))
        m = re.search(r"sst_views\(\)\.len\(\), (\d+)\)", t)
        if not m and "compacted.is_empty()" not in t:
            sys.exit("key_gap: no expectation in " + name)
        cases.append({"name": name, "global_range": rng, "ssts_kept": int(m.group(1)) if m else 0})
    return {"source": "slatedb/src/manifest/mod.rs:4928-4992", "run": run, "cases": cases}


def extract():
    return {"bound_kinds": "0 unbounded, 1 included, 2 excluded; a range is [start, end], a bound [key, kind]",
            "sst_iter": sst_iter(), "sorted_run": sorted_run(), "overlap": overlap(), "key_gap": key_gap()}


def main():
    data = extract()
    if "--check" in sys.argv:
        if json.load(open(OUT)) != data:
            sys.exit("projection_cases.json differs from the reference's tests")
        print("projection_cases.json matches the reference")
        return
    json.dump(data, open(OUT, "w"), indent=1)
    print("wrote %s" % OUT)


if __name__ == "__main__":
    main()
