"""The model of sdb_lsm_scan_mem (tests/mem_scan_cases.py) against the reference's recorded scans, against the models
it extends, against its own brute force and against the get over the same layers.  No GPU."""
import pytest

from slatedb_amd import _abi

from . import get_cases as G
from . import lsm_scan_cases as L
from . import mem_get_cases as MG
from . import mem_scan_cases as S
from . import merge_read_cases as M
from .scan_cases import EXC, INC, U


@pytest.mark.parametrize("version", [1, 2])
def test_golden_plain_cases_with_tables(version):
    cases = L.golden_cases()
    assert len(cases) == L.KEPT_CASES
    no_tree = 0
    for c in cases:
        mt = S.golden_mem_tree(c, version)
        assert mt.tables, c["description"]
        no_tree += not mt.tree.leaves
        sc = S.scan(mt, L.golden_range(c), c["max_seq"])
        assert sc.status == 0, c["description"]
        got = [[k.decode(), v.decode()] for k, v in S.values(mt, sc, False)]
        assert got == c["expected"], c["description"]
        assert [r[0] for r in sc.rows] == [k for k, _ in S.brute(mt, L.golden_range(c), c["max_seq"])[0]]
    assert no_tree == 5  # S8: five of the reference's cases live in memtables alone


@pytest.mark.parametrize("version", [1, 2])
def test_golden_merge_scan_cases(version):
    cases = S.merge_golden_cases()
    assert len(cases) == S.KEPT_MERGE_CASES
    for c in cases:
        mt = S.golden_mem_tree(c, version)
        assert mt.tables, c["description"]
        sc = S.scan(mt, L.golden_range(c), c["max_seq"], chain=True)
        assert sc.status == 0
        got = [[k.decode(), v.decode()] for k, v in S.values(mt, sc, True)]
        assert got == c["expected"], c["description"]
        # a chain runs from a table into the tree in every case: cut at the layer boundary it would differ
        assert any(len({l[0] for l in r[1]}) == 2 for r in sc.rows) or "tombstone" in c["description"]


@pytest.fixture(scope="module")
def plain():
    return L.plain_tree()


def test_no_tables_is_the_tree_model(plain):
    tree, straddler = plain
    mt = S.MemTree([], tree)
    rngs, bounds = L.bounds_for(tree, L.ranges(tree, straddler, nrandom=60), straddler)
    for rng, b in zip(rngs, bounds):
        for desc in (False, True):
            a, z = S.scan(mt, rng, b, desc), L.scan(tree, rng, b, desc)
            assert (a.status, a.ssts, a.blocks, a.candidates, a.cand_key_bytes, a.tables, a.filtered) == \
                (z.status, z.ssts, z.blocks, z.candidates, z.cand_key_bytes, [], [])
            assert [(k, s[1], s[2]) for k, s in a.rows] == z.rows
    ctree, cs = M.chain_tree()
    mt = S.MemTree([], ctree)
    for rng in L.narrow_ranges(ctree, 60) + [(None, U, None, U), (cs, INC, cs, INC), (cs, EXC, None, U)]:
        a, z = S.scan(mt, rng, None, False, chain=True), M.scan_merge(ctree, rng)
        if a.filtered:  # a point range that a filter kept out of an SST: the filtered models' ground
            continue
        assert (a.status, a.candidates, a.cand_key_bytes) == (z.status, z.candidates, z.cand_key_bytes)
        assert [(k, [l[1:] for l in ls], b, c, e) for k, ls, b, c, e in a.rows] == z.rows


def test_model_against_brute_force(plain):
    tree, straddler = plain
    mt = S.MemTree(S.little_tables(tree), tree)
    rngs, bounds = L.bounds_for(tree, L.ranges(tree, straddler, nrandom=80), straddler)
    hit = 0
    for rng, b in zip(rngs, bounds):
        sc = S.scan(mt, rng, b)
        rows, st = S.brute(mt, rng, b) if rng[1] <= EXC and rng[3] <= EXC else ([], _abi.SDB_INVALID_ARGUMENT)
        assert sc.status == st
        assert [(k, s[:3]) for k, s in sc.rows] == rows
        hit += any(s[0] == "t" for _, s in sc.rows)
    assert hit > 20


def test_point_ranges_agree_with_the_get(plain):
    """On point ranges whose tree part has no failing block the scan yields what MemTree.get finds."""
    tree, straddler = plain
    tabs = S.little_tables(tree, layered=True)  # (a get asks the layers in order, a scan the seqs: a store's layers agree)
    mt, gt = S.MemTree(tabs, tree), MG.MemTree(tabs, tree)
    keys = L.all_keys(tree)[::7] + [r[0] for t in tabs for r in t.rows][::5] + [b"", b"zz", straddler]
    seqs = sorted({r[3] for l in tree.leaves for r in l.sst.rows})
    for n, k in enumerate(keys):
        for b in (None, seqs[(n * 13) % len(seqs)], seqs[-1] + 1500 + n):
            sc, g = S.scan(mt, (k, INC, k, INC), b), gt.get(k, b)
            assert sc.status == 0
            if g.state == _abi.GET_FOUND:
                (key, src), = sc.rows
                z = gt.columns(g)
                want = ("t", z["table"], z["row"]) if z["table"] != MG.NO_TABLE else ("s", z["sst"])
                assert key == k and src[:len(want)] == want and mt.row_of(src)[3] == z["seq"]
            else:
                assert g.state in (_abi.GET_NOT_FOUND, _abi.GET_DELETED) and not sc.rows


def test_stretch_rules():
    t = MG.Table([(b"a", 0, b"1", 5, None, None), (b"a", 0, b"2", 9, None, None), (b"a\x00", 0, b"3", 7, None, None),
                  (b"ab", 2, b"", 8, None, None), (b"ab", 0, b"4", 3, None, None)])
    assert [r[0] for r in t.rows] == [b"a", b"a", b"a\x00", b"ab", b"ab"] and t.rows[0][3] == 9
    assert S.stretch(t, (b"a", INC, b"a", INC)) == (0, 2)       # every version of an included key
    assert S.stretch(t, (b"a", EXC, None, U)) == (2, 5)         # an excluded start steps over every version
    assert S.stretch(t, (None, U, b"ab", INC)) == (0, 5)        # an included end keeps every version
    assert S.stretch(t, (None, U, b"ab", EXC)) == (0, 3)
    assert S.stretch(t, (b"a", EXC, b"ab", EXC)) == (2, 3)      # a proper prefix of its neighbour is another key
    assert S.stretch(t, (b"b", INC, b"a", INC)) == (0, 0)       # empty as a set
    assert S.stretch(t, (b"a", 3, b"b", INC)) == (0, 0)         # a bound kind above 2
    assert S.stretch(MG.Table([]), (None, U, None, U)) == (0, 0)
