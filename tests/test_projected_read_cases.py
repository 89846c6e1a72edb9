"""The model of the projected tree reads (tests/projected_read_cases.py) against the reference's own pins
(tests/golden/projection_cases.json), against a second, independent oracle (every projected SST physically trimmed
to its visible rows and read without projections), and the non-vacuity of the seeded sweep the device tests run."""
import pytest

from slatedb_amd import _abi

from . import filtered_read_cases as F
from . import get_cases as G
from . import lsm_scan_cases as L
from . import projected_read_cases as P
from .scan_cases import EXC, INC, U

ALL = (None, U, None, U)


def value_leaf(keys, version=2, block_size=64):
    return G.leaf_of([(k, 0, b"value", 7, None, None) for k in keys], version, block_size)


def plain_scan_keys(tree, visible, rng):
    return [r[0] for r in P.scan(tree, visible, rng).rows]


# ------------------------------------------------------------------------------------------------
# The reference's pins
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [1, 2])
def test_golden_sst_iterator(version):
    g = P.golden()["sst_iter"]
    tree = P.projected(G.Tree([[value_leaf([k.encode() for k in g["keys"]], version)]]), [P.golden_range(g["visible"])])
    assert plain_scan_keys(tree, tree.visible, ALL) == [k.encode() for k in g["full_scan"]]
    out = P.scan(tree, tree.visible, P.golden_range(g["no_iterator_range"]))
    assert out.ssts == [] and out.rows == [] and out.blocks == set() and out.filtered == []
    for k in g["keys"]:  # the gets see the same keys
        assert (tree.get(k.encode()).state == _abi.GET_FOUND) == (k in g["full_scan"]), k


@pytest.mark.parametrize("version", [1, 2])
def test_golden_sorted_run(version):
    g = P.golden()["sorted_run"]
    run = [value_leaf([k.encode() for k in s["keys"]], version) for s in g["ssts"]]
    tree = P.projected(G.Tree([run]), [P.golden_range(s["visible"]) for s in g["ssts"]])
    assert plain_scan_keys(tree, tree.visible, ALL) == [k.encode() for k in g["full_scan"]]
    for s in g["ssts"]:
        for k in s["keys"]:
            got = tree.get(k.encode())
            assert (got.state == _abi.GET_FOUND) == (k in g["full_scan"]), k
            assert got.ssts_read == int(k in g["full_scan"])


def _physical(view):
    last = view["last"]
    return (view["first"].encode(), INC, None if last is None else last.encode(), U if last is None else INC)


def test_golden_effective_ranges_and_cover_counts():
    want = {"max_l0_overlap_edge_touching_exclusive_end_is_disjoint": [(b"a", INC, b"b", EXC), (b"b", INC, b"c", INC)],
            "max_l0_overlap_unbounded_end_via_visible_range": [(b"m", INC, b"z", INC), (b"n", INC, b"", U)],
            "max_l0_overlap_respects_visible_range": [(b"a", INC, b"m", EXC), (b"m", INC, b"z", INC)]}
    probes = [bytes([c]) + t for c in range(ord("a") - 1, ord("z") + 2) for t in (b"", b"\x00")]
    cases = P.golden()["overlap"]["cases"]
    assert sorted(c["name"] for c in cases) == sorted(want)
    for c in cases:
        E = [P.intersect(_physical(v), P.golden_range(v["visible"])) for v in c["views"]]
        assert E == want[c["name"]], c["name"]
        assert max(sum(P.holds(e, k) for e in E) for k in probes) == c["max_overlap"], c["name"]


def test_golden_key_gap():
    g = P.golden()["key_gap"]
    keys = {"a": [b"a", b"b", b"c"], "m": [b"m", b"n", b"p"]}
    run = [value_leaf(keys[s["first"]]) for s in g["run"]]
    assert [(l.first_key, l.last_key) for l in run] == [(s["first"].encode(), s["last"].encode()) for s in g["run"]]
    for c in g["cases"]:
        glob = P.golden_range(c["global_range"])
        vis = [P.intersect(P.golden_range(s["visible"]), glob) or glob for s in g["run"]]
        tree = P.projected(G.Tree([run]), vis)
        E = [P.effective(l, v) for l, v in zip(tree.leaves, vis)]
        assert sum(e is not None for e in E) == c["ssts_kept"], c["name"]
        full = P.scan(tree, vis, ALL)
        assert len(full.ssts) == c["ssts_kept"]
        for k in sum(keys.values(), []) + [b"e", b"f", b"d"]:
            got = tree.get(k)
            assert (got.state == _abi.GET_FOUND) == any(P.holds(e, k) for e in E) == (k in [r[0] for r in full.rows])
        if not c["ssts_kept"]:
            assert full.rows == [] and all(tree.get(k).ssts_read == 0 for k in (b"a", b"c", b"e", b"m"))


def test_intersect_orders_the_bounds():
    assert P.intersect((b"a", INC, b"k", INC), (b"a", EXC, b"k", EXC)) == (b"a", EXC, b"k", EXC)
    assert P.intersect((None, U, b"k", INC), (b"c", INC, None, U)) == (b"c", INC, b"k", INC)
    assert P.intersect((b"c", INC, b"c", INC), (b"c", INC, b"d", EXC)) == (b"c", INC, b"c", INC)
    assert P.intersect((b"c", INC, b"c", INC), (b"c", EXC, None, U)) is None
    assert P.intersect((b"a", INC, b"c", EXC), (b"c", INC, b"d", INC)) is None
    assert P.intersect(P.OPEN, P.OPEN) == P.OPEN


# ------------------------------------------------------------------------------------------------
# The second oracle, and the sweep
# ------------------------------------------------------------------------------------------------
_main = {}


def main():
    if not _main:
        tree = F.main_tree()
        _main.update(tree=tree, cases=F.scan_cases(tree), keys=F.get_keys(tree))
    return _main


@pytest.mark.parametrize("seed", P.SWEEP_SEEDS)
def test_scans_agree_with_trimmed_ssts(seed):
    m = main()
    tree = m["tree"]
    vis = P.random_projections(tree, seed)
    cut = P.trimmed(tree, vis)
    bounds = [None, 10**6 - 300]
    for q, (rng, prefix, pl) in enumerate(m["cases"]):
        if not F.honours_f4(tree, rng, prefix):
            continue
        for desc in (False, True):
            a = P.scan(tree, vis, rng, prefix, pl, bounds[q % 2], desc)
            b = L.scan(cut, rng, bounds[q % 2], desc)
            assert a.status == b.status, (q, rng)
            assert [P.row_value(tree, i, x) for _, i, x in a.rows] == [P.row_value(cut, i, x) for _, i, x in b.rows], (q, rng)
            assert [r[1] for r in a.rows] == [r[1] for r in b.rows]  # the SSTs keep their places


@pytest.mark.parametrize("seed", P.SWEEP_SEEDS)
def test_gets_agree_with_trimmed_ssts(seed):
    m = main()
    tree = m["tree"]
    vis = P.random_projections(tree, seed)
    ptree, cut = P.projected(tree, vis), P.trimmed(tree, vis)
    found = 0
    for q, k in enumerate(m["keys"]):
        bound = None if q % 3 else 10**6 - 200
        a, b = ptree.get(k, bound, F.LENGTHS_LEN), cut.get(k, bound)
        assert (a.state, a.sst, a.status) == (b.state, b.sst, b.status), k
        if a.row is not None:
            assert P.row_value(tree, a.sst, a.row) == P.row_value(cut, b.sst, b.row), k
            found += 1
    assert found >= 100


def test_gets_agree_with_trimmed_ssts_in_a_tree_of_operands():
    tree, straddler = G.main_tree()
    for seed in P.SWEEP_SEEDS:
        vis = P.random_projections(tree, seed)
        ptree, cut = P.projected(tree, vis), P.trimmed(tree, vis)
        for k in G.main_queries(tree, straddler)[::3] + [straddler]:
            a, b = ptree.get(k), cut.get(k)
            assert (a.state, a.sst, a.status) == (b.state, b.sst, b.status), k
            if a.row is not None:
                assert P.row_value(tree, a.sst, a.row) == P.row_value(cut, b.sst, b.row), k


@pytest.mark.parametrize("seed", P.SWEEP_SEEDS)
def test_the_sweep_is_not_vacuous(seed):
    m = main()
    vis = P.random_projections(m["tree"], seed)
    pairs, still, lose = P.sweep_stats(m["tree"], vis, m["cases"])
    assert pairs >= 100
    assert 2 * still >= pairs, (pairs, still)  # at least half of the pairs still take part
    assert 4 * lose >= pairs, (pairs, lose)  # at least a quarter lose a candidate to the projection
    assert sum(v is None for v in vis) < len(vis)


def test_open_projections_change_nothing():
    m = main()
    tree = m["tree"]
    for vis in ([None] * len(tree.leaves), [P.OPEN] * len(tree.leaves)):
        for rng, prefix, pl in m["cases"]:
            assert P.scan(tree, vis, rng, prefix, pl) == F.scan(tree, rng, prefix, pl)
        ptree = P.projected(tree, vis)
        for k in m["keys"][::5]:
            assert ptree.get(k, None, F.LENGTHS_LEN) == tree.get(k, None, F.LENGTHS_LEN)


def test_edge_tree_conditions():
    """What the device test of the bound positions needs of its tree: conditions on the input and the model alone."""
    tree = P.edge_tree()
    assert len(tree.leaves) == 12 and [l.version for l in tree.leaves] == [2] * 6 + [1] * 6
    for l in (tree.leaves[0], tree.leaves[6]):
        s = l.sst
        blocks = {b for b in range(s.nb) for x in range(s.bes[b], s.bes[b + 1]) if s.keys[x] == P.LONG}
        assert len(blocks) >= 4 and s.nb <= 40  # LONG's versions fill whole blocks: the inward walks of the edge step
    rngs = P.edge_ranges(tree)
    seqs = P.long_seqs(tree)
    for side in ("start", "end"):
        vis = P.edge_projections(tree, side)
        assert all(v[1] in (U, INC) for v in vis)
        free = [F.scan(tree, r) for r in rngs]
        proj = [P.scan(tree, vis, r) for r in rngs]
        assert sum(p.candidates < f.candidates for p, f in zip(proj, free)) >= len(rngs) // 2
        assert sum(p.candidates for p in proj) >= 1000 and sum(len(p.rows) for p in proj) >= 100
        cut = P.trimmed(tree, vis)
        for r, p in zip(rngs, proj):
            for bound in (None, seqs[len(seqs) // 2]):
                a, b = P.scan(tree, vis, r, max_seq=bound), L.scan(cut, r, bound)
                assert [P.row_value(tree, i, x) for _, i, x in a.rows] == [P.row_value(cut, i, x) for _, i, x in b.rows]


def test_get_shape_conditions():
    tree, vis, k = P.straddle_run()
    pt = P.projected(tree, vis)
    left = [r[3] for r in tree.leaves[0].sst.rows if r[0] == k]
    right = [r[3] for r in tree.leaves[1].sst.rows if r[0] == k]
    assert left and right and min(left) > max(right) and pt.chain(k) == [1] and F.Tree(tree.runs).chain(k) == [0, 1]
    got = pt.get(k)
    assert got.sst == 1 and got.ssts_read == 1 and tree.leaves[1].sst.rows[got.row][3] == max(right)
    assert pt.get(k, min(right) - 1).state == _abi.GET_NOT_FOUND  # below the visible versions
    assert pt.get(k, max(left)).sst == 1  # above them: the hidden, newer versions do not answer
    assert pt.chain(b"") == [] and pt.chain(b"t00") == []  # below every effective start
    tree, vis = P.hidden_l0()
    pt = P.projected(tree, vis)
    g = pt.get(P.K1)
    assert (g.state, g.sst, g.ssts_read, g.ssts_filtered) == (_abi.GET_FOUND, 1, 1, 0)
    assert P.row_value(tree, 1, g.row)[3] == b"old" and F.Tree(tree.runs).get(P.K1).sst == 0
    assert [r for r in P.scan(tree, vis, (None, U, P.K2, EXC)).rows if r[0] == P.K1] == [(P.K1, 1, g.row)]
    assert P.scan(tree, vis, ALL).status == _abi.SDB_MERGE_OPERATOR_MISSING  # K2's winner is the older SST's operand
    from . import merge_read_cases as M
    mg = M.get_merge(P.merge_view(tree, vis), P.K2)
    assert [i for i, _, _ in mg.links] == [1, 1, 1] and mg.base and mg.ssts_read == 1
    assert [i for i, _, _ in M.get_merge(F.Tree(tree.runs), P.K2).links] == [0, 1, 1, 1]


def test_point_by_projection_asks_point():
    """A wide range over an SST whose visible range holds one absent key: Point(k) rules the SST out (P4); under a
    LENGTHS policy the pair has no length, so the SST takes part."""
    tree, present, absent = P.point_tree()
    assert all(present in l.sst.keys and absent not in l.sst.keys and l.first_key < absent < l.last_key for l in tree.leaves)
    wide = F.prefix_range(F.tenant(1))
    for prefix in (None, F.tenant(1)):
        out = P.scan(tree, [(absent, INC, absent, INC)] * 3, wide, prefix, F.LENGTHS_LEN)
        assert out.rows == [] and out.candidates == 0
        assert out.filtered == [0] and out.ssts == [1, 2]  # the full key under FIXED(4) with whole keys
        # LENGTHS without whole keys: no length, None; DELIM probes "t01:", which the SST holds
        out = P.scan(tree, [(present, INC, present, INC)] * 3, wide, prefix, F.LENGTHS_LEN)
        assert [r[0] for r in out.rows] == [present] and out.ssts == [0, 1, 2] and out.candidates == 3
    # the range's own point keeps its probe_len: LENGTHS probes "t01", DELIM "t01:", FIXED the full key
    out = P.scan(tree, [None] * 3, (absent, INC, absent, INC), None, F.LENGTHS_LEN)
    assert out.filtered == [0] and out.ssts == [1, 2]
