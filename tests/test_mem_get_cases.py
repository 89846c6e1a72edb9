"""CPU checks of the model of sdb_lsm_get_mem (tests/mem_get_cases.py): the reference's recorded gets with their
mem / imm layers as device-style tables, the same answers whether a layer is a table or an SST, and the model with no
tables against the tree models it continues."""
import pytest

from slatedb_amd import _abi

from . import get_cases as G
from . import mem_get_cases as MG
from . import merge_read_cases as M


def _key_and_bound(c):
    return c["query_key"].encode(), c["max_seq"]


def _row_facts(mt, sst_tree, g_mem, g_sst):
    """(state, value bytes, seq) of a get by the layered model and by the all-SST model."""
    cm = mt.columns(g_mem)
    cs = sst_tree.columns(g_sst)
    vm = MG.value_of(mt, cm) if cm["state"] == _abi.GET_FOUND or cm["state"] == _abi.GET_MERGE_OPERAND else b""
    vs = b""
    if g_sst.row is not None and cs["val_len"]:
        vs = sst_tree.leaves[g_sst.sst].sst.data[cs["val_off"]:cs["val_off"] + cs["val_len"]].tobytes()
    return (cm["state"], cm["status"], vm, cm["seq"], cm["flags"], cm["expire_ts"]), \
        (cs["state"], cs["status"], vs, cs["seq"], cs["flags"], cs["expire_ts"])


@pytest.mark.parametrize("version", [2, 1])
def test_model_reproduces_golden_gets(version):
    cases = G.golden_cases()
    assert len(cases) == G.KEPT_CASES
    with_table = only_tables = 0
    for c in cases:
        mt = MG.golden_mem_tree(c, version)
        with_table += bool(mt.tables)
        only_tables += bool(mt.tables) and not mt.tree.leaves
        key, bound = _key_and_bound(c)
        g = mt.get(key, bound)
        cols = mt.columns(g)
        if c["expected"] is None:
            assert g.state in (_abi.GET_NOT_FOUND, _abi.GET_DELETED), c["description"]
        else:
            assert g.state == _abi.GET_FOUND and MG.value_of(mt, cols) == c["expected"].encode(), c["description"]
        # a layer as a table or as an SST: the same answer
        sst_tree = G.golden_tree(c, version)
        a, b = _row_facts(mt, sst_tree, g, sst_tree.get(key, bound))
        assert a == b, c["description"]
        if g.table != MG.NO_TABLE:  # M3, M5
            assert cols["sst"] == _abi.NO_SST and cols["ssts_read"] == 0 and not g.need and mt.ends_in_tables(key, bound)
    assert with_table >= 16 and only_tables >= 7  # the coverage the fixtures give: no case skipped


@pytest.mark.parametrize("version", [2, 1])
def test_model_reproduces_golden_merge_gets(version):
    cases = M.golden()["get_cases"]
    assert len(cases) == M.KEPT_GET
    for c in cases:
        mt = MG.golden_mem_tree(c, version)
        assert mt.tables, c["description"]  # all 11 have a table layer
        key, bound = _key_and_bound(c)
        g = mt.get_merge(key, bound)
        assert g.status == 0, c["description"]
        assert mt.folded(key, g) == (None if c["expected"] is None else c["expected"].encode()), c["description"]
        # a layer as a table or as an SST: state, value, seq and links agree
        sst_tree = G.golden_tree(c, version)
        s = M.get_merge(sst_tree, key, bound)
        assert (g.state, g.base, g.cts, g.ets) == (s.state, s.base, s.cts, s.ets), c["description"]
        assert len(g.links) == len(s.links)
        for lm, ls in zip(g.links, s.links):
            rm, rs = mt.row_of(lm), sst_tree.leaves[ls[0]].sst.rows[ls[1]]
            assert (rm[0], rm[3], rm[4]) == (rs[0], rs[3], rs[4])
            assert mt.link_bytes(lm) == sst_tree.leaves[ls[0]].sst.data[rs[1]:rs[1] + rs[2]].tobytes()
        assert mt.merge_columns(g)["seq"] == M.get_columns(sst_tree, s)["seq"]
        assert M.folded(sst_tree, key, s.links, s.base) == mt.folded(key, g) or not s.links


def test_no_tables_is_the_tree_model():
    """M6 in the model: with no tables get / get_merge are get_cases.Tree.get / merge_read_cases.get_merge."""
    tree, straddler = M.chain_tree()
    keys = M.chain_queries(tree, straddler)
    bounds = M.chain_bounds(tree, keys)
    mt = MG.MemTree([], tree)
    for k, b in list(zip(keys, bounds)) + [(k, None) for k in keys]:
        g, want = mt.get_merge(k, b), M.get_merge(tree, k, b)
        have = mt.merge_columns(g)
        assert have.pop("table") == MG.NO_TABLE and have.pop("row") == 0
        assert have == M.get_columns(tree, want), k
        assert [l[1:] for l in g.links] == [(i, x, blk) for i, x, blk in want.links]
        p, pw = mt.get(k, b), tree.get(k, b)
        assert p.tree == pw and p.table == MG.NO_TABLE and p.need == pw.need


def test_table_rules():
    """M2 on a table by hand: bounds, an above-bound tombstone, a key that is a prefix of its neighbour."""
    t = MG.Table([(b"a", 0, b"v1", 5, None, None), (b"a", 2, b"", 9, None, None), (b"a\x00", 0, b"n", 7, None, 3),
                  (b"ab", 1, b"op", 8, 4, None), (b"", 0, b"e", 2, None, None)])
    assert [r[0] for r in t.rows] == [b"", b"a", b"a", b"a\x00", b"ab"] and [r[3] for r in t.rows[1:3]] == [9, 5]
    mt = MG.MemTree([t], G.Tree([]))
    assert mt.get(b"a").state == _abi.GET_DELETED and mt.get(b"a", 8).state == _abi.GET_FOUND  # the tombstone above 8 hides nothing
    assert mt.get(b"a", 4).state == _abi.GET_NOT_FOUND and mt.get(b"a", 4).table == MG.NO_TABLE
    assert mt.get(b"").row == 0 and mt.get(b"a\x00").row == 3 and mt.get(b"a\x00", 6).state == _abi.GET_NOT_FOUND
    g = mt.get(b"ab")
    assert (g.state, g.status) == (_abi.GET_MERGE_OPERAND, _abi.SDB_MERGE_OPERATOR_MISSING)
    assert mt.columns(g)["create_ts"] == 4 and mt.columns(mt.get(b"a\x00"))["expire_ts"] == 3
    assert mt.get(b"b").state == _abi.GET_NOT_FOUND and mt.get(b"A").state == _abi.GET_NOT_FOUND


def test_chain_across_layers():
    """M4 by hand: table -> table -> L0 -> sorted run; a tombstone in a table; sequence order per table."""
    t0 = MG.Table([(b"k", 1, b"d", 40, 7, None), (b"k", 1, b"c", 39, None, 90)])
    t1 = MG.Table([(b"k", 1, b"b", 30, 9, 50)])
    tree = G.Tree([[G.leaf_of([(b"k", 1, b"a", 20, None, None)], 2, 4096)], [G.leaf_of([(b"k", 0, b"base", 10, None, None)], 1, 4096)]])
    mt = MG.MemTree([t0, t1], tree)
    g = mt.get_merge(b"k")
    assert [l[0] for l in g.links] == ["t", "t", "t", "s", "s"] and g.base and (g.cts, g.ets) == (9, 50)
    assert mt.folded(b"k", g) == b"baseabcd" and g.state == _abi.GET_MERGE_OPERAND and g.ssts_read == 2
    assert not mt.ends_in_tables(b"k", None, True) and mt.ends_in_tables(b"k", None, False)
    dead = MG.MemTree([t0, MG.Table([(b"k", 2, b"", 35, 1, 2)])], tree)
    g = dead.get_merge(b"k")
    assert len(g.links) == 2 and not g.base and (g.cts, g.ets) == (7, 90) and not g.need and g.ssts_read == 0
    assert dead.ends_in_tables(b"k", None, True) and dead.folded(b"k", g) == b"cd"
    wrong = MG.MemTree([t1, t0], tree)
    assert wrong.get_merge(b"k").status == _abi.SDB_INVALID_SEQUENCE_ORDER
    assert wrong.get_merge(b"k", 30).status == 0
