"""GPU parity of sdb_lsm_get_mem (device memtables in front of the tree, slatedb_amd/csrc/sdb_get.hip) against the
model of tests/mem_get_cases.py, every column of every query and link: the search's boundaries, the order of the
layers, the reference's recorded cases, chains across layers, laziness (M5), no tables (M6), no tree (M7), a
malformed table (M9), tables straight from the WAL replay, HIP graph capture with workspace reuse, and a workspace
canary."""
import random

import numpy as np
import pytest

from slatedb_amd import _abi, merge, replay

from . import get_cases as G
from . import mem_get_cases as MG
from . import merge_read_cases as M
from . import replay_cases as R
from . import test_gpu_get as TG
from .read_harness import (canaried_workspace, check_get_summary, compare, dev_tables, dev_tree, host, intact, rt, to_dev,  # noqa: F401
                           u64, view_of)

pytestmark = pytest.mark.gpu

U64_MAX = G.U64_MAX
SENTINEL = 0x5A
GET_COLS = ("state", "status", "sst", "block", "val_off", "val_len", "seq", "flags", "ssts_read", "ssts_filtered", "table",
            "row")
LINK_COLS = ("sst", "block", "val_off", "val_len", "seq", "flags", "table", "row")


def call(rt, mem, dev, keys, bounds=None, chain=False, **kw):
    return host(rt.lsm_get_mem_device(mem, dev, None, keys, max_seq=bounds, merge=chain, fill=SENTINEL, **kw))


def _columns(cols, keys, h, skip=()):
    compare([f for f in GET_COLS if f not in skip], [dict(c, key=k) for c, k in zip(cols, keys)], lambda f: h[f], "get")


def _blocks(mt, keys, bounds, got, h, chain):
    """blocks_checked: at least what the queries need, at most what the queries the tables do not end cover (M5)."""
    need = set().union(*[g.need for g in got]) if got else set()
    cover = set()
    for q, k in enumerate(keys):
        cover |= mt.covering_blocks(k, None if bounds is None else bounds[q], chain)
    assert need <= cover
    assert len(need) <= h["sum_blocks_checked"] <= len(cover), (len(need), h["sum_blocks_checked"], len(cover))


def check(mt, keys, bounds, h, skip=()):
    """A call without a chain: every column of every query, table and row, the summary.  Returns the model's results."""
    got = [mt.get(k, None if bounds is None else bounds[q]) for q, k in enumerate(keys)]
    _columns([mt.columns(g) for g in got], keys, h, skip)
    check_get_summary(got, [q for q, g in enumerate(got) if g.status and g.state == _abi.GET_NOT_FOUND], h)
    _blocks(mt, keys, bounds, got, h, False)
    return got


def check_chain(mt, keys, bounds, h, cap=1 << 40):
    """A call with a chain: the per-query columns, the links with their layer, both summaries."""
    n = len(keys)
    got = [mt.get_merge(k, None if bounds is None else bounds[q]) for q, k in enumerate(keys)]
    _columns([mt.merge_columns(g) for g in got], keys, h)
    check_get_summary(got, [q for q, g in enumerate(got) if g.status], h)
    _blocks(mt, keys, bounds, got, h, True)
    chains = [g.links for g in got]
    starts = np.concatenate([[0], np.cumsum([len(c) for c in chains])]).astype(np.int64)
    assert (h["chain_start"][:n + 1].astype(np.int64) == starts).all()
    total = int(starts[-1])
    assert h["csum_num_links"] == total and h["csum_max_chain_len"] == max([len(c) for c in chains] + [0])
    if total > cap:
        assert h["csum_status"] == _abi.SDB_LIMIT_EXCEEDED
        for f in LINK_COLS + ("create_ts", "expire_ts"):
            assert (h["chain_" + f].view(np.uint8) == SENTINEL).all(), f  # no link column written
        return got
    assert h["csum_status"] == 0
    compare(LINK_COLS, [mt.link_columns(l) for c in chains for l in c], lambda f: h["chain_" + f], "link")
    for f in LINK_COLS:  # nothing behind the last link
        assert (h["chain_" + f][total:].view(np.uint8) == SENTINEL).all(), f
    return got


# ------------------------------------------------------------------------------------------------
# Search boundaries (M2), on tables alone (M7)
# ------------------------------------------------------------------------------------------------
SIZES = (0, 1, 2, 3, 5, 64, 65, 257)
LONG = b"L" * 299
SPECIAL = [b"", b"a", b"a\x00", b"ab", LONG + b"x", LONG + b"y"]


def boundary_table(n, seed):
    """A table of exactly n rows: keys with 1 to 6 versions; the special neighbours (the empty key, a / a\\0 / ab, two
    300-byte keys that differ in the last byte) from 64 rows on, some of them in the small tables."""
    rng = random.Random(1000 * n + seed)
    pool = SPECIAL + [b"k%03d" % (3 * i) for i in range(120)]
    if n < 64:
        rng.shuffle(pool)
    es, seq = [], 10**6 + seed
    for key in pool:
        for _ in range(rng.randint(1, 6)):
            if len(es) == n:
                break
            kind = rng.choice([0, 0, 0, 2, 1])
            es.append((key, kind, b"" if kind == 2 else bytes(rng.randrange(256) for _ in range(rng.choice([0, 1, 9, 40]))),
                       seq, rng.choice([None, rng.randrange(1, 1 << 40)]), rng.choice([None, None, rng.randrange(1, 1 << 40)])))
            seq -= rng.randint(1, 3)
    assert len(es) == n
    return MG.Table(es)


def boundary_queries(tables):
    """(keys, bounds): around every key of the tables, and for every key bounds around each of its versions."""
    keys, bounds = [], []

    def add(k, b):
        keys.append(k)
        bounds.append(U64_MAX if b is None else max(0, int(b)))

    present = sorted({r[0] for t in tables for r in t.rows})
    for k in [b"", b"\x00", b"a", b"a\x00", b"a\x00\x00", b"ab", b"b", LONG, LONG + b"x", LONG + b"y", LONG + b"z", b"zzzz",
              b"\xff" * 5]:
        add(k, None)
    for t in tables:
        if t.rows:
            first, last = t.rows[0][0], t.rows[-1][0]
            for k in (first, last, first[:-1], last + b"\x00", last[:-1] + b"\xff" if last else b"\x01"):
                add(k, None)
    for k in present:
        add(k + b"\x00", None)  # between neighbours; the key is a proper prefix of this one
        add(k[:-1], None)
        seqs = sorted({r[3] for t in tables for r in t.rows if r[0] == k}, reverse=True)
        for b in [None, seqs[0] + 1, seqs[-1] - 1, 0] + seqs + [s - 1 for s in seqs]:
            add(k, b)
    return keys, bounds


@pytest.mark.parametrize("size", SIZES + ("all",))
def test_search_boundaries(rt, size):
    tables = [boundary_table(n, j) for j, n in enumerate(SIZES)] if size == "all" else [boundary_table(size, 0)]
    mt = MG.MemTree(tables, G.Tree([]))
    keys, bounds = boundary_queries(tables)
    mem, dev = dev_tables(rt, tables), dev_tree(rt, mt.tree)
    assert dev["num_ssts"] == 0
    got = check(mt, keys, bounds, call(rt, mem, dev, keys, bounds))
    h = call(rt, mem, dev, keys)  # max_seq NULL
    free = check(mt, keys, None, h)
    assert h["sum_blocks_checked"] == 0
    if size == "all" or size >= 64:
        states = {g.state for g in got}
        assert {_abi.GET_FOUND, _abi.GET_DELETED, _abi.GET_NOT_FOUND} <= states
        # a bound below a key's versions lands on the next key, or on n for the last key: nothing found
        last = tables[-1].rows[-1]
        assert any(k == last[0] and b < last[3] and g.state == _abi.GET_NOT_FOUND for k, b, g in zip(keys, bounds, got))
        assert any(g.row > 0 and f.table == g.table and f.row < g.row for g, f in zip(got, free) if g.table != MG.NO_TABLE)
    if size == "all":
        assert {g.table for g in got} >= set(range(1, len(SIZES)))  # every table with rows decides some query
    elif size >= 64:
        assert any(g.row == size - 1 for g in got) and any(g.table == 0 and g.row == 0 for g in got)  # the last row, the first
    check_chain(mt, keys, bounds, call(rt, mem, dev, keys, bounds, chain=True))


# ------------------------------------------------------------------------------------------------
# Layer order: three tables over the main tree of get_cases.py
# ------------------------------------------------------------------------------------------------
_layers = {}


def layers(rt):
    """The main tree under three tables, built once.  By key number (even: in the tree) modulo 12:
    0   a value in tables 0 and 2 (and in L0 for many)     2   a tombstone in table 0 above a value in table 1
    4   a tombstone in table 1 (hides what the tree has)   6   a merge operand in table 2
    8, 10 only in the tree;  odd numbers are absent but for 1 modulo 12: a value in table 2 only."""
    if _layers:
        return _layers
    m = TG.main(rt)
    tree = m["tree"]
    t0, t1, t2 = [], [], []
    for i in range(0, 400):
        k = b"k%05d" % i
        if i % 12 == 0:
            t0.append((k, 0, b"new%d" % i, 3_000_000 + i, i if i % 24 == 0 else None, None))
            t2.append((k, 0, b"old%d" % i, 1_500_000 + i, None, 77 + i))
        elif i % 12 == 2:
            t0.append((k, 2, b"", 3_000_000 + i, None, None))
            t1.append((k, 0, b"under%d" % i, 2_000_000 + i, None, None))
        elif i % 12 == 4:
            t1.append((k, 2, b"", 2_000_000 + i, 5, 6))
        elif i % 12 == 6:
            t2.append((k, 1, b"+%d" % i, 1_500_000 + i, None, None))
            t2.append((k, 1, b"-%d" % i, 1_400_000 + i, 9, None))
        elif i % 12 == 1:
            t2.append((k, 0, b"only", 1_500_000 + i, None, None))
    tables = [MG.Table(t) for t in (t0, t1, t2)]
    mt = MG.MemTree(tables, tree)
    keys, bounds = G.bounded_queries(tree, m["queries"], m["straddler"])
    for t in tables:  # and every table version as a bound, and just under it
        for r in t.rows:
            keys += [r[0], r[0]]
            bounds += [r[3], r[3] - 1]
    _layers.update(mt=mt, tables=tables, mem=dev_tables(rt, tables), dev=m["dev"], queries=m["queries"], keys=keys,
                   bounds=bounds)
    return _layers


def test_layer_order(rt):
    s = layers(rt)
    mt, tree = s["mt"], s["mt"].tree
    free = check(mt, s["queries"], None, call(rt, s["mem"], s["dev"], s["queries"]))
    got = check(mt, s["keys"], s["bounds"], call(rt, s["mem"], s["dev"], s["keys"], s["bounds"]))
    by_key = dict(zip(s["queries"], free))
    assert by_key[b"k00024"].table == 0 and tree.get(b"k00024").state != _abi.GET_NOT_FOUND  # tables 0, 2 and the tree
    hidden = [k for k, g in by_key.items() if g.table == 1 and g.state == _abi.GET_DELETED and tree.get(k).state == _abi.GET_FOUND]
    assert len(hidden) >= 5  # a tombstone in table 1 hides an L0 / sorted-run value
    # an above-bound tombstone in table 0 does not hide table 1's value
    assert any(g.table == 1 and g.state == _abi.GET_FOUND and by_key[k].table == 0 and by_key[k].state == _abi.GET_DELETED
               for k, g in zip(s["keys"], got))
    assert sum(1 for g in free if g.table == MG.NO_TABLE and g.state == _abi.GET_FOUND) >= 30  # only in the tree
    assert sum(1 for g in free if g.table == MG.NO_TABLE and g.state == _abi.GET_NOT_FOUND) >= 30  # absent
    assert {g.table for g in free} == {0, 1, 2, MG.NO_TABLE} and any(g.state == _abi.GET_MERGE_OPERAND and g.table == 2 for g in free)
    # under a bound below every table version the tree answers as if there were no tables
    assert any(g.table == MG.NO_TABLE and g.tree.row is not None and by_key[k].table != MG.NO_TABLE for k, g in zip(s["keys"], got))
    cg = check_chain(mt, s["keys"], s["bounds"], call(rt, s["mem"], s["dev"], s["keys"], s["bounds"], chain=True))
    assert any(g.links and g.links[0][0] == "t" and g.links[-1][0] == "s" for g in cg)  # a chain from a table into the tree


# ------------------------------------------------------------------------------------------------
# The reference's recorded cases
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [2, 1])
def test_golden_get_cases(rt, version):
    cases = G.golden_cases()
    assert len(cases) == G.KEPT_CASES
    for c in cases:
        mt = MG.golden_mem_tree(c, version, bloom=(len(c["entries"]) % 2 == 0))
        key = c["query_key"].encode()
        bounds = None if c["max_seq"] is None else [c["max_seq"]]
        h = call(rt, dev_tables(rt, mt.tables) if mt.tables else None, dev_tree(rt, mt.tree), [key], bounds)
        got = check(mt, [key], bounds, h)
        if c["expected"] is None:
            assert int(h["state"][0]) in (_abi.GET_NOT_FOUND, _abi.GET_DELETED), c["description"]
        else:
            assert int(h["state"][0]) == _abi.GET_FOUND, c["description"]
            cols = {f: int(u64(h[f][:1], f)[0]) for f in ("val_off", "val_len", "table", "sst")}
            assert MG.value_of(mt, cols) == c["expected"].encode(), c["description"]
        assert got[0].table == (int(h["table"][0]) & 0xFFFFFFFF)


@pytest.mark.parametrize("version", [2, 1])
def test_golden_merge_cases(rt, version):
    cases = M.golden()["get_cases"]
    assert len(cases) == M.KEPT_GET
    for c in cases:
        mt = MG.golden_mem_tree(c, version)
        key = c["query_key"].encode()
        bounds = None if c["max_seq"] is None else [c["max_seq"]]
        h = call(rt, dev_tables(rt, mt.tables), dev_tree(rt, mt.tree), [key], bounds, chain=True)
        check_chain(mt, [key], bounds, h)
        out = merge.fold_chains_mem([key], h, MG.host_tables(mt.tables), [l.sst.data for l in mt.tree.leaves], M.OP)
        assert out[0] == (None if c["expected"] is None else c["expected"].encode()), c["description"]


# ------------------------------------------------------------------------------------------------
# Chains across layers (M4)
# ------------------------------------------------------------------------------------------------
def test_chains(rt):
    op = lambda k, v, s, cts=None, ets=None: (k, 1, v, s, cts, ets)  # noqa: E731
    val = lambda k, v, s, cts=None, ets=None: (k, 0, v, s, cts, ets)  # noqa: E731
    t0 = MG.Table([op(b"one", b"3", 93), op(b"one", b"2", 92, 11, None), op(b"one", b"1", 91, None, 500), val(b"one", b"base", 90, 4, 900),
                   op(b"one", b"below", 89),                                        # behind the base: never a link
                   op(b"far", b"d", 80, 7), op(b"far", b"c", 79, None, 60),          # table -> table -> L0 -> sorted run
                   op(b"dead", b"y", 70, 1, 2), op(b"dead", b"x", 69),               # ended by table 1's tombstone
                   op(b"open", b"q", 60),                                            # an exhausted chain
                   op(b"bad", b"n", 50)])                                            # table 1 holds a higher seq
    t1 = MG.Table([op(b"far", b"b", 78, 9, 50), (b"dead", 2, b"", 68, 100, 1), val(b"dead", b"gone", 67), op(b"bad", b"m", 55),
                   val(b"plain", b"p", 40, None, 8)])
    tree = G.Tree([[G.leaf_of([op(b"far", b"a", 30), op(b"open", b"p", 29, 3, 4), val(b"zz", b"z", 28)], 2, 4096)],
                   [G.leaf_of([val(b"far", b"base", 10, None, 70), val(b"dead", b"older", 9), val(b"bad", b"l", 8)], 1, 4096)]])
    mt = MG.MemTree([t0, t1], tree)
    keys = [b"one", b"far", b"dead", b"open", b"bad", b"plain", b"zz", b"none", b"far", b"one", b"bad"]
    bounds = [U64_MAX] * 8 + [79, 91, 50]
    mem, dev = dev_tables(rt, mt.tables), dev_tree(rt, tree)
    h = call(rt, mem, dev, keys, bounds, chain=True)
    got = check_chain(mt, keys, bounds, h)
    by = dict(zip(keys[:8], got))
    assert [l[0] for l in by[b"one"].links] == ["t"] * 4 and by[b"one"].base and (by[b"one"].cts, by[b"one"].ets) == (11, 500)
    assert [l[:2] for l in by[b"far"].links] == [("t", 0), ("t", 0), ("t", 1), ("s", 0), ("s", 1)] and by[b"far"].ets == 50
    assert len(by[b"dead"].links) == 2 and not by[b"dead"].base and (by[b"dead"].cts, by[b"dead"].ets) == (1, 2)  # not folded
    assert len(by[b"open"].links) == 2 and not by[b"open"].base and by[b"open"].state == _abi.GET_MERGE_OPERAND
    assert by[b"bad"].status == _abi.SDB_INVALID_SEQUENCE_ORDER and got[10].status == 0
    out = merge.fold_chains_mem(keys, h, MG.host_tables(mt.tables), [l.sst.data for l in tree.leaves], M.OP)
    assert out[:4] == [b"base123", b"baseabcd", b"xy", b"pq"] and out[4] is None and out[5] == b"p"
    total = sum(len(g.links) for g in got)
    short = call(rt, mem, dev, keys, bounds, chain=True, cap_links=total - 1)
    check_chain(mt, keys, bounds, short, cap=total - 1)
    assert short["csum_num_links"] == total and short["csum_status"] == _abi.SDB_LIMIT_EXCEEDED
    check_chain(mt, keys, bounds, call(rt, mem, dev, keys, bounds, chain=True, cap_links=total), cap=total)
    check(mt, keys, bounds, call(rt, mem, dev, keys, bounds))  # the same layers without a chain


# ------------------------------------------------------------------------------------------------
# Laziness (M5)
# ------------------------------------------------------------------------------------------------
def test_laziness(rt):
    m = TG.main(rt)
    tree, keys = m["tree"], m["queries"]
    i = 2  # the second L0 SST with entries, as test_get_lazy_errors breaks it
    leaf = tree.leaves[i]
    bad, reach, _, _ = TG.pick_bad_block(tree, i, keys)
    runs, j = [], 0
    for r in tree.runs:  # ... and the L0 SST after it claims an invalid version
        runs.append([G.Leaf(l.sst, l.bloom is not None, {bad: _abi.SDB_CHECKSUM_MISMATCH} if j + x == i else None,
                            3 if j + x == 3 else l.version) for x, l in enumerate(r)])
        j += len(r)
    broken = G.Tree(runs)
    views = [view_of(l) for l in broken.leaves]
    data = leaf.sst.data.copy()
    data[int(leaf.sst.block_off[bad]) + 5] ^= 0x40
    views[i] = view_of(broken.leaves[i], data=data)
    dev = dev_tree(rt, broken, views)
    plain = [broken.get(k) for k in keys]
    failing = [q for q, g in enumerate(plain) if g.status in (_abi.SDB_CHECKSUM_MISMATCH, _abi.SDB_INVALID_VERSION)]
    assert set(reach) <= set(failing) and {plain[q].status for q in failing} == {_abi.SDB_CHECKSUM_MISMATCH, _abi.SDB_INVALID_VERSION}
    saved = failing[::2]  # a table decides every other failing query; the rest still need the tree
    left = [q for q in failing if keys[q] not in {keys[x] for x in saved}]
    assert saved and left
    tab = MG.Table([(keys[q], 0, b"mem%d" % q, 5_000_000 + q, None, None) for q in sorted(set(saved), key=lambda q: keys[q])])
    opt = MG.Table([(keys[q], 1, b"op%d" % q, 6_000_000 + q, None, None) for q in sorted(set(saved), key=lambda q: keys[q])])
    for chain, tables in ((False, [tab]), (True, [opt, tab])):  # with a chain: an operand, then the base value that ends it
        mt = MG.MemTree(tables, broken)
        mem = dev_tables(rt, tables)
        h = call(rt, mem, dev, keys, None, chain=chain)
        got = (check_chain if chain else check)(mt, keys, None, h)
        for q in saved:  # decided in the tables: clean, and no SST consulted
            assert got[q].status == 0 and int(h["status"][q]) == 0 and int(h["ssts_read"][q]) == 0 and int(h["ssts_filtered"][q]) == 0
            assert (int(h["table"][q]) & 0xFFFFFFFF) == 0
        for q in left:  # undecided and in need of the block / the view: the error
            assert int(h["status"][q]) == plain[q].status and int(h["state"][q]) == _abi.GET_NOT_FOUND
        only = [keys[q] for q in saved]
        ho = call(rt, mem, dev, only, None, chain=chain)
        (check_chain if chain else check)(mt, only, None, ho)
        assert ho["sum_blocks_checked"] == 0 and ho["sum_num_failed"] == 0
        assert ho["sum_num_merge" if chain else "sum_num_found"] == len(only)


# ------------------------------------------------------------------------------------------------
# No tables (M6), no tree (M7), a malformed table (M9)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [False, True])
def test_no_tables_is_the_projected_call(rt, chain):
    s = layers(rt)
    keys, bounds = s["keys"], s["bounds"]
    n = len(keys)
    want = host(rt.lsm_get_projected_device(s["dev"], None, None, keys, max_seq=bounds, merge=chain, fill=SENTINEL))
    for mem in (None, rt.mem_tables_device([])):
        h = call(rt, mem, s["dev"], keys, bounds, chain=chain)
        for f, a in want.items():
            assert np.array_equal(a, h[f]), f  # every column, both summaries, chain_start and the link columns
        assert ((h["table"][:n].astype(np.int64) & 0xFFFFFFFF) == MG.NO_TABLE).all() and not h["row"][:n].any()
        if chain:
            total = int(h["csum_num_links"])
            assert total > 100
            assert ((h["chain_table"][:total].astype(np.int64) & 0xFFFFFFFF) == MG.NO_TABLE).all() and not h["chain_row"][:total].any()
            assert (h["chain_table"][total:].view(np.uint8) == SENTINEL).all()
    (check_chain if chain else check)(MG.MemTree([], s["mt"].tree), keys, bounds, h)


def test_no_tree(rt):
    s = layers(rt)
    tables, keys, bounds = s["tables"], s["keys"][:300], s["bounds"][:300]
    of_empty = G.Tree([[G.Leaf(G.EmptySst())], [G.Leaf(G.EmptySst()), G.Leaf(G.EmptySst())]])
    for tree in (G.Tree([]), of_empty):  # num_ssts == 0; SSTs without a block: total_blocks == 0
        dev = dev_tree(rt, tree)
        assert dev["total_blocks"] == 0
        mt = MG.MemTree(tables, tree)
        got = check(mt, keys, bounds, call(rt, s["mem"], dev, keys, bounds))
        assert sum(1 for g in got if g.table != MG.NO_TABLE) >= 20
        h = call(rt, s["mem"], dev, keys, bounds, chain=True)
        check_chain(mt, keys, bounds, h)
        assert h["sum_blocks_checked"] == 0
    h = call(rt, s["mem"], s["dev"], [], None, chain=True)  # tables present, no key
    assert not h["summary"].any() and not h["chain_summary"].any() and int(h["chain_start"][0]) == 0
    assert not call(rt, s["mem"], s["dev"], [])["summary"].any()


def test_malformed_table(rt):
    s = layers(rt)
    keys = s["queries"][:100]
    n = len(keys)
    druns = s["mem"]["_runs"]
    structs = [r.to_ctypes() for r in druns]
    assert structs[1].n > 0
    structs[1].seq = None
    bad = rt.mem_tables_device(structs)
    for chain in (False, True):
        h = call(rt, bad, s["dev"], keys, None, chain=chain)
        assert (h["status"][:n] == _abi.SDB_INVALID_ARGUMENT).all() and not h["state"][:n].any()
        assert ((h["sst"][:n].astype(np.int64) & 0xFFFFFFFF) == _abi.NO_SST).all()
        assert ((h["table"][:n].astype(np.int64) & 0xFFFFFFFF) == MG.NO_TABLE).all() and not h["row"][:n].any()
        for f in ("block", "val_off", "val_len", "seq", "flags"):
            assert not h[f][:n].any(), f
        assert h["sum_num_failed"] == n and h["sum_status"] == _abi.SDB_INVALID_ARGUMENT and h["sum_blocks_checked"] == 0
        if chain:
            assert h["csum_num_links"] == 0 and not h["chain_start"][:n + 1].any()
    check(s["mt"], keys, None, call(rt, s["mem"], s["dev"], keys))  # the well-formed tables still answer


# ------------------------------------------------------------------------------------------------
# Tables straight from the WAL replay
# ------------------------------------------------------------------------------------------------
def test_tables_from_the_replay(rt):
    import torch
    rng = random.Random(17)
    pool = sorted({bytes(rng.choice(b"abc") for _ in range(rng.randint(1, 4))) for _ in range(25)})
    batches = [[R.rand_row(rng, rng.choice(pool), 100 * b + rng.randint(1, 25)) for _ in range(70 if b == 0 else 65)]
               for b in range(3)]
    prm = rt.params()
    model = None
    for limit in range(200, 40000, 100):  # a memtable limit that closes one table before the last batch
        model = replay.replay_model(batches, None, prm, limit)
        if len(model["tables"]) == 2:
            break
    assert len(model["tables"]) == 2 and model["summary"]["rows_replaced"] > 0 and model["summary"]["rows_in"] == 200
    run, start = R.as_run(batches)
    replayed = rt.wal_replay_device(rt.DeviceRun.from_host(run), start, None, prm, limit)
    assert len(replayed) == 2 and [t.n for t in replayed] == [len(t["rows"]) for t in model["tables"]]
    # search order: the table replayed last is the newest
    tables = [MG.Table(t["rows"]) for t in reversed(model["tables"])]
    mem = rt.mem_tables_device([t.as_run() for t in reversed(replayed)])
    mt = MG.MemTree(tables, G.Tree([]))
    keys, bounds = boundary_queries(tables)
    h = call(rt, mem, dev_tree(rt, mt.tree), keys, bounds)
    got = check(mt, keys, bounds, h, skip=("val_off",))  # the replay's tables share one value arena
    torch.cuda.synchronize()
    arena = replayed[0].cols["val_bytes"].cpu().numpy()
    hits = 0
    for q, g in enumerate(got):
        if g.table != MG.NO_TABLE and g.state != _abi.GET_DELETED:
            vo, vl = int(h["val_off"][q]), int(h["val_len"][q])
            assert arena[vo:vo + vl].tobytes() == tables[g.table].value(g.row), keys[q]
            hits += 1
    assert hits >= 50 and {g.table for g in got} >= {0, 1}
    hc = call(rt, mem, dev_tree(rt, mt.tree), keys, bounds, chain=True)  # and the links' tables and rows
    want = [mt.get_merge(k, b) for k, b in zip(keys, bounds)]
    assert [int(x) for x in np.diff(hc["chain_start"][:len(keys) + 1])] == [len(g.links) for g in want]
    links = [l for g in want for l in g.links]
    assert [int(x) for x in hc["chain_row"][:len(links)]] == [l[2] for l in links]
    assert [int(x) for x in hc["chain_table"][:len(links)]] == [l[1] for l in links]


# ------------------------------------------------------------------------------------------------
# Graph capture, workspace reuse, workspace canary (M10)
# ------------------------------------------------------------------------------------------------
def test_graph_capture_and_workspace_reuse(rt):
    import torch
    s = layers(rt)
    mt, dev, mem = s["mt"], s["dev"], s["mem"]
    keys, bounds = s["keys"][:200], s["bounds"][:200]
    n = len(keys)
    keys2, bounds2 = keys[::-1], [b if b in (0, U64_MAX) else b - 1 for b in bounds[::-1]]

    def tensors(ks, bs):
        kb, ko = rt.keys_columnar(ks)
        return to_dev(kb), to_dev(ko), to_dev(np.array(bs, np.uint64))

    kb, ko, ms = tensors(keys, bounds)
    kb2, ko2, ms2 = tensors(keys2, bounds2)
    assert kb.numel() == kb2.numel()
    ws = torch.empty(rt.read_workspace_bytes("sdb_lsm_get_mem", dev, n, merge=True, tables=mem), dtype=torch.uint8, device="cuda")
    get = lambda k, b, chain=False, **kw: rt.lsm_get_mem_device(mem, dev, None, k, max_seq=b, merge=chain, fill=SENTINEL,  # noqa: E731
                                                                workspace=ws, **kw)
    # calls back to back on one workspace, with and without a chain, no reset and no synchronisation between them
    r1 = get((kb, ko, n), ms)
    r2 = get((kb2, ko2, n), ms2, chain=True, cap_links=8 * n)
    r3 = get((kb, ko, n), None)
    check(mt, keys, bounds, host(r1))
    check_chain(mt, keys2, bounds2, host(r2), cap=8 * n)
    check(mt, keys, None, host(r3))
    for chain in (False, True):  # one captured call, replayed after the key and max_seq tensors are overwritten in place
        kw = dict(chain=True, cap_links=8 * n) if chain else {}
        first = (kb.clone(), ko.clone(), ms.clone())
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):  # the first launch (function attributes) outside the capture
            warm = get((kb, ko, n), ms, stream=st, **kw)
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        holder = {}
        with torch.cuda.graph(g, stream=st):
            holder["res"] = get((kb, ko, n), ms, stream=st, **kw)
        for ks, bs, src in ((keys, bounds, first), (keys2, bounds2, (kb2, ko2, ms2)), (keys, bounds, first)):
            for dst, t in zip((kb, ko, ms), src):
                dst.copy_(t)
            for k, t in holder["res"].items():
                if k.startswith("_"):
                    continue
                if k.startswith("chain_") and k not in ("chain_start", "chain_summary"):
                    t.view(torch.uint8).fill_(SENTINEL)  # the link columns: untouched behind the last link
                else:
                    t.zero_()
            torch.cuda.synchronize()
            g.replay()
            if chain:
                check_chain(mt, ks, bs, host(holder["res"]), cap=8 * n)
            else:
                check(mt, ks, bs, host(holder["res"]))
        del warm, g


@pytest.mark.parametrize("chain", [False, True])
def test_workspace_canary(rt, chain):
    """A workspace of exactly the advertised size inside guard bands: the call writes nothing outside it."""
    s = layers(rt)
    mem, dev = s["mem"], s["dev"]
    keys, bounds = s["keys"][:257], s["bounds"][:257]
    big, ws = canaried_workspace(rt, "sdb_lsm_get_mem", dev, len(keys), merge=chain, tables=mem)
    h = host(rt.lsm_get_mem_device(mem, dev, None, keys, max_seq=bounds, merge=chain, fill=SENTINEL, workspace=ws))
    (check_chain if chain else check)(s["mt"], keys, bounds, h)
    intact(big, ws.numel())
