"""GPU parity of the merging reads (sdb_lsm_get_merge in slatedb_amd/csrc/sdb_get.hip, sdb_lsm_scan_merge in
sdb_lsm_scan.hip) against the model of tests/merge_read_cases.py: every per-query / per-row column, every link
column, chain_start and both summaries, for V2, V1 and mixed trees; the reference's recorded cases end to end
through slatedb_amd.merge.fold; chains across blocks, SSTs and runs; aggregates; lazy errors; the sequence order;
capacities; trees without operands against sdb_lsm_get / sdb_lsm_scan; degenerate inputs, a malformed tree, HIP
graph capture and workspace reuse."""
import numpy as np
import pytest

from slatedb_amd import _abi, merge

from . import get_cases as G
from . import lsm_scan_cases as L
from . import merge_read_cases as M
from . import test_gpu_get as TG
from .read_harness import check_get_summary, compare, device_tree, host, rt, to_dev, view_of  # noqa: F401
from .scan_cases import EXC, INC, U

pytestmark = pytest.mark.gpu

U64_MAX = G.U64_MAX
SENTINEL = 0x5A
LINK_COLS = ("sst", "block", "val_off", "val_len", "seq", "flags")


def check_links(tree, chains, h, cap):
    """chain_start, the chain summary and, where they fit, every link column; else the untouched sentinel."""
    n = len(chains)
    starts = np.concatenate([[0], np.cumsum([len(c) for c in chains])]).astype(np.int64)
    assert (h["chain_start"][:n + 1].astype(np.int64) == starts).all()
    total = int(starts[-1])
    assert h["csum_num_links"] == total and h["csum_max_chain_len"] == max([len(c) for c in chains] + [0])
    if total > cap:
        assert h["csum_status"] == _abi.SDB_LIMIT_EXCEEDED
        for f in LINK_COLS + ("create_ts", "expire_ts"):
            assert (h["chain_" + f].view(np.uint8) == SENTINEL).all(), f  # no link column written
        return
    assert h["csum_status"] == 0
    compare(LINK_COLS, [M.link_columns(tree, l) for c in chains for l in c], lambda f: h["chain_" + f], "link")
    for f in LINK_COLS:  # nothing behind the last link
        assert (h["chain_" + f][total:].view(np.uint8) == SENTINEL).all(), f


def check_get(tree, keys, bounds, h, cap=1 << 40):
    """Every column of every query, the links and both summaries against the model.  Returns the model's results."""
    got = [M.get_merge(tree, k, None if bounds is None else bounds[q]) for q, k in enumerate(keys)]
    compare(TG.GET_COLS, [dict(M.get_columns(tree, g), key=k) for g, k in zip(got, keys)], lambda f: h[f], "get")
    check_get_summary(got, [q for q, g in enumerate(got) if g.status], h)
    check_links(tree, [g.links for g in got], h, cap)
    return got


def check_scan(tree, rngs, bounds, desc, h, cap=1 << 40):
    """Every row column, the links and both summaries against the model.  Returns the model's results."""
    exp = [M.scan_merge(tree, r, None if bounds is None else bounds[q], desc) for q, r in enumerate(rngs)]
    n = len(rngs)
    assert (h["range_status"][:n].astype(np.int64) == np.array([e.status for e in exp], np.int64)).all()
    assert (h["range_ssts"][:n].astype(np.int64) == np.array([len(e.ssts) for e in exp], np.int64)).all()
    rows = [r for e in exp for r in e.rows]
    starts = np.concatenate([[0], np.cumsum([len(e.rows) for e in exp])]).astype(np.int64)
    assert (h["range_entry_start"][:n + 1].astype(np.int64) == starts).all()
    failed = [q for q, e in enumerate(exp) if e.status]
    assert h["sum_num_entries"] == len(rows) and h["sum_key_bytes"] == sum(len(r[0]) for r in rows)
    assert h["sum_num_candidates"] == sum(e.candidates for e in exp)
    assert h["sum_num_failed_ranges"] == len(failed) and h["sum_status"] == (exp[failed[0]].status if failed else 0)
    ko = h["key_off"][:len(rows) + 1].astype(np.int64)
    assert (ko == np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])])).all()
    assert h["key_arena"][:int(ko[-1])].tobytes() == b"".join(r[0] for r in rows)
    compare(("sst", "val_off", "val_len", "seq", "flags"), [dict(M.scan_columns(tree, r), key=r[0]) for r in rows], lambda f: h[f], "row")
    check_links(tree, [r[1] for r in rows], h, cap)
    return exp


def folded_from_device(tree, keys, h):
    return merge.fold_chains(keys, h, [l.sst.data for l in tree.leaves], M.OP)


_trees = {}


def chain(rt, versions):
    """A chain tree, its device form and its queries, built once per format mix."""
    if versions not in _trees:
        tree, straddler = M.chain_tree(versions)
        _trees[versions] = dict(tree=tree, straddler=straddler, dev=device_tree(rt, tree),
                                queries=M.chain_queries(tree, straddler))
    return _trees[versions]


# ------------------------------------------------------------------------------------------------
# 1. the reference's recorded cases, end to end
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [2, 1])
def test_golden_gets(rt, version):
    cases = M.golden()["get_cases"]
    assert len(cases) == M.KEPT_GET
    for c in cases:
        tree = G.golden_tree(c, version, bloom=(len(c["entries"]) % 2 == 0))
        key = c["query_key"].encode()
        bounds = None if c["max_seq"] is None else [c["max_seq"]]
        h = host(rt.lsm_get_merge_device(device_tree(rt, tree), None, [key], max_seq=bounds, fill=SENTINEL))
        check_get(tree, [key], bounds, h)
        (got,) = folded_from_device(tree, [key], h)
        assert got == (None if c["expected"] is None else c["expected"].encode()), c["description"]


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("version", [2, 1])
def test_golden_iterator_cases(rt, version, desc):
    cases = M.golden()["iter_cases"]
    assert len(cases) == M.KEPT_ITER
    for c in cases:
        for split in (1, 2):
            tree = M.iter_tree(c, version, split=split)
            rngs = [(None, U, None, U)]
            h = host(rt.lsm_scan_merge_device(device_tree(rt, tree), rngs, descending=desc, fill=SENTINEL))
            (exp,) = check_scan(tree, rngs, None, desc, h)
            keys = [r[0] for r in exp.rows]
            vals = folded_from_device(tree, keys, h)
            got = [(k, 1 if int(h["flags"][i]) & _abi.FLAG_MERGE_OPERAND else 0, vals[i], int(h["seq"][i]),
                    int(h["expire_ts"][i]) if int(h["flags"][i]) & _abi.FLAG_HAS_EXPIRE_TS else None)
                   for i, k in enumerate(keys)]
            want = M.iter_expected(c)
            assert got == (want[::-1] if desc else want), (c["name"], split)


# ------------------------------------------------------------------------------------------------
# 2. get chains across blocks, SSTs and runs; filters; snapshot bounds
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("versions", ["mixed", 2, 1])
def test_get_merge_chains(rt, versions):
    m = chain(rt, versions)
    tree, keys = m["tree"], m["queries"]
    assert 200 <= len(keys) <= 300 and len(keys) % 64
    h = host(rt.lsm_get_merge_device(m["dev"], None, keys, fill=SENTINEL))
    got = check_get(tree, keys, None, h)
    ops = [g for g in got if g.state == _abi.GET_MERGE_OPERAND]
    assert len(ops) >= 40 and any(len(g.links) == 1 for g in ops) and max(len(g.links) for g in ops) >= 12
    assert any(g.base for g in ops) and any(not g.base for g in ops)
    assert any({3, 4} <= {i for i, _, _ in g.links} for g in ops)  # across the cut of the sorted run
    vals = folded_from_device(tree, keys, h)
    for q, g in enumerate(got):
        assert vals[q] == (M.folded(tree, keys[q], g.links, g.base) if g.links else None)
    # bounds above, inside and below the chains
    bounds = M.chain_bounds(tree, keys)
    hb = host(rt.lsm_get_merge_device(m["dev"], None, keys, max_seq=bounds, fill=SENTINEL))
    gb = check_get(tree, keys, bounds, hb)
    inside = sum(1 for a, b in zip(got, gb) if a.links and b.links and a.links != b.links and set(b.links) < set(a.links))
    assert inside >= 5 and any(b == 0 for b in bounds) and any(b == U64_MAX for b in bounds)


def test_aggregates_and_a_tombstone_base(rt):
    """Mixed and missing timestamps across links; a tombstone base carrying timestamps is folded by the scan and
    not by the get."""
    newer = [(b"a", 1, b"3", 30, None, 500), (b"a", 1, b"2", 29, 11, None), (b"b", 1, b"y", 28, 5, 900),
             (b"c", 1, b"n", 27, None, None), (b"d", 0, b"v", 26, 3, 4)]
    older = [(b"a", 1, b"1", 20, 40, 300), (b"a", 0, b"0", 19, 7, 800), (b"b", 2, b"", 18, 99, 100),
             (b"c", 1, b"m", 17, None, None), (b"e", 1, b"solo", 16, None, 6)]
    for version in (2, 1):
        tree = G.Tree([[G.leaf_of(newer, version, 64)], [G.leaf_of(older, version, 64)]])
        dev = device_tree(rt, tree)
        keys = [b"a", b"b", b"c", b"d", b"e", b"f"]
        h = host(rt.lsm_get_merge_device(dev, None, keys, fill=SENTINEL))
        check_get(tree, keys, None, h)
        assert h["state"][:6].tolist() == [3, 3, 3, 1, 3, 0] and h["chain_start"].tolist() == [0, 4, 5, 7, 8, 9, 9]
        both = _abi.FLAG_HAS_CREATE_TS | _abi.FLAG_HAS_EXPIRE_TS
        assert (int(h["create_ts"][0]), int(h["expire_ts"][0]), int(h["flags"][0])) == (40, 300, both)
        # b: the tombstone ends the chain and its 99 / 100 stay out; no base
        assert (int(h["create_ts"][1]), int(h["expire_ts"][1]), int(h["flags"][1])) == (5, 900, both | _abi.FLAG_MERGE_OPERAND)
        assert int(h["flags"][2]) == _abi.FLAG_MERGE_OPERAND and int(h["flags"][3]) == both
        rngs = [(None, U, None, U), (b"b", INC, b"b", INC)]
        hs = host(rt.lsm_scan_merge_device(dev, rngs, fill=SENTINEL))
        check_scan(tree, rngs, None, False, hs)
        # b through the scan: the tombstone is the base; its create_ts is folded (V1 tombstones carry no expire_ts)
        assert [int(hs[f][5]) for f in ("create_ts", "expire_ts", "flags")] == [99, 100 if version == 2 else 900, both]
        assert hs["chain_start"][:7].tolist() == [0, 4, 5, 7, 8, 9, 10]


# ------------------------------------------------------------------------------------------------
# 4. / 5. lazy errors, the sequence order, an invalid view
# ------------------------------------------------------------------------------------------------
def pick_bad_block(tree, i, keys):
    """A block of leaf i and the queries whose block range there holds it: those whose chain reaches the SST
    (they fail), those whose chain ended before it, and those the filter keeps out."""
    leaf, clean = tree.leaves[i], [M.get_merge(tree, k) for k in keys]
    last = lambda g: max([x for x, _, _ in g.links] + ([g.sst] if g.row is not None else []) + [-1])  # noqa: E731
    for b in range(leaf.sst.nb - 1):
        over = [q for q, k in enumerate(keys) if leaf.covers(k) and TG.block_range(leaf, k)[0] <= b < TG.block_range(leaf, k)[1]]
        kept_out = [q for q in over if tree.step(i, keys[q])[0] == "filtered"]
        ended = lambda g: g.state == _abi.GET_DELETED or g.base or g.state == _abi.GET_FOUND  # noqa: E731
        before = [q for q in over if q not in kept_out and ended(clean[q]) and last(clean[q]) < i]
        # the chain passes through the SST or ends in it: with links on both sides, the block is INSIDE the chain
        reach = [q for q in over if q not in kept_out and q not in before]
        inside = [q for q in reach if clean[q].links and min(x for x, _, _ in clean[q].links) < i <= last(clean[q])]
        if kept_out and before and inside:
            return b, reach, inside, before, kept_out
    raise AssertionError("no block of the SST serves the test")


@pytest.mark.parametrize("how", ["crc", "block_off"])
def test_get_merge_lazy_errors(rt, how):
    m = chain(rt, "mixed")
    tree, keys = m["tree"], m["queries"]
    i = 2  # the last L0 SST; it has a filter
    leaf = tree.leaves[i]
    assert leaf.bloom is not None
    bad, reach, inside, before, kept_out = pick_bad_block(tree, i, keys)
    views = [view_of(l) for l in tree.leaves]
    if how == "crc":
        status, block_status = _abi.SDB_CHECKSUM_MISMATCH, {bad: _abi.SDB_CHECKSUM_MISMATCH}
        data = leaf.sst.data.copy()
        data[int(leaf.sst.block_off[bad]) + 5] ^= 0x40
        views[i] = view_of(leaf, data=data)
    else:
        status, block_status = _abi.SDB_CORRUPT_BLOCK, {bad: _abi.SDB_CORRUPT_BLOCK, bad + 1: _abi.SDB_CHECKSUM_MISMATCH}
        off = leaf.sst.block_off.copy()
        off[bad + 1] = off[bad] + 3
        views[i] = view_of(leaf, block_off=off)
    model = TG.broken(tree, i, block_status)
    h = host(rt.lsm_get_merge_device(device_tree(rt, model, views), None, keys, fill=SENTINEL))
    got = check_get(model, keys, None, h)
    clean = [M.get_merge(tree, k) for k in keys]
    assert all(got[q].status == status and not got[q].links for q in reach)
    for q in reach:
        assert int(h["state"][q]) == 0 and (int(h["sst"][q]) & 0xFFFFFFFF) == _abi.NO_SST
        assert not any(int(h[f][q]) for f in ("block", "val_off", "val_len", "seq", "flags", "create_ts", "expire_ts"))
    for q in before + kept_out:  # behind the chain's end, or filtered: the block never surfaces
        assert got[q] == clean[q] and got[q].status == 0, keys[q]
    assert inside and h["sum_num_failed"] == sum(1 for g in got if g.status)


def test_sequence_order_and_an_invalid_view(rt):
    # a tree the store did not write: the older SST holds a higher seq behind an operand
    new = [(b"k", 1, b"b", 50, None, None), (b"m", 1, b"x", 49, None, None), (b"z", 0, b"v", 48, None, None)]
    old = [(b"k", 1, b"a", 60, None, None), (b"m", 0, b"base", 40, None, None), (b"z", 1, b"w", 70, None, None)]
    tree = G.Tree([[G.leaf_of(new, 2, 4096)], [G.leaf_of(old, 1, 4096)]])
    keys = [b"k", b"m", b"z", b"k"]
    bounds = [U64_MAX, U64_MAX, U64_MAX, 55]  # under the bound the older SST's version is not seen
    h = host(rt.lsm_get_merge_device(device_tree(rt, tree), None, keys, max_seq=bounds, fill=SENTINEL))
    got = check_get(tree, keys, bounds, h)
    assert [g.status for g in got] == [_abi.SDB_INVALID_SEQUENCE_ORDER, 0, 0, 0]
    assert h["state"][:4].tolist() == [0, 3, 1, 3] and h["chain_start"].tolist() == [0, 0, 2, 3, 4]
    assert h["sum_status"] == _abi.SDB_INVALID_SEQUENCE_ORDER and h["sum_num_failed"] == 1
    # a view of version 3 in the middle of the chain fails the chains that reach it
    m = chain(rt, "mixed")
    runs, j = [], 0
    for r in m["tree"].runs:
        runs.append([G.Leaf(l.sst, l.bloom is not None, None, 3 if j + x == 1 else l.version) for x, l in enumerate(r)])
        j += len(r)
    model = G.Tree(runs)
    keys = m["queries"]
    h = host(rt.lsm_get_merge_device(device_tree(rt, model), None, keys, fill=SENTINEL))
    got = check_get(model, keys, None, h)
    clean = [M.get_merge(m["tree"], k) for k in keys]
    hit = [q for q, g in enumerate(got) if g.status == _abi.SDB_INVALID_VERSION]
    assert 5 < len(hit) < len(keys) - 5
    assert any(clean[q].links and clean[q].links[0][0] == 0 for q in hit)  # a chain that began before the view
    assert any(g.status == 0 and g.links and g.links[-1][0] == 0 and c == g for g, c in zip(got, clean))  # ended before it


# ------------------------------------------------------------------------------------------------
# 6. capacities
# ------------------------------------------------------------------------------------------------
def test_get_merge_capacity(rt):
    m = chain(rt, 2)
    tree, keys = m["tree"], m["queries"]
    total = sum(len(M.get_merge(tree, k).links) for k in keys)
    assert total > len(keys)
    for cap in (0, total - 1, total):
        h = host(rt.lsm_get_merge_device(m["dev"], None, keys, cap_links=cap, fill=SENTINEL))
        check_get(tree, keys, None, h, cap=cap)  # the per-query columns and chain_start are valid either way
        assert (h["csum_status"] == 0) == (cap == total)
    h = host(rt.lsm_get_merge_device(m["dev"], None, keys, fill=SENTINEL))  # sized by a first call
    check_get(tree, keys, None, h)
    assert h["chain_sst"].size == total


def test_scan_merge_capacity_order(rt):
    """Candidates, then rows, then links; the totals and chain_start on each failure; no link column written."""
    m = chain(rt, "mixed")
    tree = m["tree"]
    rngs = [(b"k0010", INC, b"k0040", INC), (None, U, b"k0008", EXC), (M.CUT_KEY, INC, M.CUT_KEY, INC)]
    exp = [M.scan_merge(tree, r) for r in rngs]
    ce, ckb = sum(e.candidates for e in exp), sum(e.cand_key_bytes for e in exp)
    rows = [r for e in exp for r in e.rows]
    nr, kb, nl = len(rows), sum(len(r[0]) for r in rows), sum(len(r[1]) for r in rows)
    assert nl > nr > 3
    run = lambda cand, cap, cl: host(rt.lsm_scan_merge_device(m["dev"], rngs, cand=cand, cap=cap, cap_links=cl,  # noqa: E731
                                                               fill=SENTINEL))
    untouched = lambda h: all((h["chain_" + f].view(np.uint8) == SENTINEL).all() for f, _ in rt.CHAIN_COLUMNS)  # noqa: E731
    h = run((ce - 1, ckb), (nr, kb), nl)  # the candidates do not fit
    assert h["sum_status"] == _abi.SDB_LIMIT_EXCEEDED and h["sum_num_candidates"] == ce and h["sum_num_entries"] == 0
    assert h["csum_status"] == _abi.SDB_LIMIT_EXCEEDED and untouched(h) and not h["chain_start"].any()
    h = run((ce, ckb), (nr - 1, kb), nl)  # the rows do not fit
    assert h["sum_status"] == _abi.SDB_LIMIT_EXCEEDED and h["sum_num_entries"] == nr and h["sum_key_bytes"] == kb
    assert h["csum_status"] == _abi.SDB_LIMIT_EXCEEDED and h["csum_num_links"] == nl and untouched(h)
    assert not h["chain_start"].any() and not h["seq"].any()
    for cl in (0, nl - 1):  # the rows fit, the links do not: rows complete, chain_start valid, no link column
        h = run((ce, ckb), (nr, kb), cl)
        check_scan(tree, rngs, None, False, h, cap=cl)
        assert h["sum_status"] == 0 and h["csum_status"] == _abi.SDB_LIMIT_EXCEEDED and untouched(h)
    h = run((ce, ckb), (nr, kb), nl)  # exact
    check_scan(tree, rngs, None, False, h, cap=nl)
    assert h["csum_status"] == 0
    h = host(rt.lsm_scan_merge_device(m["dev"], rngs, fill=SENTINEL))  # the wrapper retries once
    check_scan(tree, rngs, None, False, h)


# ------------------------------------------------------------------------------------------------
# 7. scans
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("versions", ["mixed", 2, 1])
def test_scan_merge_chains(rt, versions, desc):
    m = chain(rt, versions)
    tree = m["tree"]
    rngs = [(None, U, None, U), (M.CUT_KEY, INC, M.CUT_KEY, INC), (M.CUT_KEY, EXC, None, U), (b"k0020", INC, b"k0060", EXC),
            (b"k0020", INC, b"k0060", EXC), (b"k0041", INC, b"k0041", INC), (b"k0090", INC, b"k0010", INC)]
    rngs += L.narrow_ranges(tree, count=200, seed=9)
    h = host(rt.lsm_scan_merge_device(m["dev"], rngs, descending=desc, fill=SENTINEL))
    exp = check_scan(tree, rngs, None, desc, h)
    full = exp[0].rows
    assert len(full) >= 60 and max(len(r[1]) for r in full) >= 12 and any(len(r[1]) == 1 for r in full)
    assert any({3, 4} <= {i for i, _, _ in r[1]} for r in full)  # (every key has a value in the oldest run: a base)
    keys = [r[0] for e in exp for r in e.rows]
    vals = folded_from_device(tree, keys, h)
    want = [M.folded(tree, r[0], r[1], r[2]) for e in exp for r in e.rows]
    assert vals == want
    a, b = int(h["range_entry_start"][3]), int(h["range_entry_start"][4])  # overlapping ranges: a copy each
    assert b - a == len(exp[3].rows) > 5 and (h["seq"][a:b] == h["seq"][b:b + (b - a)]).all()
    la, lb, lc = (int(h["chain_start"][x]) for x in (a, b, b + (b - a)))
    assert lb - la == lc - lb and (h["chain_seq"][la:lb] == h["chain_seq"][lb:lc]).all()
    if not desc:
        keys0 = [r[0] for r in full]
        seqs = sorted({r[3] for l in tree.leaves for r in l.sst.rows})
        rng = np.random.default_rng(4)
        rb = rngs[:60]
        bounds = [U64_MAX if q % 4 == 0 else seqs[int(rng.integers(0, len(seqs)))] for q in range(len(rb))]
        hb = host(rt.lsm_scan_merge_device(m["dev"], rb, max_seq=bounds, fill=SENTINEL))
        eb = check_scan(tree, rb, bounds, False, hb)
        assert 0 < len(eb[1].rows) + len(eb[0].rows) and len(eb[0].rows) <= len(keys0)


def side_by_side(version):
    """A value winner, an operand winner with a value base, one with a tombstone base, one with no base, a tombstone
    winner and an operand hidden behind a newer value, side by side, spread over three SSTs."""
    a = [(b"k1", 0, b"v1", 90, None, None), (b"k2", 1, b"c", 89, None, None), (b"k3", 1, b"y", 88, None, 9),
         (b"k5", 2, b"", 86, None, None), (b"k6", 0, b"new", 85, None, None)]
    b = [(b"k2", 1, b"b", 70, None, None), (b"k3", 2, b"", 69, 12, None), (b"k4", 1, b"q", 68, None, None),
         (b"k5", 1, b"gone", 67, None, None), (b"k6", 1, b"hidden", 66, None, None)]
    c = [(b"k2", 0, b"a", 50, None, None), (b"k2", 1, b"older", 49, None, None), (b"k3", 0, b"dead", 48, None, None),
         (b"k4", 1, b"p", 47, None, None), (b"k6", 0, b"oldest", 46, None, None)] + \
        [(b"k7%02d" % x, 0, b"pad" * 8, 40 - x, None, None) for x in range(12)]
    return G.Tree([[G.leaf_of(a, version, 64)], [G.leaf_of(b, version, 64)], [G.leaf_of(c, version, 64)]])


@pytest.mark.parametrize("desc", [False, True])
def test_scan_merge_side_by_side(rt, desc):
    for version in (2, 1):
        tree = side_by_side(version)
        rngs = [(None, U, None, U), (b"k2", INC, b"k4", INC), (b"k3", INC, b"k6", INC), (b"k70", INC, None, U)]
        h = host(rt.lsm_scan_merge_device(device_tree(rt, tree), rngs, descending=desc, fill=SENTINEL))
        exp = check_scan(tree, rngs, None, desc, h)
        rows = exp[0].rows[::-1] if desc else exp[0].rows
        assert [r[0] for r in rows[:5]] == [b"k1", b"k2", b"k3", b"k4", b"k6"]
        assert [(len(r[1]), r[2]) for r in rows[:5]] == [(1, True), (3, True), (1, True), (2, False), (1, True)]
        vals = folded_from_device(tree, [r[0] for r in exp[0].rows], h)
        want = [b"v1", b"abc", b"y", b"pq", b"new"]
        assert (vals[::-1] if desc else vals)[:5] == want
        # a failing block fails only its range: the last block of the oldest SST holds only k7.. keys
        leaf = tree.leaves[2]
        bad = leaf.sst.nb - 1
        data = leaf.sst.data.copy()
        data[int(leaf.sst.block_off[bad]) + 5] ^= 0x40
        views = [view_of(l) for l in tree.leaves]
        views[2] = view_of(leaf, data=data)
        model = TG.broken(tree, 2, {bad: _abi.SDB_CHECKSUM_MISMATCH})
        hb = host(rt.lsm_scan_merge_device(device_tree(rt, model, views), rngs, descending=desc, fill=SENTINEL))
        eb = check_scan(model, rngs, None, desc, hb)
        assert [e.status for e in eb] == [_abi.SDB_CHECKSUM_MISMATCH, 0, 0, _abi.SDB_CHECKSUM_MISMATCH]
        assert eb[1].rows == exp[1].rows and eb[2].rows == exp[2].rows


# ------------------------------------------------------------------------------------------------
# 8. a tree without operands: the plain entry points' answers, chains of one
# ------------------------------------------------------------------------------------------------
def test_no_operands_equals_the_plain_reads(rt):
    tree, straddler = M.no_operand_tree()
    dev = device_tree(rt, tree)
    keys = G.main_queries(tree, straddler)[:300]
    bounds = G.bounded_queries(tree, keys, straddler)[1][:len(keys)]
    plain = host(rt.lsm_get_device(dev, None, keys, max_seq=bounds))
    h = host(rt.lsm_get_merge_device(dev, None, keys, max_seq=bounds, fill=SENTINEL))
    for f, _ in rt.GET_FIELDS:
        assert (plain[f] == h[f]).all(), f
    assert (plain["summary"] == h["summary"]).all()
    n = np.diff(h["chain_start"].astype(np.int64))
    assert (n == (h["state"][:len(keys)] == _abi.GET_FOUND)).all() and h["csum_max_chain_len"] == 1
    check_get(tree, keys, bounds, h)
    rngs = L.ranges(tree, straddler)[:120]
    for desc in (False, True):
        p = rt.lsm_scan_device(dev, rngs, descending=desc)
        hs = host(rt.lsm_scan_merge_device(dev, rngs, descending=desc, fill=SENTINEL))
        ph = {k: v.cpu().numpy() for k, v in p.items() if not k.startswith("_")}
        ne = int(ph["summary"][0])
        assert ne > 150 and (ph["summary"] == hs["summary"]).all()
        for f in ("range_entry_start", "range_status", "range_ssts"):
            assert (ph[f] == hs[f]).all(), f
        for f in ("key_off", "sst", "val_off", "val_len", "seq", "flags", "create_ts", "expire_ts"):
            assert (ph[f][:ne] == hs[f][:ne]).all(), f
        assert ph["key_arena"][:int(ph["summary"][1])].tobytes() == hs["key_arena"][:int(ph["summary"][1])].tobytes()
        assert (hs["chain_start"][:ne + 1] == np.arange(ne + 1)).all() and hs["csum_num_links"] == ne
        assert (hs["chain_seq"][:ne] == hs["seq"][:ne]).all() and (hs["chain_sst"][:ne] == hs["sst"][:ne]).all()


# ------------------------------------------------------------------------------------------------
# 9. degenerate inputs, a malformed tree, graph capture, workspace reuse
# ------------------------------------------------------------------------------------------------
def test_degenerate(rt):
    m = chain(rt, "mixed")
    h = host(rt.lsm_get_merge_device(m["dev"], None, [], fill=SENTINEL))
    assert not h["summary"].any() and not h["chain_summary"].any() and h["chain_start"].tolist() == [0]
    h = host(rt.lsm_scan_merge_device(m["dev"], [], fill=SENTINEL))
    assert not h["summary"].any() and not h["chain_summary"].any() and int(h["chain_start"][0]) == 0
    keys = [b"a", b"", b"k0002"]
    of_empty = G.Tree([[G.Leaf(G.EmptySst())], [G.Leaf(G.EmptySst()), G.Leaf(G.EmptySst())]])
    for dev in (rt.lsm_tree_device([], []), device_tree(rt, of_empty)):
        h = host(rt.lsm_get_merge_device(dev, None, keys, max_seq=[5, 6, 7], cap_links=4, fill=SENTINEL))
        assert not h["summary"].any() and not h["chain_summary"].any() and not h["chain_start"].any()
        assert not h["state"][:3].any() and not h["status"][:3].any()
        assert ((h["sst"][:3].astype(np.int64) & 0xFFFFFFFF) == _abi.NO_SST).all()
        assert (h["chain_seq"].view(np.uint8) == SENTINEL).all()
        h = host(rt.lsm_scan_merge_device(dev, [(None, U, None, U), (b"a", INC, b"b", INC)], fill=SENTINEL))
        assert not h["summary"].any() and not h["chain_summary"].any() and not h["range_entry_start"].any()


@pytest.mark.parametrize("what", ["block_base", "run_start"])
def test_malformed_tree(rt, what):
    m = chain(rt, "mixed")
    dev, keys = m["dev"], m["queries"][:100]
    if what == "block_base":
        bb = dev["_block_base"].clone()
        bb[3] -= 1
        t = TG.with_arrays(rt, dev, block_base=bb)
    else:
        rs = dev["_run_start"].clone()
        rs[2], rs[3] = 3, 2
        t = TG.with_arrays(rt, dev, run_start=rs)
    n = len(keys)
    h = host(rt.lsm_get_merge_device(t, None, keys, cap_links=64, fill=SENTINEL))
    assert (h["status"][:n] == _abi.SDB_INVALID_ARGUMENT).all() and not h["state"][:n].any()
    assert h["sum_num_failed"] == n and h["sum_blocks_checked"] == 0 and not h["chain_start"].any()
    assert h["csum_num_links"] == 0 and h["csum_status"] == 0 and (h["chain_seq"].view(np.uint8) == SENTINEL).all()
    rngs = [(None, U, None, U), (b"k0010", INC, b"k0020", INC)]
    hs = host(rt.lsm_scan_merge_device(t, rngs, cand=(4096, 1 << 16), cap=(4096, 1 << 16), cap_links=4096, fill=SENTINEL))
    assert (hs["range_status"][:2] == _abi.SDB_INVALID_ARGUMENT).all() and hs["sum_num_entries"] == 0
    assert hs["csum_num_links"] == 0 and (hs["chain_seq"].view(np.uint8) == SENTINEL).all()
    check_get(m["tree"], keys, None, host(rt.lsm_get_merge_device(dev, None, keys, fill=SENTINEL)))  # the tree still answers


def test_graph_capture_and_workspace_reuse(rt):
    import torch
    m = chain(rt, "mixed")
    tree, dev = m["tree"], m["dev"]
    keys = m["queries"][:200]
    bounds = M.chain_bounds(tree, keys)
    keys2, bounds2 = keys[::-1], [b if b in (0, U64_MAX) else b - 1 for b in bounds[::-1]]
    cap = 4096

    def tensors(ks, bs):
        kb, ko = rt.keys_columnar(ks)
        return to_dev(kb), to_dev(ko), to_dev(np.array(bs, np.uint64))

    kb, ko, ms = tensors(keys, bounds)
    kb2, ko2, ms2 = tensors(keys2, bounds2)
    n = len(keys)
    assert kb.numel() == kb2.numel()
    ws = torch.empty(rt.read_workspace_bytes("sdb_lsm_get_merge", dev, n), dtype=torch.uint8, device="cuda")
    call = lambda k, o, b, s=None: rt.lsm_get_merge_device(dev, None, (k, o, n), max_seq=b, stream=s, workspace=ws,  # noqa: E731
                                                           cap_links=cap, fill=SENTINEL)
    r1, r2, r3 = call(kb, ko, ms), call(kb2, ko2, ms2), call(kb, ko, None)  # one workspace, no reset in between
    check_get(tree, keys, bounds, host(r1))
    check_get(tree, keys2, bounds2, host(r2))
    check_get(tree, keys, None, host(r3))
    first = (kb.clone(), ko.clone(), ms.clone())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # the first launch (function attributes) outside the capture
        warm = call(kb, ko, ms, s)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    holder = {}
    with torch.cuda.graph(g, stream=s):
        holder["res"] = call(kb, ko, ms, s)
    for ks, bs, src in ((keys, bounds, first), (keys2, bounds2, (kb2, ko2, ms2))):
        for dst, t in zip((kb, ko, ms), src):
            dst.copy_(t)
        for k, t in holder["res"].items():
            if not k.startswith("_"):
                t.view(torch.uint8).fill_(SENTINEL) if k.startswith("chain_") and k[6:] in dict(rt.CHAIN_COLUMNS) else t.zero_()
        torch.cuda.synchronize()
        g.replay()
        check_get(tree, ks, bs, host(holder["res"]))
    del warm
    # the scan: captured with fixed capacities, replayed twice over ranges overwritten in place
    ra = [(b"k0010", INC, b"k0050", INC), (None, U, b"k0020", EXC), (M.CUT_KEY, INC, M.CUT_KEY, INC)]
    rb = [(b"k0060", INC, b"k0090", EXC), (None, U, b"k0006", INC), (b"k0100", INC, b"k0140", INC)]
    cols = lambda rs: {k: to_dev(a) for k, a in rt.scan_ranges_columnar(rs).items()}  # noqa: E731
    ta, tb = cols(ra), cols(rb)
    assert all(ta[k].numel() == tb[k].numel() for k in ta)
    live = {k: v.clone() for k, v in ta.items()}
    live["n"] = 3
    cand, capr = (8192, 1 << 17), (2048, 1 << 15)
    wss = torch.empty(rt.read_workspace_bytes("sdb_lsm_scan_merge", dev, 3, cand), dtype=torch.uint8, device="cuda")
    scall = lambda st=None: rt.lsm_scan_merge_device(dev, live, stream=st, workspace=wss, cand=cand, cap=capr,  # noqa: E731
                                                     cap_links=cap, fill=SENTINEL)
    check_scan(tree, ra, None, False, host(scall()))
    with torch.cuda.stream(s):
        warm = scall(s)
    s.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2, stream=s):
        holder["scan"] = scall(s)
    for rs, src in ((rb, tb), (ra, ta)):
        for k in src:
            live[k].copy_(src[k])
        for k, t in holder["scan"].items():
            if not k.startswith("_"):
                t.view(torch.uint8).fill_(SENTINEL) if k.startswith("chain_") and k[6:] in dict(rt.CHAIN_COLUMNS) else t.zero_()
        torch.cuda.synchronize()
        g2.replay()
        check_scan(tree, rs, None, False, host(holder["scan"]))
    del warm
