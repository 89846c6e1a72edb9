"""GPU parity of sdb_lsm_scan_mem (device memtables merged ahead of the tree, slatedb_amd/csrc/sdb_lsm_scan.hip)
against the model of tests/mem_scan_cases.py, every column of every row and link: the stretches' boundaries, the
order of the sources and max_seq, the reference's recorded cases, chains across layers, no laziness (S5), the
capacities (S6), no tables (S7), no tree (S8), a malformed table (S9), tables straight from the WAL replay, HIP graph
capture with the tables changed in place, and a workspace canary."""
import random

import numpy as np
import pytest

from slatedb_amd import _abi, merge, replay

from . import get_cases as G
from . import lsm_scan_cases as L
from . import mem_get_cases as MG
from . import mem_scan_cases as S
from . import merge_read_cases as M
from . import replay_cases as R
from . import test_gpu_get as TG
from .read_harness import (Filled, canaried_workspace, check_scan_core, compare, dev_tables, dev_tree, device_tree, host,  # noqa: F401
                           intact, rt, to_dev, totals, u64, untouched, view_of)
from .scan_cases import EXC, INC, U

pytestmark = pytest.mark.gpu

U64_MAX = G.U64_MAX
SENTINEL = 0xA5
ROW_COLS = ("sst", "table", "row", "val_off", "val_len", "seq", "flags")
LINK_COLS = ("sst", "block", "table", "row", "val_off", "val_len", "seq", "flags")


def scan(rt, mem, dev, rngs, bounds=None, desc=False, chain=False, **kw):
    return host(rt.lsm_scan_mem_device(mem, dev, rngs, max_seq=bounds, descending=desc, merge=chain, fill=SENTINEL, **kw))


def model(mt, rngs, bounds, desc, chain):
    return [S.scan(mt, r, None if bounds is None else bounds[q], desc, chain) for q, r in enumerate(rngs)]


def check_ranges(exp, h):
    """range_status, range_ssts, range_tables, range_filtered and the summary's block word against the model."""
    n = len(exp)
    for f, want in (("range_status", [e.status for e in exp]), ("range_ssts", [len(e.ssts) for e in exp]),
                    ("range_tables", [len(e.tables) for e in exp]), ("range_filtered", [len(e.filtered) for e in exp])):
        bad = np.nonzero(h[f][:n].astype(np.int64) != np.array(want, np.int64))[0]
        assert not bad.size, (f, int(bad[0]), want[int(bad[0])], int(h[f][int(bad[0])]))
    assert h["sum_blocks_checked"] == len(set().union(*[e.blocks for e in exp]))
    assert int(h["num_filtered"][0]) == sum(len(e.filtered) for e in exp)


def check(mt, rngs, bounds, desc, chain, h, exp=None, cap_links=1 << 40):
    """Every column of every row (and link), both summaries, against the model.  Returns the model's results."""
    exp = exp or model(mt, rngs, bounds, desc, chain)
    check_ranges(exp, h)
    rows = check_scan_core(exp, h)
    compare(ROW_COLS, [S.columns(mt, r) for r in rows], lambda f: h[f], "row")
    if chain:
        links = [l for r in rows for l in r[1]]
        cs = np.concatenate([[0], np.cumsum([len(r[1]) for r in rows])]).astype(np.int64)
        assert (h["chain_start"][:len(rows) + 1].astype(np.int64) == cs).all()
        assert h["csum_num_links"] == len(links) and h["csum_max_chain_len"] == max([len(r[1]) for r in rows] + [0])
        if len(links) > cap_links:
            assert h["csum_status"] == _abi.SDB_LIMIT_EXCEEDED
            for f in LINK_COLS + ("create_ts", "expire_ts"):
                assert (h["chain_" + f].view(np.uint8) == SENTINEL).all(), f
        else:
            assert h["csum_status"] == 0
            compare(LINK_COLS, [S.link_columns(mt, l) for l in links], lambda f: h["chain_" + f], "link")
    return exp


_layers = {}


def layers(rt):
    """The plain tree with three little tables over its key space, on the device, built once."""
    if not _layers:
        tree, straddler = L.plain_tree()
        tables = S.little_tables(tree)
        rngs, bounds = L.bounds_for(tree, L.ranges(tree, straddler, nrandom=60), straddler)
        _layers.update(tree=tree, straddler=straddler, tables=tables, mt=S.MemTree(tables, tree), dev=device_tree(rt, tree),
                       mem=dev_tables(rt, tables), rngs=rngs[:160], bounds=bounds[:160])
    return _layers


# ------------------------------------------------------------------------------------------------
# S2: the stretches' boundaries
# ------------------------------------------------------------------------------------------------
def boundary_tables():
    """Tables of 0, 1, 63, 64, 65 and 257 rows: stretches end on and across a wave and a 256-thread workgroup.  Keys
    of 1 to 9 bytes, so a pair's key-byte span starts at any alignment; every third key has three versions; the
    largest holds a key that is a proper prefix of its neighbours."""
    out, seq = [], 2_000_000
    for t, size in enumerate((0, 1, 63, 64, 65, 257)):
        es, k = [], 0
        if size == 257:
            es = [(b"a", 0, b"A", seq + 1, None, None), (b"a", 0, b"A0", seq, None, None), (b"a\x00", 0, b"", seq + 2, None, 77),
                  (b"ab", 2, b"", seq + 3, None, None), (b"ab", 0, b"B", seq - 1, 5, None)]
        while len(es) < size:
            key = b"m%d" % t + b"x" * (k % 7) + b"%02d" % k
            for v in range(3 if k % 3 == 0 else 1):
                if len(es) < size:
                    es.append((key, 0 if v != 1 else 2, b"" if v == 1 else b"v%d.%d" % (k, v), seq + 10 * k - v, None,
                               1000 + k if k % 5 == 0 else None))
            k += 1
        out.append(MG.Table(es))
        assert len(out[-1].rows) == size
    return out


def boundary_ranges(tables):
    out = [(None, U, None, U), (b"a", INC, b"a", INC), (b"a", EXC, b"ab", EXC), (b"a", INC, b"a\x00", EXC),
           (b"a\x00", INC, b"ab", INC), (b"a", EXC, None, U), (None, U, b"a", INC), (None, U, b"a", EXC)]
    for t in tables:
        keys = sorted({r[0] for r in t.rows})
        if not keys:
            continue
        f, l = keys[0], keys[-1]
        m = next((k for k in keys[len(keys) // 2:] if sum(1 for r in t.rows if r[0] == k) > 1), keys[len(keys) // 2])
        for sk in (INC, EXC):
            for ek in (INC, EXC):
                out += [(f, sk, l, ek), (f, sk, m, ek), (m, sk, l, ek), (m, sk, m, ek), (m + b"\x00", sk, l, ek),
                        (b"\x00", sk, l + b"\xff", ek), (f[:-1], sk, m[:-1], ek)]
        out += [(None, U, m, INC), (None, U, m, EXC), (m, EXC, None, U), (m, INC, None, U), (l + b"\xff", INC, None, U),
                (None, U, f, EXC), (l, INC, f, INC), (m, EXC, m, INC), (f, 3, l, INC), (f, INC, l, 3)]
    return out


@pytest.mark.parametrize("desc", [False, True])
def test_stretch_boundaries(rt, desc):
    s = layers(rt)
    tables = boundary_tables()
    mt = S.MemTree(tables, s["tree"])
    rngs = boundary_ranges(tables)
    h = scan(rt, dev_tables(rt, tables), s["dev"], rngs, None, desc)
    exp = check(mt, rngs, None, desc, False, h)
    assert {len(e.tables) for e in exp} >= {0, 1, 5} and sum(1 for e in exp if e.status) == 10
    assert max(e.candidates for e in exp) > 700 and sum(1 for e in exp if e.rows and not e.ssts) > 50
    # each table alone, without a tree: every stretch by itself
    none = dev_tree(rt, G.Tree([]))
    for t in tables[1:]:
        check(S.MemTree([t], G.Tree([])), rngs[:40], None, desc, False, scan(rt, dev_tables(rt, [t]), none, rngs[:40], None, desc))


# ------------------------------------------------------------------------------------------------
# S1 / S3: the order of the sources, max_seq
# ------------------------------------------------------------------------------------------------
def test_source_order_and_max_seq(rt):
    v = lambda k, val, seq, kind=0: (k, kind, val, seq, None, None)  # noqa: E731
    t0 = MG.Table([v(b"dup", b"t0", 50), v(b"nb", b"new", 90), v(b"nb2", b"new", 90), v(b"tb", b"", 95, 2)])
    t1 = MG.Table([v(b"dup", b"t1", 50), v(b"dup2", b"t1", 50), v(b"nb", b"seen", 55), v(b"th", b"", 50, 2)])
    es = [v(b"dup", b"s", 50), v(b"dup2", b"s", 50), v(b"nb2", b"seen", 40), v(b"tb", b"kept", 30), v(b"th", b"hidden", 20)]
    for version in (1, 2):
        mt = S.MemTree([t0, t1], G.Tree([[G.leaf_of(sorted(es), version, 64)]]))
        keys = [b"dup", b"dup2", b"nb", b"nb2", b"tb", b"th"]
        rngs = [(None, U, None, U)] * 2 + [(k, INC, k, INC) for k in keys] * 2
        bounds = [U64_MAX, 60] + [U64_MAX] * 6 + [60] * 6
        for desc in (False, True):
            h = scan(rt, dev_tables(rt, [t0, t1]), dev_tree(rt, mt.tree), rngs, bounds, desc)
            exp = check(mt, rngs, bounds, desc, False, h)
        src = lambda e: {k: s[:2] for k, s in e.rows}  # noqa: E731
        assert src(exp[0]) == {b"dup": ("t", 0), b"dup2": ("t", 1), b"nb": ("t", 0), b"nb2": ("t", 0)}  # tb, th: tombstones
        assert src(exp[1]) == {b"dup": ("t", 0), b"dup2": ("t", 1), b"nb": ("t", 1), b"nb2": ("s", 0), b"tb": ("s", 0)}
        assert all(e.candidates >= len(e.rows) for e in exp) and exp[0].candidates == 13


# ------------------------------------------------------------------------------------------------
# The reference's recorded scans
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [1, 2])
def test_golden_cases(rt, version):
    done = 0
    for chain, cases in ((False, L.golden_cases()), (True, S.merge_golden_cases())):
        for c in cases:
            mt = S.golden_mem_tree(c, version)
            rngs, bounds = [L.golden_range(c)], None if c["max_seq"] is None else [c["max_seq"]]
            res = rt.lsm_scan_mem_device(dev_tables(rt, mt.tables), dev_tree(rt, mt.tree), rngs, max_seq=bounds, merge=chain)
            h = host(res)
            check(mt, rngs, bounds, False, chain, h)
            tvals = MG.host_tables(mt.tables)
            data = [l.sst.data for l in mt.tree.leaves]
            if chain:
                got = merge.fold_scan_mem(h, tvals, data, M.OP)
            else:
                got = []
                for i in range(h["sum_num_entries"]):
                    t, vo, vl = int(h["table"][i]), int(h["val_off"][i]), int(h["val_len"][i])
                    src = tvals[t] if t >= 0 else data[int(h["sst"][i])]
                    got.append((h["key_arena"][int(h["key_off"][i]):int(h["key_off"][i + 1])].tobytes(), bytes(src[vo:vo + vl])))
            assert [[k.decode(), v.decode()] for k, v in got] == c["expected"], c["description"]
            done += 1
    assert done == L.KEPT_CASES + S.KEPT_MERGE_CASES


# ------------------------------------------------------------------------------------------------
# S4: chains through the tables and into the tree
# ------------------------------------------------------------------------------------------------
def chain_layers():
    tree, _ = M.chain_tree()
    o = lambda k, val, seq, kind=1, cts=None, ets=None: (k, kind, val, seq, cts, ets)  # noqa: E731
    l0 = tree.leaves[0].sst
    l0_key = next(r[0] for r in l0.rows if r[4] & _abi.FLAG_MERGE_OPERAND and r[0] != M.CUT_KEY)
    t0 = [o(M.CUT_KEY, b"T0a", 3_000_002), o(M.CUT_KEY, b"T0b", 3_000_001, ets=9), o(b"k9one", b"x", 3_000_010),
          o(b"k9one", b"y", 3_000_009, cts=4), o(b"k9one", b"base", 3_000_008, 0), o(b"k9one", b"old", 3_000_007),
          o(b"k9val", b"op", 3_000_020), o(b"k9tomb", b"op", 3_000_030, ets=50), o(l0_key, b"top", 3_000_040)]
    t1 = [o(M.CUT_KEY, b"T1", 2_000_001, cts=11), o(b"k9val", b"base", 2_000_020, 0, ets=7), o(b"k9tomb", b"", 2_000_030, 2, ets=3),
          o(b"k9tomb", b"older", 2_000_029)]
    tables = [MG.Table(t0), MG.Table(t1)] + S.little_tables(tree, seed=8, kinds=(1, 1, 1, 0, 2), ntab=1, per=30)
    rngs = L.narrow_ranges(tree, 80) + [(None, U, None, U), (M.CUT_KEY, INC, M.CUT_KEY, INC), (b"k9", INC, b"k9z", EXC),
                                        (l0_key, INC, l0_key, INC)]
    return S.MemTree(tables, tree), rngs, l0_key


@pytest.mark.parametrize("desc", [False, True])
def test_chains_across_layers(rt, desc):
    mt, rngs, l0_key = chain_layers()
    mem, dev = dev_tables(rt, mt.tables), dev_tree(rt, mt.tree)
    h = scan(rt, mem, dev, rngs, None, desc, chain=True)
    exp = check(mt, rngs, None, desc, True, h)
    by_key = {r[0]: r for r in exp[len(rngs) - 4].rows}  # the unbounded range
    where = lambda k: [l[:2] for l in by_key[k][1]]  # noqa: E731
    # (chain_tree: 3 L0 SSTs, then the sorted run that holds the cut key, then the run of values)
    assert where(M.CUT_KEY)[:3] == [("t", 0), ("t", 0), ("t", 1)] and all(l[0] == "s" and l[1] >= 3 for l in where(M.CUT_KEY)[3:])
    assert len(where(M.CUT_KEY)) >= 6  # two tables, then both sides of the cut
    assert where(b"k9one") == [("t", 0)] * 3 and by_key[b"k9one"][2]  # inside one table, ended by its value
    assert where(b"k9val") == [("t", 0), ("t", 1)] and by_key[b"k9val"][2]  # a value base in a table
    assert where(b"k9tomb") == [("t", 0)] and by_key[b"k9tomb"][2] and by_key[b"k9tomb"][4] == 3  # a tombstone base, folded
    assert where(l0_key)[0] == ("t", 0) and ("s", 0) in where(l0_key)  # from a table into an L0 SST
    vals = merge.fold_scan_mem(h, MG.host_tables(mt.tables), [l.sst.data for l in mt.tree.leaves], M.OP)
    assert vals == [(r[0], S.folded(mt, r)) for e in exp for r in e.rows]
    # without a chain the operand winners fail their ranges, in a table as in an SST
    plain = check(mt, rngs, None, desc, False, scan(rt, mem, dev, rngs, None, desc))
    assert sum(1 for e in plain if e.status == _abi.SDB_MERGE_OPERATOR_MISSING) > 20
    # cap_links one short, then exact
    nc, ckb = sum(e.candidates for e in exp), sum(e.cand_key_bytes for e in exp)
    ne, nl = sum(len(e.rows) for e in exp), sum(len(r[1]) for e in exp for r in e.rows)
    kw = dict(cand=(nc, ckb), cap=(ne, ckb))
    check(mt, rngs, None, desc, True, scan(rt, mem, dev, rngs, None, desc, chain=True, cap_links=nl - 1, **kw), exp, cap_links=nl - 1)
    h = scan(rt, mem, dev, rngs, None, desc, chain=True, cap_links=nl, **kw)
    check(mt, rngs, None, desc, True, h, exp, cap_links=nl)


# ------------------------------------------------------------------------------------------------
# S5: nothing is lazy
# ------------------------------------------------------------------------------------------------
def test_a_table_shields_no_block_error(rt):
    s = layers(rt)
    tree = s["tree"]
    i = 6
    leaf = tree.leaves[i]
    bad = leaf.sst.nb // 2
    data = leaf.sst.data.copy()
    data[int(leaf.sst.block_off[bad]) + 5] ^= 0x40
    views = [view_of(l) for l in tree.leaves]
    views[i] = view_of(leaf, data=data)
    broken = TG.broken(tree, i, {bad: _abi.SDB_CHECKSUM_MISMATCH})
    lo, hi = leaf.sst.keys[leaf.sst.bes[bad]], leaf.sst.keys[leaf.sst.bes[bad + 1] - 1]
    inside = [k for k in L.all_keys(tree) if lo <= k <= hi]
    cover = MG.Table([(k, 0, b"mem", 5_000_000 + n, None, None) for n, k in enumerate(inside)])  # every key of the range, newest
    mt = S.MemTree([cover] + s["tables"], broken)
    rngs = [(lo, INC, hi, INC), (inside[0], INC, inside[0], INC)] + s["rngs"][:100]
    h = scan(rt, dev_tables(rt, mt.tables), device_tree(rt, broken, views), rngs)
    exp = check(mt, rngs, None, False, False, h)
    assert exp[0].status == exp[1].status == _abi.SDB_CHECKSUM_MISMATCH and exp[0].tables[0] == 0 and not exp[0].rows
    clean = model(S.MemTree([cover] + s["tables"], tree), rngs, None, False, False)
    base = int(tree.block_base[i])
    rest = [q for q, e in enumerate(clean) if base + bad not in e.blocks]
    assert len(rest) >= 40 and all(exp[q] == clean[q] for q in rest)  # the other ranges are unaffected


# ------------------------------------------------------------------------------------------------
# S6: capacity
# ------------------------------------------------------------------------------------------------
def one_call(rt, mem, dev, rngs, cand, cap, cap_links=None, ws=None):
    """One sdb_lsm_scan_mem call with the given capacities, without policies, projections and prefixes and with a chain
    iff cap_links is given, over outputs pre-filled with SENTINEL -> host(result)."""
    return host(rt.lsm_scan_mem_device(mem, dict(dev, _policies=None), rngs, workspace=ws, cand=cand, cap=cap, cap_links=cap_links,
                                       merge=cap_links is not None, alloc=Filled(SENTINEL)))


def test_capacity(rt):
    s = layers(rt)
    tables = boundary_tables()
    mt = S.MemTree(tables, s["tree"])
    mem = dev_tables(rt, tables)
    alone = S.MemTree([], s["tree"])
    few = lambda rs, most: [r for r in rs if S.scan(alone, r).candidates <= most and r[1] <= EXC and r[3] <= EXC]  # noqa: E731
    rngs = few(boundary_ranges(tables), 0)[:90] + few(s["rngs"], 40)[:15]  # the tables' own ranges, and a few of the tree's
    exp = model(mt, rngs, None, False, False)
    nc, ckb = sum(e.candidates for e in exp), sum(e.cand_key_bytes for e in exp)
    ne, kb = sum(len(e.rows) for e in exp), sum(len(r[0]) for e in exp for r in e.rows)
    tree_only = model(alone, rngs, None, False, False)
    assert 0 < ne < nc and sum(e.candidates for e in tree_only) * 4 < nc  # the need is mostly table rows
    columns = ["key_arena", "key_off", "table", "row"] + [f for f, _ in rt.LSM_SCAN_COLUMNS]
    for short in ((nc - 1, ckb), (nc, ckb - 1), (0, 0)):  # the staging one candidate / one key byte short, and none
        h = one_call(rt, mem, s["dev"], rngs, short, (ne, kb))
        assert h["sum_status"] == _abi.SDB_LIMIT_EXCEEDED
        assert (h["sum_num_candidates"], h["sum_candidate_key_bytes"]) == (nc, ckb)
        assert h["sum_num_entries"] == 0 and h["sum_key_bytes"] == 0 and untouched(h, columns, SENTINEL)
        assert not h["range_entry_start"][:len(rngs) + 1].any()
        check_ranges(exp, h)
    for short in ((ne - 1, kb), (ne, kb - 1), (0, 0)):  # exact staging, the columns one entry / one key byte short
        h = one_call(rt, mem, s["dev"], rngs, (nc, ckb), short)
        assert h["sum_status"] == _abi.SDB_LIMIT_EXCEEDED
        assert (h["sum_num_entries"], h["sum_key_bytes"]) == (ne, kb) and untouched(h, columns, SENTINEL)
        starts = np.concatenate([[0], np.cumsum([len(e.rows) for e in exp])])
        assert (h["range_entry_start"][:len(rngs) + 1] == starts).all()
        check_ranges(exp, h)
    h = one_call(rt, mem, s["dev"], rngs, (nc, ckb), (ne, kb))  # exact capacities: every row, nothing past them
    check(mt, rngs, None, False, False, h, exp)
    assert (h["key_arena"][kb:] == SENTINEL).all()
    for f in columns[2:]:
        assert (h[f][ne:].view(np.uint8) == SENTINEL).all(), f


# ------------------------------------------------------------------------------------------------
# No tables (S7), no tree (S8), a malformed table (S9)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [False, True])
def test_no_tables_is_the_projected_call(rt, chain):
    tree, straddler = M.chain_tree() if chain else L.plain_tree()
    dev = device_tree(rt, tree)
    rngs = L.narrow_ranges(tree, 100) + [(None, U, None, U), (straddler, INC, None, U)]
    bounds = [U64_MAX if q % 3 else 999_000 for q in range(len(rngs))]
    n = len(rngs)
    proj = [None if i % 2 else (L.all_keys(tree)[10], INC, L.all_keys(tree)[-10], EXC) for i in range(len(tree.leaves))]
    prefixes = [b"k0" if q % 4 == 0 else None for q in range(n)]
    for desc in (False, True):
        kw = dict(prefixes=prefixes, max_seq=bounds, descending=desc, merge=chain, fill=SENTINEL)
        want = host(rt.lsm_scan_projected_device(dev, proj, rngs, **kw))
        for mem in (None, rt.mem_tables_device([])):
            h = host(rt.lsm_scan_mem_device(mem, dev, rngs, projections=proj, **kw))
            for f, a in want.items():
                assert np.array_equal(a, h[f]), f  # every column, counter, summary word and chain column
            ne = h["sum_num_entries"]
            assert ne > 100 and (h["table"][:ne] == -1).all() and not h["row"][:ne].any() and not h["range_tables"][:n].any()
            if chain:
                nl = int(h["csum_num_links"])
                assert nl > ne and (h["chain_table"][:nl] == -1).all() and not h["chain_row"][:nl].any()
                assert (h["chain_table"][nl:].view(np.uint8) == SENTINEL).all()
    # and the model without tables is the call without tables
    check(S.MemTree([], tree), rngs, bounds, False, chain, scan(rt, None, dev, rngs, bounds, False, chain))


def test_no_tree(rt):
    s = layers(rt)
    tables, rngs, bounds = s["tables"], s["rngs"][:120] + [(None, U, None, U)], s["bounds"][:120] + [U64_MAX]
    of_empty = G.Tree([[G.Leaf(G.EmptySst())], [G.Leaf(G.EmptySst()), G.Leaf(G.EmptySst())]])
    for tree in (G.Tree([]), of_empty):  # num_ssts == 0; SSTs without a block: total_blocks == 0
        dev = dev_tree(rt, tree)
        assert dev["total_blocks"] == 0
        mt = S.MemTree(tables, tree)
        for desc in (False, True):
            h = scan(rt, s["mem"], dev, rngs, bounds, desc)
            exp = check(mt, rngs, bounds, desc, False, h)
            assert h["sum_blocks_checked"] == 0 and not h["range_ssts"].any() and not h["range_filtered"].any()
        assert len(exp[-1].rows) > 50
        check(mt, rngs, bounds, False, True, scan(rt, s["mem"], dev, rngs, bounds, False, chain=True))
    h = scan(rt, s["mem"], s["dev"], [], None, chain=True)  # tables present, no range
    assert not h["summary"].any() and not h["chain_summary"].any() and int(h["chain_start"][0]) == 0
    assert not scan(rt, s["mem"], s["dev"], [])["summary"].any()


def test_malformed_table(rt):
    s = layers(rt)
    rngs = s["rngs"][:100]
    n = len(rngs)
    structs = [r.to_ctypes() for r in s["mem"]["_runs"]]
    assert structs[1].n > 0
    for how in ("seq", "n"):
        broken = [r.to_ctypes() for r in s["mem"]["_runs"]]
        if how == "seq":
            broken[1].seq = None
        else:
            broken[2].n = 1 << 31
        bad = rt.mem_tables_device(broken)
        for chain in (False, True):
            h = host(rt.lsm_scan_mem_device(bad, s["dev"], rngs, merge=chain, fill=SENTINEL))
            assert (h["range_status"][:n] == _abi.SDB_INVALID_ARGUMENT).all()
            assert not h["range_ssts"][:n].any() and not h["range_tables"][:n].any() and not h["range_entry_start"].any()
            assert h["sum_num_failed_ranges"] == n and h["sum_status"] == _abi.SDB_INVALID_ARGUMENT
            assert h["sum_blocks_checked"] == 0 and h["sum_num_entries"] == 0 and h["sum_num_candidates"] == 0
            if chain:
                assert h["csum_num_links"] == 0
    check(s["mt"], rngs, None, False, False, scan(rt, s["mem"], s["dev"], rngs))  # the well-formed tables still answer


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
    model_ = None
    for limit in range(200, 40000, 100):  # a memtable limit that closes one table before the last batch
        model_ = replay.replay_model(batches, None, prm, limit)
        if len(model_["tables"]) == 2:
            break
    assert len(model_["tables"]) == 2
    run, start = R.as_run(batches)
    replayed = rt.wal_replay_device(rt.DeviceRun.from_host(run), start, None, prm, limit)
    assert [t.n for t in replayed] == [len(t["rows"]) for t in model_["tables"]]
    tables = [MG.Table(t["rows"]) for t in reversed(model_["tables"])]  # the table replayed last is the newest
    mem = rt.mem_tables_device([t.as_run() for t in reversed(replayed)])  # no host copy: the replay's device columns
    mt = S.MemTree(tables, G.Tree([]))
    keys = sorted({r[0] for t in tables for r in t.rows})
    rngs = [(None, U, None, U), (b"b", INC, b"c", EXC), (b"a", EXC, b"bb", INC)] + [(k, INC, k, INC) for k in keys[::3]] + \
        [(keys[i], (INC, EXC)[i % 2], keys[min(len(keys) - 1, i + 4)], (EXC, INC)[i % 2]) for i in range(0, len(keys), 2)]
    seqs = sorted({r[3] for t in tables for r in t.rows})
    bounds = [U64_MAX if q % 3 == 0 else seqs[(7 * q) % len(seqs)] for q in range(len(rngs))]
    arena = None
    for chain in (False, True):
        h = scan(rt, mem, dev_tree(rt, mt.tree), rngs, bounds, chain=chain)
        # the replay's tables share one value arena: val_off is judged through the bytes it names
        exp = model(mt, rngs, bounds, False, chain)
        rows = [r for e in exp for r in e.rows]
        # (the replayed rows hold merge operands: without a chain those ranges fail, with one every range answers)
        assert h["sum_num_entries"] == len(rows) > (50 if chain else 5) and h["sum_status"] != _abi.SDB_LIMIT_EXCEEDED
        assert h["sum_num_failed_ranges"] == sum(1 for e in exp if e.status) and (chain or h["sum_num_failed_ranges"] >= 5)
        check_ranges(exp, h)
        cols = [S.columns(mt, r) for r in rows]
        for f in ("table", "row", "val_len", "seq", "flags"):
            assert (u64(h[f][:len(rows)], f) == np.array([c[f] for c in cols], np.uint64)).all(), f
        torch.cuda.synchronize()
        arena = replayed[0].cols["val_bytes"].cpu().numpy() if arena is None else arena
        for i, c in enumerate(cols):
            vo, vl = int(h["val_off"][i]), int(h["val_len"][i])
            assert arena[vo:vo + vl].tobytes() == mt.value(("t", c["table"], c["row"])), rows[i][0]
        if chain:
            links = [l for r in rows for l in r[1]]
            assert [int(x) for x in h["chain_row"][:len(links)]] == [l[2] for l in links]
            assert [int(x) for x in h["chain_table"][:len(links)]] == [l[1] for l in links]
        assert {c["table"] for c in cols} == {0, 1}


# ------------------------------------------------------------------------------------------------
# Graph capture with the tables changed in place, workspace reuse, workspace canary (S10)
# ------------------------------------------------------------------------------------------------
def test_graph_capture_tables_changed_in_place(rt):
    import torch
    s = layers(rt)
    tree, dev = s["tree"], s["dev"]
    rngs = s["rngs"][:100]
    n = len(rngs)
    # two sets of tables of one shape: the same keys and value bytes; a tombstone becomes an empty value and an empty
    # value a tombstone, and every other table's seqs rise above everything else's, so other rows win
    tabs_a = s["tables"]
    tabs_b = []
    for j, t in enumerate(tabs_a):
        es = [(r[0], 2 if r[4] & _abi.FLAG_TOMBSTONE else 0, t.value(i), r[3], r[5], r[6]) for i, r in enumerate(t.rows)]
        tabs_b.append(MG.Table([(k, 0 if kind == 2 else (2 if not v else 0), v, seq + 10_000_000 * (j % 2), c, e)
                                for k, kind, v, seq, c, e in es]))
        assert [r[0] for r in tabs_b[-1].rows] == [r[0] for r in t.rows]
        assert tabs_b[-1].run.val_base.shape == t.run.val_base.shape
    mts = (S.MemTree(tabs_a, tree), S.MemTree(tabs_b, tree))
    assert model(mts[0], rngs, None, False, False) != model(mts[1], rngs, None, False, False)
    druns = [rt.DeviceRun.from_host(t.run) for t in tabs_a]
    other = [rt.DeviceRun.from_host(t.run) for t in tabs_b]
    mem = rt.mem_tables_device(druns)
    exps = [model(mt, rngs, None, False, False) for mt in mts]
    cand = (max(sum(e.candidates for e in x) for x in exps), max(sum(e.cand_key_bytes for e in x) for x in exps))
    rg = {k: to_dev(a) for k, a in rt.scan_ranges_columnar(rngs).items()}
    rg["n"] = n
    big, ws = canaried_workspace(rt, "sdb_lsm_scan_mem", dev, n, cand, tables=mem, byte=0x5A)
    kw = dict(workspace=ws, cand=cand, cap=cand)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):  # the first launch (function attributes) outside the capture
        warm = rt.lsm_scan_mem_device(mem, dev, rg, stream=st, **kw)
    st.synchronize()
    check(mts[0], rngs, None, False, False, host(warm), exps[0])
    g = torch.cuda.CUDAGraph()
    holder = {}
    with torch.cuda.graph(g, stream=st):
        holder["res"] = rt.lsm_scan_mem_device(mem, dev, rg, stream=st, **kw)
    saved = [[x.clone() for x in d.t] for d in druns]
    checked = []
    for which, src in ((1, [d.t for d in other]), (0, saved)):  # the tables' contents replaced in place between replays
        for d, tensors in zip(druns, src):
            for dst, t in zip(d.t, tensors):
                assert dst.shape == t.shape
                dst.copy_(t)
        for k, t in holder["res"].items():
            if not k.startswith("_"):
                t.zero_()
        torch.cuda.synchronize()
        g.replay()
        h = host(holder["res"])
        check(mts[which], rngs, None, False, False, h, exps[which])
        checked.append(h["sum_blocks_checked"])
    assert checked[0] == checked[1] > 0
    intact(big, ws.numel(), 0x5A)  # exactly workspace_bytes, no more
    del g


@pytest.mark.parametrize("chain", [False, True])
def test_workspace_canary(rt, chain):
    """A workspace of exactly the advertised size inside guard bands: the call writes nothing outside it."""
    mt, rngs, _ = chain_layers()
    mem, dev = dev_tables(rt, mt.tables), dev_tree(rt, mt.tree)
    exp = model(mt, rngs, None, False, chain)
    nc, ckb = totals(exp)[0]
    big, ws = canaried_workspace(rt, "sdb_lsm_scan_mem", dev, len(rngs), (nc, ckb), chain, mem, byte=0x5A)
    h = one_call(rt, mem, dev, rngs, (nc, ckb), (nc, ckb), cap_links=nc if chain else None, ws=ws)
    check(mt, rngs, None, False, chain, h, exp)
    intact(big, ws.numel(), 0x5A)
