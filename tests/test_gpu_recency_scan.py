"""GPU parity of sdb_lsm_scan_recency (Db::scan_prefix_by_recency; slatedb_amd/csrc/sdb_lsm_scan.hip, the k_lr_* kernels)
against the model of tests/recency_cases.py: every column of every row, every range_* array and every summary word.
The trees are tiny: at most 3 tables of at most 8 rows, at most 5 SSTs of at most 4 blocks of 64 bytes, at most 16
ranges per call."""
import numpy as np
import pytest

from slatedb_amd import _abi

from . import filtered_read_cases as F
from . import get_cases as G
from . import malformed_blocks as MB
from . import mem_get_cases as MG
from . import mem_scan_cases as S
from . import recency_cases as RC
from . import test_gpu_get as TG
from . import test_gpu_mem_scan as MS
from .read_harness import (Filled, canaried_workspace, check_scan_core, compare, dev_tables, host, intact, rt, to_dev,  # noqa: F401
                           totals, untouched, view_of)
from .scan_cases import EXC, INC, U

pytestmark = pytest.mark.gpu

U64_MAX = G.U64_MAX
SENTINEL = MS.SENTINEL
BS = 64  # the smallest block size of the encoder fixtures
PX = b"px:"
ALL = RC.prefix_range(PX)
BAD = _abi.SDB_CHECKSUM_MISMATCH


def v(key, val, seq, kind=0, ets=None):
    return (key, kind, b"" if kind == 2 else val, seq, None, ets)


class Layers:
    """A MemTree with its device forms.  corrupt: [(leaf, block)]: one byte of the block flipped on the device and
    SDB_CHECKSUM_MISMATCH in the model."""

    def __init__(self, rt, tables, runs, corrupt=(), views=None):
        self.mt = S.MemTree(tables, G.Tree(runs))
        leaves = self.mt.tree.leaves
        assert len(tables) <= 3 and all(len(t.rows) <= 8 for t in tables) and len(leaves) <= 5
        assert all(l.sst.nb <= 4 for l in leaves)
        views = views or [view_of(l) for l in leaves]
        for i, b in corrupt:
            data = leaves[i].sst.data.copy()
            data[int(leaves[i].sst.block_off[b]) + 5] ^= 0x40
            views[i] = view_of(leaves[i], data=data)
            leaves[i].block_status[b] = BAD
        self.dev = rt.lsm_tree_device(views, [len(r) for r in runs])
        self.mem = dev_tables(rt, tables) if tables else None


def case(rng=ALL, prefix=PX, bound=None, limit=0):
    return dict(rng=rng, prefix=prefix, bound=bound, limit=limit)


def call(rt, x, cases, desc=False, visible=None, **kw):
    assert len(cases) <= 16
    bounds = None if all(c["bound"] is None for c in cases) else [U64_MAX if c["bound"] is None else c["bound"] for c in cases]
    limits = None if all(not c["limit"] for c in cases) else [c["limit"] for c in cases]
    res = rt.lsm_scan_recency_device(x.mem, x.dev, [c["rng"] for c in cases], projections=visible,
                                     prefixes=[c["prefix"] for c in cases] or None, max_seq=bounds, limit=limits, descending=desc, **kw)
    return host(res)


def model(x, cases, desc=False, visible=None, fits=True):
    return [RC.scan_recency(x.mt, c["rng"], c["prefix"], c["bound"], c["limit"], desc, visible, fits=fits) for c in cases]


def check_ranges(exp, h):
    n = len(exp)
    for f, want in (("range_status", [e.status for e in exp]), ("range_ssts", [len(e.ssts) for e in exp]),
                    ("range_tables", [len(e.tables) for e in exp]), ("range_filtered", [len(e.filtered) for e in exp]),
                    ("range_sources_read", [e.sources_read for e in exp]), ("range_visible", [e.visible for e in exp])):
        assert h[f][:n].astype(np.int64).tolist() == want, f
    assert h["sum_blocks_checked"] == len(set().union(*[e.blocks for e in exp]))
    assert int(h["num_filtered"][0]) == sum(len(e.filtered) for e in exp)
    failed = [q for q, e in enumerate(exp) if e.status]
    assert h["sum_num_failed_ranges"] == len(failed)
    assert h["sum_num_candidates"] == sum(e.candidates for e in exp)
    assert h["sum_candidate_key_bytes"] == sum(e.cand_key_bytes for e in exp)


def check(x, cases, desc, h, visible=None, exp=None):
    """Every column of every row, every range array, every summary word.  Returns the model's results."""
    exp = exp or model(x, cases, desc, visible)
    check_ranges(exp, h)
    rows = check_scan_core(exp, h)
    compare(MS.ROW_COLS, [RC.columns(x.mt, r) for r in rows], lambda f: h[f], "row")
    return exp


def keys_of(e):
    return [(k, src[0], src[1]) for k, src in e.rows]


# ------------------------------------------------------------------------------------------------
# R1 / R2: the order of the sources, nothing deduplicated
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [1, 2])
def test_source_order_and_no_dedup(rt, version):
    """One key in a table, an L0 SST and a run: a tombstone in the middle source, an operand in the oldest."""
    t0 = MG.Table([v(b"px:a", b"new", 30), v(b"px:b", b"tb", 31), v(b"qq:x", b"no", 32)])
    l0 = G.leaf_of([v(b"px:a", b"", 20, 2), v(b"px:c", b"lc", 21)], version, BS)
    run = G.leaf_of([v(b"px:a", b"op", 10, 1), v(b"px:a", b"base", 9), v(b"pw:z", b"no", 8)], version, BS)
    x = Layers(rt, [t0], [[l0], [run]])
    for desc in (False, True):
        cases = [case(), case(RC.prefix_range(b"px:a"), b"px:a"), case(RC.prefix_range(b"zz"), b"zz"), case((None, U, None, U), None)]
        exp = check(x, cases, desc, call(rt, x, cases, desc))
    assert keys_of(exp[1]) == [(b"px:a", "t", 0), (b"px:a", "s", 0), (b"px:a", "s", 1), (b"px:a", "s", 1)]
    assert [RC.kind_of(x.mt.row_of(s)[4]) for _, s in exp[1].rows] == [0, 2, 1, 0] and exp[1].sources_read == 3
    assert not exp[2].rows and exp[2].sources_read == 0 and len(exp[3].rows) == 8


@pytest.mark.parametrize("version", [1, 2])
def test_golden_cases(rt, version):
    for c in RC.golden_cases():
        mt = S.golden_mem_tree(c, version)
        x = Layers(rt, mt.tables, mt.tree.runs)
        p = c["prefix"].encode()
        cases = [case(RC.prefix_range(p), p, c["max_seq"])]
        h = call(rt, x, cases)
        check(x, cases, False, h)
        got = []
        for i in range(h["sum_num_entries"]):
            t, vo, vl = int(h["table"][i]), int(h["val_off"][i]), int(h["val_len"][i])
            src = x.mt.tables[t].run.val_base if t >= 0 else x.mt.tree.leaves[int(h["sst"][i])].sst.data
            got.append([h["key_arena"][int(h["key_off"][i]):int(h["key_off"][i + 1])].tobytes().decode(),
                        RC.kind_of(int(h["flags"][i])), bytes(src[vo:vo + vl]).decode()])
        assert got == c["expected"], c["description"]


# ------------------------------------------------------------------------------------------------
# R3: key groups, ascending and descending
# ------------------------------------------------------------------------------------------------
def group_layers(rt, version):
    """An SST whose key px:k has three versions that straddle a block boundary; a run of two SSTs cut inside the three
    versions of px:m; a key that is a proper prefix of its neighbour; single-row sources."""
    pad = b"x" * 8
    es = [v(b"px:a", pad, 50), v(b"px:k", pad, 49), v(b"px:k", pad, 48), v(b"px:k", pad, 47), v(b"px:k\x00", pad, 46),
          v(b"px:kk", pad, 45), v(b"px:z", pad, 44)]
    l0 = G.leaf_of(es, version, BS)
    s = l0.sst
    where = [max(b for b in range(s.nb) if s.bes[b] <= i) for i, k in enumerate(s.keys) if k == b"px:k"]
    assert len(set(where)) > 1, "px:k straddles a block boundary"
    r0 = G.leaf_of([v(b"px:b", b"1", 30), v(b"px:m", b"m3", 29), v(b"px:m", b"m2", 28)], version, BS)
    r1 = G.leaf_of([v(b"px:m", b"m1", 27), v(b"px:n", b"n", 26)], version, BS)
    one = G.leaf_of([v(b"px:k", b"only", 5)], version, BS)
    t0 = MG.Table([v(b"px:k", b"t", 90)])
    return Layers(rt, [t0], [[l0], [r0, r1], [one]])


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("version", [1, 2])
def test_key_groups(rt, version, desc):
    x = group_layers(rt, version)
    cases = [case(), case(RC.prefix_range(b"px:k"), b"px:k"), case((b"px:k", INC, b"px:k", INC), b"px:k"),
             case(RC.prefix_range(b"px:m"), b"px:m"), case((b"px:k", EXC, b"px:m", INC)), case(limit=3), case(limit=5)]
    exp = check(x, cases, desc, call(rt, x, cases, desc))
    run = [(k, x.mt.row_of(s)[3]) for k, s in exp[3].rows]
    # R1 / R3: the run's SSTs last to first when descending, each ordered on its own, nothing joined across them
    assert run == ([(b"px:m", 27), (b"px:m", 29), (b"px:m", 28)] if desc else [(b"px:m", 29), (b"px:m", 28), (b"px:m", 27)])
    l0 = [(k, x.mt.row_of(s)[3]) for k, s in exp[1].rows if s[:2] == ("s", 0)]
    want = [(b"px:k", 49), (b"px:k", 48), (b"px:k", 47), (b"px:k\x00", 46), (b"px:kk", 45)]
    assert l0 == ([want[4], want[3]] + want[:3] if desc else want)


def test_v2_block_without_restarts_descending(rt):
    """The last block of a V2 SST with its restart table removed (count 0): it is walked ascending in both
    directions, and its rows come back."""
    leaf = G.leaf_of([v(b"px:%02d" % i, b"v" * 12, 40 - i) for i in range(6)], 2, BS)
    s = leaf.sst
    off = [int(o) for o in s.block_off]
    payloads = [s.data.tobytes()[off[k]:off[k + 1] - 4] for k in range(s.nb)]
    L = MB.Layout(payloads[-1], 2)
    payloads[-1] = L.build(offs=[], count=0)
    assert MB.walk(payloads[-1], 2)[0] == 0
    data, block_off = MB.arena(payloads)
    x = Layers(rt, [], [[leaf]], views=[view_of(leaf, data=data, block_off=block_off)])
    for desc in (False, True):
        cases = [case(), case(limit=2)]
        exp = check(x, cases, desc, call(rt, x, cases, desc))
        assert len(exp[0].rows) == 6 and exp[0].status == 0


# ------------------------------------------------------------------------------------------------
# R2: max_seq
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("desc", [False, True])
def test_max_seq(rt, desc):
    t0 = MG.Table([v(b"px:a", b"t", 90), v(b"px:b", b"t", 91)])
    l0 = G.leaf_of([v(b"px:a", b"3", 53), v(b"px:a", b"2", 52), v(b"px:a", b"1", 51), v(b"px:c", b"c", 50)], 2, BS)
    run = G.leaf_of([v(b"px:a", b"old", 10)], 1, BS)
    x = Layers(rt, [t0], [[l0], [run]])
    # 60 hides the whole table: it is passed and counted as read; 52 hides the newest version inside a group
    cases = [case(bound=60), case(bound=52), case(bound=52, limit=2), case(bound=5), case(bound=60, limit=4), case()]
    exp = check(x, cases, desc, call(rt, x, cases, desc))
    assert exp[0].sources_read == 3 and exp[0].tables == [0] and all(s[0] == "s" for _, s in exp[0].rows)
    assert [x.mt.row_of(s)[3] for _, s in exp[1].rows if s[:2] == ("s", 0)] == ([50, 52, 51] if desc else [52, 51, 50])
    assert exp[3].sources_read == 3 and not exp[3].rows and exp[3].visible == 0
    assert exp[4].sources_read == 2 and exp[4].visible == 4


# ------------------------------------------------------------------------------------------------
# R5: limit and laziness
# ------------------------------------------------------------------------------------------------
def lazy_layers(rt, corrupt=()):
    """Table (2 rows), L0 SST 0 (4 rows, 2 blocks), run of SSTs 1 and 2 (2 + 2 rows), L0-like run SST 3 (1 row)."""
    pad = b"y" * 20
    t0 = MG.Table([v(b"px:a", b"t", 90), v(b"px:b", b"t", 91)])
    l0 = G.leaf_of([v(b"px:a", pad, 54), v(b"px:a", pad, 53), v(b"px:c", pad, 52), v(b"px:d", pad, 51)], 2, BS)
    assert l0.sst.nb >= 2
    r0 = G.leaf_of([v(b"px:a", b"r", 30), v(b"px:b", b"r", 29)], 1, BS)
    r1 = G.leaf_of([v(b"px:e", b"r", 28), v(b"px:f", b"r", 27)], 1, BS)
    old = G.leaf_of([v(b"px:a", b"o", 5)], 2, BS)
    return Layers(rt, [t0], [[l0], [r0, r1], [old]], corrupt)


@pytest.mark.parametrize("desc", [False, True])
def test_limit(rt, desc):
    x = lazy_layers(rt)
    # 0, 1, exactly the table's visible rows (the next source is not opened), one more, mid key group, exactly two
    # sources, inside the run, larger than everything: mixed per range in one call
    limits = [0, 1, 2, 3, 4, 6, 8, 9, 11, 12, 100]
    cases = [case(limit=n) for n in limits]
    exp = check(x, cases, desc, call(rt, x, cases, desc))
    assert [e.sources_read for e in exp] == [4, 1, 1, 2, 2, 2, 3, 3, 4, 4, 4]
    assert [len(e.rows) for e in exp] == [11, 1, 2, 3, 4, 6, 8, 9, 11, 11, 11]
    assert [e.visible for e in exp] == [11, 2, 2, 6, 6, 6, 10, 10, 11, 11, 11]


def test_laziness_of_errors(rt):
    lb = 1  # the L0 SST's last block: beyond its first row
    for desc in (False, True):
        # a corrupt block in a source after the stop source: status OK and the rows are returned
        x = lazy_layers(rt, [(3, 0)])
        cases = [case(limit=2), case(limit=6), case(limit=10), case(limit=11), case(), case(RC.prefix_range(b"px:e"), b"px:e")]
        exp = check(x, cases, desc, call(rt, x, cases, desc))
        assert [e.status for e in exp] == [0, 0, 0, BAD, BAD, 0] and len(exp[2].rows) == 10 and exp[3].sources_read == 4
        # in the stop source beyond the L-th row: a failed range with no rows; before the stop source: failed
        x = lazy_layers(rt, [(0, lb)])
        cases = [case(limit=2), case(limit=3), case(limit=8), case(), case(RC.prefix_range(b"px:a"), b"px:a", limit=3)]
        exp = check(x, cases, desc, call(rt, x, cases, desc))
        assert [e.status for e in exp[:4]] == [0, BAD, BAD, BAD]
        assert exp[1].sources_read == 2 and not exp[1].rows and exp[1].visible == 0
        # a run is one source: its second SST fails the range whose limit its first SST satisfies
        x = lazy_layers(rt, [(2, 0)])
        cases = [case(limit=6), case(limit=7), case(RC.prefix_range(b"px:a"), b"px:a")]
        exp = check(x, cases, desc, call(rt, x, cases, desc))
        assert [e.status for e in exp] == [0, BAD, 0]
    # limit 0: the first failing source in walk order decides; the other ranges of the call are unaffected
    x = lazy_layers(rt, [(3, 0)])
    x.mt.tree.leaves[1].version = 3  # and an invalid version in the run before it
    views = [view_of(l) for l in x.mt.tree.leaves]
    data = x.mt.tree.leaves[3].sst.data.copy()
    data[int(x.mt.tree.leaves[3].sst.block_off[0]) + 5] ^= 0x40
    views[3] = view_of(x.mt.tree.leaves[3], data=data)
    x.dev = rt.lsm_tree_device(views, [1, 2, 1])
    cases = [case(), case(limit=6), case(limit=7), case(RC.prefix_range(b"px:e"), b"px:e"), case(RC.prefix_range(b"px:c"), b"px:c")]
    exp = check(x, cases, False, call(rt, x, cases))
    assert [e.status for e in exp] == [_abi.SDB_INVALID_VERSION, 0, _abi.SDB_INVALID_VERSION, 0, 0]


# ------------------------------------------------------------------------------------------------
# Filters and views
# ------------------------------------------------------------------------------------------------
def test_prefix_filtered_sst_is_not_opened(rt):
    pol = F.Policy(F.FIXED, 3, 0)
    l0 = F.build_leaf(sorted([v(b"pw:a", b"1", 50), v(b"py:a", b"2", 49)]), 2, BS, pol)  # meets px:'s range, holds no px: key
    l1 = F.build_leaf([v(b"px:a", b"3", 40), v(b"px:b", b"4", 39)], 1, BS, pol)
    t0 = MG.Table([v(b"px:a", b"t", 90)])
    x = Layers(rt, [t0], [[l0], [l1]], corrupt=[(0, 0)])
    cases = [case(), case(limit=1), case(prefix=None), case(RC.prefix_range(b"p"), b"p")]
    exp = check(x, cases, False, call(rt, x, cases))
    assert exp[0].filtered == [0] and exp[0].status == 0 and exp[0].sources_read == 2 and len(exp[0].rows) == 3
    assert exp[2].status == BAD and not exp[2].filtered  # without the prefix the SST is opened, and fails the range
    assert exp[3].status == BAD  # a prefix shorter than the extractor's probes nothing


@pytest.mark.parametrize("desc", [False, True])
def test_projected_view_cuts_a_key_group(rt, desc):
    x = group_layers(rt, 2)
    # SST 0's view ends between px:k and px:k\0 and starts behind px:a; the run's first SST shows nothing of px:m
    visible = [(b"px:b", INC, b"px:k", INC), (None, U, b"px:m", EXC), None, None]
    cases = [case(), case(RC.prefix_range(b"px:k"), b"px:k"), case(limit=4), case(RC.prefix_range(b"px:m"), b"px:m")]
    exp = check(x, cases, desc, call(rt, x, cases, desc, visible), visible)
    assert [k for k, s in exp[1].rows if s[:2] == ("s", 0)] == [b"px:k"] * 3
    assert [x.mt.row_of(s)[3] for _, s in exp[3].rows] == [27]


# ------------------------------------------------------------------------------------------------
# R6: capacity
# ------------------------------------------------------------------------------------------------
def one_call(rt, x, cases, cand, cap, desc=False, ws=None):
    """One sdb_lsm_scan_recency call with the given capacities, without policies and projections, over outputs
    pre-filled with SENTINEL -> host(result)."""
    return host(rt.lsm_scan_recency_device(x.mem, dict(x.dev, _policies=None), [c["rng"] for c in cases],
                                           prefixes=[c["prefix"] for c in cases], limit=[c["limit"] for c in cases], descending=desc,
                                           workspace=ws, cand=cand, cap=cap, alloc=Filled(SENTINEL)))


def test_capacity(rt):
    x = lazy_layers(rt, [(3, 0)])
    cases = [case(limit=n) for n in (0, 3, 6, 10)] + [case(RC.prefix_range(b"px:a"), b"px:a", limit=2)]
    exp = model(x, cases)
    short = model(x, cases, fits=False)
    nc, ckb = sum(e.candidates for e in exp), sum(e.cand_key_bytes for e in exp)
    ne, kb = sum(len(e.rows) for e in exp), sum(len(r[0]) for e in exp for r in e.rows)
    assert 0 < ne < nc and exp[0].status == BAD and exp[1].status == 0 and short[1].status == BAD
    columns = ["key_arena", "key_off", "table", "row"] + [f for f, _ in rt.LSM_SCAN_COLUMNS]
    for less in ((nc - 1, ckb), (nc, ckb - 1), (0, 0)):  # the staging one candidate / one key byte short, and none
        h = one_call(rt, x, cases, less, (ne, kb))
        assert h["sum_status"] == _abi.SDB_LIMIT_EXCEEDED
        assert h["sum_num_entries"] == 0 and h["sum_key_bytes"] == 0 and untouched(h, columns, SENTINEL)
        assert not h["range_entry_start"][:len(cases) + 1].any()
        check_ranges(short, h)  # R6: the statuses of limit 0, nothing read
    for less in ((ne - 1, kb), (ne, kb - 1), (0, 0)):  # exact staging, the columns one entry / one key byte short
        h = one_call(rt, x, cases, (nc, ckb), less)
        assert h["sum_status"] == _abi.SDB_LIMIT_EXCEEDED
        assert (h["sum_num_entries"], h["sum_key_bytes"]) == (ne, kb) and untouched(h, columns, SENTINEL)
        assert h["range_entry_start"][:len(cases) + 1].tolist() == np.concatenate([[0], np.cumsum([len(e.rows) for e in exp])]).tolist()
        check_ranges(exp, h)
    h = one_call(rt, x, cases, (nc, ckb), (ne, kb))  # exact capacities: every row, nothing past them
    check(x, cases, False, h, exp=exp)
    assert (h["key_arena"][kb:] == SENTINEL).all()
    for f in columns[2:]:
        assert (h[f][ne:].view(np.uint8) == SENTINEL).all(), f


# ------------------------------------------------------------------------------------------------
# R7: no tables, no tree, malformed inputs
# ------------------------------------------------------------------------------------------------
def test_no_tables_and_no_tree(rt):
    x = lazy_layers(rt)
    cases = [case(), case(limit=5), case(RC.prefix_range(b"px:a"), b"px:a")]
    full = check(x, cases, False, call(rt, x, cases))
    tables = x.mt.tables
    for mem in (None, rt.mem_tables_device([])):  # S7: the tree alone; no row names a table
        y = lazy_layers(rt)
        y.mt.tables, y.mem = [], mem
        h = call(rt, y, cases)
        exp = check(y, cases, False, h)
        ne = h["sum_num_entries"]
        assert ne == 9 + 5 + 4 and (h["table"][:ne] == -1).all() and not h["row"][:ne].any() and not h["range_tables"][:3].any()
        assert exp[0].rows == [r for r in full[0].rows if r[1][0] == "s"]
    of_empty = G.Tree([[G.Leaf(G.EmptySst())]])
    for tree in (G.Tree([]), of_empty):  # S8: the tables alone
        z = Layers(rt, tables, tree.runs)
        for desc in (False, True):
            h = call(rt, z, cases, desc)
            exp = check(z, cases, desc, h)
            assert h["sum_blocks_checked"] == 0 and not h["range_ssts"].any() and len(exp[0].rows) == 2
    z = Layers(rt, [], [])  # neither: every range is empty, nothing is read
    h = call(rt, z, cases)
    check(z, cases, False, h)
    assert not h["summary"].any() and not h["range_sources_read"].any() and not h["range_visible"].any()
    h = call(rt, x, [])  # no range
    assert not h["summary"].any()


def test_malformed_table_and_tree(rt):
    x = lazy_layers(rt)
    cases = [case(), case(limit=2), case(RC.prefix_range(b"zz"), b"zz")]
    n = len(cases)
    broken = [r.to_ctypes() for r in x.mem["_runs"]]
    broken[0].seq = None
    rs = x.dev["_run_start"].clone()
    rs[1], rs[2] = 3, 1  # not monotone
    for mem, dev in ((rt.mem_tables_device(broken), x.dev), (x.mem, TG.with_arrays(rt, x.dev, run_start=rs))):
        h = host(rt.lsm_scan_recency_device(mem, dev, [c["rng"] for c in cases], prefixes=[c["prefix"] for c in cases],
                                            limit=[c["limit"] for c in cases]))
        assert (h["range_status"][:n] == _abi.SDB_INVALID_ARGUMENT).all()
        assert not h["range_ssts"][:n].any() and not h["range_tables"][:n].any() and not h["range_entry_start"].any()
        assert not h["range_sources_read"][:n].any() and not h["range_visible"][:n].any()
        assert h["sum_num_failed_ranges"] == n and h["sum_status"] == _abi.SDB_INVALID_ARGUMENT
        assert h["sum_blocks_checked"] == 0 and h["sum_num_entries"] == 0 and h["sum_num_candidates"] == 0
    bad_kind = [case((b"px:", 3, None, U)), case()]
    check(x, bad_kind, False, call(rt, x, bad_kind))  # a bad bound kind fails its range alone
    check(x, cases, False, call(rt, x, cases))  # the well-formed inputs still answer


# ------------------------------------------------------------------------------------------------
# The relation with sdb_lsm_scan_mem, graph capture, the workspace canary
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [10, 13])
def test_first_occurrence_per_key_is_the_mem_scan(rt, seed):
    """On a well-formed tree (every newer source holds higher seqs), limit 0, ascending: the first occurrence per key
    in walk order, tombstones dropped, is what sdb_lsm_scan_mem returns, on the device."""
    mt = RC.layered_tree(seed, kinds=(0, 0, 2), ntab=2, nl0=1, run_ssts=(2, 2), nkeys=10, tiny=True)
    x = Layers(rt, mt.tables, mt.tree.runs)
    rngs = [RC.prefix_range(b"px:"), RC.prefix_range(b"px:0"), (None, U, None, U), RC.prefix_range(b"py"), (b"px:03", INC, b"px:03", INC)]
    cases = [case(r, None) for r in rngs]
    h = call(rt, x, cases)
    check(x, cases, False, h)
    g = host(rt.lsm_scan_mem_device(x.mem, x.dev, rngs))
    assert g["sum_status"] == 0 and h["sum_num_candidates"] == g["sum_num_candidates"]
    for q in range(len(rngs)):
        first = {}
        for i in range(int(h["range_entry_start"][q]), int(h["range_entry_start"][q + 1])):
            key = h["key_arena"][int(h["key_off"][i]):int(h["key_off"][i + 1])].tobytes()
            first.setdefault(key, i)
        mine = [(k, i) for k, i in sorted(first.items()) if not int(h["flags"][i]) & _abi.FLAG_TOMBSTONE]
        a, b = int(g["range_entry_start"][q]), int(g["range_entry_start"][q + 1])
        assert len(mine) == b - a
        for (key, i), j in zip(mine, range(a, b)):
            assert key == g["key_arena"][int(g["key_off"][j]):int(g["key_off"][j + 1])].tobytes()
            for f in MS.ROW_COLS + ("create_ts", "expire_ts"):
                assert h[f][i] == g[f][j], (f, key)


def test_graph_capture_tables_changed_in_place(rt):
    import torch
    x = lazy_layers(rt)
    cases = [case(limit=n) for n in (0, 1, 3, 7)]
    n = len(cases)
    t_b = MG.Table([v(b"px:a", b"t", 40), v(b"px:b", b"t", 95)])  # the same keys and value bytes, other seqs: under the bound
    mts = (x.mt, S.MemTree([t_b], x.mt.tree))
    bounds = [60] * n
    for c in cases:
        c["bound"] = 60
    exps = []
    for mt in mts:
        x.mt = mt
        exps.append(model(x, cases))
    assert exps[0] != exps[1]
    druns = [rt.DeviceRun.from_host(t.run) for t in mts[0].tables]
    other = [rt.DeviceRun.from_host(t.run) for t in mts[1].tables]
    mem = rt.mem_tables_device(druns)
    cand = (max(sum(e.candidates for e in ex) for ex in exps), max(sum(e.cand_key_bytes for e in ex) for ex in exps))
    rg = {k: to_dev(a) for k, a in rt.scan_ranges_columnar([c["rng"] for c in cases]).items()}
    rg["n"] = n
    px = {k: None if a is None else to_dev(a) for k, a in rt.scan_prefixes_columnar([c["prefix"] for c in cases]).items()}
    lim, bnd = to_dev(np.array([c["limit"] for c in cases], np.uint64)), to_dev(np.array(bounds, np.uint64))
    big, ws = canaried_workspace(rt, "sdb_lsm_scan_recency", x.dev, n, cand, tables=mem, byte=0x5A)
    kw = dict(prefixes=px, max_seq=bnd, limit=lim, workspace=ws, cand=cand, cap=cand)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):  # the first launch (function attributes) outside the capture
        warm = rt.lsm_scan_recency_device(mem, x.dev, rg, stream=st, **kw)
    st.synchronize()
    x.mt = mts[0]
    check(x, cases, False, host(warm), exp=exps[0])
    g = torch.cuda.CUDAGraph()
    holder = {}
    with torch.cuda.graph(g, stream=st):
        holder["res"] = rt.lsm_scan_recency_device(mem, x.dev, rg, stream=st, **kw)
    saved = [[t.clone() for t in d.t] for d in druns]
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
        x.mt = mts[which]
        check(x, cases, False, host(holder["res"]), exp=exps[which])
    intact(big, ws.numel(), 0x5A)  # exactly workspace_bytes, no more
    del g


@pytest.mark.parametrize("desc", [False, True])
def test_workspace_canary(rt, desc):
    """A workspace of exactly the advertised size inside guard bands: the call writes nothing outside it."""
    x = group_layers(rt, 2)
    cases = [case(), case(limit=4), case(RC.prefix_range(b"px:k"), b"px:k")]
    exp = model(x, cases, desc)
    nc, ckb = totals(exp)[0]
    big, ws = canaried_workspace(rt, "sdb_lsm_scan_recency", x.dev, len(cases), (nc, ckb), tables=x.mem, byte=0x5A)
    check(x, cases, desc, one_call(rt, x, cases, (nc, ckb), (nc, ckb), desc, ws=ws), exp=exp)
    intact(big, ws.numel(), 0x5A)
