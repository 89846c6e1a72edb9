"""GPU parity of the projected tree reads (sdb_lsm_scan_projected, sdb_lsm_get_projected) against the model of
tests/projected_read_cases.py, every column and counter: the seeded sweep of random projections, every position of
a visible bound (a block's index key, mid-block, between blocks, outside the SST, on a key whose versions fill whole
blocks), degenerate visible ranges and the filter query they make, the get shapes (a run cut inside a key, the
key-gap run, hidden newer versions through get, scan and both merge forms), errors behind a projection, malformed
projections, NULL and open projections against the filtered calls, the capacity protocol and canaries."""
import ctypes as C

import numpy as np
import pytest

from slatedb_amd import _abi

from . import filtered_read_cases as F
from . import get_cases as G
from . import lsm_scan_cases as L
from . import merge_read_cases as M
from . import projected_read_cases as P
from . import test_gpu_filtered_reads as FR
from . import test_gpu_get as TG
from . import test_gpu_lsm_scan as LS
from . import test_gpu_merge_reads as TM
from .read_harness import Guard, device_tree, host, rt, to_dev, totals, view_of  # noqa: F401
from .scan_cases import EXC, INC, U, partitions_covering_range

pytestmark = pytest.mark.gpu

ALL = (None, U, None, U)
BAD = _abi.SDB_INVALID_ARGUMENT


_trees = {}


def fixture(rt, name, build=None):
    """A tree built once with its device form: the trees of filtered_read_cases by name, or what `build` returns
    (a tree, or a tuple that starts with one)."""
    if name not in _trees:
        made = build() if build else getattr(F, name)()
        tree = made[0] if isinstance(made, tuple) else made
        _trees[name] = dict(tree=tree, made=made, dev=device_tree(rt, tree))
    return _trees[name]


def plain_cases(rngs):
    return [(r, None, -1) for r in rngs]


def model(tree, vis, cases, bounds=None, desc=False):
    return [P.scan(tree, vis, r, p, pl, None if bounds is None else bounds[q], desc) for q, (r, p, pl) in enumerate(cases)]


def call(rt, dev, vis, cases, bounds=None, desc=False, **kw):
    return rt.lsm_scan_projected_device(dev, vis, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases],
                                        max_seq=bounds, descending=desc, **kw)


def scan_and_check(rt, m, vis, cases, bounds=None, desc=False):
    exp = model(m["tree"], vis, cases, bounds, desc)
    h = host(call(rt, m["dev"], vis, cases, bounds, desc))
    FR.check(m["tree"], cases, bounds, desc, h, exp)
    return exp, h


def get_and_check(rt, m, vis, keys, bounds=None):
    """Every column of the gets against projected_read_cases.Tree (probe_len NULL on both sides)."""
    pt = P.projected(m["tree"], vis)
    h = host(rt.lsm_get_projected_device(m["dev"], None, vis, keys, max_seq=bounds))
    got = TG.check(pt, keys, bounds, h)
    TG.check_blocks_checked(pt, keys, got, h)
    return got, h


# ------------------------------------------------------------------------------------------------
# The seeded sweep (the cases tests/test_projected_read_cases.py holds against the trimmed SSTs)
# ------------------------------------------------------------------------------------------------
def sweep_cases(tree):
    return F.scan_cases(tree) + plain_cases(L.narrow_ranges(tree, 40))


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("seed", P.SWEEP_SEEDS)
def test_sweep_scan(rt, seed, desc):
    m = fixture(rt, "main_tree")
    tree, cases = m["tree"], sweep_cases(m["tree"])
    vis = P.random_projections(tree, seed)
    assert len(cases) >= 65 and len(cases) * len(tree.leaves) > 256  # a wave of pairs spans SSTs; several workgroups
    bounds = FR.seq_bounds(tree, len(cases)) if desc else None
    exp, h = scan_and_check(rt, m, vis, cases, bounds, desc)
    free = [F.scan(tree, r, p, pl, None if bounds is None else bounds[q], desc) for q, (r, p, pl) in enumerate(cases)]
    assert sum(e.candidates for e in exp) < sum(e.candidates for e in free) and sum(len(e.rows) for e in exp) >= 200


@pytest.mark.parametrize("seed", P.SWEEP_SEEDS)
def test_sweep_get(rt, seed):
    m = fixture(rt, "main_tree")
    tree = m["tree"]
    keys = F.get_keys(tree)[::3]
    assert len(keys) * len(tree.runs) > 256
    vis = P.random_projections(tree, seed)
    got, _ = get_and_check(rt, m, vis, keys)
    free = [tree.get(k) for k in keys]
    assert sum(g.state == _abi.GET_FOUND for g in got) >= 50
    assert sum((a.state, a.sst) != (b.state, b.sst) for a, b in zip(got, free)) >= 20  # the projections matter
    get_and_check(rt, m, vis, keys, FR.seq_bounds(tree, len(keys), seed))


def test_sweep_without_policies(rt):
    """get_cases.main_tree, policies NULL (the plain whole-key filters of sdb_lsm_get): an SST without blocks, two
    runs of three, one cut inside a key's versions, merge operands."""
    tree, straddler = G.main_tree()
    m = dict(tree=tree, dev=device_tree(rt, tree))
    assert m["dev"]["_policies"] is None and sum(l.bloom is not None for l in tree.leaves) >= 6
    keys = G.main_queries(tree, straddler)[::2] + [straddler]
    cases = plain_cases(L.ranges(tree, straddler)[:80])
    for seed in P.SWEEP_SEEDS[:2]:
        vis = P.random_projections(tree, seed)
        got, _ = get_and_check(rt, m, vis, keys)
        assert sum(g.ssts_filtered for g in got) >= 50
        pm = dict(tree=P.projected(tree, vis), dev=m["dev"])
        scan_and_check(rt, pm, vis, cases)
        res = rt.lsm_get_projected_device(m["dev"], None, vis, keys, merge=True, fill=TM.SENTINEL)
        TM.check_get(P.merge_view(pm["tree"], vis), keys, None, host(res))


# ------------------------------------------------------------------------------------------------
# Where a visible bound falls
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("side", ["start", "end"])
def test_visible_bound_positions(rt, side, desc):
    m = fixture(rt, "edge_tree", P.edge_tree)
    tree = m["tree"]
    vis = P.edge_projections(tree, side)
    cases = plain_cases(P.edge_ranges(tree))
    seqs = P.long_seqs(tree)
    for bounds in (None, [seqs[(7 * q) % len(seqs)] - (q % 2) for q in range(len(cases))]):  # inside LONG's versions
        exp, h = scan_and_check(rt, m, vis, cases, bounds, desc)
        assert sum(e.candidates for e in exp) >= 1000
    keys = L.all_keys(tree) + [P.LONG + b"\x00", b"a", b"z"] + [k for l in (tree.leaves[0], tree.leaves[6]) for k in P.edge_keys(l)]
    get_and_check(rt, m, vis, keys)
    get_and_check(rt, m, vis, [P.LONG] * len(seqs), seqs)


# ------------------------------------------------------------------------------------------------
# Degenerate visible ranges and the filter query (P4)
# ------------------------------------------------------------------------------------------------
def test_degenerate_visible_ranges(rt):
    m = fixture(rt, "point_tree", P.point_tree)
    tree, present, absent = m["made"]
    wide = F.prefix_range(F.tenant(1))
    cases = [(wide, None, -1), (wide, F.tenant(1), F.LENGTHS_LEN), (ALL, None, -1), ((present, INC, present, INC), None, F.LENGTHS_LEN),
             ((absent, INC, absent, INC), F.tenant(1), F.LENGTHS_LEN), ((F.key(1, 10), INC, F.key(1, 90), EXC), F.tenant(1), F.LENGTHS_LEN)]
    keys = [present, absent, F.key(0, 5), F.key(2, 99), b"", b"zz"] + L.all_keys(tree)[::7]
    point = lambda k: [(k, INC, k, INC)] * 3  # noqa: E731
    for desc in (False, True):
        exp, h = scan_and_check(rt, m, point(absent), cases, None, desc)  # exactly one absent key: a point view
        assert exp[0].filtered == [0] and exp[1].filtered == [0] and exp[0].ssts == [1, 2]  # LENGTHS: None, it takes part
        assert h["sum_num_entries"] == 0 and list(h["range_filtered"][:2]) == [1, 1]
        exp, h = scan_and_check(rt, m, point(present), cases, None, desc)  # exactly one present key
        assert [r[0] for r in exp[0].rows] == [present] and exp[0].candidates == 3 and exp[4].ssts == []
        beyond = [(b"zz", INC, None, U), (None, U, b"a", INC), (b"t01:", INC, b"t01:", EXC)]  # disjoint from the SSTs; empty
        exp, h = scan_and_check(rt, m, beyond, cases, None, desc)
        assert h["sum_blocks_checked"] == 0 and not h["range_ssts"][:len(cases)].any() and h["sum_num_filtered"] == 0
        scan_and_check(rt, m, [P.OPEN, None, (b"", INC, None, U)], cases, None, desc)
    for vis in (point(absent), point(present), beyond, [P.OPEN] * 3):
        got, h = get_and_check(rt, m, vis, keys)
    assert [g.state for g in get_and_check(rt, m, beyond, keys)[0]] == [_abi.GET_NOT_FOUND] * len(keys)
    assert get_and_check(rt, m, beyond, keys)[1]["sum_blocks_checked"] == 0


# ------------------------------------------------------------------------------------------------
# Get shapes
# ------------------------------------------------------------------------------------------------
def test_run_cut_inside_a_key(rt):
    m = fixture(rt, "straddle_run", P.straddle_run)
    tree, vis, k = m["made"]
    seqs = G.key_seqs(tree, k)
    keys = [k] * (2 * len(seqs) + 2) + [b"", b"t00", k + b"\x00", k[:-1]] + L.all_keys(tree)[::5]
    bounds = [b for s in seqs for b in (s, s - 1)] + [G.U64_MAX, 0] + [G.U64_MAX] * (len(keys) - 2 * len(seqs) - 2)
    got, h = get_and_check(rt, m, vis, keys, bounds)
    assert {g.sst for g in got[:2 * len(seqs) + 2]} == {1, _abi.NO_SST} and got[2 * len(seqs)].ssts_read == 1
    assert (h["sst"][:2] == 1).all()  # bounds at the hidden, newer versions: the right SST answers
    rngs = [(k, INC, k, INC), ALL, (None, U, k, INC), (k, INC, None, U), (None, U, k, EXC), (k, EXC, None, U)]
    for desc in (False, True):
        scan_and_check(rt, m, vis, plain_cases(rngs), None, desc)
        scan_and_check(rt, m, vis, plain_cases([rngs[0]] * len(seqs) + rngs), seqs + [min(seqs) - 1] * len(rngs), desc)


def test_key_gap_run(rt):
    g = P.golden()["key_gap"]
    for c in g["cases"]:
        tree, vis = P.key_gap_run(c)
        m = dict(tree=tree, dev=device_tree(rt, tree))
        keys = [b"a", b"b", b"c", b"d", b"e", b"f", b"g", b"m", b"n", b"p", b"q", b""]
        got, h = get_and_check(rt, m, vis, keys)
        exp, hs = scan_and_check(rt, m, vis, plain_cases([ALL, (b"a", INC, b"z", INC), (b"e", INC, b"g", EXC), (b"c", INC, b"m", INC)]))
        assert len(exp[0].ssts) == c["ssts_kept"]
        if not c["ssts_kept"]:
            assert h["sum_num_not_found"] == len(keys) and not h["ssts_read"][:len(keys)].any() and hs["sum_blocks_checked"] == 0
        else:
            assert [r[0] for r in exp[0].rows] == [b"b", b"c"]


def link_values(tree, h, item):
    """(sst, seq, flags, value bytes) of the links of query / row `item`, from the device's columns."""
    a, b = int(h["chain_start"][item]), int(h["chain_start"][item + 1])
    out = []
    for d in range(a, b):
        i, vo, vl = int(h["chain_sst"][d]), int(h["chain_val_off"][d]), int(h["chain_val_len"][d])
        out.append((i, int(h["chain_seq"][d]), int(h["chain_flags"][d]), tree.leaves[i].sst.data[vo:vo + vl].tobytes()))
    return out


def test_hidden_newer_versions(rt):
    """Two L0 SSTs with disjoint views: what the newer one holds outside its view shadows nothing and links nothing."""
    m = fixture(rt, "hidden_l0", P.hidden_l0)
    tree, vis = m["made"]
    keys = [P.K1, P.K2, b"x010", b"x025", b"x040", b"x055", b"x000"]
    got, h = get_and_check(rt, m, vis, keys)
    assert (got[0].state, got[0].sst, got[0].ssts_read) == (_abi.GET_FOUND, 1, 1) and P.row_value(tree, 1, got[0].row)[3] == b"old"
    assert got[1].status == _abi.SDB_MERGE_OPERATOR_MISSING and got[1].sst == 1
    free = host(rt.lsm_get_filtered_device(m["dev"], None, keys))
    assert int(free["sst"][0]) == 0 and int(free["sst"][1]) == 0  # unprojected, the newer SST answers both
    rngs = [(None, U, P.K2, EXC), (P.K1, INC, P.K1, INC), ALL, (b"x020", INC, b"x045", INC), (P.K2, INC, None, U)]
    for desc in (False, True):
        exp, _ = scan_and_check(rt, m, vis, plain_cases(rngs), None, desc)
        assert (P.K1, 1) in [(r[0], r[1]) for r in exp[0].rows] and exp[2].status == _abi.SDB_MERGE_OPERATOR_MISSING
    # the merging get: every column and link against merge_read_cases.get_merge over leaves that cover what E holds
    view = P.merge_view(tree, vis)
    res = rt.lsm_get_projected_device(m["dev"], None, vis, keys, merge=True, fill=TM.SENTINEL)
    mg = TM.check_get(view, keys, None, host(res))
    assert [i for i, _, _ in mg[1].links] == [1, 1, 1] and mg[1].base and mg[1].ssts_read == 1 and mg[0].ssts_read == 1
    # the merging scan: rows and links against merge_read_cases.scan_merge over the trimmed SSTs
    cut = P.trimmed(tree, vis)
    for desc in (False, True):
        hs = host(rt.lsm_scan_projected_device(m["dev"], vis, rngs, merge=True, descending=desc))
        exp = [M.scan_merge(cut, r, None, desc) for r in rngs]
        rows = [r for e in exp for r in e.rows]
        assert hs["sum_status"] == 0 and hs["csum_status"] == 0 and hs["sum_num_entries"] == len(rows)
        assert hs["sum_num_candidates"] == sum(e.candidates for e in exp)
        assert list(hs["range_ssts"][:len(rngs)]) == [len(e.ssts) for e in exp]
        assert hs["csum_num_links"] == sum(len(r[1]) for r in rows) and hs["csum_max_chain_len"] == 3
        for x, (key, links, base, _, _) in enumerate(rows):
            assert hs["key_arena"][int(hs["key_off"][x]):int(hs["key_off"][x + 1])].tobytes() == key
            want = [(i,) + P.row_value(cut, i, r)[1:] for i, r, _ in links]
            assert link_values(tree, hs, x) == want, key
        k2 = next(r for r in exp[2].rows if r[0] == P.K2)
        assert [i for i, _, _ in k2[1]] == [1, 1, 1]  # the hidden SST's operand is no link


# ------------------------------------------------------------------------------------------------
# Errors behind a projection
# ------------------------------------------------------------------------------------------------
def null_arrays(rt, dev, i):
    """The device tree with SST i's index_keys pointer NULL."""
    import torch
    ssts = dev["_ssts"].clone()
    words = ssts.view(torch.int64)
    words[(i * C.sizeof(_abi.SstView) + _abi.SstView.index_keys.offset) // 8] = 0
    return TG.with_arrays(rt, dev, ssts=ssts)


def error_tree(rt, tree, bad_block):
    """SST 0 with a corrupt block, SST 1 with a version that does not exist, SST 2 with a NULL array."""
    l0 = tree.leaves[0]
    data = l0.sst.data.copy()
    data[int(l0.sst.block_off[bad_block]) + 5] ^= 0x40
    views = [view_of(l) for l in tree.leaves]
    views[0] = view_of(l0, data=data)
    views[1]["sst_version"] = 3
    return null_arrays(rt, device_tree(rt, tree, views), 2)


def test_errors_no_view_reaches_never_surface(rt):
    tree, present, absent = P.point_tree()
    l0 = tree.leaves[0]
    t2 = F.prefix_range(F.tenant(2))
    bs, be = partitions_covering_range(l0.sst.index_keys, *t2)
    assert be - bs >= 3
    bad = bs + 1  # a block of tenant 2 inside SST 0
    lo, hi = l0.sst.keys[l0.sst.bes[bad] - 1], l0.sst.keys[l0.sst.bes[bad + 1]]
    assert partitions_covering_range(l0.sst.index_keys, None, U, lo, INC)[1] <= bad
    dev = error_tree(rt, tree, bad)
    m = dict(tree=tree, dev=dev)
    # SST 0 is seen up to the key before the broken block; the views of SSTs 1 and 2 hold no key of theirs
    vis = [(None, U, lo, INC), (b"zz", INC, None, U), (None, U, b"a", EXC)]
    cases = [(F.prefix_range(F.tenant(t)), F.tenant(t), F.LENGTHS_LEN) for t in range(3)] + plain_cases([ALL, (lo, INC, hi, INC), (present, INC, present, INC)])
    for desc in (False, True):
        exp, h = scan_and_check(rt, m, vis, cases, None, desc)
        assert not h["range_status"][:len(cases)].any() and h["sum_num_entries"] >= 40
    keys = L.all_keys(tree)[::2] + [hi, lo, present, absent]
    got, h = get_and_check(rt, m, vis, keys)
    assert h["sum_num_failed"] == 0 and h["sum_num_found"] >= 20
    # the same faults where a view partly covers them fail what reaches them, as today
    broken = FR.broken_tree(FR.broken_tree(tree, 0, {bad: _abi.SDB_CHECKSUM_MISMATCH}), 1, version=3)
    mid = l0.sst.keys[l0.sst.bes[bad] + 1]
    vis = [(None, U, mid, INC), (F.key(1, 0), INC, None, U), (None, U, b"a", EXC)]
    mb = dict(tree=broken, dev=dev)
    exp, h = scan_and_check(rt, mb, vis, cases)
    assert [e.status for e in exp[:4]] == [0, _abi.SDB_INVALID_VERSION, _abi.SDB_CHECKSUM_MISMATCH, _abi.SDB_CHECKSUM_MISMATCH]
    got, h = get_and_check(rt, mb, vis, keys)
    assert {g.status for g in got} == {0, _abi.SDB_INVALID_VERSION, _abi.SDB_CHECKSUM_MISMATCH}
    # a NULL array that a view reaches: SDB_INVALID_ARGUMENT at that SST's place
    h = host(call(rt, dev, [(None, U, b"a", EXC), (b"zz", INC, None, U), None], plain_cases([ALL, (b"a", INC, b"b", INC)])))
    assert list(h["range_status"][:2]) == [BAD, 0] and list(h["range_ssts"][:2]) == [1, 0]


# ------------------------------------------------------------------------------------------------
# P5: malformed projections
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["start_excluded", "start_kind", "end_kind", "start_off", "end_off"])
def test_malformed_projection(rt, what):
    import torch
    m = fixture(rt, "main_tree")
    tree, dev = m["tree"], m["dev"]
    vis = P.random_projections(tree, P.SWEEP_SEEDS[1])
    good = {k: to_dev(a) for k, a in rt.projections_columnar(vis).items()}
    good["n"] = len(vis)
    assert int(good["start_kind"][3]) == INC and int(good["start_off"][4]) > 0 and int(good["end_off"][4]) > 0
    bad = {k: (v.clone() if hasattr(v, "clone") else v) for k, v in good.items()}
    if what == "start_excluded":
        bad["start_kind"][3] = EXC
    elif what == "start_kind":
        bad["start_kind"][3] = 3
    elif what == "end_kind":
        bad["end_kind"][3] = 3
    else:
        bad[what][3] = int(bad[what][4]) + 1  # descends behind SST 3
    cases = sweep_cases(tree)[:70]
    n = len(cases)
    exp = model(tree, vis, cases)
    cand = totals(exp)[0]
    ws = torch.empty(rt.read_workspace_bytes("sdb_lsm_scan_projected", dev, n, cand), dtype=torch.uint8, device="cuda")
    kw = dict(workspace=ws, cand=cand, cap=cand)
    r1 = call(rt, dev, bad, cases, **kw)  # back to back on one workspace, no reset between them
    r2 = call(rt, dev, good, cases, **kw)
    h = host(r1)
    assert (h["range_status"][:n] == BAD).all() and h["sum_blocks_checked"] == 0 and h["sum_num_failed_ranges"] == n
    assert h["sum_num_entries"] == 0 and h["sum_num_candidates"] == 0 and h["sum_num_filtered"] == 0 and h["sum_status"] == BAD
    assert not h["range_ssts"][:n].any() and not h["range_entry_start"][:n + 1].any()
    FR.check(tree, cases, None, False, host(r2), exp)
    keys = F.get_keys(tree)[::9]
    wsg = torch.empty(rt.read_workspace_bytes("sdb_lsm_get_projected", dev, len(keys)), dtype=torch.uint8, device="cuda")
    g1 = rt.lsm_get_projected_device(dev, None, bad, keys, workspace=wsg)
    g2 = rt.lsm_get_projected_device(dev, None, good, keys, workspace=wsg)
    h = host(g1)
    assert (h["status"][:len(keys)] == BAD).all() and not h["state"][:len(keys)].any() and h["sum_blocks_checked"] == 0
    assert h["sum_num_failed"] == len(keys) and not h["ssts_read"][:len(keys)].any()
    TG.check(P.projected(tree, vis), keys, None, host(g2))


# ------------------------------------------------------------------------------------------------
# P6: NULL and open projections are the filtered calls
# ------------------------------------------------------------------------------------------------
def same_tensors(h, g):
    import torch
    torch.cuda.synchronize()
    for k in g:
        if not k.startswith("_"):
            assert h[k].shape == g[k].shape and bool((h[k] == g[k]).all()), k


@pytest.mark.parametrize("name", ["main_tree", "merge_tree"])
def test_null_and_open_projections_equal_the_filtered_calls(rt, name):
    m = fixture(rt, name)
    tree, dev = m["tree"], m["dev"]
    cases = F.scan_cases(tree)
    rngs, px, pl = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    keys = F.get_keys(tree)[::3]
    opened = [[None] * len(tree.leaves), [P.OPEN] * len(tree.leaves)]
    for merge in (False, True):
        for desc in (False, True):
            g = rt.lsm_scan_filtered_device(dev, rngs, px, pl, descending=desc, merge=merge, fill=0x5A)
            cand = (int(g["summary"][2]), int(g["summary"][3]))
            kw = dict(descending=desc, merge=merge, fill=0x5A, cand=cand, cap=cand, cap_links=cand[0])
            g = rt.lsm_scan_filtered_device(dev, rngs, px, pl, **kw)
            for vis in [None] + opened:
                same_tensors(rt.lsm_scan_projected_device(dev, vis, rngs, px, pl, **kw), g)
        g = rt.lsm_get_filtered_device(dev, None, keys, [F.LENGTHS_LEN] * len(keys), merge=merge, fill=0x5A)
        cl = int(g["chain_summary"][0]) if merge else None
        g = rt.lsm_get_filtered_device(dev, None, keys, [F.LENGTHS_LEN] * len(keys), merge=merge, fill=0x5A, cap_links=cl)
        for vis in [None] + opened:
            same_tensors(rt.lsm_get_projected_device(dev, None, vis, keys, [F.LENGTHS_LEN] * len(keys), merge=merge, fill=0x5A,
                                                     cap_links=cl), g)


# ------------------------------------------------------------------------------------------------
# Capacity and canaries
# ------------------------------------------------------------------------------------------------
def test_scan_capacity_and_canaries(rt):
    m = fixture(rt, "main_tree")
    tree = m["tree"]
    cases = sweep_cases(tree)
    vis = P.random_projections(tree, P.SWEEP_SEEDS[1])
    exp = model(tree, vis, cases)
    cand, cap = totals(exp)
    free = totals([F.scan(tree, r, p, pl) for r, p, pl in cases])[0]
    assert cand[0] < free[0] - 100  # the candidates fit only because of the projections
    guard = Guard()  # the workspace, of exactly the advertised size, and every output array come from it
    res = call(rt, m["dev"], vis, cases, cand=cand, cap=cap, alloc=guard)
    guard.check()
    FR.check(tree, cases, None, False, host(res), exp)
    guard = Guard()
    res = call(rt, m["dev"], vis, cases, cand=(cand[0] - 1, cand[1]), cap=cap, alloc=guard)
    guard.check()
    h = host(res)
    assert h["sum_status"] == _abi.SDB_LIMIT_EXCEEDED and h["sum_num_entries"] == 0
    assert (h["sum_num_candidates"], h["sum_candidate_key_bytes"]) == cand  # the model's totals
    LS.check_ranges(exp, h)
    assert (h["range_filtered"][:len(exp)] == np.array([len(e.filtered) for e in exp])).all()
    h = host(call(rt, m["dev"], [None] * len(vis), cases, cand=cand, cap=cap, alloc=Guard()))  # unprojected they do not fit
    assert h["sum_status"] == _abi.SDB_LIMIT_EXCEEDED and (h["sum_num_candidates"], h["sum_candidate_key_bytes"]) == free


def test_get_canaries(rt):
    m = fixture(rt, "main_tree")
    tree, dev = m["tree"], m["dev"]
    keys = F.get_keys(tree)[::3]
    vis = P.random_projections(tree, P.SWEEP_SEEDS[2])
    guard = Guard()
    first = rt.lsm_get_projected_device(dev, None, vis, keys, alloc=guard)
    # twice in one workspace and the same arrays, no reset
    res = rt.lsm_get_projected_device(dev, None, vis, keys, workspace=first["_ws"], alloc=lambda name, *_: first[name])
    guard.check()
    TG.check(P.projected(tree, vis), keys, None, host(res))
