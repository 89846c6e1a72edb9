"""GPU parity of the filtered tree reads (sdb_lsm_scan_filtered, sdb_lsm_get_filtered) against the model of
tests/filtered_read_cases.py, every column and counter: prefix scans over a tree of mixed filter policies (both
orders, snapshot bounds, point ranges, prefixes shorter and longer than the extractor's, LENGTHS answers), a tree
of one policy (the per-range hash), no false negatives against sdb_lsm_scan, NULL policies and prefixes against the
unfiltered calls, errors behind the filter, capacities, the merge variants, the gets a tree without whole-key hashes
needs, workspace reuse and canaries after the workspace and every output array."""
import numpy as np
import pytest

from slatedb_amd import _abi

from . import filtered_read_cases as F
from . import get_cases as G
from . import lsm_scan_cases as L
from . import test_gpu_get as TG
from . import test_gpu_lsm_scan as LS
from .read_harness import Filled, Guard, device_tree, host, rt, to_dev, totals, view_of  # noqa: F401
from .scan_cases import INC, partitions_covering_range

pytestmark = pytest.mark.gpu

U64_MAX = G.U64_MAX


_trees = {}


def fixture(rt, name):
    """A tree of filtered_read_cases, its device form and its unfiltered device form, built once."""
    if name not in _trees:
        tree = getattr(F, name)()
        _trees[name] = dict(tree=tree, dev=device_tree(rt, tree), plain=device_tree(rt, tree, plain=True))
    return _trees[name]


def model(tree, cases, bounds, desc, probe="given"):
    return [F.scan(tree, r, p, pl if probe == "given" else None, None if bounds is None else bounds[q], desc)
            for q, (r, p, pl) in enumerate(cases)]


def call(rt, dev, cases, bounds=None, desc=False, probe="given", **kw):
    pl = [c[2] for c in cases] if probe == "given" else ([-1] * len(cases) if probe == "minus" else None)
    return rt.lsm_scan_filtered_device(dev, [c[0] for c in cases], [c[1] for c in cases], pl, max_seq=bounds,
                                       descending=desc, **kw)


def check(tree, cases, bounds, desc, h, exp):
    """Every column of every row and the summary (test_gpu_lsm_scan.check), range_filtered and num_filtered."""
    LS.check(tree, [c[0] for c in cases], bounds, desc, h, exp)
    want = np.array([len(e.filtered) for e in exp], np.int64)
    assert (h["range_filtered"][:len(exp)].astype(np.int64) == want).all(), np.nonzero(h["range_filtered"][:len(exp)] != want)
    assert h["sum_num_filtered"] == int(want.sum())


def same_rows(h, g, n):
    """The rows of two scans agree: counts, keys and every column."""
    assert (h["range_entry_start"][:n + 1] == g["range_entry_start"][:n + 1]).all()
    assert (h["range_status"][:n] == g["range_status"][:n]).all()
    ne, kb = h["sum_num_entries"], h["sum_key_bytes"]
    assert (ne, kb) == (g["sum_num_entries"], g["sum_key_bytes"])
    assert (h["key_off"][:ne + 1] == g["key_off"][:ne + 1]).all() and (h["key_arena"][:kb] == g["key_arena"][:kb]).all()
    for f in ("sst", "val_off", "val_len", "seq", "flags", "create_ts", "expire_ts"):
        assert (h[f][:ne] == g[f][:ne]).all(), f


def seq_bounds(tree, n, seed=1):
    rng = np.random.default_rng(seed)
    seqs = sorted({r[3] for l in tree.leaves for r in l.sst.rows})
    pick = lambda: (U64_MAX, 0, seqs[int(rng.integers(0, len(seqs)))])[int(rng.choice(3, p=[0.3, 0.1, 0.6]))]  # noqa: E731
    return [pick() for _ in range(n)]


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("bounded", [False, True])
def test_scan_mixed_policies(rt, desc, bounded):
    m = fixture(rt, "main_tree")
    tree, cases = m["tree"], F.scan_cases(m["tree"])
    bounds = seq_bounds(tree, len(cases)) if bounded else None
    exp = model(tree, cases, bounds, desc)
    h = host(call(rt, m["dev"], cases, bounds, desc))
    check(tree, cases, bounds, desc, h, exp)
    assert h["sum_num_filtered"] >= 40 and sum(len(e.rows) for e in exp) >= 300
    # no false negatives: every range honours F4, so the rows are those of sdb_lsm_scan over the same tree
    g = host(rt.lsm_scan_device(m["plain"], [c[0] for c in cases], max_seq=bounds, descending=desc))
    same_rows(h, g, len(cases))
    # (a ruled-out SST holds no key of such a range, so the candidates agree too; the blocks do not: the unfiltered
    # scan checks the covering blocks of every SST whose interval meets a tenant)
    assert h["sum_num_candidates"] == g["sum_num_candidates"]
    some = [cases[t] for t in (2, 5, 6)]  # tenants no L0 SST holds, inside every L0 SST's interval
    hb = host(call(rt, m["dev"], some, None, desc))["sum_blocks_checked"]
    gb = host(rt.lsm_scan_device(m["plain"], [c[0] for c in some], descending=desc))["sum_blocks_checked"]
    assert hb == len(set().union(*[e.blocks for e in model(tree, some, None, desc)])) and 0 < hb < gb


@pytest.mark.parametrize("probe", ["minus", "none"])
def test_scan_lengths_without_an_answer(rt, probe):
    """probe_len all -1, and a NULL array: the LENGTHS SST has nothing to probe for a prefix and is never ruled out
    for one; a point range still probes its full key there."""
    m = fixture(rt, "main_tree")
    tree, cases = m["tree"], F.scan_cases(m["tree"])
    exp = model(tree, cases, None, False, probe)
    h = host(call(rt, m["dev"], cases, probe=probe))
    check(tree, cases, None, False, h, exp)
    given = model(tree, cases, None, False)
    assert sum(2 in e.filtered for e in given) > sum(2 in e.filtered for e in exp) > 0
    assert all(F.is_point(c[0]) for c, e in zip(cases, exp) if 2 in e.filtered)


@pytest.mark.parametrize("desc", [False, True])
def test_scan_one_policy(rt, desc):
    """Every SST under FIXED(4) without whole keys: the policies agree, so the probe is hashed once per range."""
    m = fixture(rt, "uniform_tree")
    tree = m["tree"]
    keys = L.all_keys(tree)
    cases = [(F.prefix_range(F.tenant(t)), F.tenant(t), -1) for t in range(F.TENANTS)]
    cases += [(F.prefix_range(b"t0"), b"t0", -1), (F.prefix_range(b"t03:00"), b"t03:00", -1), ((None, 0, None, 0), None, -1)]
    for k in [keys[3], keys[len(keys) // 2], b"t0", b"t03", F.key(5, 100), F.key(6, 101)]:  # points: the extracted prefix,
        cases += [((k, INC, k, INC), k[:4], -1), ((k, INC, k, INC), None, -1)]             # or nothing for a short key
    exp = model(tree, cases, None, desc)
    h = host(call(rt, m["dev"], cases, None, desc))
    check(tree, cases, None, desc, h, exp)
    assert h["sum_num_filtered"] >= 8 and exp[-3].rows == [] and exp[-3].filtered  # an absent tenant's point is pruned
    short = [e for c, e in zip(cases, exp) if c[0][0] in (b"t0", b"t03") and F.is_point(c[0])]
    assert len(short) == 4 and all(len(e.rows) == 1 and not e.filtered for e in short)
    same_rows(h, host(rt.lsm_scan_device(m["plain"], [c[0] for c in cases], descending=desc)), len(cases))


def test_null_policies_and_prefixes_equal_the_unfiltered_calls(rt):
    p = LS.plain(rt)
    rngs = p["ranges"][:200]
    for desc in (False, True):
        h = host(rt.lsm_scan_filtered_device(p["dev"], rngs, descending=desc))
        g = host(rt.lsm_scan_device(p["dev"], rngs, descending=desc))
        for k in g:
            assert (np.asarray(h[k]) == np.asarray(g[k])).all(), k
        assert h["sum_num_filtered"] == 0 and not h["range_filtered"].any()
    h = rt.lsm_scan_filtered_device(p["dev"], rngs, merge=True)
    g = rt.lsm_scan_merge_device(p["dev"], rngs)
    import torch
    torch.cuda.synchronize()
    for k in g:
        if not k.startswith("_"):
            assert bool((h[k] == g[k]).all()), k
    m = TG.main(rt)  # filters on most SSTs: the plain policy probes the full key, as sdb_lsm_get does
    keys, bounds = G.bounded_queries(m["tree"], m["queries"], m["straddler"])
    for b in (None, bounds):
        h = host(rt.lsm_get_filtered_device(m["dev"], None, keys, max_seq=b))
        g = host(rt.lsm_get_device(m["dev"], None, keys, max_seq=b))
        for k in g:
            assert (np.asarray(h[k]) == np.asarray(g[k])).all(), k
        assert h["ssts_filtered"].sum() > 100


def broken_tree(tree, i, block_status=None, version=None):
    l = tree.leaves[i]
    leaves = list(tree.leaves)
    leaves[i] = F.Leaf(l.sst, l.policy, l.bloom, l.num_probes, block_status, version)
    it = iter(leaves)
    return F.Tree([[next(it) for _ in r] for r in tree.runs])


@pytest.mark.parametrize("how", ["crc", "version"])
def test_errors_behind_the_filter(rt, how):
    """SST 0 holds tenant 0 and is ruled out for tenant 1: a corrupt block, or a version that does not exist, fails
    tenant 0's range and is never seen by tenant 1's."""
    m = fixture(rt, "main_tree")
    tree = m["tree"]
    pairs = {(t, i): out for t, i, out, _ in F.prefix_pairs(tree)}
    assert pairs[(1, 0)] and not pairs[(0, 0)]
    leaf = tree.leaves[0]
    rng_b = F.prefix_range(F.tenant(0))
    bs, be = partitions_covering_range(leaf.sst.index_keys, rng_b[0], rng_b[1], rng_b[2], rng_b[3])
    bad = (bs + be) // 2
    views = [view_of(l) for l in tree.leaves]
    if how == "crc":
        status = _abi.SDB_CHECKSUM_MISMATCH
        data = leaf.sst.data.copy()
        data[int(leaf.sst.block_off[bad]) + 5] ^= 0x40
        views[0] = view_of(leaf, data=data)
        broken = broken_tree(tree, 0, {bad: status})
    else:
        status = _abi.SDB_INVALID_VERSION
        views[0]["sst_version"] = 3
        broken = broken_tree(tree, 0, version=3)
    cases = [(F.prefix_range(F.tenant(t)), F.tenant(t), F.LENGTHS_LEN) for t in range(F.TENANTS)] + [((None, 0, None, 0), None, -1)]
    exp = model(broken, cases, None, False)
    h = host(call(rt, device_tree(rt, broken, views), cases))
    check(broken, cases, None, False, h, exp)
    clean = model(tree, cases, None, False)
    assert exp[0].status == status and not exp[0].rows and exp[-1].status == status
    assert exp[1].status == 0 and exp[1].rows == clean[1].rows and len(exp[1].rows) > 10 and 0 in exp[1].filtered
    failing = [q for q, e in enumerate(exp) if e.status]
    reach = [q for q, e in enumerate(exp) if (bad in e.blocks if how == "crc" else 0 in e.ssts)]  # SST 0's blocks come first
    assert failing == reach and 2 <= len(failing) < len(cases)


def test_scan_capacity(rt):
    m = fixture(rt, "main_tree")
    tree = m["tree"]
    # the last range breaks F4 (keys of every tenant under tenant 1's prefix): the SSTs ruled out for it hold
    # candidates, which the call neither stages nor counts, and the rows of the range come without theirs
    cases = F.scan_cases(tree) + [((None, 0, None, 0), F.tenant(1), F.LENGTHS_LEN)]
    exp = model(tree, cases, None, False)
    cand, cap = totals(exp)
    free = L.scan(tree, cases[-1][0])
    assert 0 < exp[-1].candidates < free.candidates - 100 and 0 < len(exp[-1].rows) < len(free.rows)
    h = host(call(rt, m["dev"], cases, cand=(cand[0] - 1, cand[1]), cap=cap, alloc=Filled(0xA5)))
    assert h["sum_status"] == _abi.SDB_LIMIT_EXCEEDED and h["sum_num_entries"] == 0
    assert (h["sum_num_candidates"], h["sum_candidate_key_bytes"]) == cand
    LS.check_ranges(exp, h)  # range_status, range_ssts and blocks_checked stay valid, and so do the filter's counts
    assert (h["range_filtered"][:len(exp)] == np.array([len(e.filtered) for e in exp])).all()
    assert h["sum_num_filtered"] == sum(len(e.filtered) for e in exp) > 0
    check(tree, cases, None, False, host(call(rt, m["dev"], cases, cand=cand, cap=cap, alloc=Filled(0xA5))), exp)


def test_scan_canaries(rt):
    """A workspace of exactly the advertised size and every output array of exactly its size, 0xA5 around each."""
    m = fixture(rt, "main_tree")
    tree, cases = m["tree"], F.scan_cases(m["tree"])
    exp = model(tree, cases, None, False)
    cand, cap = totals(exp)
    guard = Guard()
    res = call(rt, m["dev"], cases, cand=cand, cap=cap, alloc=guard)
    guard.check()
    check(tree, cases, None, False, host(res), exp)


def test_scan_workspace_reuse(rt):
    import torch
    m = fixture(rt, "main_tree")
    tree, cases = m["tree"], F.scan_cases(m["tree"])
    other = cases[::-1][:30]
    bounds = seq_bounds(tree, len(other), 2)
    exp, exp2 = model(tree, cases, None, False), model(tree, other, bounds, True)
    cand = totals(exp)[0]
    dev = m["dev"]
    ws = torch.empty(rt.read_workspace_bytes("sdb_lsm_scan_filtered", dev, len(cases), cand), dtype=torch.uint8, device="cuda")
    kw = dict(workspace=ws, cand=cand, cap=cand)
    r1 = call(rt, dev, cases, **kw)  # back to back on one workspace, no reset and no synchronisation between them
    r2 = call(rt, dev, other, bounds, True, **kw)
    r3 = call(rt, dev, cases, **kw)
    assert r1["_ws"] is ws and r2["_ws"] is ws and r3["_ws"] is ws
    check(tree, cases, None, False, host(r1), exp)
    check(tree, other, bounds, True, host(r2), exp2)
    check(tree, cases, None, False, host(r3), exp)


def test_scan_bad_policy_kind_and_prefix_offsets(rt):
    m = fixture(rt, "main_tree")
    tree = m["tree"]
    views = [view_of(l) for l in tree.leaves]
    views[0]["policy"] = (4, 4, 0)  # no such extractor: SST 0 fails what reaches it, its filter rules nothing out
    dev = device_tree(rt, tree, views)
    cases = [(F.prefix_range(F.tenant(t)), F.tenant(t), F.LENGTHS_LEN) for t in range(F.TENANTS)]
    h = host(call(rt, dev, cases))
    free = [L.scan(tree, c[0]) for c in cases]
    assert (h["range_status"][:8] == _abi.SDB_INVALID_ARGUMENT).all() and all(0 in e.ssts for e in free)
    exp = model(tree, cases, None, False)
    assert (h["range_filtered"][:8] == np.array([len([i for i in e.filtered if i != 0]) for e in exp])).all()
    keys = [F.key(0, 1), F.key(1, 1), b"t99:"]
    g = host(rt.lsm_get_filtered_device(dev, None, keys))
    assert list(g["status"][:3]) == [_abi.SDB_INVALID_ARGUMENT, _abi.SDB_INVALID_ARGUMENT, 0]  # t99: is outside SST 0
    # prefix offsets that descend: the call is malformed, every range fails
    px = {k: to_dev(a) for k, a in rt.scan_prefixes_columnar([c[1] for c in cases], [c[2] for c in cases]).items()}
    px["prefix_off"][3] = 100
    h = host(rt.lsm_scan_filtered_device(m["dev"], [c[0] for c in cases], px))
    assert (h["range_status"][:8] == _abi.SDB_INVALID_ARGUMENT).all() and h["sum_blocks_checked"] == 0
    assert h["sum_num_filtered"] == 0 and h["sum_num_failed_ranges"] == 8


def test_scan_merge_variant(rt):
    """Operand chains across SSTs under tenant prefixes: rows, links and chain_start are sdb_lsm_scan_merge's."""
    import torch
    m = fixture(rt, "merge_tree")
    tree = m["tree"]
    keys = L.all_keys(tree)
    cases = [(F.prefix_range(F.tenant(t)), F.tenant(t), -1) for t in range(F.TENANTS)]
    cases += [((F.key(t, 20), INC, F.key(t, 70), INC), F.tenant(t), -1) for t in (0, 4, 7)]
    cases += [((k, INC, k, INC), k[:4], -1) for k in keys[::25]] + [((None, 0, None, 0), None, -1)]
    rngs = [c[0] for c in cases]
    for desc in (False, True):
        h = call(rt, m["dev"], cases, None, desc, merge=True)
        g = rt.lsm_scan_merge_device(m["plain"], rngs, descending=desc)
        torch.cuda.synchronize()
        ne, nl = int(g["summary"][0]), int(g["chain_summary"][0])
        assert ne > 100 and nl > ne and int(h["summary"][0]) == ne and int(h["chain_summary"][0]) == nl
        assert int(h["num_filtered"][0]) >= 15 and int(h["summary"][5]) <= int(g["summary"][5])
        assert bool((h["range_entry_start"] == g["range_entry_start"]).all()) and bool((h["range_status"] == g["range_status"]).all())
        assert bool((h["chain_start"][:ne + 1] == g["chain_start"][:ne + 1]).all())
        assert bool((h["key_arena"][:int(g["summary"][1])] == g["key_arena"][:int(g["summary"][1])]).all())
        for f, _ in rt.LSM_SCAN_COLUMNS:
            assert bool((h[f][:ne] == g[f][:ne]).all()), f
        for f, _ in rt.CHAIN_COLUMNS:
            assert bool((h["chain_" + f][:nl] == g["chain_" + f][:nl]).all()), f
    # without an operator a winning operand fails its range, as in sdb_lsm_scan
    h = host(call(rt, m["dev"], cases))
    exp = model(tree, cases, None, False)
    check(tree, cases, None, False, h, exp)
    assert sum(e.status == _abi.SDB_MERGE_OPERATOR_MISSING for e in exp) >= 8


@pytest.mark.parametrize("name", ["main_tree", "uniform_tree"])
def test_get(rt, name):
    """Present, absent, deleted and bounded queries against the model; every present key is found, which the
    unfiltered get cannot do on the tree without whole-key hashes."""
    m = fixture(rt, name)
    tree = m["tree"]
    keys = F.get_keys(tree)
    pl = [F.LENGTHS_LEN] * len(keys)
    h = host(rt.lsm_get_filtered_device(m["dev"], None, keys, pl))
    got = TG.check(tree, keys, None, h)
    TG.check_blocks_checked(tree, keys, got, h)
    states = [g.state for g in got]
    assert states.count(_abi.GET_FOUND) >= 200 and states.count(_abi.GET_DELETED) >= 20 and states.count(_abi.GET_NOT_FOUND) >= 150
    assert sum(g.ssts_filtered for g in got) >= 300
    for k, g in zip(keys, got):
        rows, _ = L.brute(tree, (k, INC, k, INC))
        assert (g.state == _abi.GET_FOUND) == bool(rows), k
    bounds = seq_bounds(tree, len(keys), 3)
    h = host(rt.lsm_get_filtered_device(m["dev"], None, keys, pl, max_seq=bounds))
    TG.check(tree, keys, bounds, h)
    if name == "uniform_tree":  # the full-key probe of sdb_lsm_get loses present keys here
        u = host(rt.lsm_get_device(m["dev"], None, keys))
        assert int((u["state"][:len(keys)] == _abi.GET_FOUND).sum()) < states.count(_abi.GET_FOUND) // 2


def test_get_merge_variant(rt):
    """The merging get over filters: the links are those of sdb_lsm_get_merge over the same tree without filters."""
    import torch
    m = fixture(rt, "merge_tree")
    keys = F.get_keys(m["tree"])
    h = rt.lsm_get_filtered_device(m["dev"], None, keys, merge=True)
    g = rt.lsm_get_merge_device(m["plain"], None, keys)
    torch.cuda.synchronize()
    nl = int(g["chain_summary"][0])
    assert nl > len(keys) // 2 and int(h["chain_summary"][0]) == nl and int(g["chain_summary"][1]) >= 2
    assert bool((h["chain_start"] == g["chain_start"]).all())
    for f, _ in rt.CHAIN_COLUMNS:
        assert bool((h["chain_" + f][:nl] == g["chain_" + f][:nl]).all()), f
    for f, _ in rt.GET_FIELDS:
        if f not in ("ssts_read", "ssts_filtered"):
            assert bool((h[f] == g[f]).all()), f
    assert int(h["ssts_filtered"].sum()) > 300 and int(g["ssts_filtered"].sum()) == 0
    assert bool((h["ssts_read"] <= g["ssts_read"]).all())


def test_get_merge_under_policies_that_differ(rt):
    """The merging get with a probe per SST (the policies do not agree) and a run cut inside a key: links, offsets
    and columns are those of sdb_lsm_get_merge over the same tree without filters."""
    import torch
    m = fixture(rt, "mixed_merge_tree")
    keys = F.get_keys(m["tree"])
    h = rt.lsm_get_filtered_device(m["dev"], None, keys, probe_len=[F.LENGTHS_LEN] * len(keys), merge=True)
    g = rt.lsm_get_merge_device(m["plain"], None, keys)
    torch.cuda.synchronize()
    nl = int(g["chain_summary"][0])
    assert nl > len(keys) // 2 and int(h["chain_summary"][0]) == nl and int(g["chain_summary"][1]) >= 3
    assert int(h["chain_summary"][2]) == 0 and int(g["chain_summary"][2]) == 0
    assert bool((h["chain_start"] == g["chain_start"]).all())
    for f, _ in rt.CHAIN_COLUMNS:
        assert bool((h["chain_" + f][:nl] == g["chain_" + f][:nl]).all()), f
    for f, _ in rt.GET_FIELDS:
        if f not in ("ssts_read", "ssts_filtered"):
            assert bool((h[f] == g[f]).all()), f
    assert int(h["ssts_filtered"].sum()) > 0 and int(g["ssts_filtered"].sum()) == 0
    assert bool((h["ssts_read"] <= g["ssts_read"]).all())


def test_get_filtered_with_a_chain_degenerate(rt):
    """No keys, and keys over a tree without SSTs: the chain summary, chain_start[0..nkeys] and the get summary are
    zeroed whatever they held, every query is NOT_FOUND with no SST, no link is written."""
    import torch
    m = fixture(rt, "mixed_merge_tree")
    words = {"summary": 0x5A5A, "chain_start": 77, "chain_summary": 77}

    def preset(name, count, dtype, fill):  # what every output holds before the call; the link columns byte by byte
        if fill:
            return torch.full((max(count, 1) * dtype.itemsize,), fill, dtype=torch.uint8, device="cuda").view(dtype)
        return torch.full((max(count, 1),), words.get(name, 0x5A), dtype=dtype, device="cuda")

    for dev, keys in ((m["dev"], []), (rt.lsm_tree_device([], []), [b"a", b"", b"t03:0001"])):
        n = len(keys)
        h = host(rt.lsm_get_filtered_device(dev, None, keys, merge=True, cap_links=4, fill=0x5A, alloc=preset))
        assert not h["chain_summary"].any() and not h["chain_start"][:n + 1].any() and not h["summary"].any()
        assert (h["chain_seq"].view(np.uint8) == 0x5A).all()
        if n:
            assert (h["state"] == _abi.GET_NOT_FOUND).all() and not h["status"].any()
            assert ((h["sst"].astype(np.int64) & 0xFFFFFFFF) == _abi.NO_SST).all()
            for f in ("block", "val_off", "val_len", "seq", "flags", "create_ts", "expire_ts", "ssts_read", "ssts_filtered"):
                assert not h[f].any(), f
        else:
            assert (h["state"] == 0x5A).all()


def test_get_canaries_and_workspace_reuse(rt):
    m = fixture(rt, "main_tree")
    tree, dev = m["tree"], m["dev"]
    keys = F.get_keys(tree)
    n = len(keys)
    guard = Guard()
    kb, ko = (to_dev(a) for a in rt.keys_columnar(keys[::-1]))
    first = rt.lsm_get_filtered_device(dev, None, (kb, ko, n), alloc=guard)
    b, o = rt.keys_columnar(keys)  # again in the same workspace and arrays, no reset: the second call's results stand
    kb.copy_(to_dev(b)[:kb.numel()])
    ko.copy_(to_dev(o))
    res = rt.lsm_get_filtered_device(dev, None, (kb, ko, n), workspace=first["_ws"], alloc=lambda name, *_: first[name])
    guard.check()
    TG.check(tree, keys, None, host(res))


def test_graph_capture(rt):
    """Both calls captured into one HIP graph as a linear sequence, replayed after their outputs were cleared."""
    import torch
    m = fixture(rt, "main_tree")
    tree, dev, cases = m["tree"], m["dev"], F.scan_cases(m["tree"])
    exp = model(tree, cases, None, False)
    cand = totals(exp)[0]
    rg = {k: to_dev(a) for k, a in rt.scan_ranges_columnar([c[0] for c in cases]).items()}
    rg["n"] = len(cases)
    px = {k: to_dev(a) for k, a in rt.scan_prefixes_columnar([c[1] for c in cases], [c[2] for c in cases]).items()}
    keys = F.get_keys(tree)
    kb, ko = (to_dev(a) for a in rt.keys_columnar(keys))
    wss = torch.empty(rt.read_workspace_bytes("sdb_lsm_scan_filtered", dev, len(cases), cand), dtype=torch.uint8, device="cuda")
    wsg = torch.empty(rt.read_workspace_bytes("sdb_lsm_get_filtered", dev, len(keys)), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def both():
        return (rt.lsm_scan_filtered_device(dev, rg, px, stream=s, workspace=wss, cand=cand, cap=cand),
                rt.lsm_get_filtered_device(dev, None, (kb, ko, len(keys)), stream=s, workspace=wsg))

    with torch.cuda.stream(s):  # the first launches (function attributes) outside the capture
        both()
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rs, rg_ = both()
    for _ in range(2):
        for r in (rs, rg_):
            for k, t in r.items():
                if not k.startswith("_"):
                    t.fill_(0x5A if t.dtype == torch.uint8 else 0)
        g.replay()
        torch.cuda.synchronize()
        check(tree, cases, None, False, host(rs), exp)
        TG.check(tree, keys, None, host(rg_))
