"""GPU parity of the batched Db::get (sdb_lsm_get, slatedb_amd/csrc/sdb_get.hip) against the model of
tests/get_cases.py, every column of every query: a mixed tree (L0 + sorted runs, V1 and V2, filters, an SST
without blocks, a key straddling two SSTs of a run), snapshot bounds, the reference's own table, merge
operands, lazy errors, a malformed tree, degenerate inputs, HIP graph capture and workspace reuse."""
import numpy as np
import pytest

from slatedb_amd import _abi

from . import get_cases as G
from .read_harness import check_get_summary, compare, device_tree, host, rt, to_dev, view_of  # noqa: F401

pytestmark = pytest.mark.gpu

U64_MAX = G.U64_MAX
GET_COLS = ("state", "status", "sst", "block", "val_off", "val_len", "seq", "flags", "ssts_read", "ssts_filtered")


def check(tree, keys, bounds, h):
    """Every column of every query, and the summary, against the model.  Returns the model's results."""
    got = [tree.get(k, None if bounds is None else bounds[q]) for q, k in enumerate(keys)]
    compare(GET_COLS, [dict(tree.columns(g), key=k) for g, k in zip(got, keys)], lambda f: h[f], "get")
    check_get_summary(got, [q for q, g in enumerate(got) if g.status and g.state == _abi.GET_NOT_FOUND], h)
    return got


def check_blocks_checked(tree, keys, got, h):
    need = set().union(*[g.need for g in got]) if got else set()
    cover = set().union(*[tree.covering_blocks(k) for k in keys]) if keys else set()
    assert need <= cover
    assert len(need) <= h["sum_blocks_checked"] <= len(cover), (len(need), h["sum_blocks_checked"], len(cover))


_main = {}


def main(rt):
    """The main tree, its device form and its queries, built once."""
    if not _main:
        tree, straddler = G.main_tree()
        _main.update(tree=tree, straddler=straddler, dev=device_tree(rt, tree), queries=G.main_queries(tree, straddler))
    return _main


def test_main_tree_shape(rt):
    m = main(rt)
    tree = m["tree"]
    assert [len(r) for r in tree.runs] == [1, 1, 1, 1, 1, 3, 3]
    assert sorted({l.version for l in tree.leaves}) == [1, 2] and tree.leaves[1].sst.nb == 0
    assert any(l.bloom is None for l in tree.leaves if l.sst.nb) and any(l.bloom is not None for l in tree.leaves)
    a, b = tree.leaves[5], tree.leaves[6]  # the cut of the newer run lies inside the straddling key's versions
    assert a.last_key == b.first_key == m["straddler"]
    assert [i for i in tree.chain(m["straddler"]) if i in (5, 6, 7)] == [5, 6]
    for l in tree.leaves:
        if l.sst.nb:
            assert l.sst.straddling_key(min_versions=2) is not None  # versions straddle blocks in every SST


def test_get_unbounded(rt):
    m = main(rt)
    tree, keys = m["tree"], m["queries"]
    assert 450 <= len(keys) <= 700
    h = host(rt.lsm_get_device(m["dev"], None, keys))
    got = check(tree, keys, None, h)
    check_blocks_checked(tree, keys, got, h)
    states = [g.state for g in got]
    for st in (_abi.GET_FOUND, _abi.GET_DELETED, _abi.GET_NOT_FOUND, _abi.GET_MERGE_OPERAND):
        assert states.count(st) >= 20, st
    oldest = {len(tree.leaves) - 3, len(tree.leaves) - 2, len(tree.leaves) - 1}
    assert sum(1 for g in got if g.sst in oldest) >= 30  # keys present only in the oldest run
    assert len({g.sst for g in got}) >= 10  # every SST with entries decides some query
    assert max(g.ssts_filtered for g in got) >= 4 and max(g.ssts_read for g in got) >= 3


def test_get_max_seq(rt):
    m = main(rt)
    tree, straddler = m["tree"], m["straddler"]
    keys, bounds = G.bounded_queries(tree, m["queries"], straddler)
    h = host(rt.lsm_get_device(m["dev"], None, keys, max_seq=bounds))
    got = check(tree, keys, bounds, h)
    check_blocks_checked(tree, keys, got, h)
    free = {k: tree.get(k) for k in set(keys)}
    # the visible version sits in a later block of the SST that holds the newest one
    assert sum(1 for k, g in zip(keys, got) if g.row is not None and g.sst == free[k].sst and g.block > free[k].block) >= 5
    # ... and in the next SST of the run: the straddling key, decided by the SST after the cut
    assert any(k == straddler and g.sst == 6 and 5 in tree.chain(k) for k, g in zip(keys, got))
    # a tombstone at the bound decides DELETED; just above the bound it hides nothing
    pairs = 0
    for q in range(len(keys) - 1):
        if keys[q] == keys[q + 1] and bounds[q] == bounds[q + 1] + 1 and got[q].state == _abi.GET_DELETED \
                and tree.columns(got[q])["seq"] == bounds[q] and got[q + 1].state == _abi.GET_FOUND:
            pairs += 1
    assert pairs >= 3
    assert any(b == 0 for b in bounds) and any(b == U64_MAX for b in bounds)


@pytest.mark.parametrize("version", [2, 1])
def test_get_golden_cases(rt, version):
    """The reference's LayerPriorityTestCase table through the device: the recorded expectation."""
    cases = G.golden_cases()
    assert len(cases) == G.KEPT_CASES
    for c in cases:
        tree = G.golden_tree(c, version, bloom=(len(c["entries"]) % 2 == 0))
        key = c["query_key"].encode()
        bounds = None if c["max_seq"] is None else [c["max_seq"]]
        h = host(rt.lsm_get_device(device_tree(rt, tree), None, [key], max_seq=bounds))
        check(tree, [key], bounds, h)
        if c["expected"] is None:
            assert int(h["state"][0]) in (_abi.GET_NOT_FOUND, _abi.GET_DELETED), c["description"]
        else:
            assert int(h["state"][0]) == _abi.GET_FOUND, c["description"]
            data = tree.leaves[int(h["sst"][0])].sst.data
            vo, vl = int(h["val_off"][0]), int(h["val_len"][0])
            assert data[vo:vo + vl].tobytes() == c["expected"].encode(), c["description"]


def test_get_merge_operand(rt):
    tree = G.Tree([[G.leaf_of([(b"a", 0, b"x", 95, None, None), (b"k", 1, b"op", 90, None, 77)], 2, 4096)],
                   [G.leaf_of([(b"k", 0, b"base", 50, None, None), (b"z", 0, b"y", 40, None, None)], 1, 4096)]])
    keys, bounds = [b"k", b"k", b"k", b"k"], [U64_MAX, 90, 89, 49]
    h = host(rt.lsm_get_device(device_tree(rt, tree), None, keys, max_seq=bounds))
    check(tree, keys, bounds, h)
    assert h["state"][:4].tolist() == [_abi.GET_MERGE_OPERAND, _abi.GET_MERGE_OPERAND, _abi.GET_FOUND, _abi.GET_NOT_FOUND]
    assert h["status"][:4].tolist() == [_abi.SDB_MERGE_OPERATOR_MISSING, _abi.SDB_MERGE_OPERATOR_MISSING, 0, 0]
    assert h["sst"][:3].tolist() == [0, 0, 1] and int(h["seq"][0]) == 90 and int(h["val_len"][0]) == 2
    assert int(h["expire_ts"][0]) == 77 and h["sum_num_merge"] == 2 and h["sum_num_failed"] == 0 and h["sum_status"] == 0


def broken(tree, i, block_status):
    """The tree with blocks of leaf i broken in the model: {block: status}."""
    runs, j = [], 0
    for r in tree.runs:
        runs.append([G.Leaf(l.sst, l.bloom is not None, block_status if j + x == i else None, l.version)
                     for x, l in enumerate(r)])
        j += len(r)
    return G.Tree(runs)


def block_range(leaf, key):
    return G.partitions_covering_range(leaf.sst.index_keys, key, G.INC, key, G.INC)


def pick_bad_block(tree, i, keys):
    """A block of leaf i, and of the queries whose block range there holds it: those that reach it (they will
    fail), those the first L0 SST answers before it, and those the filter keeps out of the SST.  The block
    nearest the middle for which none of the three is empty."""
    leaf, nb = tree.leaves[i], tree.leaves[i].sst.nb
    clean = [tree.get(k) for k in keys]
    for b in sorted(range(nb - 1), key=lambda b: abs(b - nb // 2)):
        over = [q for q, k in enumerate(keys) if leaf.covers(k) and block_range(leaf, k)[0] <= b < block_range(leaf, k)[1]]
        kept_out = [q for q in over if tree.step(i, keys[q])[0] == "filtered"]
        before = [q for q in over if q not in kept_out and clean[q].sst == 0]
        reach = [q for q in over if q not in kept_out and (clean[q].sst & 0xFFFFFFFF) >= i]
        if kept_out and before and reach:
            return b, reach, before, kept_out
    raise AssertionError("no block of the SST serves the test")


@pytest.mark.parametrize("how", ["crc", "block_off"])
def test_get_lazy_errors(rt, how):
    m = main(rt)
    tree, keys = m["tree"], m["queries"]
    i = 2  # the second L0 SST with entries; it has a filter
    leaf = tree.leaves[i]
    assert leaf.bloom is not None
    bad, reach, before, kept_out = pick_bad_block(tree, i, keys)
    views = [view_of(l) for l in tree.leaves]
    if how == "crc":
        status, block_status = _abi.SDB_CHECKSUM_MISMATCH, {bad: _abi.SDB_CHECKSUM_MISMATCH}
        data = leaf.sst.data.copy()
        data[int(leaf.sst.block_off[bad]) + 5] ^= 0x40
        views[i] = view_of(leaf, data=data)
    else:  # the block's end cut to 3 bytes: Block::decode cannot hold it, and the next block starts astray
        status, block_status = _abi.SDB_CORRUPT_BLOCK, {bad: _abi.SDB_CORRUPT_BLOCK, bad + 1: _abi.SDB_CHECKSUM_MISMATCH}
        off = leaf.sst.block_off.copy()
        off[bad + 1] = off[bad] + 3
        views[i] = view_of(leaf, block_off=off)
    model = broken(tree, i, block_status)
    h = host(rt.lsm_get_device(device_tree(rt, model, views), None, keys))
    got = check(model, keys, None, h)
    clean = [tree.get(k) for k in keys]
    failing = [q for q, g in enumerate(got) if g.status not in (0, _abi.SDB_MERGE_OPERATOR_MISSING)]
    assert set(reach) <= set(failing) and all(got[q].status == status for q in reach)
    for q in failing:
        assert int(h["state"][q]) == _abi.GET_NOT_FOUND and (int(h["sst"][q]) & 0xFFFFFFFF) == _abi.NO_SST
        assert not any(int(h[f][q]) for f in ("block", "val_off", "val_len", "seq", "flags", "create_ts", "expire_ts"))
    # the first L0 SST answered, or the filter kept the query out of the bad SST: the bad block never surfaces
    for q in before + kept_out + [q for q in range(len(keys)) if q not in failing]:
        assert got[q][:7] == clean[q][:7], keys[q]
    assert h["sum_num_failed"] == len(failing) and h["sum_status"] == got[failing[0]].status


def test_get_invalid_version_view(rt):
    m = main(rt)
    tree, keys = m["tree"], m["queries"][:200]
    runs, j = [], 0
    for r in tree.runs:
        runs.append([G.Leaf(l.sst, l.bloom is not None, None, 3 if j + x == 3 else l.version) for x, l in enumerate(r)])
        j += len(r)
    model = G.Tree(runs)
    h = host(rt.lsm_get_device(device_tree(rt, model), None, keys))
    got = check(model, keys, None, h)
    hit = [g for g in got if g.status == _abi.SDB_INVALID_VERSION]
    assert 5 < len(hit) < len(keys) - 5


def with_arrays(rt, dev, **arrays):
    """The device tree with some of its index arrays replaced (well-formed allocations, wrong numbers)."""
    t = dict(dev)
    t.update({"_" + k: v for k, v in arrays.items()})
    t["lsm"] = _abi.LsmView(t["_ssts"].data_ptr(), t["num_ssts"], t["num_runs"], t["_run_start"].data_ptr(),
                            t["_first_key_bytes"].data_ptr(), t["_first_key_off"].data_ptr(),
                            t["_last_key_bytes"].data_ptr(), t["_last_key_off"].data_ptr(),
                            t["_block_base"].data_ptr(), t["total_blocks"])
    return t


@pytest.mark.parametrize("what", ["block_base", "block_base_total", "run_start"])
def test_get_malformed_tree(rt, what):
    m = main(rt)
    keys = m["queries"][:100]
    dev = m["dev"]
    if what == "block_base":  # disagrees with a view's num_blocks (the sums still end at total_blocks)
        bb = dev["_block_base"].clone()
        bb[3] -= 1
        t = with_arrays(rt, dev, block_base=bb)
    elif what == "block_base_total":
        bb = dev["_block_base"].clone()
        bb[-1] -= 1
        t = with_arrays(rt, dev, block_base=bb)
    else:  # not monotone
        rs = dev["_run_start"].clone()
        rs[2], rs[3] = 3, 2
        t = with_arrays(rt, dev, run_start=rs)
    h = host(rt.lsm_get_device(t, None, keys))
    n = len(keys)
    assert (h["status"][:n] == _abi.SDB_INVALID_ARGUMENT).all() and not h["state"][:n].any()
    assert ((h["sst"][:n].astype(np.int64) & 0xFFFFFFFF) == _abi.NO_SST).all()
    for f in ("block", "val_off", "val_len", "seq", "flags"):
        assert not h[f][:n].any(), f
    assert h["sum_num_failed"] == n and h["sum_status"] == _abi.SDB_INVALID_ARGUMENT and h["sum_blocks_checked"] == 0
    again = host(rt.lsm_get_device(dev, None, keys))  # the well-formed tree still answers
    check(m["tree"], keys, None, again)


def test_get_degenerate(rt):
    m = main(rt)
    h = host(rt.lsm_get_device(m["dev"], None, []))
    assert not h["summary"].any()
    keys = [b"a", b"", b"k00002"]
    empty_tree = G.Tree([])
    of_empty = G.Tree([[G.Leaf(G.EmptySst())], [G.Leaf(G.EmptySst()), G.Leaf(G.EmptySst())]])
    for tree in (empty_tree, of_empty):
        dev = device_tree(rt, tree) if tree.leaves else rt.lsm_tree_device([], [])
        assert dev["total_blocks"] == 0
        h = host(rt.lsm_get_device(dev, None, keys, max_seq=[5, 6, 7]))
        assert not h["summary"].any()
        assert not h["state"][:3].any() and not h["status"][:3].any()
        assert ((h["sst"][:3].astype(np.int64) & 0xFFFFFFFF) == _abi.NO_SST).all()
        for f in ("block", "val_off", "val_len", "seq", "flags", "ssts_read", "ssts_filtered"):
            assert not h[f][:3].any(), f


def test_get_graph_capture_and_workspace_reuse(rt):
    import torch
    m = main(rt)
    tree, dev, straddler = m["tree"], m["dev"], m["straddler"]
    keys, bounds = G.bounded_queries(tree, m["queries"][:200], straddler)
    n = len(keys)
    keys2, bounds2 = keys[::-1], [b if b in (0, U64_MAX) else b - 1 for b in bounds[::-1]]

    def tensors(ks, bs):
        kb, ko = rt.keys_columnar(ks)
        return to_dev(kb), to_dev(ko), to_dev(np.array(bs, np.uint64))

    kb, ko, ms = tensors(keys, bounds)
    kb2, ko2, ms2 = tensors(keys2, bounds2)
    assert kb.numel() == kb2.numel()
    ws = torch.empty(rt.read_workspace_bytes("sdb_lsm_get", dev, n), dtype=torch.uint8, device="cuda")
    # two calls back to back on one workspace, no reset and no synchronisation between them
    r1 = rt.lsm_get_device(dev, None, (kb, ko, n), max_seq=ms, workspace=ws)
    r2 = rt.lsm_get_device(dev, None, (kb2, ko2, n), max_seq=ms2, workspace=ws)
    r3 = rt.lsm_get_device(dev, None, (kb, ko, n), workspace=ws)
    check(tree, keys, bounds, host(r1))
    check(tree, keys2, bounds2, host(r2))
    check(tree, keys, None, host(r3))
    # one captured call, replayed after the key and max_seq tensors are overwritten in place
    first = (kb.clone(), ko.clone(), ms.clone())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # the first launch (function attributes) outside the capture
        warm = rt.lsm_get_device(dev, None, (kb, ko, n), max_seq=ms, stream=s, workspace=ws)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    holder = {}
    with torch.cuda.graph(g, stream=s):
        holder["res"] = rt.lsm_get_device(dev, None, (kb, ko, n), max_seq=ms, stream=s, workspace=ws)
    for ks, bs, src in ((keys, bounds, first), (keys2, bounds2, (kb2, ko2, ms2)), (keys, bounds, first)):
        for dst, t in zip((kb, ko, ms), src):
            dst.copy_(t)
        for k, t in holder["res"].items():
            if not k.startswith("_"):
                t.zero_()
        torch.cuda.synchronize()
        g.replay()
        check(tree, ks, bs, host(holder["res"]))
    del warm
