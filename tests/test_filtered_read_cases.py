"""CPU checks of the filtered tree reads (sdb_lsm_scan_filtered, sdb_lsm_get_filtered): the fixture tree shows what
the device tests rely on, the model of tests/filtered_read_cases.py agrees with a brute-force read wherever the
caller keeps F4, and the C ABI carries the new structs and entry points (host checks and the no-device path)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from slatedb_amd import _abi

from . import filtered_read_cases as F
from . import lsm_scan_cases as L
from .scan_cases import INC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "slatedb_amd.h")
NEW = ("sdb_lsm_scan_filtered", "sdb_lsm_scan_filtered_workspace_bytes", "sdb_lsm_get_filtered",
       "sdb_lsm_get_filtered_workspace_bytes")


@pytest.fixture(scope="module")
def tree():
    return F.main_tree()


@pytest.fixture(scope="module")
def lib():
    from slatedb_amd import runtime
    return runtime.lib()


def test_fixture_shape(tree):
    assert [len(r) for r in tree.runs] == [1, 1, 1, 3]
    assert all(100 <= len(l.sst.rows) <= 200 for l in tree.leaves)
    assert sorted({l.version for l in tree.leaves}) == [1, 2]
    for l in tree.leaves:
        assert 3 <= len({k[:4] for k in l.sst.keys}) <= 5 and l.sst.nb > 4
    kinds = [(l.policy.kind, l.policy.no_whole_key) for l in tree.leaves]
    assert kinds[:4] == [(F.FIXED, 0), (F.DELIM, 1), (F.LENGTHS, 0), (F.NONE, 0)]
    assert tree.leaves[4].bloom is None and len(tree.leaves[5].bloom) == 0
    assert all(len(tree.leaves[i].bloom) > 0 for i in range(4)) and tree.leaves[2].num_probes == 1


def test_fixture_conditions(tree):
    """What the seed was picked for: conditions on the input, so the device tests see pruning, a false positive and
    no false negative."""
    pairs = F.prefix_pairs(tree)
    assert len(pairs) >= 30
    assert 3 * sum(1 for _, _, out, _ in pairs if out) >= len(pairs)  # 1. a third of the pairs of rule 1 is ruled out
    assert any(not out and not holds and tree.leaves[i].bloom is not None and len(tree.leaves[i].bloom)
               for _, i, out, holds in pairs)  # 2. a false positive of a filter that had something to probe
    assert not any(out and holds for _, _, out, holds in pairs)  # 3. no false negative


def test_model_equals_brute_force(tree):
    cases = F.scan_cases(tree)
    assert 40 <= len(cases) <= 80
    pruned = 0
    for rng, prefix, pl in cases:
        assert F.honours_f4(tree, rng, prefix), (rng, prefix)
        for bound in (None, 10**6 - 300):
            got = F.scan(tree, rng, prefix, pl, bound)
            plain = L.scan(tree, rng, bound)
            rows, status = L.brute(tree, rng, bound)
            assert got.status == status == 0 and got.rows == rows == plain.rows, (rng, prefix)
            assert sorted(got.ssts + got.filtered) == plain.ssts and got.blocks <= plain.blocks
            assert got.candidates <= plain.candidates
            pruned += len(got.filtered)
            assert F.scan(tree, rng, prefix, pl, bound, True).rows == rows[::-1]
    assert pruned >= 40
    # a point range asks Point(key) whatever the prefix says; without a prefix a range that is no point asks nothing
    k = L.all_keys(tree)[40]
    assert F.query((k, INC, k, INC), b"zz") == (k, False) and F.query(F.prefix_range(b"t01:"), None) is None
    assert F.scan(tree, (k, INC, k, INC), b"zz").rows == L.brute(tree, (k, INC, k, INC))[0]


def test_model_get_finds_every_key():
    for tree in (F.main_tree(), F.uniform_tree()):
        keys = F.get_keys(tree)
        held = set(L.all_keys(tree))
        filtered = 0
        for k in keys:
            g = tree.get(k, probe_len=F.LENGTHS_LEN)
            rows, _ = L.brute(tree, (k, INC, k, INC))
            assert (g.state == _abi.GET_FOUND) == bool(rows), k
            assert g.state != _abi.GET_NOT_FOUND or k not in held or not rows
            filtered += g.ssts_filtered
        assert filtered >= 100
    # the probe the unfiltered get sends (the full key) finds nothing in a filter without whole-key hashes
    tree = F.uniform_tree()
    from oracle import oracle as O
    l = tree.leaves[0]
    miss = [k for k in l.sst.keys if not O.might_contain(l.bloom, l.num_probes, k)]
    assert len(miss) * 2 > len(l.sst.keys)


def test_mixed_merge_tree_conditions():
    """What the merging get under policies that do not agree needs of its tree: conditions on the input alone."""
    from . import merge_read_cases as M
    t = F.mixed_merge_tree()
    assert [len(r) for r in t.runs] == [1, 1, 1, 2] and len({tuple(l.policy) for l in t.leaves}) > 1
    assert [(l.policy.kind, l.policy.no_whole_key) for l in t.leaves[:4]] == [(F.FIXED, 0), (F.DELIM, 1), (F.LENGTHS, 0), (F.NONE, 0)]
    assert t.leaves[4].bloom is None and all(len(l.bloom) > 0 for l in t.leaves[:4])
    chains = [{i for i, _, _ in M.get_merge(t, k).links} for k in L.all_keys(t)]
    assert any({3, 4} <= c for c in chains)  # a chain spans the run's cut
    assert any(min(c) < 3 <= max(c) for c in chains if c)  # a chain crosses from an L0 SST into the run
    assert max(len(M.get_merge(t, k).links) for k in L.all_keys(t)) >= 3


def test_an_empty_bitmap_rules_out_what_has_a_probe(tree):
    l = F.Leaf(tree.leaves[0].sst, F.Policy(F.FIXED, 4, 0), tree.leaves[0].bloom[:0], 6)
    assert F.ruled_out(l, (b"t00:0001", False)) and F.ruled_out(l, (b"t00:", True))
    assert not F.ruled_out(l, (b"t0", True)) and not F.ruled_out(l, None)


def test_abi_symbols_and_layouts(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "slatedb_amd", "libslatedb_amd.so")]).decode()
    exported = set(re.findall(r" T (sdb_\w+)", out))
    assert set(NEW) <= exported and set(NEW) <= set(_abi.SIGNATURES)
    structs = {"sdb_filter_policy": _abi.FilterPolicy, "sdb_scan_prefixes": _abi.ScanPrefixes,
               "sdb_scan_filter_out": _abi.ScanFilterOut}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, "int main(void){"]
    for cname, py in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in py._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-o", exe, src])
        got = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    for cname, py in structs.items():
        assert int(got[cname]) == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(py, f).offset, (cname, f)
    assert lib.sdb_abi_version() == 2


def _scan_args(n=1):
    """Host structs that pass every host check of sdb_lsm_scan_filtered for n ranges over a tree of one SST."""
    keep = [(C.c_uint64 * 64)() for _ in range(8)]
    p = [C.addressof(k) for k in keep]
    lsm = _abi.LsmView(p[0], 1, 1, p[0], p[0], p[0], p[0], p[0], p[0], 4)
    rg = _abi.ScanRanges(n, p[1], p[1], p[1], p[1], p[1], p[1])
    out = _abi.LsmScanOut(p[2], p[2], p[2], p[2], 0, p[2], p[2], p[2], p[2], p[2], p[2], p[2], p[2], 0, p[3])
    px = _abi.ScanPrefixes(p[4], p[4], p[4], None)
    fout = _abi.ScanFilterOut(p[5], p[6])
    return keep, lsm, rg, out, px, fout


def test_scan_filtered_host_checks(lib):
    keep, lsm, rg, out, px, fout = _scan_args()
    wsb = lib.sdb_lsm_scan_filtered_workspace_bytes(4, 1, 1, 1, 0, 0, 0)
    assert wsb > lib.sdb_lsm_scan_workspace_bytes(4, 1, 1, 1, 0, 0) - 256
    assert lib.sdb_lsm_scan_filtered_workspace_bytes(4, 1, 1, 1, 8, 64, 1) > lib.sdb_lsm_scan_merge_workspace_bytes(4, 1, 1, 1, 8, 64) - 256
    ws = (C.c_uint8 * (wsb + 256))()
    call = lambda px_, fout_, ws_=ws, n=wsb: lib.sdb_lsm_scan_filtered(  # noqa: E731
        C.byref(lsm), None, C.byref(rg), px_, None, 0, 0, 0, C.byref(out), None, fout_, ws_, n, None)
    assert call(C.byref(px), None) == _abi.SDB_INVALID_ARGUMENT  # a NULL fout
    assert call(None, None) == _abi.SDB_INVALID_ARGUMENT
    for bad in (_abi.ScanFilterOut(None, fout.num_filtered), _abi.ScanFilterOut(fout.range_filtered, None)):
        assert call(C.byref(px), C.byref(bad)) == _abi.SDB_INVALID_ARGUMENT  # a NULL array inside it
    for bad in (_abi.ScanPrefixes(None, px.prefix_off, px.has_prefix, None), _abi.ScanPrefixes(px.prefix_bytes, None, px.has_prefix, None),
                _abi.ScanPrefixes(px.prefix_bytes, px.prefix_off, None, None)):
        assert call(C.byref(bad), C.byref(fout)) == _abi.SDB_INVALID_ARGUMENT
    assert call(C.byref(px), C.byref(fout), ws, wsb - 1) == _abi.SDB_INVALID_ARGUMENT  # a short workspace
    if lib.sdb_device_count() == 0:  # after the host checks, without a device
        assert call(C.byref(px), C.byref(fout)) == _abi.SDB_DEVICE_ERROR
        assert call(None, C.byref(fout)) == _abi.SDB_DEVICE_ERROR


def test_get_filtered_host_checks(lib):
    keep = [(C.c_uint64 * 64)() for _ in range(4)]
    p = [C.addressof(k) for k in keep]
    lsm = _abi.LsmView(p[0], 1, 1, p[0], p[0], p[0], p[0], p[0], p[0], 4)
    out = _abi.GetOut(*([p[1]] * 12), p[2])
    assert lib.sdb_lsm_get_filtered_workspace_bytes(4, 1, 1, 3, 0) == lib.sdb_lsm_get_workspace_bytes(4, 1, 1, 3)
    assert lib.sdb_lsm_get_filtered_workspace_bytes(4, 1, 1, 3, 1) == lib.sdb_lsm_get_merge_workspace_bytes(4, 1, 1, 3)
    wsb = lib.sdb_lsm_get_filtered_workspace_bytes(4, 1, 1, 1, 0)
    ws = (C.c_uint8 * (wsb + 256))()
    call = lambda out_, keys, n=wsb: lib.sdb_lsm_get_filtered(C.byref(lsm), None, keys, p[3], 1, None, None, out_, None,  # noqa: E731
                                                             ws, n, None)
    assert call(None, p[3]) == _abi.SDB_INVALID_ARGUMENT
    assert call(C.byref(out), None) == _abi.SDB_INVALID_ARGUMENT
    assert call(C.byref(out), p[3], wsb - 1) == _abi.SDB_INVALID_ARGUMENT
    if lib.sdb_device_count() == 0:
        assert call(C.byref(out), p[3]) == _abi.SDB_DEVICE_ERROR
