"""The ten tree-read wrappers of slatedb_amd.runtime over a stub library, on CPU tensors: which C symbol each calls, the
retry once on SDB_LIMIT_EXCEEDED with the capacities the rules give, no retry when every capacity was passed, the
workspace rule, the error text and the result keys (the literals below are the keys of the wrappers before the two
families were folded into _lsm_get and _lsm_scan; the _projected and _mem wrappers make the filtered wrapper's assertions,
and theirs on the keys they add and on what the library sees as `proj` and `mem`)."""
import ctypes as C

import pytest
import torch

from slatedb_amd import _abi, runtime as rt

GET = {f for f, _ in rt.GET_FIELDS} | {"summary"}
CHAIN = {"chain_start", "chain_summary", "chain_sst", "chain_block", "chain_val_off", "chain_val_len", "chain_seq",
         "chain_flags", "chain_create_ts", "chain_expire_ts"}
SCAN = {"range_entry_start", "range_status", "range_ssts", "summary", "key_arena", "key_off", "sst", "val_off", "val_len",
        "seq", "flags", "create_ts", "expire_ts"}
FILT = {"range_filtered", "num_filtered"}
MEM, MEM_CHAIN, MEM_SCAN = {"table", "row"}, {"chain_table", "chain_row"}, {"range_tables"}
WS = 4096  # what the stub's sizers answer


class Stream:
    cuda_stream = None

    def synchronize(self):
        pass


class Lib:
    """Records (symbol, cand_entries, cand_key_bytes, cap_entries, key_arena_cap, cap_links) per entry-point call and
    the sizers called; on its first entry-point call writes `scan` = (num_candidates, candidate_key_bytes) with
    SDB_LIMIT_EXCEEDED into the scan summary and `links` with SDB_LIMIT_EXCEEDED into the chain summary."""

    def __init__(self, scan=None, links=None, status=0):
        self.scan, self.links, self.status, self.calls, self.sizers, self.args = scan, links, status, [], [], []

    def __getattr__(self, name):
        if name.endswith("_workspace_bytes"):
            return lambda *a: self.sizers.append((name, a)) or WS
        return lambda *a: self.entry(name, a)

    def entry(self, name, args):
        objs = {type(a._obj): a._obj for a in args if hasattr(a, "_obj")}
        out, chain = objs.get(_abi.LsmScanOut), objs.get(_abi.ChainOut)
        ints = [a for a in args if isinstance(a, int) and not isinstance(a, bool)]
        first = not self.calls
        self.args.append(args)
        self.calls.append((name,) + ((ints[-4], ints[-3], out.cap_entries, out.key_arena_cap) if out is not None else ()) +
                          ((chain.cap_links,) if chain is not None else ()))
        if first and out is not None and self.scan:
            sm = (C.c_int64 * 7).from_address(out.summary)
            sm[2], sm[3], sm[6] = self.scan[0], self.scan[1], _abi.SDB_LIMIT_EXCEEDED
        if first and chain is not None and self.links:
            cm = (C.c_int64 * 3).from_address(chain.summary)
            cm[0], cm[2] = self.links, _abi.SDB_LIMIT_EXCEEDED
        return self.status


TREE = {"lsm": _abi.LsmView(), "device": "cpu", "total_blocks": 3, "num_ssts": 2, "num_runs": 2, "_policies": None}
KEYS = [b"a", b"bb", b"ccc"]
RANGES = [(b"a", _abi.BOUND_INCLUDED, b"c", _abi.BOUND_EXCLUDED), (None, _abi.BOUND_UNBOUNDED, None, _abi.BOUND_UNBOUNDED)]

GETS = {"sdb_lsm_get": (lambda **k: rt.lsm_get_device(TREE, None, KEYS, stream=Stream(), **k), False),
        "sdb_lsm_get_merge": (lambda **k: rt.lsm_get_merge_device(TREE, None, KEYS, stream=Stream(), **k), True),
        "sdb_lsm_get_filtered": (lambda **k: rt.lsm_get_filtered_device(TREE, None, KEYS, stream=Stream(), **k), None),
        "sdb_lsm_get_projected": (lambda **k: rt.lsm_get_projected_device(TREE, None, None, KEYS, stream=Stream(), **k), None),
        "sdb_lsm_get_mem": (lambda **k: rt.lsm_get_mem_device(None, TREE, None, KEYS, stream=Stream(), **k), None)}
SCANS = {"sdb_lsm_scan": (lambda **k: rt.lsm_scan_device(TREE, RANGES, stream=Stream(), **k), False),
         "sdb_lsm_scan_merge": (lambda **k: rt.lsm_scan_merge_device(TREE, RANGES, stream=Stream(), **k), True),
         "sdb_lsm_scan_filtered": (lambda **k: rt.lsm_scan_filtered_device(TREE, RANGES, stream=Stream(), **k), None),
         "sdb_lsm_scan_projected": (lambda **k: rt.lsm_scan_projected_device(TREE, None, RANGES, stream=Stream(), **k), None),
         "sdb_lsm_scan_mem": (lambda **k: rt.lsm_scan_mem_device(None, TREE, RANGES, stream=Stream(), **k), None)}
VISIBLE = [None, (b"a", _abi.BOUND_INCLUDED, b"b", _abi.BOUND_EXCLUDED)]  # one visible range per SST of TREE


def public(res):
    return {k for k in res if not k.startswith("_")}


def variants(merging):
    """(extra keyword arguments, the call has a chain) of a wrapper: the filtered ones go both ways."""
    return [({}, merging)] if merging is not None else [({"merge": False}, False), ({"merge": True}, True)]


@pytest.mark.parametrize("symbol", sorted(GETS))
def test_get_wrappers(monkeypatch, symbol):
    call, merging = GETS[symbol]
    mem = symbol.endswith("_mem")
    for kw, merge in variants(merging):
        get, chain = GET | (MEM if mem else set()), CHAIN | (MEM_CHAIN if mem else set())  # what the wrapper's result holds
        # links that do not fit: sized at nkeys first, then at the reported num_links; the plain get has nothing to size
        lib = Lib(links=17)
        monkeypatch.setattr(rt, "lib", lambda: lib)
        res = call(**kw)
        assert lib.calls == ([(symbol, len(KEYS)), (symbol, 17)] if merge else [(symbol,)])
        assert {s for s, _ in lib.sizers} == {symbol + "_workspace_bytes"}
        assert lib.sizers[0][1] == ((0,) if mem else ()) + (3, 2, 2, len(KEYS)) + ((int(merge),) if merging is None else ())
        assert public(res) == (get | chain if merge else get)
        assert res["_ws"].numel() == WS and int(res["_keys"][1][-1]) == 6
        if merge:  # links that fit at nkeys, and a given capacity: one call
            lib = Lib()
            monkeypatch.setattr(rt, "lib", lambda: lib)
            call(**kw)
            assert lib.calls == [(symbol, len(KEYS))]
            lib = Lib(links=17)
            monkeypatch.setattr(rt, "lib", lambda: lib)
            assert public(call(cap_links=5, **kw)) == get | chain
            assert lib.calls == [(symbol, 5)]
        # the caller's workspace is used as it is and must hold the call
        lib = Lib()
        monkeypatch.setattr(rt, "lib", lambda: lib)
        ws = torch.empty(WS + 8, dtype=torch.uint8)
        assert call(workspace=ws, **kw)["_ws"] is ws
        with pytest.raises(AssertionError, match="workspace too small"):
            call(workspace=torch.empty(WS - 1, dtype=torch.uint8), **kw)
        lib = Lib(status=_abi.SDB_INVALID_ARGUMENT)
        monkeypatch.setattr(rt, "lib", lambda: lib)
        with pytest.raises(rt.SdbError, match=symbol + ": "):
            call(**kw)


@pytest.mark.parametrize("symbol", sorted(SCANS))
def test_scan_wrappers(monkeypatch, symbol):
    call, merging = SCANS[symbol]
    for kw, merge in variants(merging):
        want = SCAN | (CHAIN if merge else set()) | (FILT if merging is None else set())
        if symbol.endswith("_mem"):
            want |= MEM | MEM_SCAN | (MEM_CHAIN if merge else set())
        L = (lambda x: (x,)) if merge else (lambda x: ())  # cap_links travels only with a chain
        nine = {} if symbol == "sdb_lsm_scan" else {"cap_links": 9}  # lsm_scan_device has no such argument

        def run(lib, **more):
            monkeypatch.setattr(rt, "lib", lambda: lib)
            res = call(**more, **kw)
            assert public(res) == want and {s for s, _ in lib.sizers} == {symbol + "_workspace_bytes"}
            return lib.calls

        # nothing given: no staging room first, then everything sized like the reported staging
        assert run(Lib(scan=(40, 900))) == [(symbol, 0, 0, 0, 0) + L(0), (symbol, 40, 900, 40, 900) + L(40)]
        # the staging is max(given, reported); a given cap and cap_links stay
        assert run(Lib(scan=(40, 900)), cand=(50, 100)) == [(symbol, 50, 100, 0, 0) + L(0), (symbol, 50, 900, 50, 900) + L(50)]
        got = run(Lib(scan=(40, 900)), cap=(7, 70), **nine)
        assert got == [(symbol, 0, 0, 7, 70) + L(9), (symbol, 40, 900, 7, 70) + L(9)]
        # links alone that do not fit: a retry where there is a chain, and only there
        got = run(Lib(links=123), cand=(50, 100), cap=(7, 70))
        assert got == ([(symbol, 50, 100, 7, 70, 0), (symbol, 50, 100, 7, 70, 50)] if merge else [(symbol, 50, 100, 7, 70)])
        # nothing exceeded: one call; every capacity given: one call whatever the summaries say
        assert run(Lib()) == [(symbol, 0, 0, 0, 0) + L(0)]
        assert run(Lib(scan=(40, 900), links=123), cand=(5, 6), cap=(7, 8), **nine) == [(symbol, 5, 6, 7, 8) + L(9)]
        if not merge:  # without a chain cap_links is no capacity of the call
            assert run(Lib(scan=(40, 900), links=123), cand=(5, 6), cap=(7, 8)) == [(symbol, 5, 6, 7, 8)]
        # a workspace that is too small is replaced, unless the caller fixed the staging
        small = torch.empty(WS - 1, dtype=torch.uint8)
        lib = Lib()
        monkeypatch.setattr(rt, "lib", lambda: lib)
        res = call(workspace=small, **kw)
        assert res["_ws"] is not small and res["_ws"].numel() == WS
        big = torch.empty(WS, dtype=torch.uint8)
        assert call(workspace=big, cand=(1, 1), cap=(1, 1), **nine, **kw)["_ws"] is big
        with pytest.raises(AssertionError, match="workspace too small"):
            call(workspace=small, cand=(1, 1), **kw)
        lib = Lib(status=_abi.SDB_LIMIT_EXCEEDED)
        monkeypatch.setattr(rt, "lib", lambda: lib)
        with pytest.raises(rt.SdbError, match=symbol + ": "):
            call(**kw)


def ranges_of(arg):
    """What the library got for a const sdb_scan_ranges *: None, or (n, the arrays are all there)."""
    return None if arg is None else (arg._obj.n, all(getattr(arg._obj, f) for f, _ in _abi.ScanRanges._fields_[1:]))


@pytest.mark.parametrize("merge", [False, True])
def test_proj_and_mem_positions(monkeypatch, merge):
    """The projections are the argument behind lsm, the memtables the first: NULL for None, else the caller's."""
    tables = {"mem": _abi.MemView(0x1000, 3, 0), "num_tables": 3}
    calls = {"sdb_lsm_get_projected": lambda p, t: rt.lsm_get_projected_device(TREE, None, p, KEYS, stream=Stream(), merge=merge),
             "sdb_lsm_scan_projected": lambda p, t: rt.lsm_scan_projected_device(TREE, p, RANGES, stream=Stream(), merge=merge),
             "sdb_lsm_get_mem": lambda p, t: rt.lsm_get_mem_device(t, TREE, None, KEYS, projections=p, stream=Stream(), merge=merge),
             "sdb_lsm_scan_mem": lambda p, t: rt.lsm_scan_mem_device(t, TREE, RANGES, projections=p, stream=Stream(), merge=merge)}
    for symbol, call in calls.items():
        mem = symbol.endswith("_mem")
        for proj, tabs in ((None, None), (VISIBLE, tables)):
            lib = Lib()
            monkeypatch.setattr(rt, "lib", lambda: lib)
            res = call(proj, tabs)
            assert [c[0] for c in lib.calls] == [symbol]
            args = lib.args[0]
            assert len(args) == len(_abi.SIGNATURES[symbol][1])
            assert args[1 if mem else 0]._obj is TREE["lsm"]
            assert ranges_of(args[2 if mem else 1]) == (None if proj is None else (len(VISIBLE), True))
            assert (res["_projections"] is None) == (proj is None)
            if mem:
                assert (args[0] is None) if tabs is None else (args[0]._obj is tables["mem"])
                assert lib.sizers[0][1][0] == (0 if tabs is None else 3) and res["_mem"] is tabs
                assert isinstance(args[10 if "_scan" in symbol else 9]._obj, _abi.LsmScanOut if "_scan" in symbol else _abi.GetOut)
                mout = args[11 if "_scan" in symbol else 10]._obj
                assert mout.table == res["table"].data_ptr() and mout.row == res["row"].data_ptr()
                if "_scan" in symbol:
                    assert mout.range_tables == res["range_tables"].data_ptr()
                mchain = args[13 if "_scan" in symbol else 12]
                assert (mchain is not None) == merge
                if merge:
                    assert mchain._obj.table == res["chain_table"].data_ptr() and mchain._obj.row == res["chain_row"].data_ptr()
