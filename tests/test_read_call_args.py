"""The host-side argument checks of the ten tree-read entry points (sdb_lsm_get / sdb_lsm_scan, each plain, _merge,
_filtered, _projected and _mem), on the CPU: the sdb_status of every malformed call, and which check wins where two
apply.  Every expectation is read off sdb_api.cpp's lsm_get_call and lsm_scan_call: the NULL top-level arguments (and
the mem / chain pairing), then the limits, then the tree's arrays, the projections, the outputs, the chain and the
workspace, SDB_DEVICE_ERROR last.

The calls run over host arrays, so only malformed calls are made when a device is visible: they return before any
launch.  The well-formed ones, which end in SDB_DEVICE_ERROR, run only without a device."""
import ctypes as C

import numpy as np
import pytest

from slatedb_amd import _abi

INV, LIM, DEV = _abi.SDB_INVALID_ARGUMENT, _abi.SDB_LIMIT_EXCEEDED, _abi.SDB_DEVICE_ERROR
GET_TAIL = ("ws", "wsb", "stream")
# the arguments of each entry point in C order, under one name each
SYMS = {
    "sdb_lsm_get": ("lsm", "key_bytes", "key_off", "n", "max_seq", "out") + GET_TAIL,
    "sdb_lsm_get_merge": ("lsm", "key_bytes", "key_off", "n", "max_seq", "out", "chain") + GET_TAIL,
    "sdb_lsm_get_filtered": ("lsm", "policies", "key_bytes", "key_off", "n", "probe_len", "max_seq", "out", "chain") + GET_TAIL,
    "sdb_lsm_get_projected": ("lsm", "proj", "policies", "key_bytes", "key_off", "n", "probe_len", "max_seq", "out",
                              "chain") + GET_TAIL,
    "sdb_lsm_get_mem": ("mem", "lsm", "proj", "policies", "key_bytes", "key_off", "n", "probe_len", "max_seq", "out", "mout",
                        "chain", "mchain") + GET_TAIL,
    "sdb_lsm_scan": ("lsm", "ranges", "max_seq", "desc", "ce", "ckb", "out") + GET_TAIL,
    "sdb_lsm_scan_merge": ("lsm", "ranges", "max_seq", "desc", "ce", "ckb", "out", "chain") + GET_TAIL,
    "sdb_lsm_scan_filtered": ("lsm", "policies", "ranges", "prefixes", "max_seq", "desc", "ce", "ckb", "out", "chain",
                              "fout") + GET_TAIL,
    "sdb_lsm_scan_projected": ("lsm", "proj", "policies", "ranges", "prefixes", "max_seq", "desc", "ce", "ckb", "out",
                               "chain", "fout") + GET_TAIL,
    "sdb_lsm_scan_mem": ("mem", "lsm", "proj", "policies", "ranges", "prefixes", "max_seq", "desc", "ce", "ckb", "out",
                         "mout", "chain", "mchain", "fout") + GET_TAIL,
}
# the sizer's arguments, named as the shape below names them
SIZERS = {s: (("ntab",) if s.endswith("_mem") else ()) + ("total_blocks", "num_ssts", "num_runs", "n") +
          (("ce", "ckb") if "_scan" in s else ()) + (() if s in ("sdb_lsm_get", "sdb_lsm_scan") or s.endswith("_merge") else ("merge",))
          for s in SYMS}
N, CAP, CAPL, NTAB, CE, CKB = 2, 4, 4, 2, 8, 64  # the well-formed call: two queries, one SST in one run, three blocks
LSM_ARRAYS = ("ssts", "run_start", "first_key_bytes", "first_key_off", "last_key_bytes", "last_key_off", "block_base")
RANGE_ARRAYS = ("start_bytes", "start_off", "start_kind", "end_bytes", "end_off", "end_kind")
COLUMNS = ("val_off", "val_len", "seq", "flags", "create_ts", "expire_ts")
GET_OUT = ("state", "status", "sst", "block") + COLUMNS + ("ssts_read", "ssts_filtered", "summary")
SCAN_OUT = ("range_entry_start", "range_status", "range_ssts", "key_arena", "key_off", "sst") + COLUMNS + ("summary",)
CHAIN = ("chain_start", "sst", "block") + COLUMNS + ("summary",)


@pytest.fixture(scope="module")
def lib():
    from slatedb_amd import runtime
    return runtime.lib()


def test_tables_match_the_signatures():
    for s, names in SYMS.items():
        assert len(names) == len(_abi.SIGNATURES[s][1]), s
        assert len(SIZERS[s]) == len(_abi.SIGNATURES[s + "_workspace_bytes"][1]), s


def call(lib, entry, edits=()):
    """One call of `entry` over host arrays: the well-formed call with `edits` applied.  An edit is a top-level argument
    name -> its value (None: NULL), "object.field" -> the field's value, or "short_ws" -> True: one byte short of what
    the sizer asks for the well-formed shape."""
    edits = dict(edits)
    scan, keep = "_scan" in entry, []

    def arr(count, dt=np.uint64):
        keep.append(np.zeros(max(count, 1), dt))
        return keep[-1].ctypes.data

    view, runs, gs, ss, cs = (_abi.SstView * 1)(), (_abi.Run * NTAB)(), _abi.GetSummary(), _abi.LsmScanSummary(), _abi.ChainSummary()
    o = {"lsm": _abi.LsmView(C.addressof(view), 1, 1, arr(2, np.uint32), arr(8, np.uint8), arr(2), arr(8, np.uint8), arr(2),
                             arr(2), 3),
         "proj": _abi.ScanRanges(1, arr(8, np.uint8), arr(2), arr(1, np.uint8), arr(8, np.uint8), arr(2), arr(1, np.uint8)),
         "ranges": _abi.ScanRanges(N, arr(8, np.uint8), arr(N + 1), arr(N, np.uint8), arr(8, np.uint8), arr(N + 1),
                                   arr(N, np.uint8)),
         "prefixes": _abi.ScanPrefixes(arr(8, np.uint8), arr(N + 1), arr(N, np.uint8), arr(N, np.int32)),
         "mem": _abi.MemView(C.addressof(runs), NTAB, 0),
         "mchain": _abi.MemChainOut(arr(CAPL, np.uint32), arr(CAPL)),
         "fout": _abi.ScanFilterOut(arr(N, np.uint32), arr(1)),
         "chain": _abi.ChainOut(arr((CAP if scan else N) + 1), *[arr(CAPL) for _ in range(8)], CAPL, C.addressof(cs))}
    if scan:
        o["out"] = _abi.LsmScanOut(arr(N + 1), arr(N, np.int32), arr(N, np.uint32), arr(64, np.uint8), 64, arr(CAP + 1),
                                   *[arr(CAP) for _ in range(7)], CAP, C.addressof(ss))
        o["mout"] = _abi.MemScanOut(arr(CAP, np.uint32), arr(CAP), arr(N, np.uint32))
    else:
        o["out"] = _abi.GetOut(*[arr(N) for _ in range(12)], C.addressof(gs))
        o["mout"] = _abi.MemGetOut(arr(N, np.uint32), arr(N))
    plain = {"key_bytes": arr(8, np.uint8), "key_off": arr(N + 1), "n": N, "max_seq": arr(N), "probe_len": arr(N, np.int32),
             "policies": arr(4, np.uint32), "desc": 0, "ce": CE, "ckb": CKB, "stream": None}
    shape = {"ntab": NTAB, "total_blocks": 3, "num_ssts": 1, "num_runs": 1, "n": N, "ce": CE, "ckb": CKB, "merge": 1}
    wsb = getattr(lib, entry + "_workspace_bytes")(*[shape[a] for a in SIZERS[entry]])
    plain.update(ws=arr(wsb, np.uint8), wsb=wsb - 1 if edits.pop("short_ws", False) else wsb)
    for name, value in edits.items():
        if "." in name:
            setattr(o[name.split(".")[0]], name.split(".")[1], value)
        elif name == "n" and scan:
            o["ranges"].n = value
        elif name in o:
            assert value is None
            o[name] = None
        else:
            plain[name] = value
    args = [plain[a] if a in plain else (C.byref(o[a]) if o[a] is not None else None) for a in SYMS[entry]]
    return getattr(lib, entry)(*args)


def has(entry, *names):
    return all(n in SYMS[entry] for n in names)


def malformed(entry):
    """[(edits, status)] of `entry`: every malformed call this file pins."""
    scan, mem = "_scan" in entry, entry.endswith("_mem")
    chain_needed = entry.endswith("_merge")
    cases = []

    def add(status, **edits):
        cases.append(({k.replace("__", "."): v for k, v in edits.items()}, status))

    # NULL top-level arguments that the call needs
    for a in ("lsm", "out", "ws") + (("ranges",) if scan else ("key_bytes", "key_off")) + (("chain",) if chain_needed else ()):
        add(INV, **{a: None})
    for a in ("fout", "mout"):
        if has(entry, a):
            add(INV, **{a: None})
    add(INV, short_ws=True)
    if mem:  # chain and mchain go together
        add(INV, chain=None)
        add(INV, mchain=None)
        add(INV, mem__tables=None)
    # NULL required fields
    fields = [("lsm", LSM_ARRAYS), ("out", SCAN_OUT if scan else GET_OUT)]
    fields += [("ranges", RANGE_ARRAYS)] if scan else []
    fields += [("chain", CHAIN)] if has(entry, "chain") else []
    fields += [("fout", ("range_filtered", "num_filtered"))] if has(entry, "fout") else []
    fields += [("prefixes", ("prefix_bytes", "prefix_off", "has_prefix"))] if has(entry, "prefixes") else []
    fields += [("proj", RANGE_ARRAYS)] if has(entry, "proj") else []
    fields += [("mout", ("table", "row") + (("range_tables",) if scan else ())), ("mchain", ("table", "row"))] if mem else []
    for obj, names in fields:
        for f in names:
            add(INV, **{obj + "__" + f: None})
    if has(entry, "proj"):  # one projection per SST
        add(INV, proj__n=0)
        add(INV, proj__n=2)
    # the limits, each at its bound (passes: the workspace is then far too short) and one past it
    per = 1 + (NTAB if mem else 0)  # per-item state: a query's runs, a range's SSTs, and the tables
    limits = [{"n": (1 << 40) // per + 1}, {"lsm__total_blocks": 0xFFFFFFFF}, {"lsm__num_ssts": 0xFFFFFFFF}]
    add(INV, n=(1 << 40) // per)
    add(INV, lsm__total_blocks=0xFFFFFFFE)
    add(INV, lsm__num_ssts=0xFFFFFFFE)
    if scan:
        limits += [{"ce": (1 << 40) + 1}, {"ckb": (1 << 44) + 1}]
        add(INV, ce=1 << 40)
        add(INV, ckb=1 << 44)
    for lim in limits:
        add(LIM, **lim)
        # a limit wins against the tree's arrays, the projections, the outputs' fields and the workspace ...
        add(LIM, lsm__ssts=None, **lim)
        add(LIM, lsm__block_base=None, **lim)
        add(LIM, ws=None, **lim)
        add(LIM, short_ws=True, **lim)
        add(LIM, out__summary=None, **lim)
        if scan:
            add(LIM, ranges__start_bytes=None, **lim)
        if has(entry, "chain"):
            add(LIM, chain__chain_start=None, **lim)
        if has(entry, "proj"):
            add(LIM, proj__n=2, **lim)
        if mem:
            add(LIM, mout__table=None, **lim)
        # ... and loses against a NULL top-level argument and the mem / chain pairing, which are checked first
        add(INV, out=None, **lim)
        if chain_needed:
            add(INV, chain=None, **lim)
        if has(entry, "fout"):
            add(INV, fout=None, **lim)
        if mem:
            add(INV, mout=None, **lim)
            add(INV, mchain=None, **lim)
            add(INV, mem__tables=None, **lim)
    if has(entry, "chain"):  # NULL out against NULL chain: one status either way
        add(INV, out=None, chain=None)
        add(INV, out__summary=None, chain__summary=None)
    return cases


@pytest.mark.parametrize("entry", sorted(SYMS))
def test_malformed_calls(lib, entry):
    for edits, want in malformed(entry):
        assert call(lib, entry, edits) == want, (entry, edits)


def wellformed(entry):
    """[edits] of `entry` that leave the call well-formed: it passes every host check."""
    scan, mem = "_scan" in entry, entry.endswith("_mem")
    cases = [{}, {"max_seq": None}, {"stream": None}]
    cases += [{a: None} for a in ("policies", "probe_len", "proj", "prefixes") if has(entry, a)]
    cases += [{"prefixes.probe_len": None}] if has(entry, "prefixes") else []
    if has(entry, "chain") and not entry.endswith("_merge"):  # no chain: no merge
        cases += [{"chain": None, "mchain": None} if mem else {"chain": None}]
    if has(entry, "chain"):  # no room for a link: the link columns may be NULL
        cases += [dict({"chain.cap_links": 0}, **{"chain." + f: None for f in CHAIN[1:-1]},
                       **({"mchain.table": None, "mchain.row": None} if mem else {}))]
    if mem:
        cases += [{"mem": None}, {"mem.num_tables": 0, "mem.tables": None}]
    # nothing to search: the arrays that only hold per-item values may be NULL
    none = {"n": 0, "ranges.start_bytes": None, "out.range_status": None, "out.range_ssts": None} if scan else \
        dict({"n": 0, "key_bytes": None, "key_off": None}, **{"out." + f: None for f in GET_OUT[:-1]})
    if scan and has(entry, "fout"):
        none.update({"fout.range_filtered": None, "fout.num_filtered": None, "prefixes.prefix_bytes": None})
    if mem:
        none.update({"mout.range_tables": None} if scan else {"mout.table": None, "mout.row": None})
    cases += [none, {"lsm.num_ssts": 0, "proj.n": 0, **{"lsm." + f: None for f in LSM_ARRAYS}}]
    if scan:  # no room for a row or a key byte
        cases += [dict({"out.cap_entries": 0, "out.key_arena_cap": 0, "out.key_arena": None},
                       **{"out." + f: None for f in ("sst",) + COLUMNS},
                       **({"mout.table": None, "mout.row": None} if mem else {}))]
    return cases


@pytest.mark.parametrize("entry", sorted(SYMS))
def test_wellformed_calls_need_a_device(lib, entry):
    if lib.sdb_device_count() > 0:  # with a device the call would go on to launch over these host arrays
        return
    for edits in wellformed(entry):
        assert call(lib, entry, edits) == DEV, (entry, edits)
