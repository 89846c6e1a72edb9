"""The four job methods of slatedb_amd.runtime.Compactor over a stub library, without a device: which C symbol each
calls, the order and the values of its arguments (the run count, nruns from run_start and from its absence, the input
version, max_sst_size, the stream), that only the merge forms pass a callback with a NULL context and set
operator_state, and that the status is stored and returned with the SST count the library wrote (the literals below are
the calls of the methods before run / run_merge and run_ssts / run_ssts_merge shared their marshalling)."""
import ctypes as C
from types import SimpleNamespace

import pytest

from slatedb_amd import _abi, runtime as rt

HANDLE = 0x5DB0
SSTS = 7  # what the stub writes into *num_ssts
MAX_SST = 123456789
STREAM = 0xABC0


class Ten:
    """A stand-in for a device tensor."""

    def __init__(self, ptr, numel=0):
        self.ptr, self.n = ptr, numel

    def data_ptr(self):
        return self.ptr

    def numel(self):
        return self.n


class Lib:
    def __init__(self, status=0):
        self.status, self.calls = status, []

    def sdb_compactor_create(self, device):
        return HANDLE

    def sdb_compactor_destroy(self, handle):
        assert handle == HANDLE

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            C.cast(args[-1], C.POINTER(C.c_uint32))[0] = SSTS  # byref(num_ssts)
            return self.status
        return entry


class Operator:
    def merge_batch(self, key, existing, operands):
        return (existing or b"") + b"".join(operands)


def runs(k):
    return [rt.DeviceRun(10 + r, *[Ten(0x1000 * (r + 1) + 8 * f) for f in range(9)], 0, 0) for r in range(k)]


def inputs(k):
    return [SimpleNamespace(data=Ten(0x100000 * (i + 1)), block_off=Ten(0x200000 * (i + 1), 4 + i), num_entries=50 + i,
                            key_bytes=500 + i, val_bytes=5000 + i) for i in range(k)]


@pytest.fixture
def compactor(monkeypatch):
    """compactor(status) -> (a Compactor over a stub library that answers `status`, the stub); closed while the stub
    is still in place."""
    made = []

    def make(status=0):
        lib = Lib(status)
        monkeypatch.setattr(rt, "lib", lambda: lib)
        monkeypatch.setattr(rt, "require_device", lambda: None)
        c = rt.Compactor()
        made.append(c)
        assert c.h == HANDLE and not lib.calls
        return c, lib
    yield make
    for c in made:
        c.close()
        assert c.h is None


def deref(arg, ctype):
    assert type(arg._obj) is ctype
    return arg._obj


def check_tail(args, ret, prm, merge, op_state):
    """What follows the inputs in every job: ret, [callback, NULL context,] params, max_sst_size, stream, num_ssts."""
    assert deref(args[0], _abi.Retention) is ret
    if merge:
        assert isinstance(args[1], _abi.MERGE_BATCH_FN) and args[2] is None
        assert set(op_state) == {"result", "error"} and op_state["result"] is None and op_state["error"] is None
        args = args[:1] + args[3:]
    assert len(args) == 5 and not any(isinstance(a, _abi.MERGE_BATCH_FN) for a in args)
    assert deref(args[1], _abi.SstParams) is prm
    assert args[2] == MAX_SST and args[3] == STREAM
    assert type(args[4]._obj) is C.c_uint32


@pytest.mark.parametrize("status", [0, _abi.SDB_INVALID_ARGUMENT])
@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("nruns", [0, 1, 3])
def test_run_wrappers(compactor, nruns, merge, status):
    c, lib = compactor(status)
    ret, prm, dr = _abi.Retention(), rt.params(), runs(nruns)
    if merge:
        got = c.run_merge(dr, ret, Operator(), prm, MAX_SST, stream=STREAM)
    else:
        got = c.run(dr, ret, prm, MAX_SST, stream=STREAM)
    assert got == (status, SSTS) and c.status == status
    assert hasattr(c, "operator_state") == merge
    (name, args), = lib.calls
    assert name == ("sdb_compactor_run_merge" if merge else "sdb_compactor_run")
    assert len(args) == (10 if merge else 8)
    assert args[0] == HANDLE and args[2] == nruns
    cr = args[1]
    assert cr._type_ is _abi.Run and len(cr) == max(nruns, 1)
    for r in range(nruns):
        assert cr[r].n == 10 + r
        assert [getattr(cr[r], f) for f, _ in _abi.Run._fields_[1:]] == [0x1000 * (r + 1) + 8 * f for f in range(9)]
    check_tail(args[3:], ret, prm, merge, getattr(c, "operator_state", None))


@pytest.mark.parametrize("status", [0, _abi.SDB_LIMIT_EXCEEDED])
@pytest.mark.parametrize("merge", [False, True])
@pytest.mark.parametrize("ninputs,run_start,nruns", [(0, None, 0), (3, None, 3), (4, [0, 1, 4], 2), (2, [0, 0, 2, 2], 3)])
def test_run_ssts_wrappers(compactor, ninputs, run_start, nruns, merge, status):
    c, lib = compactor(status)
    ret, prm, ins = _abi.Retention(), rt.params(), inputs(ninputs)
    if merge:
        got = c.run_ssts_merge(ins, ret, Operator(), prm, MAX_SST, input_version=1, run_start=run_start, stream=STREAM)
    else:
        got = c.run_ssts(ins, ret, prm, MAX_SST, input_version=1, run_start=run_start, stream=STREAM)
    assert got == (status, SSTS) and c.status == status
    assert hasattr(c, "operator_state") == merge
    (name, args), = lib.calls
    assert name == ("sdb_compactor_run_ssts_merge" if merge else "sdb_compactor_run_ssts")
    assert len(args) == (13 if merge else 11)
    assert args[0] == HANDLE and args[2] == ninputs and args[4] == nruns and args[5] == 1
    ci = args[1]
    assert ci._type_ is _abi.CompactionInput and len(ci) == max(ninputs, 1)
    for i in range(ninputs):
        assert (ci[i].data, ci[i].block_off, ci[i].num_blocks) == (0x100000 * (i + 1), 0x200000 * (i + 1), 3 + i)
        assert (ci[i].num_entries, ci[i].key_bytes, ci[i].val_bytes) == (50 + i, 500 + i, 5000 + i)
    if run_start is None:
        assert args[3] is None
    else:
        assert args[3]._type_ is C.c_uint32 and list(args[3]) == run_start
    check_tail(args[6:], ret, prm, merge, getattr(c, "operator_state", None))


def test_defaults(compactor):
    """input_version 2, no run_start and no stream unless given."""
    c, lib = compactor()
    ret, prm = _abi.Retention(), rt.params()
    c.run(runs(1), ret, prm, MAX_SST)
    c.run_merge(runs(1), ret, Operator(), prm, MAX_SST)
    c.run_ssts(inputs(2), ret, prm, MAX_SST)
    c.run_ssts_merge(inputs(2), ret, Operator(), prm, MAX_SST)
    (_, a), (_, b), (_, s), (_, t) = lib.calls
    assert a[6] is None and b[8] is None and s[9] is None and t[11] is None
    assert (s[3], s[4], s[5]) == (None, 2, 2) and (t[3], t[4], t[5]) == (None, 2, 2)


def test_operator_callback(compactor):
    """The callback the merge forms pass reaches the operator, and operator_state keeps its result and its error."""
    c, lib = compactor()
    c.run_merge(runs(1), _abi.Retention(), Operator(), rt.params(), MAX_SST)
    cb = lib.calls[0][1][4]
    key, ex, o1, o2 = (C.c_uint8 * 1)(107), (C.c_uint8 * 2)(98, 99), (C.c_uint8 * 1)(120), (C.c_uint8 * 2)(121, 122)
    ops = (_abi.u8p * 2)(C.cast(o1, _abi.u8p), C.cast(o2, _abi.u8p))
    lens = (C.c_uint64 * 2)(1, 2)
    res, rl = _abi.u8p(), C.c_uint64(0)
    assert cb(None, key, 1, ex, 2, ops, lens, 2, C.byref(res), C.byref(rl)) == 0
    assert C.string_at(res, rl.value) == b"bcxyz" and c.operator_state["error"] is None
    assert bytes(c.operator_state["result"]) == b"bcxyz"

    class Bad:
        def merge_batch(self, key, existing, operands):
            raise ValueError("no")
    c.run_merge(runs(1), _abi.Retention(), Bad(), rt.params(), MAX_SST)
    cb = lib.calls[1][1][4]
    assert cb(None, key, 1, None, 0, ops, lens, 2, C.byref(res), C.byref(rl)) == 1
    assert isinstance(c.operator_state["error"], ValueError)
