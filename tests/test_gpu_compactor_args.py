"""The argument checks of the five compaction job entry points (sdb_compactor_run, _run_merge, _run_ssts,
_run_ssts_merge, _run_ssts_ranged; sdb_compactor.cpp): the status of every malformed call, the order of the checks
where two apply, and the state a failed call leaves in the handle.  Every call goes through ctypes on one live handle
over two one-block SSTs of three rows each; where a limit needs a count, the arrays are zeroed structs (an empty run
or input is legal).  The last test runs one good job per entry point on that handle against the oracle."""
import ctypes as C
import types

import pytest

from oracle import oracle as O
from slatedb_amd import _abi, merge
from slatedb_amd.batch import Run

from . import ranged_compaction_cases as R
from .test_gpu_compaction import compact_both, compact_ssts_both
from .test_gpu_compaction_merge import merge_both
from .test_gpu_ranged_compaction import check

pytestmark = pytest.mark.gpu

OK, ARG, VER, LIM = _abi.SDB_OK, _abi.SDB_INVALID_ARGUMENT, _abi.SDB_INVALID_VERSION, _abi.SDB_LIMIT_EXCEEDED
RUNS, SSTS, RANGED = ("run", "run_merge"), ("run_ssts", "run_ssts_merge"), ("run_ssts_ranged",)
MERGE = ("run_merge", "run_ssts_merge")
MAX_RUNS2 = 32 * 32  # SDB_MAX_RUNS squared: two merge levels
ROWS = [[(b"a", 0, b"1", 6, None, None), (b"c", 0, b"3", 5, None, None), (b"e", 2, b"", 4, None, None)],
        [(b"a", 0, b"0", 3, None, None), (b"b", 0, b"2", 2, None, None), (b"e", 0, b"5", 1, None, None)]]
PRM = dict(block_size=4096)


@pytest.fixture(scope="module")
def rt():
    from slatedb_amd import runtime
    runtime.require_device()
    return runtime


@pytest.fixture(scope="module")
def x(rt):
    """The handle and the well-formed arguments every call starts from."""
    import torch
    runs = [Run.from_entries(r) for r in ROWS]
    job = R.build_job(runs, PRM)
    inputs = R.upload(job)
    assert [len(i.ikeys) for i in job.inputs] == [1, 1] and [i.num_entries for i in inputs] == [3, 3]
    views = [_abi.CompactionView(_abi.CompactionInput(i.data.data_ptr(), i.block_off.data_ptr(), 1, i.num_entries,
                                                      i.key_bytes, i.val_bytes),
                                 i.index_keys.data_ptr(), i.index_key_off.data_ptr()) for i in inputs]
    druns = [rt.DeviceRun.from_host(r) for r in runs]
    cb, state = rt.Compactor._operator_callback(merge.StringConcat)
    words = torch.zeros(64, dtype=torch.uint8, device="cuda")  # what a well-formed sdb_scan_ranges points at
    a = types.SimpleNamespace(comp=rt.Compactor(), inputs=inputs, views=views, druns=druns, cb=cb, keep=(state, words),
                              ret=O.retention(), prm=rt.params(**PRM), wal=rt.params(sst_type=_abi.SST_WAL, **PRM),
                              dummy=words.data_ptr())
    yield a
    a.comp.close()


def inputs_of(x, kind, n=2, edit=None):
    """The input array of an SST job: the two good inputs (`edit(array)` applied), or n zeroed structs."""
    ranged = kind in RANGED
    T = _abi.CompactionView if ranged else _abi.CompactionInput
    a = (T * max(n, 1))()
    if n == 2:
        for i, v in enumerate(x.views):
            a[i] = T.from_buffer_copy(bytes(v) if ranged else bytes(v.sst))
    if edit:
        edit(a)
    return a


def sst_of(kind, a, i):
    return a[i].sst if kind in RANGED else a[i]


def ranges(x, n, null=None):
    r = _abi.ScanRanges(n, *([x.dummy] * 6))
    if null:
        setattr(r, null, None)
    return r


def call(rt, x, kind, **kw):
    """One call of entry point `kind` with the good arguments, except those in kw.  -> (status, *num_ssts)"""
    ns = C.c_uint32(0)
    h = kw.get("h", x.comp.h)
    ret = kw.get("ret", C.byref(x.ret))
    tail = (kw.get("prm", C.byref(x.prm)), 1 << 30, None, kw.get("ns", C.byref(ns)))
    if kind in RUNS:
        n = kw.get("n", 2)
        runs = kw["runs"] if "runs" in kw else (_abi.Run * max(n, 1))(*([r.to_ctypes() for r in x.druns] if n == 2 else []))
        head = (runs, n)
    else:
        n = kw.get("n", 2)
        inputs = kw["inputs"] if "inputs" in kw else inputs_of(x, kind, n, kw.get("edit"))
        rs = kw.get("run_start")
        head = (inputs, n, None if rs is None else (C.c_uint32 * len(rs))(*rs), kw.get("nruns", n), kw.get("version", 2))
        if kind in RANGED:
            head += tuple(None if kw.get(k) is None else C.byref(kw[k]) for k in ("job_range", "proj"))
    op = ()
    if kind in MERGE:
        op = (kw.get("op", x.cb), None)
    elif kind in RANGED:
        op = (kw.get("op", _abi.MERGE_BATCH_FN()), None)
    st = getattr(rt.lib(), "sdb_compactor_" + kind)(h, *head, ret, *op, *tail)
    return st, ns.value


def fails(rt, x, kind, want, zeroed=True, **kw):
    """A call that fails on the host with `want`; `zeroed`: the handle then reports no SST, no merged entry and a
    zeroed summary (every failure the host detects behind the reset of the handle leaves it so; the ranged entry point
    checks ret, the input arrays and the ranges before the reset, and then leaves what the call before left)."""
    st, ns = call(rt, x, kind, **kw)
    assert (st, ns) == (want, 0), (kind, kw, st, ns)
    if zeroed:
        gm, sm = x.comp.merged()
        assert gm.n == 0 and bytes(sm) == bytes(_abi.MergeSummary())
        with pytest.raises(rt.SdbError):
            x.comp.sst(0)


# ---- the rows before "NULL ret": the status and *num_ssts only ----------------------------------------------------
@pytest.mark.parametrize("kind", MERGE)
def test_merge_entry_without_operator(rt, x, kind):
    """op == NULL at a _merge entry: SDB_INVALID_ARGUMENT, whatever the other arguments are."""
    null = _abi.MERGE_BATCH_FN()
    fails(rt, x, kind, ARG, zeroed=False, op=null)
    bad = dict(h=None, ret=None, prm=None, ns=None, op=null)
    if kind in RUNS:
        fails(rt, x, kind, ARG, zeroed=False, runs=None, **bad)
    else:
        fails(rt, x, kind, ARG, zeroed=False, inputs=None, version=0, run_start=[1, 0], nruns=1, **bad)


@pytest.mark.parametrize("kind", RUNS + SSTS + RANGED)
def test_null_handle_params_num_ssts(rt, x, kind):
    for kw in (dict(h=None), dict(prm=None), dict(ns=None)):
        fails(rt, x, kind, ARG, zeroed=False, **kw)


# ---- from "NULL ret" on: the handle reports nothing afterwards ----------------------------------------------------
@pytest.mark.parametrize("kind", RUNS + SSTS + RANGED)
def test_null_ret_or_sst_type(rt, x, kind):
    fails(rt, x, kind, ARG, ret=None)
    fails(rt, x, kind, ARG, prm=C.byref(x.wal))  # compactions write compacted SSTs
    if kind not in RUNS:
        fails(rt, x, kind, ARG, ret=None, version=3)  # before the version


@pytest.mark.parametrize("kind", RUNS + SSTS + RANGED)
def test_null_array(rt, x, kind):
    fails(rt, x, kind, ARG, **({"runs": None} if kind in RUNS else {"inputs": None}))


@pytest.mark.parametrize("kind", SSTS + RANGED)
def test_input_version(rt, x, kind):
    for v in (0, 3):
        fails(rt, x, kind, VER, version=v)
    fails(rt, x, kind, VER, version=0, n=MAX_RUNS2 + 1)  # the version before the limit


@pytest.mark.parametrize("kind", RUNS + SSTS + RANGED)
def test_run_limit(rt, x, kind):
    """SDB_MAX_RUNS^2 + 1 empty runs: SDB_LIMIT_EXCEEDED; SDB_MAX_RUNS^2: a job with nothing to write."""
    fails(rt, x, kind, LIM, n=MAX_RUNS2 + 1)
    if kind not in RUNS:  # the limit before run_start
        fails(rt, x, kind, LIM, run_start=[1] + [2] * (MAX_RUNS2 + 1), nruns=MAX_RUNS2 + 1)
    st, ns = call(rt, x, kind, n=MAX_RUNS2)
    assert (st, ns) == (OK, 0), (kind, st, ns)
    gm, sm = x.comp.merged()
    assert gm.n == 0 and sm.status == OK and sm.num_in == 0


@pytest.mark.parametrize("kind", SSTS + RANGED)
def test_run_start(rt, x, kind):
    for rs in ([1, 1, 2], [0, 1, 3], [0, 1, 1]):  # [0] != 0; [nruns] != ninputs (above, below)
        fails(rt, x, kind, ARG, run_start=rs, nruns=2)
    fails(rt, x, kind, ARG, run_start=[0, 2, 1, 2], nruns=3)  # a decreasing pair


@pytest.mark.parametrize("kind", SSTS + RANGED)
def test_input_with_blocks_and_null_array(rt, x, kind):
    fields = ("data", "block_off") + (("index_keys", "index_key_off") if kind in RANGED else ())
    for f in fields:
        def edit(a, f=f):
            setattr(a[1] if f.startswith("index") else sst_of(kind, a, 1), f, None)
        fails(rt, x, kind, ARG, edit=edit)
    # with a bad version too: the whole-SST job checks the version first, the ranged job its inputs (on entry)
    fails(rt, x, kind, ARG if kind in RANGED else VER, version=3, edit=lambda a: setattr(sst_of(kind, a, 1), "data", None))


@pytest.mark.parametrize("kind", SSTS + RANGED)
def test_declared_entries_limit(rt, x, kind):
    def edit(a):
        sst_of(kind, a, 0).num_entries = sst_of(kind, a, 1).num_entries = 1 << 30
    fails(rt, x, kind, LIM, edit=edit)


@pytest.mark.parametrize("kind", SSTS)
def test_null_data_before_declared_entries(rt, x, kind):
    def edit(a):
        a[0].num_entries = 1 << 31
        a[1].data = None
    fails(rt, x, kind, ARG, edit=edit)


def test_ranges_shape(rt, x):
    """job_range->n != 1, proj->n != ninputs, a NULL array inside either: checked on entry, before the handle is read."""
    kind = RANGED[0]
    for n in (0, 2):
        fails(rt, x, kind, ARG, job_range=ranges(x, n))
    for n in (0, 1, 3):
        fails(rt, x, kind, ARG, proj=ranges(x, n))
    for f, _ in _abi.ScanRanges._fields_[1:]:
        fails(rt, x, kind, ARG, job_range=ranges(x, 1, null=f))
        fails(rt, x, kind, ARG, proj=ranges(x, 2, null=f))


# ---- a failed call leaves the handle usable ------------------------------------------------------------------------
def test_good_jobs_after_failures(rt, x):
    """One good job per entry point on the handle of the calls above, each against the oracle; then what a NULL `ret`
    leaves of a good job's results: the ranged entry point returns before it touches the handle, the others reset it."""
    ret = O.retention(min_seq=2)
    runs = [Run.from_entries(r) for r in ROWS]
    compact_both(rt, runs, ret, PRM, 1 << 20, comp=x.comp)
    st, ns, _ = compact_ssts_both(rt, runs, ret, PRM, 1 << 20, comp=x.comp)
    assert (st, ns) == (OK, 1)
    mrows = [[(b"a", 1, b"x", 6, None, None), (b"c", 0, b"3", 5, None, None)], [(b"a", 1, b"y", 3, None, None), (b"a", 0, b"z", 2, None, None)]]
    for ssts in (False, True):
        merge_both(rt, mrows, O.retention(min_seq=0, time_seq=0), merge.StringConcat, prm_kw=PRM, comp=x.comp, ssts=ssts)
    small = R.small_job()
    ns, _, gm, _ = check(rt, x.comp, small, R.upload(small), what="after failures")
    assert ns >= 1 and gm.n > 0
    fails(rt, x, RANGED[0], ARG, zeroed=False, ret=None)
    assert x.comp.merged()[0].n == gm.n
    fails(rt, x, SSTS[0], ARG, ret=None)
