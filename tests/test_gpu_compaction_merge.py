"""GPU parity of compaction with a merge operator (sdb_compactor_run_merge / sdb_compactor_run_ssts_merge;
k_mg_chain, k_mg_chain_scan, k_mg_chain_emit and the unit forms of k_mg_keys / k_mg_emit in sdb_compact.hip, the
host fold in sdb_compactor.cpp) against the model of tests/compaction_merge_cases.py in front of the pinned C
oracle: Compactor.merged() field by field and every output SST byte for byte, and merge_stats()."""
import ctypes as C
import os
import random
import types

import numpy as np
import pytest

from oracle import oracle as O
from slatedb_amd import _abi, merge
from slatedb_amd.batch import Batch, Run

from . import compaction_merge_cases as CM
from .compaction_merge_cases import Bracket, M, T, V
from .test_compaction_oracle import rand_runs
from .test_gpu_compaction import assert_batch_same, sst_view
from .test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu
PRM = dict(block_size=4096, bloom_bits_per_key=10)
STATS = ("groups", "links", "link_bytes", "merged_bytes", "operator_calls")


@pytest.fixture(scope="module")
def rt():
    from slatedb_amd import runtime
    runtime.require_device()
    return runtime


def encoded_inputs(rt, runs, prm_kw, split=1):
    """Each run encoded by the oracle as `split` consecutive SSTs (merge operands kept as such), uploaded:
    (inputs, run_start)."""
    import torch
    inputs, run_start = [], [0]
    for r in runs:
        kind = np.where(r.flags & _abi.FLAG_TOMBSTONE, T, np.where(r.flags & _abi.FLAG_MERGE_OPERAND, M, V)).astype(np.uint8)
        mask = (np.where(r.flags & _abi.FLAG_HAS_EXPIRE_TS, _abi.TS_EXPIRE, 0) |
                np.where(r.flags & _abi.FLAG_HAS_CREATE_TS, _abi.TS_CREATE, 0)).astype(np.uint8)
        end = r.val_off[-1] + r.val_len[-1] if r.n else 0
        b = Batch(r.key_arena, r.key_off, r.val_base, np.concatenate([r.val_off, [end]]).astype(np.uint64), kind, r.seq,
                  r.create_ts, r.expire_ts, mask)
        cuts = np.linspace(0, b.n, split + 1).astype(int)
        for i in range(split):
            enc = O.encode_sst(b.slice(cuts[i], cuts[i + 1]), O.params(**prm_kw))
            sm = enc.summary
            assert sm.status == 0
            inputs.append(types.SimpleNamespace(
                data=torch.from_numpy(np.concatenate([enc.data, np.zeros(16, np.uint8)])).cuda(),
                block_off=torch.from_numpy(enc.block_off.view(np.int64)).cuda(),
                num_entries=int(sm.num_entries), key_bytes=int(sm.raw_key_size), val_bytes=int(sm.raw_val_size)))
        run_start.append(len(inputs))
    return inputs, run_start


def check_outputs(comp, st, ns, ref, what=""):
    merged, msum, cuts, ssts = ref
    assert st == msum.status == 0, (what, st, msum.status)
    gm, gsm = comp.merged()
    assert_batch_same(gm, merged, what + " merged")
    for f in ("num_out", "key_bytes", "val_bytes", "expired_values", "expired_merges"):
        assert getattr(gsm, f) == getattr(msum, f), (what, f)
    assert ns == len(ssts), (what, ns, len(ssts))
    for i, r in enumerate(ssts):
        d = comp.sst(i)
        assert (d["entry_start"], d["entry_end"]) == (cuts[i], cuts[i + 1])
        assert_same(r, sst_view(d), "%s sst %d" % (what, i))
    return gsm


def merge_both(rt, runs, ret, op, prm_kw=PRM, max_sst=1 << 20, comp=None, ssts=False, what=""):
    """run_merge (or, `ssts`, run_ssts_merge over the runs encoded as one SST each) against the model; returns the
    job's stats and merged summary."""
    import torch
    own = comp is None
    comp = comp or rt.Compactor()
    hruns = [Run.from_entries(r) for r in runs]
    if ssts:
        inputs, _ = encoded_inputs(rt, hruns, prm_kw)
        st, ns = comp.run_ssts_merge(inputs, ret, op, rt.params(**prm_kw), max_sst)
    else:
        st, ns = comp.run_merge([rt.DeviceRun.from_host(r) for r in hruns], ret, op, rt.params(**prm_kw), max_sst)
    torch.cuda.synchronize()
    want = {}
    ref = CM.expected(runs, ret, O.params(**prm_kw), max_sst, op, want)
    gsm = check_outputs(comp, st, ns, ref, what)
    ms = comp.merge_stats()
    for f in STATS:
        assert getattr(ms, f) == want[f], (what, f, getattr(ms, f), want[f])
    if own:
        comp.close()
    return ms, gsm


@pytest.mark.parametrize("case", CM.FIXTURE, ids=[c["name"] for c in CM.FIXTURE])
def test_reference_cases(rt, case):
    ret = O.retention(min_seq=case["barrier"], time_seq=0)  # a time window over every seq: retention keeps all
    run = CM.fixture_run(case)
    merge_both(rt, [run], ret, merge.StringConcat)
    comp = rt.Compactor()
    comp.run_merge([rt.DeviceRun.from_host(Run.from_entries(run))], ret, merge.StringConcat, rt.params(**PRM), 1 << 20)
    from .test_compaction_oracle import entries_of
    assert [(k, kind, v, s, x) for k, kind, v, s, _, x in entries_of(comp.merged()[0])] == \
        [(k, kind, v, s, x) for k, kind, v, s, _, x in CM.fixture_entries(case["expected"])]
    comp.close()


PARTITION = {
    "expiry_interleaved": ([(b"k", M, b"a", 9, None, None), (b"k", M, b"b", 8, None, 5), (b"k", M, b"c", 7, None, 5),
                            (b"k", M, b"d", 6, None, 7), (b"k", M, b"e", 5, None, None), (b"k", M, b"f", 4, None, None),
                            (b"k", M, b"g", 3, None, 7), (b"k", M, b"h", 2, None, 5)], None),
    "value_other_expiry_is_no_base": ([(b"k", M, b"a", 5, None, 9), (b"k", M, b"b", 4, None, 9),
                                       (b"k", V, b"v", 3, None, 8), (b"k", V, b"w", 2, None, 8)], None),
    "tombstone_base_create_ts": ([(b"k", M, b"x", 3, 10, None), (b"k", M, b"y", 2, 5, None), (b"k", T, b"", 1, 30, None)],
                                 None),
    "chain_base_chain": ([(b"k", M, b"4", 6, None, None), (b"k", M, b"3", 5, None, None), (b"k", V, b"2", 4, None, None),
                          (b"k", M, b"1", 3, None, None), (b"k", M, b"0", 2, None, None)], None),
    "barrier_at_an_operand": ([(b"k", M, b"4", 4, None, None), (b"k", M, b"3", 3, None, None),
                               (b"k", M, b"2", 2, None, None), (b"k", V, b"1", 1, None, None)], 3),
    "barrier_below_an_operand": ([(b"k", M, b"4", 4, None, None), (b"k", M, b"3", 3, None, None),
                                  (b"k", M, b"2", 2, None, None), (b"k", V, b"1", 1, None, None)], 2),
}


@pytest.mark.parametrize("name", list(PARTITION))
def test_partition_rules(rt, name):
    run, barrier = PARTITION[name]
    # one key alone, then between neighbours (its versions no longer start the stream or end it)
    for runs in ([run], [[(b"a", V, b"", 50, None, None)] + run + [(b"z", M, b"q", 60, None, None)]]):
        ms, _ = merge_both(rt, runs, O.retention(min_seq=barrier, time_seq=0), Bracket, what=name)
        assert ms.groups >= 1


def boundary_runs(L, at, nruns):
    """Counter keys, one version each, around one key whose chain of L links (L - 1 operands over a value) covers
    merged position `at`, its links dealt over `nruns` runs; then a key of 201 operands; then more counters."""
    start = max(1, at - L // 2)
    key = lambda i: b"key%08d" % i
    runs = [[] for _ in range(nruns)]
    seq = 10 ** 6
    for i in range(start):
        runs[i % nruns].append((key(i), V, b"f%d" % i, seq, None, None))
        seq -= 1
    for j in range(L):
        runs[j % nruns].append((key(start), M if j < L - 1 else V, b"%d" % j, seq, None, None))
        seq -= 1
    for j in range(201):
        runs[(j * 7) % nruns].append((key(start + 1), M, b"%d" % j, seq, None, None))
        seq -= 1
    for i in range(start + 2, start + 40):
        runs[i % nruns].append((key(i), M if i % 5 == 0 else V, b"t%d" % i, seq, None, None))
        seq -= 1
    return runs, start


@pytest.mark.parametrize("nruns", [1, 3, 8])
@pytest.mark.parametrize("at", [64, 256, 1024])
@pytest.mark.parametrize("L", [63, 65, 257, 1025])
def test_parallel_shape_boundaries(rt, L, at, nruns):
    runs, start = boundary_runs(L, at, nruns)
    assert start < at < start + L
    ms, _ = merge_both(rt, runs, O.retention(), Bracket, what="L%d at%d runs%d" % (L, at, nruns))
    tail_ops = sum(1 for i in range(start + 2, start + 40) if i % 5 == 0)
    # per group: ceil(operand links / 100) + 1, the base not counted
    assert ms.operator_calls == (-(-(L - 1) // 100) + 1) + (3 + 1) + 2 * tail_ops
    assert ms.groups == 2 + tail_ops and ms.links == L + 201 + tail_ops


def test_zero_length_operands_and_bases(rt):
    run = [(b"a", M, b"", 9, None, None), (b"a", M, b"", 8, None, None), (b"a", V, b"", 7, None, None),
           (b"b", M, b"", 6, None, None), (b"c", M, b"x", 5, None, None), (b"c", M, b"", 4, None, None),
           (b"c", T, b"", 3, None, None), (b"d", M, b"", 2, None, None), (b"d", V, b"yy", 1, None, None)]
    for op in (merge.StringConcat, Bracket):
        ms, _ = merge_both(rt, [run], O.retention(), op)
        assert ms.groups == 4 and ms.link_bytes == 3
    assert ms.merged_bytes > 0


class Blowup:
    """A merged value far longer than its inputs: 1000 bytes per input byte."""

    @staticmethod
    def merge_batch(key, existing, operands):
        return (existing or b"") + b"".join(o if len(o) > 8 else o * 1000 for o in operands)


@pytest.mark.parametrize("ssts", [False, True], ids=["run_merge", "run_ssts_merge"])
def test_merged_value_larger_than_every_input(rt, ssts):
    big = [(b"big", M, bytes([65 + j]) * 2, 300 - j, None, None) for j in range(100)]
    runs = [[(b"a%03d" % i, V, b"v%d" % i, 900 - i, None, None) for i in range(40)] + big[:50],
            big[50:] + [(b"z%03d" % i, V, b"w", 100 - i, None, None) for i in range(40)]]
    inputs = sum(len(e[2]) for r in runs for e in r)
    ms, gsm = merge_both(rt, runs, O.retention(), Blowup, ssts=ssts, max_sst=64 << 10)
    assert ms.merged_bytes == 200 * 1000 and ms.merged_bytes > 100 * inputs // 2 and gsm.val_bytes > inputs


def test_retention_interplay(rt):
    # a merged unit at or under min_seq followed by older versions: the walk stops at it only when it has a base
    run = [(b"a", M, b"3", 30, None, None), (b"a", M, b"2", 20, None, None), (b"a", V, b"1", 10, None, None),
           (b"a", V, b"0", 5, None, None), (b"b", M, b"3", 31, None, None), (b"b", M, b"2", 21, None, 7),
           (b"b", V, b"1", 11, None, None), (b"b", V, b"0", 6, None, None)]
    _, gsm = merge_both(rt, [run], O.retention(min_seq=40), Bracket)
    assert gsm.num_out == 4  # a: the Value unit; b: the Merge unit, the Merge operand, then the first value
    # filter_tombstone with a key whose only survivor is a converted expired value
    run = [(b"a", M, b"2", 9, None, 50), (b"a", V, b"1", 8, None, 50), (b"b", V, b"keep", 7, None, None),
           (b"c", M, b"x", 6, None, 50), (b"c", T, b"", 5, None, 50)]
    _, gsm = merge_both(rt, [run], O.retention(compaction_start_ts=100, filter_tombstone=True), Bracket)
    assert (gsm.num_out, gsm.expired_values, gsm.expired_merges) == (1, 2, 0)
    # an expired all-operand chain counts once
    run = [(b"a", M, b"3", 9, None, 50), (b"a", M, b"2", 8, None, 50), (b"a", M, b"1", 7, None, 50),
           (b"b", V, b"keep", 6, None, None)]
    _, gsm = merge_both(rt, [run], O.retention(compaction_start_ts=100), Bracket)
    assert (gsm.num_out, gsm.expired_values, gsm.expired_merges) == (1, 0, 1)


@pytest.mark.parametrize("seed", range(10))
def test_random(rt, seed):
    rng = random.Random(500 + seed)
    runs = rand_runs(rng, rng.randrange(1, 9), 300, 5, merge=0.4, dup_seq=seed % 3 == 0)
    ret = O.retention(min_seq=rng.choice([None, 0, 200, 700]), time_seq=rng.choice([None, 0, 400]),
                      compaction_start_ts=rng.choice([0, 1000, 5000]), filter_tombstone=bool(rng.randrange(2)))
    merge_both(rt, runs, ret, Bracket if seed % 2 else merge.StringConcat, what="seed %d" % seed)


def test_no_operands_equals_plain_job(rt):
    from .test_gpu_compaction import compact_both
    rng = random.Random(77)
    runs = rand_runs(rng, 4, 300, 4, merge=0.0)
    ret = O.retention(min_seq=300, compaction_start_ts=1000, filter_tombstone=True)
    comp = rt.Compactor()
    ms, _ = merge_both(rt, runs, ret, Bracket, comp=comp)
    assert ms.operator_calls == 0 and ms.groups == 0
    compact_both(rt, [Run.from_entries(r) for r in runs], ret, PRM, 1 << 20, comp=comp)  # sdb_compactor_run: same oracle
    assert comp.merge_stats().groups == 0
    comp.close()


def test_encoded_inputs(rt):
    """3 input SSTs in 2 runs (encode -> device decode -> merge): equals run_merge over the same entries."""
    import torch
    rng = random.Random(5)
    runs = rand_runs(rng, 2, 200, 5, tomb=0.1, merge=0.4, expire=0.0)
    hruns = [Run.from_entries(r) for r in runs]
    comp = rt.Compactor()
    ret = O.retention(min_seq=150, filter_tombstone=True)
    inputs, _ = encoded_inputs(rt, hruns, PRM, split=1)
    in3, _ = encoded_inputs(rt, hruns[:1], PRM, split=2)
    inputs = in3 + inputs[1:]
    st, ns = comp.run_ssts_merge(inputs, ret, Bracket, rt.params(**PRM), 16 << 10, run_start=[0, 2, 3])
    torch.cuda.synchronize()
    want = {}
    check_outputs(comp, st, ns, CM.expected(runs, ret, O.params(**PRM), 16 << 10, Bracket, want), "ssts")
    a, ms = comp.merged()[0], comp.merge_stats()
    assert ms.groups == want["groups"] > 0 and ms.operator_calls == want["operator_calls"]
    st, ns2 = comp.run_merge([rt.DeviceRun.from_host(r) for r in hruns], ret, Bracket, rt.params(**PRM), 16 << 10)
    assert st == 0 and ns2 == ns
    assert_batch_same(comp.merged()[0], a, "run_merge vs run_ssts_merge")
    comp.close()


def test_more_than_32_runs(rt):
    rng = random.Random(33)
    runs, seq = [], 1000
    for r in range(33):
        es = []
        for k in rng.sample([b"k1", b"k2", b"m%02d" % r], rng.randrange(1, 4)):
            es.append((k, M if k[:1] == b"k" and rng.random() < 0.8 else V, b"%d" % seq, seq, None, None))
            seq -= 1
        runs.append(sorted(es, key=lambda e: (e[0], -e[3])))
    ms, _ = merge_both(rt, runs, O.retention(), Bracket)
    assert ms.groups >= 2
    ms, _ = merge_both(rt, runs, O.retention(), Bracket, ssts=True)
    assert ms.groups >= 2


class FailOn:
    def __init__(self, key):
        self.key = key

    def merge_batch(self, key, existing, operands):
        if key == self.key:
            raise ValueError("operator failure on %r" % key)
        return Bracket.merge_batch(key, existing, operands)


def test_operator_failure(rt):
    run = [(b"a", V, b"0", 9, None, None), (b"b", M, b"2", 8, None, None), (b"b", M, b"1", 7, None, None),
           (b"c", V, b"x", 6, None, None), (b"d", M, b"2", 5, None, None), (b"d", V, b"1", 4, None, None),
           (b"e", M, b"9", 3, None, None)]
    comp = rt.Compactor()
    st, ns = comp.run_merge([rt.DeviceRun.from_host(Run.from_entries(run))], O.retention(), FailOn(b"d"),
                            rt.params(**PRM), 1 << 20)
    assert st == _abi.SDB_MERGE_OPERATOR_ERROR and ns == 0
    _, sm = comp.merged()
    heads = []
    CM.collapse([run], None, Bracket, heads=heads)
    assert sm.status == _abi.SDB_MERGE_OPERATOR_ERROR and sm.first_error_entry == heads[1] == 4
    assert isinstance(comp.operator_state["error"], ValueError)
    merge_both(rt, [run], O.retention(), Bracket, comp=comp)  # the next job on the handle succeeds
    comp.close()


def test_more_tiles_than_scan_threads(rt):
    """512 * 1024 + 2 entries: one tile more than k_mg_scan / k_mg_chain_scan scan in a pass (512 tiles of 1024
    positions), so the tile offsets of the last tile come from the second pass of the shared tile scan.  Every key
    an operand over a value; the columns and the stats in closed form."""
    import torch
    n = 512 * 1024 + 2
    m = n // 2
    keys = np.arange(m, dtype=">u4")
    flags = np.tile(np.array([_abi.FLAG_MERGE_OPERAND, 0], np.uint8), m)  # seq 2: the operand, seq 1: the value
    vals = np.empty(n, np.uint8)
    vals[0::2] = (np.arange(m) % 251).astype(np.uint8)  # operand of key i
    vals[1::2] = (np.arange(m) % 241).astype(np.uint8)  # base value of key i
    zeros = np.zeros(n, np.int64)
    run = Run(np.repeat(keys, 2).view(np.uint8), 4 * np.arange(n + 1), vals, np.arange(n), np.ones(n, np.uint32),
              np.tile(np.array([2, 1], np.uint64), m), flags, zeros, zeros)
    comp = rt.Compactor()
    st, ns = comp.run_merge([rt.DeviceRun.from_host(run)], O.retention(), merge.StringConcat, rt.params(**PRM), 1 << 30)
    torch.cuda.synchronize()
    assert st == 0 and ns == 1
    got, sm = comp.merged()
    assert (sm.status, sm.num_in, sm.num_out, sm.key_bytes, sm.val_bytes) == (0, n, m, 4 * m, 2 * m)
    assert (sm.expired_values, sm.expired_merges) == (0, 0)
    assert got.n == m
    assert np.array_equal(got.key_bytes, keys.view(np.uint8)) and np.array_equal(got.key_off, 4 * np.arange(m + 1))
    # StringConcat: the base value, then the operand
    assert np.array_equal(got.val_bytes.reshape(m, 2), np.stack([vals[1::2], vals[0::2]], axis=1))
    assert np.array_equal(got.val_off, 2 * np.arange(m + 1))
    assert np.all(got.kind == V) and np.all(got.seq == 2) and not got.ts_mask.any()
    assert not got.create_ts.any() and not got.expire_ts.any()
    ms = comp.merge_stats()
    assert (ms.groups, ms.links, ms.link_bytes, ms.merged_bytes) == (m, n, n, n)
    assert ms.operator_calls == 2 * m  # per chain: its one operand batch, then the batch results with the base
    comp.close()


@pytest.mark.parametrize("total", [1, 255, 256, 257, 1025])
def test_workspace_canaries(rt, total):
    """The buffers of the merge-operator step (per-position chain state, chain tables and staging arena, merged
    upload) sized exactly, between guard bands, everything filled with 0xA5: the outputs are the model's and no
    guard byte changes."""
    cd = C.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slatedb_amd",
                             "libslatedb_amd.so"))
    cd.sdb_diag_compactor_canaries.restype = None
    cd.sdb_diag_compactor_canaries.argtypes = [C.c_void_p, C.c_int]
    cd.sdb_diag_compactor_canary_damage.restype = C.c_int64
    cd.sdb_diag_compactor_canary_damage.argtypes = [C.c_void_p]
    # every third key a chain of three links, the last key's chain ending the stream
    run, seq, i = [], 10 ** 6, 0
    while len(run) < total:
        k = b"key%06d" % i
        n = min(3, total - len(run)) if i % 3 == 2 or total - len(run) <= 3 else 1
        for j in range(n):
            # several versions: operands over a value; one version: an operand (a chain of one link) or a value
            kind = (M if j < n - 1 else V) if n > 1 else (M if i % 2 or total == 1 else V)
            run.append((k, kind, b"v%d" % seq, seq, None, None))
            seq -= 1
        i += 1
    assert len(run) == total
    comp = rt.Compactor()
    cd.sdb_diag_compactor_canaries(comp.h, 1)
    ms, _ = merge_both(rt, [run[::2], run[1::2]] if total > 1 else [run], O.retention(), Bracket, comp=comp)
    assert ms.groups > 0
    assert cd.sdb_diag_compactor_canary_damage(comp.h) == 0
    comp.close()
