"""GPU parity of the ranged compaction (sdb_compactor_run_ssts_ranged; k_rx_cover, k_rx_clip, k_rx_gate and
k_rx_compact in sdb_compact_range.hip, run_ranged_job in sdb_compactor.cpp) against rules R1-R8 of
include/slatedb_amd.h as tests/ranged_compaction_cases.py restates them in front of the pinned C oracle: the merged
stream field by field, the cut list, every output SST byte for byte, and range_stats() exactly."""
import copy
import ctypes as C
import os
import random

import numpy as np
import pytest

from oracle import oracle as O
from slatedb_amd import _abi
from slatedb_amd import subcompaction as S
from slatedb_amd.batch import Run

from . import ranged_compaction_cases as R
from .compaction_merge_cases import Bracket
from .scan_cases import EXC, INC, U
from .test_compaction_oracle import rand_runs
from .test_gpu_compaction import assert_batch_same, sst_view
from .test_gpu_parity import assert_same
from .test_subcompaction import merged_entries

pytestmark = pytest.mark.gpu
OUT = dict(block_size=512, bloom_bits_per_key=10)
STATS = ("inputs_read", "blocks_total", "blocks_checked", "entries_decoded", "entries_in")
SUMMARY = ("num_out", "key_bytes", "val_bytes", "expired_values", "expired_merges")
ABOVE = b"\xff" * 17


def retention():
    return O.retention(min_seq=3000, compaction_start_ts=1000, filter_tombstone=True)


@pytest.fixture(scope="module")
def rt():
    from slatedb_amd import runtime
    runtime.require_device()
    return runtime


@pytest.fixture(scope="module")
def small(rt):
    job = R.small_job()
    return job, R.upload(job)


@pytest.fixture(scope="module")
def comp(rt):
    c = rt.Compactor()
    yield c
    c.close()


def run(rt, comp, job, inputs, job_range=None, projections=None, ret=None, op=None):
    import torch
    st, ns = comp.run_ssts_ranged(inputs, ret or retention(), rt.params(**OUT), R.MAX_SST, job_range, projections, operator=op,
                                  input_version=job.version, run_start=job.run_start)
    torch.cuda.synchronize()
    return st, ns


def check(rt, comp, job, inputs, job_range=None, projections=None, ret=None, op=None, what=""):
    """One ranged job against its expected value; returns (num_ssts, range stats, merged stream, merge-op stats)."""
    ret = ret or retention()
    st, ns = run(rt, comp, job, inputs, job_range, projections, ret, op)
    want = {}
    (merged, msum, cuts, ssts), rst = R.expected(job, ret, O.params(**OUT), R.MAX_SST, job_range, projections, op, want)
    assert st == msum.status == 0, (what, st, msum.status)
    gm, gsm = comp.merged()
    assert_batch_same(gm, merged, what + " merged")
    for f in SUMMARY:
        assert getattr(gsm, f) == getattr(msum, f), (what, f)
    assert gsm.num_in == rst["entries_in"], what
    assert ns == len(ssts), (what, ns, len(ssts))
    for i, ref in enumerate(ssts):
        d = comp.sst(i)
        assert (d["entry_start"], d["entry_end"]) == (cuts[i], cuts[i + 1]), what
        assert_same(ref, sst_view(d), "%s sst %d" % (what, i))
    rs = comp.range_stats()
    for f in STATS:
        assert getattr(rs, f) == rst[f], (what, f, getattr(rs, f), rst[f])
    return ns, rs, gm, want


def with_data(inputs, flips):
    """The inputs with a byte flipped inside each (input, block) of `flips` (their data copied first)."""
    out = [copy.copy(x) for x in inputs]
    for i, blk in flips:
        out[i].data = out[i].data.clone()
        out[i].data[int(out[i].block_off[blk].item()) + 10] ^= 0x5A
    return out


def bound_keys(job):
    """The keys the range tests bound with: a stored key whose versions straddle a block boundary, a block's index
    key, a key between two stored keys (each low and high in the key space)."""
    strad, idx, stored = set(), set(), set()
    for x in job.inputs:
        stored.update(x.keys)
        idx.update(x.ikeys[1:])
        for b in x.first_row[1:-1]:
            if x.keys[b - 1] == x.keys[b]:
                strad.add(x.keys[b])
    strad, idx, stored = sorted(strad), sorted(idx), sorted(stored)
    q = lambda s, f: s[int(f * len(s))]  # noqa: E731
    k = dict(s_lo=q(strad, 0.15), s_hi=q(strad, 0.85), i_lo=q(idx, 0.4), i_hi=q(idx, 0.6), b_lo=q(stored, 0.05) + b"\0",
             b_hi=q(stored, 0.95) + b"\0", k_lo=q(stored, 0.3), k_hi=q(stored, 0.7))
    assert k["b_lo"] < k["s_lo"] < k["k_lo"] < k["i_lo"] < k["i_hi"] < k["k_hi"] < k["s_hi"] < k["b_hi"]
    assert k["b_lo"] not in stored and k["b_hi"] not in stored
    return k


# ---- 1. identity (R5) -------------------------------------------------------------------------------------------
def test_identity(rt, comp, small):
    """No range and no projection: the outputs, num_ssts and the summary of run_ssts on the same handle; so do an
    unbounded job range and projections that are all None.  A wrong num_entries is still SDB_INVALID_ARGUMENT."""
    import torch
    job, inputs = small
    st, ns = comp.run_ssts(inputs, retention(), rt.params(**OUT), R.MAX_SST, run_start=job.run_start)
    torch.cuda.synchronize()
    assert st == 0 and ns >= 2
    whole, wsm = comp.merged()
    ssts = [comp.sst(i) for i in range(ns)]
    zero = comp.range_stats()
    assert all(getattr(zero, f) == 0 for f in STATS)
    for kw in (dict(), dict(job_range=(None, U, None, U), projections=[None] * len(inputs))):
        ns2, rs, gm, _ = check(rt, comp, job, inputs, what="identity", **kw)
        gsm = comp.merged()[1]
        assert ns2 == ns
        assert_batch_same(gm, whole, "identity")
        for f, _ in _abi.MergeSummary._fields_:
            assert getattr(gsm, f) == getattr(wsm, f), f
        for i in range(ns):
            d = comp.sst(i)
            assert (d["entry_start"], d["entry_end"]) == (ssts[i]["entry_start"], ssts[i]["entry_end"])
            for f in ("data", "block_off", "block_first_entry", "index_key_len", "block_stats", "bloom"):
                assert np.array_equal(d[f], ssts[i][f]), (i, f)
            assert bytes(d["summary"]) == bytes(ssts[i]["summary"]), i
        assert rs.blocks_checked == rs.blocks_total and rs.entries_in == rs.entries_decoded == wsm.num_in
    bad = [copy.copy(x) for x in inputs]
    bad[2].num_entries += 1
    st, ns = run(rt, comp, job, bad)
    assert st == _abi.SDB_INVALID_ARGUMENT and ns == 0
    assert comp.run_ssts(bad, retention(), rt.params(**OUT), R.MAX_SST, run_start=job.run_start) == (st, 0)


# ---- 2. the job-range matrix (R1-R3) ----------------------------------------------------------------------------
RANGES = {
    "unbounded": lambda k: (None, U, None, U),
    "U..=straddle": lambda k: (None, U, k["s_lo"], INC),
    "U..index": lambda k: (None, U, k["i_hi"], EXC),
    "U..=index": lambda k: (None, U, k["i_hi"], INC),
    "straddle..U": lambda k: (k["s_hi"], INC, None, U),
    "index..=stored": lambda k: (k["i_lo"], INC, k["k_hi"], INC),
    "stored..index": lambda k: (k["k_lo"], INC, k["i_hi"], EXC),
    "(between..U": lambda k: (k["b_lo"], EXC, None, U),
    "(straddle..=straddle": lambda k: (k["s_lo"], EXC, k["s_hi"], INC),
    "(index..between": lambda k: (k["i_lo"], EXC, k["b_hi"], EXC),
    "between..=between": lambda k: (k["b_lo"], INC, k["b_hi"], INC),
    "point on a straddle": lambda k: (k["s_lo"], INC, k["s_lo"], INC),
    "below..index": lambda k: (b"", INC, k["i_lo"], EXC),
    "(below..=straddle": lambda k: (b"", EXC, k["s_lo"], INC),
    "U..=below": lambda k: (None, U, b"", INC),
    "above..U": lambda k: (ABOVE, INC, None, U),
    "(stored..above": lambda k: (k["k_lo"], EXC, ABOVE, EXC),
    "start above end": lambda k: (k["k_hi"], INC, k["k_lo"], INC),
    "equal, end excluded": lambda k: (k["k_lo"], INC, k["k_lo"], EXC),
}


@pytest.mark.parametrize("name", list(RANGES))
def test_job_range(rt, comp, small, name):
    job, inputs = small
    rng = RANGES[name](bound_keys(job))
    ns, rs, gm, _ = check(rt, comp, job, inputs, job_range=rng, what=name)
    if name in ("start above end", "equal, end excluded"):  # empty as a set: nothing is read
        assert (ns, rs.blocks_checked, rs.inputs_read, gm.n) == (0, 0, 0, 0)
    elif name == "U..=below":  # at most the first block of an input (an empty index key) covers it; no row is inside
        assert (ns, rs.entries_in, gm.n) == (0, 0, 0) and rs.blocks_checked <= len(inputs)
    elif name == "above..U":  # R2's deviation: the last block of every input is checked, no row is inside
        assert (ns, rs.blocks_checked, rs.entries_in) == (0, len(inputs), 0) and rs.entries_decoded > 0
    else:
        assert rs.entries_in > 0 and (ns >= 1) == (gm.n > 0)
        if name != "unbounded" and "below" not in name and "above" not in name:
            assert rs.blocks_checked < rs.blocks_total and rs.entries_in < rs.entries_decoded


# ---- 3. projections ---------------------------------------------------------------------------------------------
def test_projections(rt, comp, small):
    job, inputs = small
    k = bound_keys(job)
    vis = [None, (k["k_lo"], INC, k["k_hi"], EXC), (None, U, k["s_hi"], INC), (k["i_lo"], INC, None, U), None,
           (b"", INC, ABOVE, INC)]
    check(rt, comp, job, inputs, projections=vis, what="projections")
    _, rs, _, _ = check(rt, comp, job, inputs, job_range=(k["s_lo"], EXC, k["i_hi"], EXC), projections=vis, what="job and projections")
    assert rs.inputs_read == len(inputs)


def test_middle_sst_of_a_run_clipped(rt, comp, small):
    """The middle SST of the sorted run clipped on both sides by its own projection, its neighbours whole: the rows it
    drops leave no gap in the run."""
    job, inputs = small
    mid = job.inputs[4]
    assert job.run_start[-2:] == [3, 6]
    vis = [None] * 6
    vis[4] = (mid.keys[len(mid.keys) // 4], INC, mid.keys[3 * len(mid.keys) // 4], EXC)
    _, rs, _, _ = check(rt, comp, job, inputs, projections=vis, what="middle")
    assert rs.inputs_read == 6 and 0 < rs.entries_decoded - rs.entries_in < len(mid.keys)
    assert rs.blocks_checked < rs.blocks_total


def test_input_with_an_empty_view_is_skipped(rt, comp, small):
    job, inputs = small
    k = bound_keys(job)
    rng = (None, U, k["k_lo"], EXC)
    vis = [None, (k["k_hi"], INC, None, U), None, None, None, None]  # V[1] is empty
    assert R.view(rng, vis[1]) is None
    broken = with_data(inputs, [(1, b) for b in range(len(job.inputs[1].ikeys))])  # every block of input 1
    _, rs, _, _ = check(rt, comp, job, broken, job_range=rng, projections=vis, what="empty view")
    assert rs.inputs_read < len(inputs)
    st, ns = run(rt, comp, job, broken, job_range=rng)  # without the projection its first block is read
    assert st == _abi.SDB_CHECKSUM_MISMATCH and ns == 0


# ---- 4. laziness (R2) -------------------------------------------------------------------------------------------
def test_only_covering_blocks_are_checked(rt, comp, small):
    job, inputs = small
    k = bound_keys(job)
    rng = (k["i_lo"], INC, k["i_hi"], EXC)
    cov = R.covering(job, rng)
    first = np.concatenate([[0], np.cumsum([len(x.ikeys) for x in job.inputs])])
    nb = [len(x.ikeys) for x in job.inputs]
    assert all(cov[i][0] > 0 and cov[i][1] - cov[i][0] >= 4 and cov[i][1] < nb[i] for i in (0, 1, 2, 4))
    # outside the cover: the block right before and the one right after, of every input
    outside = with_data(inputs, [(i, b) for i, (bs, be) in enumerate(cov) for b in (bs - 1, be) if 0 <= b < nb[i]])
    check(rt, comp, job, outside, job_range=rng, what="corrupt outside")
    # inside: the job fails with the block's status at its index among all inputs' blocks
    bs, be = cov[2]
    st, ns = run(rt, comp, job, with_data(inputs, [(2, bs + 1)]), job_range=rng)
    assert st == _abi.SDB_CHECKSUM_MISMATCH and ns == 0
    sm, rs = comp.merged()[1], comp.range_stats()
    assert sm.status == st and sm.first_error_entry == first[2] + bs + 1
    assert rs.blocks_checked == sum(e - s for s, e in cov) and rs.entries_in == 0
    # two bad covered blocks: the lower one
    st, ns = run(rt, comp, job, with_data(inputs, [(4, cov[4][0]), (1, cov[1][1] - 1)]), job_range=rng)
    assert st == _abi.SDB_CHECKSUM_MISMATCH and ns == 0
    assert comp.merged()[1].first_error_entry == first[1] + cov[1][1] - 1
    check(rt, comp, job, inputs, job_range=rng, what="after the failures")  # the handle goes on


# ---- 5. subcompactions ------------------------------------------------------------------------------------------
def test_subcompactions(rt, comp, small):
    """The planner's ranges, each through the ranged job from the encoded inputs: every range bit-exact, the merged
    streams concatenate to the whole job's, and only a block at a boundary is read by two ranges."""
    job, inputs = small
    ranges = S.plan_subcompaction_ranges(R.metas(job), 4)
    assert len(ranges) >= 2
    got, blocks, covers = [], 0, []
    for x in ranges:
        _, rs, gm, _ = check(rt, comp, job, inputs, job_range=S.range_bounds(x), what=repr(x))
        got += merged_entries(gm)
        blocks += rs.blocks_checked
        covers.append(R.covering(job, S.range_bounds(x)))
    whole, wsm, _, _ = O.compact([R.concat_runs([job.inputs[i].ref for i in range(job.run_start[r], job.run_start[r + 1])])
                                  for r in range(len(job.run_start) - 1)], retention(), O.params(**OUT), R.MAX_SST)
    assert wsm.status == 0 and got == merged_entries(whole)
    assert blocks == sum(be - bs for cov in covers for bs, be in cov if be > bs)
    for i, x in enumerate(job.inputs):  # per input: the covers tile its blocks, neighbours sharing at most one
        spans = [cov[i] for cov in covers if cov[i][1] > cov[i][0]]
        assert spans[0][0] == 0 and spans[-1][1] == len(x.ikeys)
        for (_, e0), (s1, _) in zip(spans, spans[1:]):
            assert e0 - 1 <= s1 <= e0


# ---- 6. merge operator ------------------------------------------------------------------------------------------
def test_operator_under_a_job_range(rt, comp):
    rng = random.Random(17)
    runs = [Run.from_entries(r) for r in rand_runs(rng, 4, 600, 5, tomb=0.1, merge=0.45, expire=0.0)]
    job = R.build_job(runs, dict(block_size=256), splits=[1, 1, 1, 3])
    inputs = R.upload(job)
    ret = O.retention(min_seq=1200, filter_tombstone=True)  # min_seq: the operator's barrier
    ns, rs, _, want = check(rt, comp, job, inputs, job_range=(b"ab", INC, b"cb", EXC), ret=ret, op=Bracket, what="operator")
    ms = comp.merge_stats()
    for f in ("groups", "links", "link_bytes", "merged_bytes", "operator_calls"):
        assert getattr(ms, f) == want[f], f
    assert ms.groups > 10 and ms.links > ms.groups and rs.blocks_checked < rs.blocks_total
    # chains whose links come from different input SSTs
    owners = {}
    for i, x in enumerate(job.inputs):
        for key, f in zip(x.keys, x.ref.flags):
            if f & _abi.FLAG_MERGE_OPERAND and b"ab" <= key < b"cb":
                owners.setdefault(key, set()).add(i)
    assert sum(len(v) > 1 for v in owners.values()) > 10
    check(rt, comp, job, inputs, ret=ret, op=Bracket, what="operator, whole job")


# ---- 7. V1 inputs -----------------------------------------------------------------------------------------------
def test_v1_inputs(rt, comp):
    job = R.small_job(version=1)
    inputs = R.upload(job)
    k = bound_keys(job)
    _, rs, _, _ = check(rt, comp, job, inputs, job_range=(k["s_lo"], INC, k["i_hi"], EXC), what="v1")
    assert rs.blocks_checked < rs.blocks_total
    check(rt, comp, job, inputs, what="v1 whole")


# ---- 8. more than SDB_MAX_RUNS runs -----------------------------------------------------------------------------
def test_33_runs(rt, comp):
    rng = random.Random(233)
    runs = [Run.from_entries(r) for r in rand_runs(rng, 33, 600, 5, dup_seq=True) if r]
    assert len(runs) == 33
    job = R.build_job(runs, dict(block_size=256))
    inputs = R.upload(job)
    ret = O.retention(min_seq=500, compaction_start_ts=900)
    _, rs, _, _ = check(rt, comp, job, inputs, job_range=(b"b", INC, b"cb", INC), ret=ret, what="33 runs")
    assert 0 < rs.entries_in < rs.entries_decoded
    check(rt, comp, job, inputs, ret=ret, what="33 runs whole")


# ---- 9. R6 and R7 on the device ---------------------------------------------------------------------------------
def test_counts_and_malformed_ranges(rt, comp, small):
    job, inputs = small
    k = bound_keys(job)
    rng = (k["i_lo"], INC, k["i_hi"], EXC)
    # R6: a clipped input that declares fewer entries than its cover decodes
    bs, be = R.covering(job, rng)[0]
    less = [copy.copy(x) for x in inputs]
    less[0].num_entries = int(job.inputs[0].first_row[be] - job.inputs[0].first_row[bs]) - 1
    st, ns = run(rt, comp, job, less, job_range=rng)
    assert st == _abi.SDB_INVALID_ARGUMENT and ns == 0
    less[0].num_entries += 1  # exactly its cover: an upper bound that holds
    assert run(rt, comp, job, less, job_range=rng)[0] == 0
    # R7
    good = rt.scan_ranges_columnar([rng])
    vis = rt.projections_columnar([None] * len(inputs))

    def edit(arrays, field, at, value):
        out = {f: a.copy() for f, a in arrays.items()}
        out[field][at] = value
        return out
    bad = [dict(job_range=edit(good, "start_kind", 0, 3)), dict(job_range=edit(good, "end_kind", 0, 3)),
           dict(job_range=edit(good, "start_off", 0, 40)), dict(job_range=edit(good, "end_off", 0, 40)),
           dict(projections=edit(vis, "start_kind", 3, EXC)), dict(projections=edit(vis, "end_kind", 5, 3)),
           dict(job_range=rng, projections=edit(vis, "start_off", 2, 7)), dict(projections=edit(vis, "end_off", 4, 9))]
    for kw in bad:
        st, ns = run(rt, comp, job, inputs, **kw)
        assert st == _abi.SDB_INVALID_ARGUMENT and ns == 0, kw
        rs = comp.range_stats()
        assert rs.blocks_checked == 0 and rs.entries_decoded == 0 and comp.merged()[1].status == st
    ns, _, gm, _ = check(rt, comp, job, inputs, job_range=rng, what="after the failures")  # the handle goes on
    assert run(rt, comp, job, inputs, job_range=good, projections=vis) == (0, ns)  # the same ranges as host arrays
    assert_batch_same(comp.merged()[0], gm, "arrays as given")


# ---- 10. handle reuse, under canaries ---------------------------------------------------------------------------
def test_handle_reuse_under_canaries(rt, small):
    """A ranged job (small), a whole run_ssts (larger), a ranged job with another range, on one handle whose buffers
    of the ranged input side are sized exactly between guard bands and filled with 0xA5: all three correct, no guard
    byte changed."""
    import torch
    cd = C.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slatedb_amd", "libslatedb_amd.so"))
    cd.sdb_diag_compactor_canaries.restype = None
    cd.sdb_diag_compactor_canaries.argtypes = [C.c_void_p, C.c_int]
    cd.sdb_diag_compactor_canary_damage.restype = C.c_int64
    cd.sdb_diag_compactor_canary_damage.argtypes = [C.c_void_p]
    job, inputs = small
    k = bound_keys(job)
    c = rt.Compactor()
    cd.sdb_diag_compactor_canaries(c.h, 1)
    check(rt, c, job, inputs, job_range=(k["k_lo"], INC, k["i_lo"], INC), what="small")
    assert cd.sdb_diag_compactor_canary_damage(c.h) == 0
    st, ns = c.run_ssts(inputs, retention(), rt.params(**OUT), R.MAX_SST, run_start=job.run_start)
    torch.cuda.synchronize()
    (merged, msum, cuts, ssts), _ = R.expected(job, retention(), O.params(**OUT), R.MAX_SST)
    assert st == 0 and ns == len(ssts)
    assert_batch_same(c.merged()[0], merged, "whole")
    for i, ref in enumerate(ssts):
        assert_same(ref, sst_view(c.sst(i)), "whole sst %d" % i)
    check(rt, c, job, inputs, job_range=(k["s_lo"], EXC, k["b_hi"], EXC), projections=[None, None, None, None, (b"", INC, b"", INC), None],
          what="other range")
    assert cd.sdb_diag_compactor_canary_damage(c.h) == 0
    c.close()
