"""Blocks malformed inside a valid CRC, on the device: every parser of a block against the catalogue of
tests/malformed_blocks.py.  Everything is exact.

Where the expectations come from: statuses are the literal walker's (tests/malformed_blocks.py `walk`, the
reference's text), which tests/test_malformed_blocks.py holds equal to the oracle's; the columns of the good
blocks are the oracle's.  The descending cases marked desc_from == "header" are the exception: their
SDB_CORRUPT_BLOCK is the descending rule of include/slatedb_amd.h, which the oracle does not return, so the oracle
is given those blocks with a broken checksum (it then drops them as the device must) and their status is the
walker's.

The faults overrun by one byte, every arena carries 4096 zero bytes behind the data, and the output capacities
cover a clean decode of the same bytes, so a check the device missed would show as a wrong status, not as an
access outside an allocation."""
import types

import numpy as np
import pytest

from oracle import oracle as O
from slatedb_amd import _abi

from . import malformed_blocks as MB
from .scan_cases import EXC, INC, U, Sst, empty_as_set

pytestmark = pytest.mark.gpu

SHAPE_NAMES = list(MB.SHAPES)
MODES = ["asc", "desc", "failfast"]


@pytest.fixture(scope="module")
def rt():
    from slatedb_amd import runtime
    runtime.require_device()
    return runtime


def device_decode(rt, data, off, version, mode, at=False):
    import torch
    nb = len(off) - 1
    dout = rt.DeviceDecodeOutput(nb, len(data) // 8 + 64, len(data) * 8 + 4096)
    arena = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    off = np.asarray(off, np.uint64).view(np.int64)
    start = torch.from_numpy(off[:-1].copy() if at else off).cuda()
    end = torch.from_numpy(off[1:].copy()).cuda() if at else None
    rt.decode_blocks_ex_device(arena, start, end, nb, dout, version, descending=mode == "desc", fail_fast=mode == "failfast")
    torch.cuda.synchronize()
    return dout.to_host()


def check_decode(rt, version, payloads, header, mode, what, lead=0, at=False, break_crc=()):
    """One device decode of `payloads` against the walker's statuses and the oracle's columns.  header: the blocks
    whose descending status is the header's rule."""
    from .test_gpu_parity import assert_decode_same
    desc = mode == "desc"
    data, off = MB.arena(payloads, lead, break_crc)
    want = [_abi.SDB_CHECKSUM_MISMATCH if k in break_crc else MB.walk(p, version, desc)[0] for k, p in enumerate(payloads)]
    bad = [k for k, st in enumerate(want) if st]
    got = device_decode(rt, data, off, version, mode, at)
    assert got.status == (want[bad[0]] if bad else 0), (what, got.status, want)
    assert sorted(got.bad_block.tolist()) == bad, (what, got.bad_block.tolist(), bad)
    if mode == "failfast" and bad:
        return  # read_blocks semantics: the columns of a failed call are unspecified
    odata = MB.arena(payloads, lead, set(break_crc) | (set(header) if desc else set()))[0]
    ref = O.decode_blocks(odata, off, version, descending=desc)
    assert sorted(ref.bad_block.tolist()) == bad, what
    ref.status = got.status  # (compared with the walker's above)
    assert_decode_same(ref, got, what)


def triplets(name):
    """[good, mutated, good] of every variant -> (payloads, blocks under the header's rule, ids)."""
    S = MB.shape(name)
    payloads, header, ids = [], set(), []
    for v in MB.variants(name):
        if v.desc_from == "header":
            header.add(len(payloads) + 1)
        payloads += [S.payloads[0], v.payload, S.payloads[2]]
        ids.append(v.id)
    return S, payloads, header, ids


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_decode_each_variant(rt, name, mode):
    """[good, mutated, good] per mutation, the mutated block at s & 15 of 0, 1 and 15 in turn; a fault on the block's
    last row once more as the arena's last block; fail-fast once more with the checksum broken too."""
    S = MB.shape(name)
    good0, good2 = S.payloads[0], S.payloads[2]
    for i, v in enumerate(MB.variants(name)):
        header = {1} if v.desc_from == "header" else set()
        payloads = [good0, v.payload, good2]
        check_decode(rt, S.version, payloads, header, mode, (name, v.id), MB.lead_for(payloads, 1, (0, 1, 15)[i % 3]))
        if "last" in v.id:
            check_decode(rt, S.version, [good0, good2, v.payload], {2} if header else set(), mode, (name, v.id, "last in the arena"),
                         MB.lead_for([good0, good2], 2, (15, 0, 1)[i % 3]))
        if mode == "failfast":  # the checksum is reported ahead of anything the rows would raise
            check_decode(rt, S.version, payloads, header, mode, (name, v.id, "crc too"), break_crc={1})


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_decode_all_variants_in_one_arena(rt, name, mode):
    """Every variant in one arena through block_end (sdb_decode_blocks_at's layout): the whole bad_block set."""
    S, payloads, header, _ = triplets(name)
    check_decode(rt, S.version, payloads, header, mode, name, at=True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("version", [1, 2])
def test_decode_tiny_blocks(rt, version, mode):
    """Whole blocks of 4 - 7 bytes with a correct CRC, between good blocks (load_block's tiny-block path)."""
    S = MB.shape("v2-spec-4regions-1k" if version == 2 else "v1-small-1k")
    payloads = [S.payloads[0]]
    for _, p, _ in MB.TINY:
        payloads += [p, S.payloads[2]]
    for at in (False, True):
        check_decode(rt, version, payloads, set(), mode, ("tiny", version, at), at=at)
    for k, (tname, p, want) in enumerate(MB.TINY):
        assert MB.walk(p, version, mode == "desc")[0] == want[version][mode == "desc"], tname
        check_decode(rt, version, [S.payloads[0], p, S.payloads[2]], set(), mode, (tname, version), lead=(0, 1, 15)[k % 3])


# --- sdb_sst_lookup ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_lookup(rt, name, desc):
    """The queries of tests/test_malformed_blocks.py (before, on and after the faulty row; a table fault: the block's
    first, middle and last key) on every single fault, every field against O.sst_lookup."""
    from .test_gpu_lookup import run_both
    S = MB.shape(name)
    for v in MB.singles(name):
        data, off = S.sst_with(v.payload)
        run_both(rt, data, types.SimpleNamespace(block_off=off), S.index_keys, S.index_key_off, MB.lookup_keys(S, v),
                 S.version, desc)


# --- sdb_sst_scan --------------------------------------------------------------------------------------------------
_ssts = {}


def scan_sst(name):
    S = MB.shape(name)
    if name not in _ssts:
        sst = Sst(S.batch, S.version, S.block_size, S.restart_interval)
        assert np.array_equal(sst.block_off, S.enc.block_off) and np.array_equal(sst.enc.data, S.enc.data)
        k, b = sst.keys, sst.bes
        ranges = [(None, U, None, U), (k[b[1]], INC, k[b[2] - 1], INC), (k[b[1] + 3], INC, k[b[1] + 3], INC),
                  (k[b[0]], INC, k[b[1] - 1], INC), (k[b[2]], INC, None, U), (k[b[1] - 2], EXC, k[b[2] + 2], EXC),
                  (None, U, k[b[1]], INC), (k[b[2] - 1], INC, None, U), (k[b[2]], EXC, k[b[2] + 5], INC),
                  (k[b[1] + 4], INC, k[b[1] + 2], INC)]
        _ssts[name] = (sst, ranges)
    return (S,) + _ssts[name]


@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_scan(rt, name, desc):
    """Ranges that include and exclude the mutated block, through test_gpu_scan's check: a range fails with the
    walker's status of the block exactly when its block range holds it.  The in-place faults only (the
    expectation's value offsets are the clean SST's)."""
    from .test_gpu_scan import check, host, view_of
    S, sst, ranges = scan_sst(name)
    cover = []
    for r, rg in enumerate(ranges):
        (s, e), _ = sst.expect_idx(rg)
        if s <= S.target < e and not empty_as_set(rg[0] or b"", rg[1], rg[2] or b"", rg[3]):
            cover.append(r)
    assert 3 <= len(cover) <= len(ranges) - 2
    ran = 0
    for v in MB.variants(name):
        if len(v.payload) != len(S.layout.payload):
            continue
        data, off = S.sst_with(v.payload)
        assert np.array_equal(off, sst.block_off)
        st = MB.walk(v.payload, S.version, desc)[0]
        h = host(rt.sst_scan_device(view_of(sst, data[:len(data) - MB.TAIL_PAD]), ranges, descending=desc))
        if st == 0:  # a mutation that still decodes changes the block's rows: the statuses only
            want = np.zeros(len(ranges), np.int64)
            assert np.array_equal(h["range_status"][:len(ranges)].astype(np.int64), want), v.id
            continue
        check(sst, ranges, h, desc, {r: st for r in cover})
        ran += 1
    assert ran >= 8


# --- a thin slice through three further entry points: the status passes through -------------------------------------
def first_serving_block(data, block_off, version, candidates):
    for k in candidates:
        s, e = int(block_off[k]), int(block_off[k + 1])
        faults = MB.thin_faults(bytes(data[s:e - 4]), version)
        if faults:
            return k, faults
    raise AssertionError("no block serves the three faults")


@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("i", [7, 8], ids=["v2-leaf", "v1-leaf"])
def test_lsm_scan_passes_the_status_through(rt, i, desc):
    """Beside test_scan_block_errors' CRC case, on the last SST of the newer sorted run (V2) and the first of the
    older one (V1): blocks of enough rows for the three faults."""
    from . import test_gpu_get as TG
    from .test_gpu_lsm_scan import check, host, model, plain
    m = plain(rt)
    tree, rngs = m["tree"], m["ranges"][:150]
    leaf = tree.leaves[i]
    assert leaf.version == (2 if i == 7 else 1)
    nb = leaf.sst.nb
    bad, faults = first_serving_block(leaf.sst.data, leaf.sst.block_off, leaf.version,
                                      sorted(range(nb), key=lambda b: abs(b - nb // 2)))
    clean = model(tree, rngs, None, desc)
    hit = [q for q, e in enumerate(clean) if int(tree.block_base[i]) + bad in e.blocks]
    assert hit
    for fname, payload, st in faults:
        data = leaf.sst.data.copy()
        MB.reseal(data, leaf.sst.block_off, bad, payload)
        views = [TG.view_of(l) for l in tree.leaves]
        views[i] = TG.view_of(leaf, data=data)
        broken = TG.broken(tree, i, {bad: st})
        h = host(rt.lsm_scan_device(TG.device_tree(rt, broken, views), rngs, descending=desc))
        exp = check(broken, rngs, None, desc, h)
        for q in hit:
            assert exp[q].status == st and not exp[q].rows, (fname, q)


def test_compactor_run_ssts_passes_the_status_through(rt):
    """Beside test_compactor_run_ssts_bad_inputs' CRC case: the job fails with the block's own status at its index."""
    import torch
    from .test_gpu_compaction import big_runs, encoded_inputs
    runs = big_runs(33, 8000, 3)
    prm_kw = dict(block_size=4096, bloom_bits_per_key=10)
    inputs, _, _ = encoded_inputs(rt, runs, prm_kw)
    prm, ret = rt.params(**prm_kw), O.retention()
    comp = rt.Compactor()
    clean = inputs[1].data.clone()
    host_data, bo = clean.cpu().numpy(), inputs[1].block_off.cpu().numpy().view(np.uint64)
    k, faults = first_serving_block(host_data, bo, 2, range(3, len(bo) - 1))
    for fname, payload, st in faults:
        data = host_data.copy()
        MB.reseal(data, bo, k, payload)
        inputs[1].data.copy_(torch.from_numpy(data).cuda())
        got, ns = comp.run_ssts(inputs, ret, prm, 1 << 30)
        torch.cuda.synchronize()
        assert got == st and ns == 0, (fname, got, st)
        assert comp.merged()[1].first_error_entry == inputs[0].block_off.numel() - 1 + k, fname
    inputs[1].data.copy_(clean)
    got, ns = comp.run_ssts(inputs, ret, prm, 1 << 30)
    assert got == 0 and ns == 1
    comp.close()


def test_ranged_compaction_passes_the_status_through(rt):
    """Beside test_only_covering_blocks_are_checked's CRC cases: a covered block's own status fails the job."""
    import copy

    import torch
    from . import ranged_compaction_cases as R
    from .test_gpu_ranged_compaction import bound_keys, check, run
    job = R.small_job()
    inputs = R.upload(job)
    comp = rt.Compactor()
    kk = bound_keys(job)
    rng = (kk["i_lo"], INC, kk["i_hi"], EXC)
    cov = R.covering(job, rng)
    first = np.concatenate([[0], np.cumsum([len(x.ikeys) for x in job.inputs])])
    bs, be = cov[2]
    host_data = inputs[2].data.cpu().numpy()
    bo = inputs[2].block_off.cpu().numpy().view(np.uint64)
    k, faults = first_serving_block(host_data, bo, job.version, range(bs + 1, be))
    for fname, payload, st in faults:
        data = host_data.copy()
        MB.reseal(data, bo, k, payload)
        broken = [copy.copy(x) for x in inputs]
        broken[2].data = torch.from_numpy(data).cuda()
        got, ns = run(rt, comp, job, broken, job_range=rng)
        assert got == st and ns == 0, (fname, got, st)
        sm = comp.merged()[1]
        assert sm.status == st and sm.first_error_entry == first[2] + k, fname
    check(rt, comp, job, inputs, job_range=rng, what="after the failures")
    comp.close()
