"""The encode's block chain where the groups are composed side by side: k_anchor runs one workgroup per group
of chunks, each composes its group's tables and arrives at the SST's counter, and the last one to arrive walks
the groups and writes every chunk's anchor.  The shapes are the smallest at which that can go wrong (kChunk =
2048 entries per chunk, at least 16 chunks per group): a partial last chunk, several groups, a workspace used
twice in a row (the counter is re-zeroed by every call), a set whose members have different group counts, block
sizes on both sides of a chunk, long candidate tables, errors, and key lengths around the 16 bytes k_facts
preloads on the lanes where a wave hands its neighbour's values over.  Every case goes through sdb_encode_ssts
and is compared bit for bit with the oracle (test_gpu_parity.assert_same)."""
import numpy as np
import pytest

from oracle import oracle as O
from slatedb_amd import _abi, datasets
from slatedb_amd.batch import Batch

from . import encode_cases as E
from .test_gpu_parity import assert_same, rt  # noqa: F401

pytestmark = pytest.mark.gpu

CHUNK = 2048


class _Got:
    """A DeviceSstOutput in the shape assert_same reads."""

    def __init__(self, out):
        sm = out.summary_host()
        self.status = sm.status
        self.summary = {f: getattr(sm, f) for f, _ in _abi.SstSummary._fields_}
        if sm.status == 0:
            for f, v in out.to_host().items():
                if f != "summary":
                    setattr(self, f, v)


def encode_set(rt, batches, prior=None, **kw):  # noqa: F811
    """One sdb_encode_ssts call over `batches`: its outputs.  With `prior` (as many entries per SST, other
    rows), a call over those runs first, back to back on the same stream, workspace and outputs: the second
    call finds the counter and the tables of another chain."""
    import torch
    prm = rt.params(**kw)
    dbs = [b.to_device("cuda") for b in batches]
    cap = lambda i: max(b[i].logical_bytes() for b in (batches, prior or batches))
    outs = [rt.DeviceSstOutput(b.n, cap(i), cap(i), prm, workspace=False) for i, b in enumerate(batches)]
    ws = rt.ssts_workspace(dbs, prm)
    if prior is not None:
        assert [b.n for b in prior] == [b.n for b in batches]
        pdbs = [b.to_device("cuda") for b in prior]
        assert rt.ssts_workspace(pdbs, prm).numel() == ws.numel()
        rt.encode_ssts_device(pdbs, outs, prm, ws)
    rt.encode_ssts_device(dbs, outs, prm, ws)
    torch.cuda.synchronize()
    return [_Got(o) for o in outs]


def check_set(rt, batches, what, prior=None, **kw):  # noqa: F811
    refs = [O.encode_sst(b, O.params(**kw)) for b in batches]
    gots = encode_set(rt, batches, prior=prior, **kw)
    for i, (ref, got) in enumerate(zip(refs, gots)):
        assert_same(ref, got, "%s [sst %d, n=%d]" % (what, i, batches[i].n))
    return refs, gots


def test_one_group_partial_last_chunk(rt):  # noqa: F811
    check_set(rt, [datasets.d1(n=CHUNK * 3 + 5)], "one group, partial last chunk")


def test_several_groups_same_workspace_twice(rt):  # noqa: F811
    """20 chunks are two groups (16 + 4).  The second call finds the counter the first one left, and tables of
    shorter rows: with a counter that is not zeroed again, no workgroup is the last one and the anchors stay."""
    b = datasets.d1(n=CHUNK * 20)
    check_set(rt, [b], "two groups")
    check_set(rt, [b], "two groups, second call on the same workspace", prior=[datasets.d1(n=b.n, value_len=57)])


def test_set_with_different_group_counts(rt):  # noqa: F811
    bs = [datasets.d1(sst_index=i, n=n) for i, n in enumerate((1, CHUNK - 1, CHUNK * 5 + 1))]
    check_set(rt, bs, "set of three", prior=[datasets.d1(sst_index=9, n=b.n, value_len=31) for b in bs])
    # more chunks than one group in one member only
    bs = [datasets.d1(sst_index=i, n=n) for i, n in enumerate((CHUNK * 17 + 3, 2, CHUNK * 16))]
    check_set(rt, bs, "set of three, one and two groups")


@pytest.mark.parametrize("block_size,value_len", [(64, 100), (65536, 100), (65536, 0)],
                         ids=["bs64", "bs65536", "bs65536-short-rows"])
def test_block_sizes_around_a_chunk(rt, block_size, value_len):  # noqa: F811
    """64: a block per row, 2048 blocks per chunk.  65536: ~560 rows per block, every chunk table entry leaves
    the chunk at once; with 28-byte rows a block is longer than the lookahead and the serial walk answers."""
    b = datasets.d1(n=CHUNK * 4, value_len=value_len)
    refs, _ = check_set(rt, [b], "block_size %d" % block_size, block_size=block_size)
    per_block = b.n / refs[0].summary.num_blocks
    assert (per_block > 1024) == (value_len == 0) and (per_block == 1) == (block_size == 64)


@pytest.mark.parametrize("block_size", [1024, 4096])
def test_long_candidate_tables(rt, block_size):  # noqa: F811
    """13-byte rows: a block of block_size / 13 entries, so every chunk table has that many candidates (76 and
    307: more than a wave of them, and close to the lookahead of 343)."""
    b = E.tiny_rows(CHUNK * 18)
    refs, _ = check_set(rt, [b], "tiny rows, block_size %d" % block_size, block_size=block_size)
    longest = refs[0].summary.max_block_entries
    assert 64 < longest <= E.seg_look(block_size)
    assert E.anchor_path(b.n, longest, block_size) == "lds"


def _with_empty_first_key(b):
    """`b` behind one entry whose key is empty."""
    z64, z8 = np.zeros(1, np.uint64), np.zeros(1, np.uint8)
    return Batch(b.key_bytes, np.concatenate([z64, b.key_off]), b.val_bytes, np.concatenate([z64, b.val_off]),
                 np.concatenate([z8, b.kind]), np.concatenate([z64, b.seq]),
                 np.concatenate([np.zeros(1, np.int64), b.create_ts]),
                 np.concatenate([np.zeros(1, np.int64), b.expire_ts]), np.concatenate([z8, b.ts_mask]))


def test_mixed_kinds_and_errors(rt):  # noqa: F811
    n = CHUNK * 3 + 5
    good = datasets.d3(seed=11, n=n)
    bad_kind = datasets.d3(seed=11, n=n)
    bad_kind.kind[4100] = 7
    empty = _with_empty_first_key(datasets.d3(seed=11, n=n - 1))
    both = _with_empty_first_key(datasets.d3(seed=11, n=n - 1))
    both.kind[4100] = 7
    refs, gots = check_set(rt, [good, bad_kind, empty, both], "mixed kinds",
                           prior=[datasets.d3(seed=12, n=n) for _ in range(4)])
    assert [r.status for r in refs] == [0, _abi.SDB_INVALID_ARGUMENT, _abi.SDB_EMPTY_KEY, _abi.SDB_EMPTY_KEY]
    assert [g.summary["first_error_entry"] for g in gots[1:]] == [4100, 0, 0]
    assert refs[0].summary.num_deletes and refs[0].summary.num_merges


KEY_LENS = (1, 15, 17, 300)


def key_length_batch(n, seed=5):
    """Keys of 1, 15, 17 and 300 bytes in a seeded random order.  Runs of three entries share their first byte
    and a filler, so neighbours of equal length share all but their last bytes (300: far past the 16 bytes
    k_facts preloads) and neighbours of different lengths the shorter one's head; a one-byte key is a byte no
    other key starts with, so no key is a proper prefix of the one before it."""
    rng = np.random.default_rng(seed)
    lens = rng.choice(KEY_LENS, n)
    es = []
    for i, kl in enumerate(lens):
        key = b"\x00" if kl == 1 else bytes([1 + (i // 3) % 250]) + b"q" * (int(kl) - 5) + int(i).to_bytes(4, "big")
        es.append((key, 0, bytes(rng.integers(0, 256, int(rng.integers(0, 40)), dtype=np.uint8)), i, None, None))
    return Batch.from_entries(es), lens


def test_key_lengths_on_wave_boundaries(rt):  # noqa: F811
    n = CHUNK * 2 + 64
    b, lens = key_length_batch(n)
    # k_facts: entry e is lane e % 64; lane 63 loads its own next offset, lane 0 its own previous key
    for lane in (0, 1, 62, 63):
        assert set(lens[lane::64]) == set(KEY_LENS), lane
    refs, _ = check_set(rt, [b], "key lengths")
    assert refs[0].status == 0
    check_set(rt, [b], "key lengths, V1", sst_version=1)
