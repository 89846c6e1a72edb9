"""Workspace canaries of the write side, through the C ABI: every entry point that takes a workspace gets one
of exactly the size its sdb_*_workspace_bytes function advertises, 257 bytes into a buffer filled with 0xA5.
Every output must be the oracle's, and not one byte before or after the workspace may change.  The fill also
catches a kernel that relies on a zeroed workspace.  (sdb_sst_lookup's canary is in test_gpu_lookup.py.)

The runtime helpers marshal the arguments; CanaryLib stands between them and the library and swaps the
workspace they allocated for the canaried one."""
import numpy as np
import pytest

from oracle import oracle as O
from slatedb_amd import _abi
from slatedb_amd.batch import Batch, Run

pytestmark = pytest.mark.gpu

LEAD, TAIL = 257, 512
# entry point -> (position of its `workspace` argument, the function that sizes it)
WORKSPACE_ARG = {
    "sdb_encode_ssts": (4, "sdb_encode_ssts_workspace_bytes"),
    "sdb_sst_cuts": (6, "sdb_sst_cuts_workspace_bytes"),
    "sdb_decode_blocks_ex": (7, "sdb_decode_workspace_bytes"),
    "sdb_merge_runs": (4, "sdb_merge_runs_workspace_bytes"),
    "sdb_bloom_build": (6, "sdb_bloom_workspace_bytes"),
    "sdb_bloom_build_prefix": (11, "sdb_bloom_prefix_workspace_bytes"),
    "sdb_decompress_plan": (5, "sdb_decompress_workspace_bytes"),
    "sdb_decompress_blocks_once": (10, "sdb_decompress_once_workspace_bytes"),
    "sdb_compress_blocks": (9, "sdb_compress_workspace_bytes"),
}


class CanaryLib:
    """The library, with every workspace replaced by one of the size last advertised for it, inside canaries."""

    def __init__(self, real):
        self.real, self.advertised, self.buffers = real, {}, []

    def __getattr__(self, name):
        import torch
        f = getattr(self.real, name)
        if name.endswith("_workspace_bytes"):
            def size(*a):
                self.advertised[name] = f(*a)
                return self.advertised[name]
            return size
        if name not in WORKSPACE_ARG:
            return f
        at, sized_by = WORKSPACE_ARG[name]

        def call(*a):
            wsb = self.advertised[sized_by]
            big = torch.full((LEAD + wsb + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
            self.buffers.append((name, big, wsb))
            a = list(a)
            a[at], a[at + 1] = big.data_ptr() + LEAD, wsb
            return f(*a)
        return call

    def check(self, calls):
        """Every canary byte is intact; `calls`: the entry points that must have run, in order."""
        import torch
        torch.cuda.synchronize()
        assert [name for name, _, _ in self.buffers] == calls
        for name, big, wsb in self.buffers:
            assert bool((big[:LEAD] == 0xA5).all()), name + ": bytes before the workspace changed"
            assert bool((big[LEAD + wsb:] == 0xA5).all()), name + ": bytes after the workspace changed"
        self.buffers = []


@pytest.fixture
def rt(monkeypatch):
    from slatedb_amd import runtime
    runtime.require_device()
    canary = CanaryLib(runtime.lib())
    monkeypatch.setattr(runtime, "lib", lambda: canary)
    runtime.canary = canary
    yield runtime
    del runtime.canary


def entries(n, step=2):
    """The lookup canary's recipe: 47-byte rows, a tombstone, create / expire timestamps on some rows."""
    return [(b"key%04d" % (step * i), _abi.KIND_TOMBSTONE if i == 21 else _abi.KIND_VALUE, b"v" * 40, 1000 - i,
             7 + i if i % 3 == 0 else None, 90 + i if i % 4 == 1 else None) for i in range(n)]


B60 = Batch.from_entries(entries(60))
FILTERS = {"none": dict(bloom_bits_per_key=0), "whole10": dict(bloom_bits_per_key=10),
           "fixed4": dict(bloom_bits_per_key=10, prefix_kind=1, prefix_arg=4)}


@pytest.mark.parametrize("version", [1, 2])
@pytest.mark.parametrize("filt", list(FILTERS))
def test_encode_ssts_canaries(rt, version, filt):
    """Three SSTs in one call (60, 0 and 37 entries: the second and third slot bases), no filter / the fused
    bloom / a prefix-extractor filter."""
    from .test_gpu_configs import _encode_set
    from .test_gpu_parity import assert_same
    kw = dict(block_size=1024, sst_version=version, **FILTERS[filt])
    batches = [B60, Batch.from_entries([]), Batch.from_entries(entries(37, step=3))]
    got = _encode_set(rt, batches, rt.params(**kw))
    rt.canary.check(["sdb_encode_ssts"])
    for i, b in enumerate(batches):
        ref = O.encode_sst(b, O.params(**kw))
        assert_same(ref, got[i], "sst %d" % i)
        assert (ref.summary.bloom_len > 0) == (filt != "none" and b.n > 0)
    assert len(O.encode_sst(B60, O.params(**kw)).block_off) - 1 in (3, 4)


def test_sst_cuts_canaries(rt):
    from .test_gpu_compaction import cuts_both
    cuts = cuts_both(rt, B60, O.params(block_size=1024, bloom_bits_per_key=0), 1000)
    rt.canary.check(["sdb_sst_cuts"])
    assert len(cuts) - 1 >= 2


@pytest.mark.parametrize("version", [1, 2])
def test_decode_blocks_canaries(rt, version):
    """The blocks of the 60-entry SST, ascending and descending, and a call with no block."""
    import torch
    from .test_gpu_parity import assert_decode_same
    e = O.encode_sst(B60, O.params(block_size=1024, sst_version=version, bloom_bits_per_key=0))
    nb = len(e.block_off) - 1
    arena = torch.from_numpy(np.concatenate([e.data, np.zeros(64, np.uint8)])).cuda()
    boff = torch.from_numpy(e.block_off.view(np.int64)).cuda()
    for desc in (False, True):
        dout = rt.DeviceDecodeOutput(nb, B60.n, int(B60.key_off[-1]))
        rt.decode_blocks_ex_device(arena, boff, None, nb, dout, version, descending=desc)
        rt.canary.check(["sdb_decode_blocks_ex"])
        assert_decode_same(O.decode_blocks(e.data, e.block_off, version, descending=desc), dout.to_host(), "desc %d" % desc)
    dout = rt.DeviceDecodeOutput(0, 1, 16)
    rt.decode_blocks_ex_device(arena, boff, None, 0, dout, version)
    rt.canary.check(["sdb_decode_blocks_ex"])
    sm = dout.summary_host()
    assert (sm.status, sm.num_entries, sm.key_bytes, sm.num_bad_blocks) == (0, 0, 0, 0)


def test_merge_runs_canaries(rt):
    """Three runs of about 20 entries over overlapping keys, one tombstone."""
    from .test_gpu_compaction import merge_both
    runs = [Run.from_entries([(b"key%04d" % (3 * i + r), _abi.KIND_TOMBSTONE if (r, i) == (1, 7) else _abi.KIND_VALUE,
                               b"r%d-%d" % (r, i), 100 * (r + 1) + i, None, 50 + i if i % 5 == 0 else None)
                              for i in range(19 + r)]) for r in range(3)]
    runs[2] = Run.from_entries([(b"key%04d" % (3 * i), _abi.KIND_VALUE, b"newer", 900 + i, None, None) for i in range(21)])
    ref, rsm = merge_both(rt, runs, O.retention())
    rt.canary.check(["sdb_merge_runs"])
    assert rsm.status == 0 and rsm.num_in == 19 + 20 + 21 and 0 < rsm.num_out


@pytest.mark.parametrize("bpk", [10, 24])
def test_bloom_build_canaries(rt, bpk):
    """60 keys at 10 bits per key (6 probes: the dense plan) and at 24 (16 probes: more than either the dense
    or the binned plan holds, kBinMaxK = 15, so the atomic build runs and leaves the workspace alone; the binned
    plan's slots are bound by the same function as the fused bloom's, which test_encode_ssts_canaries covers)."""
    import torch
    got = rt.BloomFilterPolicy(bpk).build_device(torch.from_numpy(B60.key_bytes).cuda(),
                                                 torch.from_numpy(B60.key_off.view(np.int64)).cuda(), B60.n)
    rt.canary.check(["sdb_bloom_build"])
    assert np.array_equal(got.cpu().numpy(), O.bloom_build(B60.key_bytes, B60.key_off, bpk))


def test_bloom_build_prefix_canaries(rt):
    import torch
    got = rt.bloom_build_prefix_device(torch.from_numpy(B60.key_bytes).cuda(),
                                       torch.from_numpy(B60.key_off.view(np.int64)).cuda(), B60.n, 10, 1, 4, True)
    rt.canary.check(["sdb_bloom_build_prefix"])
    assert np.array_equal(got.cpu().numpy(), O.bloom_build_prefix(B60.key_bytes, B60.key_off, 10, 1, 4, True))


@pytest.mark.parametrize("codec", [O.CODEC_LZ4, O.CODEC_SNAPPY, O.CODEC_ZLIB, O.CODEC_ZSTD])
def test_codec_canaries(rt, codec):
    """Four blocks through sdb_compress_blocks, then sdb_decompress_plan + sdb_decompress_blocks and
    sdb_decompress_blocks_once on the compressed bytes.  Zlib's slots of 512 bytes are shorter than the blocks,
    so the overflow lists, the second plan and the packed run, the whole decode-once workspace, are used."""
    from . import test_gpu_codec, test_gpu_codec_once
    from .test_gpu_codec_write import compressed_on_device
    e = O.encode_sst(B60, O.params(block_size=1024, bloom_bits_per_key=0))
    assert len(e.block_off) - 1 == 4
    comp, coff = compressed_on_device(rt, codec, e.data, e.block_off)
    rt.canary.check(["sdb_compress_blocks"])
    r = O.decompress_blocks(codec, comp, coff)  # the compressor's oracle: its bytes decompress to the blocks
    assert r.first_err == test_gpu_codec_once.NONE
    assert b"".join(r.out[int(a):int(b)].tobytes() for a, b in zip(r.out_start, r.out_end)) == e.data.tobytes()
    test_gpu_codec._check(codec, comp, coff)
    rt.canary.check(["sdb_decompress_plan"])
    spilled = test_gpu_codec_once._check(codec, comp, coff, 512)[4]
    rt.canary.check(["sdb_decompress_blocks_once"])
    assert spilled >= 1 or codec != O.CODEC_ZLIB
