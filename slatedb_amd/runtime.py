"""Host-side front-end of libslatedb_amd.so (ctypes over the C ABI in include/slatedb_amd.h).

Mirrors the reference's surface for this path:
  * SstBuilder            <- EncodedSsTableBuilder add()/build()/next_block() (sst_builder.rs:224-417)
  * BloomFilterPolicy     <- FilterPolicy "_bf" / BloomFilterBuilder (filter_policy.rs:170-283,
                             filter.rs:40-90); encode() = Filter::encode (filter.rs:177-180)
  * read_blocks()         <- SsTableFormat::read_blocks + DataBlockIterator (format/sst.rs:938-999)
  * encode_sst_device()   <- the batched device entry point used by bench.py

The HIP library is mandatory: a missing .so or a machine without a HIP device raises; nothing
falls back to a CPU implementation.
"""
import ctypes as C
import functools
import os

import numpy as np

from . import _abi
from .batch import Batch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libslatedb_amd.so")
# tuning experiments only: an alternative in-tree build of the same library
if os.environ.get("SDB_LIBRARY"):
    LIB_PATH = os.path.join(HERE, os.path.basename(os.environ["SDB_LIBRARY"]))

_lib = None


class SdbError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        super().__init__("%s: %s" % (what or "slatedb_amd", _abi.STATUS_NAMES.get(status, status)))


def lib():
    """Load libslatedb_amd.so (fails loudly if it has not been built).

    torch is imported first on purpose: torch ships its own libamdhip64.so with the same soname
    (libamdhip64.so.7) as /opt/rocm's, so loading it first makes our library bind to the HIP runtime
    torch already uses — one runtime per process, so torch streams, events and allocations are
    valid handles for our kernels.  (The Rust/C host links /opt/rocm's runtime as usual.)"""
    global _lib
    if _lib is None:
        try:
            import torch  # noqa: F401
            if torch.cuda.is_available():
                torch.cuda.init()
        except ImportError:
            pass
        if not os.path.exists(LIB_PATH):
            raise ImportError("libslatedb_amd.so not built: run `python __graft_entry__.py build` "
                              "(hipcc --offload-arch=gfx950)")
        _lib = _abi.bind(C.CDLL(LIB_PATH), partial=bool(os.environ.get("SDB_LIBRARY")))
    return _lib


def device_count():
    return lib().sdb_device_count()


def require_device():
    if device_count() <= 0:
        raise SdbError(_abi.SDB_DEVICE_ERROR, "no HIP device visible")


def params(block_size=4096, sst_version=2, restart_interval=16, bloom_bits_per_key=10,
           min_filter_keys=0, sst_type=_abi.SST_COMPACTED, prefix_kind=0, prefix_arg=0, no_whole_key=0):
    return _abi.SstParams(block_size, sst_version, restart_interval, bloom_bits_per_key,
                          min_filter_keys, sst_type, prefix_kind, prefix_arg, no_whole_key)


def filter_name(prm, extractor_name=None):
    """FilterPolicy::name of BloomFilterPolicy (filter_policy.rs:237-250): "_bf[:p=<extractor>][:wh=0]"."""
    name = "_bf"
    if prm.prefix_kind:
        name += ":p=" + (extractor_name or {1: "fixed%d" % prm.prefix_arg, 2: "delim%d" % prm.prefix_arg,
                                            3: "custom"}[prm.prefix_kind])
    if prm.no_whole_key:
        name += ":wh=0"
    return name.encode()


def bloom_build_prefix_device(key_bytes, key_off, n, bpk, kind, arg=0, whole=True, prefix_len=None, stream=None):
    """sdb_bloom_build_prefix over device tensors -> the bitmap (torch uint8, device-counted length)."""
    import torch
    dev = key_bytes.device
    cap = lib().sdb_bloom_filter_bytes(2 * n, bpk) + 16
    bm = torch.empty((cap + 3) // 4 * 4, dtype=torch.uint8, device=dev)
    ln = torch.zeros(1, dtype=torch.int64, device=dev)
    wsb = lib().sdb_bloom_prefix_workspace_bytes(n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    sp = None if stream is None else (stream.cuda_stream if hasattr(stream, "cuda_stream") else stream)
    st = lib().sdb_bloom_build_prefix(key_bytes.data_ptr(), key_off.data_ptr(),
                                      None if prefix_len is None else prefix_len.data_ptr(), n, bpk, kind, arg,
                                      int(whole), bm.data_ptr(), cap, ln.data_ptr(), ws.data_ptr(), wsb, sp)
    if st:
        raise SdbError(st, "sdb_bloom_build_prefix")
    torch.cuda.synchronize()
    L = int(ln.item())
    if L < 0:
        raise SdbError(_abi.SDB_INVALID_ARGUMENT, "sdb_bloom_build_prefix (prefix longer than its key)")
    return bm[:L]


def might_match_device(bitmap, num_probes, whole, kind, arg, key_bytes, key_off, n, is_prefix=None,
                       query_prefix_len=None, stream=None):
    """sdb_bloom_might_match over device tensors -> torch uint8 results."""
    import torch
    res = torch.zeros(max(n, 1), dtype=torch.uint8, device=key_bytes.device)
    sp = None if stream is None else (stream.cuda_stream if hasattr(stream, "cuda_stream") else stream)
    st = lib().sdb_bloom_might_match(bitmap.data_ptr() if bitmap.numel() else None, bitmap.numel(), num_probes,
                                     int(whole), kind, arg, key_bytes.data_ptr(), key_off.data_ptr(),
                                     None if is_prefix is None else is_prefix.data_ptr(),
                                     None if query_prefix_len is None else query_prefix_len.data_ptr(), n,
                                     res.data_ptr(), sp)
    if st:
        raise SdbError(st, "sdb_bloom_might_match")
    return res[:n]


def _u8(ptr, n):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (n,)) if n else np.zeros(0, np.uint8)


def _arr(ptr, ctype, n, dtype):
    if not n:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), (n,)).view(dtype)


class EncodedSst:
    """Data section + bloom of one SST (host copies)."""

    def __init__(self, res, params_):
        sm = res.summary
        self.status = sm.status
        self.summary = {f: getattr(sm, f) for f, _ in _abi.SstSummary._fields_}
        ok = sm.status == 0
        nb = sm.num_blocks if ok else 0
        self.data = _u8(res.data, sm.data_len if ok else 0).copy()
        self.block_off = _arr(res.block_off, C.c_uint64, nb + 1 if ok else 0, np.uint64).copy()
        self.block_first_entry = _arr(res.block_first_entry, C.c_uint32, nb + 1 if ok else 0, np.uint32).copy()
        self.index_key_len = _arr(res.index_key_len, C.c_uint32, nb, np.uint32).copy()
        self.block_stats = _arr(res.block_stats, C.c_uint16, 3 * nb, np.uint16).reshape(-1, 3).copy()
        self.bloom = _u8(res.bloom, sm.bloom_len if sm.status == 0 else 0).copy()
        self.num_probes = sm.num_probes
        self.filter_built = bool(sm.filter_built)
        self.timings_ms = {"h2d": res.h2d_ms, "kernel": res.kernel_ms, "d2h": res.d2h_ms}
        self.sst_version = params_.sst_version
        self._next = 0

    @property
    def num_blocks(self):
        return len(self.index_key_len)

    def block(self, k):
        """Encoded block k: Block::encode() ++ crc32 BE (EncodedSsTableBlock.encoded_bytes)."""
        return self.data[int(self.block_off[k]):int(self.block_off[k + 1])].tobytes()

    def next_block(self):
        """EncodedSsTableBuilder::next_block (sst_builder.rs:274-276)."""
        if self._next >= self.num_blocks:
            return None
        b = self.block(self._next)
        self._next += 1
        return b

    def filter_block(self, name="_bf"):
        """Composite filter block bytes incl. CRC (format/sst.rs:394-421, 525-554)."""
        import struct
        import zlib
        if not self.filter_built:
            return b""
        enc = struct.pack(">H", self.num_probes) + self.bloom.tobytes()
        comp = struct.pack(">HH", 1, len(name)) + name.encode() + struct.pack(">Q", len(enc)) + enc
        return comp + struct.pack(">I", zlib.crc32(comp))


def sst_footer(batch, enc, sst_version=2, sst_type=_abi.SST_COMPACTED, filter_name=None, compression=0):
    """Footer bytes after the data section (sdb_sst_footer; EncodedSsTableFooterBuilder::build,
    format/sst.rs:383-487).  `enc` is an encode result with host arrays (EncodedSst, the
    DeviceSstOutput.to_host() dict wrapped by `_FooterView`, or anything with data/block_off/
    block_first_entry/index_key_len/block_stats/bloom/summary).  For SST_WAL the block first keys
    are the first entries' seq numbers, big-endian (wal/slatedb/sst_builder.rs:137-155), and there
    is no last entry, stats or filter.  Host code: no device needed."""
    sm = enc.summary if isinstance(enc.summary, _abi.SstSummary) else _abi.SstSummary(**enc.summary)
    nb = len(enc.block_off) - 1 if len(enc.block_off) else 0
    starts = np.asarray(enc.block_first_entry[:nb], np.int64)
    if sst_type == _abi.SST_WAL:
        seqs = (np.zeros(batch.n, np.uint64) if batch.seq is None else batch.seq)[starts]
        fk = seqs.astype(">u8").view(np.uint8).copy()
        fko = np.arange(nb + 1, dtype=np.uint64) * 8
        first = fk[:8].tobytes() if nb else None
        last = None
    else:
        ikl = np.asarray(enc.index_key_len[:nb], np.uint64)
        fko = np.zeros(nb + 1, np.uint64)
        fko[1:] = np.cumsum(ikl)
        ks = batch.key_off[starts] if nb else np.zeros(0, np.uint64)
        idx = np.repeat(ks - fko[:-1], ikl.astype(np.int64)) + np.arange(int(fko[-1]), dtype=np.uint64)
        fk = batch.key_bytes[idx.astype(np.int64)].copy() if len(idx) else np.zeros(1, np.uint8)
        first = batch.key(0) if batch.n else None
        last = batch.key(batch.n - 1) if batch.n else None
    boff = np.ascontiguousarray(enc.block_off[:nb], np.uint64)
    bst = np.ascontiguousarray(np.asarray(enc.block_stats, np.uint16).reshape(-1))
    bloom = np.ascontiguousarray(np.asarray(enc.bloom, np.uint8))
    fk = np.ascontiguousarray(fk if len(fk) else np.zeros(1, np.uint8))
    wal = sst_type == _abi.SST_WAL
    fi = _abi.FooterIn(sst_version, sst_type, 0 if wal else int(bool(sm.filter_built)), sm.num_probes,
                       int(sm.data_len), nb, boff.ctypes.data, fk.ctypes.data, fko.ctypes.data,
                       first, len(first or b""), last, len(last or b""),
                       None if wal else C.addressof(sm), bst.ctypes.data if len(bst) else None,
                       bloom.ctypes.data if len(bloom) else None, 0 if wal else int(sm.bloom_len),
                       filter_name, compression, 0)
    n = C.c_uint64(0)
    cap = lib().sdb_sst_footer_bound(C.byref(fi))
    out = np.empty(max(cap, 1), np.uint8)
    st = lib().sdb_sst_footer(C.byref(fi), out.ctypes.data, cap, C.byref(n))
    if st:
        raise SdbError(st, "sdb_sst_footer")
    return out[:n.value].tobytes()


def sst_object(batch, enc, sst_version=2, sst_type=_abi.SST_COMPACTED, filter_name=None):
    """The whole SST object (data section ++ footer) that write_sst stores."""
    return np.asarray(enc.data, np.uint8).tobytes() + sst_footer(batch, enc, sst_version, sst_type, filter_name)


class Encoder:
    """Host-buffer encoder (device arena + pinned staging + its own stream)."""

    def __init__(self, prm=None, device=0):
        require_device()
        self.params = prm or params()
        self._h = lib().sdb_encoder_create(device, C.byref(self.params))
        if not self._h:
            raise SdbError(_abi.SDB_DEVICE_ERROR, "sdb_encoder_create")

    def encode(self, batch, copy=True):
        kb = batch.to_ctypes()
        res = _abi.SstHostResult()
        st = lib().sdb_encoder_encode_host(self._h, C.byref(kb), C.byref(res))
        if not copy:  # the raw SstHostResult view (valid until the next call)
            return st, res
        out = EncodedSst(res, self.params)
        out.status = st
        return out

    def encode_many(self, batches, copy=True):
        """sdb_encoder_encode_host_many: several SSTs with overlapped transfers.  copy=False returns the
        raw SstHostResult views (valid until the next call) instead of EncodedSst copies."""
        kbs = (_abi.KvBatch * max(len(batches), 1))(*[b.to_ctypes() for b in batches])
        res = (_abi.SstHostResult * max(len(batches), 1))()
        st = lib().sdb_encoder_encode_host_many(self._h, len(batches), kbs, res)
        self.last_status = st
        if not copy:
            return st, res
        return [EncodedSst(res[i], self.params) for i in range(len(batches))]

    def close(self):
        if self._h:
            lib().sdb_encoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SstBuilder:
    """EncodedSsTableBuilder mirror: add() entries in order, then build() encodes on the GPU."""

    def __init__(self, prm=None, device=0):
        require_device()
        self.params = prm or params()
        self._h = lib().sdb_sst_builder_new(device, C.byref(self.params))
        if not self._h:
            raise SdbError(_abi.SDB_DEVICE_ERROR, "sdb_sst_builder_new")

    def add(self, key, value=b"", seq=0, kind=_abi.KIND_VALUE, create_ts=None, expire_ts=None):
        key = bytes(key)
        value = bytes(value or b"")
        st = lib().sdb_sst_builder_add(self._h, key, len(key), kind, value, len(value), seq,
                                       create_ts is not None, create_ts or 0, expire_ts is not None,
                                       expire_ts or 0)
        if st:
            raise SdbError(st, "add")

    def add_value(self, key, value, create_ts=None, expire_ts=None):
        """EncodedSsTableBuilder::add_value (sst_builder.rs:257-272): seq 0."""
        self.add(key, value, 0, _abi.KIND_VALUE, create_ts, expire_ts)

    def build(self):
        res = _abi.SstHostResult()
        st = lib().sdb_sst_builder_build(self._h, C.byref(res))
        out = EncodedSst(res, self.params)
        out.status = st
        return out

    def close(self):
        if self._h:
            lib().sdb_sst_builder_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BloomFilterPolicy:
    """FilterPolicy "_bf" with whole-key filtering (filter_policy.rs:170-283)."""

    NAME = "_bf"

    def __init__(self, bits_per_key=10):
        self.bits_per_key = bits_per_key

    def name(self):
        return self.NAME

    def num_probes(self):
        return lib().sdb_bloom_num_probes(self.bits_per_key)

    def estimate_size(self, num_keys):
        return lib().sdb_bloom_filter_bytes(num_keys, self.bits_per_key) + 2

    def build_device(self, key_bytes, key_off, n, stream=None):
        """Bitmap over device-resident keys -> torch uint8 tensor (device)."""
        import torch
        fb = lib().sdb_bloom_filter_bytes(n, self.bits_per_key)
        bm = torch.empty((fb + 3) // 4 * 4 or 4, dtype=torch.uint8, device=key_bytes.device)
        wsb = lib().sdb_bloom_workspace_bytes(n, self.bits_per_key)
        ws = torch.empty(wsb, dtype=torch.uint8, device=key_bytes.device)
        st = lib().sdb_bloom_build(key_bytes.data_ptr(), key_off.data_ptr(), n, self.bits_per_key,
                                   bm.data_ptr(), fb, ws.data_ptr(), wsb, stream)
        if st:
            raise SdbError(st, "sdb_bloom_build")
        return bm[:fb]

    def build(self, batch_or_keys):
        """Filter::encode bytes: u16 BE num_probes ++ bitmap (filter.rs:177-180)."""
        import struct
        import torch
        require_device()
        if isinstance(batch_or_keys, Batch):
            kbytes, koff = batch_or_keys.key_bytes, batch_or_keys.key_off
        else:
            keys = [bytes(k) for k in batch_or_keys]
            koff = np.zeros(len(keys) + 1, np.uint64)
            koff[1:] = np.cumsum([len(k) for k in keys]) if keys else []
            kbytes = np.frombuffer(b"".join(keys) or b"\0", np.uint8)
        n = len(koff) - 1
        dk = torch.from_numpy(np.ascontiguousarray(kbytes)).cuda() if kbytes.size else torch.zeros(16, dtype=torch.uint8, device="cuda")
        do = torch.from_numpy(np.ascontiguousarray(koff).view(np.uint8)).cuda()
        bm = self.build_device(dk, do, n)
        torch.cuda.synchronize()
        return struct.pack(">H", self.num_probes()) + bm.cpu().numpy().tobytes()


def might_contain(bitmap, num_probes, keys):
    """Batched BloomFilter::might_contain over host keys; returns a bool array."""
    import torch
    require_device()
    keys = [bytes(k) for k in keys]
    koff = np.zeros(len(keys) + 1, np.uint64)
    koff[1:] = np.cumsum([len(k) for k in keys]) if keys else []
    kb = np.frombuffer(b"".join(keys) or b"\0", np.uint8).copy()
    dk = torch.from_numpy(kb).cuda()
    do = torch.from_numpy(koff.view(np.uint8)).cuda()
    bm = np.ascontiguousarray(bitmap, np.uint8)
    dbm = torch.from_numpy(np.concatenate([bm, np.zeros(4, np.uint8)])).cuda()
    res = torch.zeros(max(len(keys), 1), dtype=torch.uint8, device="cuda")
    st = lib().sdb_bloom_might_contain(dbm.data_ptr(), bm.size, num_probes, dk.data_ptr(), do.data_ptr(),
                                       len(keys), res.data_ptr(), None)
    if st:
        raise SdbError(st, "sdb_bloom_might_contain")
    torch.cuda.synchronize()
    return res.cpu().numpy()[:len(keys)].astype(bool)


class Decoded:
    pass


class Decoder:
    def __init__(self, device=0):
        require_device()
        self._h = lib().sdb_decoder_create(device)
        if not self._h:
            raise SdbError(_abi.SDB_DEVICE_ERROR, "sdb_decoder_create")

    def decode(self, blocks, block_off, sst_version=2):
        blocks = np.ascontiguousarray(blocks, np.uint8)
        block_off = np.ascontiguousarray(block_off, np.uint64)
        nb = len(block_off) - 1
        res = _abi.DecodeHostResult()
        st = lib().sdb_decoder_decode_host(self._h, blocks.ctypes.data if blocks.size else None,
                                           block_off.ctypes.data, nb, sst_version, C.byref(res))
        d = Decoded()
        d.status = st
        sm = res.summary
        d.summary = {f: getattr(sm, f) for f, _ in _abi.DecodeSummary._fields_}
        n = sm.num_entries if st in (0, 3, 4, 9) else 0
        d.n = n
        d.block_entry_start = _arr(res.block_entry_start, C.c_uint64, nb + 1, np.uint64).copy()
        d.key_off = _arr(res.key_off, C.c_uint64, n + 1, np.uint64).copy()
        d.key_arena = _u8(res.key_arena, sm.key_bytes).copy()
        d.val_off = _arr(res.val_off, C.c_uint64, n, np.uint64).copy()
        d.val_len = _arr(res.val_len, C.c_uint32, n, np.uint32).copy()
        d.seq = _arr(res.seq, C.c_uint64, n, np.uint64).copy()
        d.flags = _u8(res.flags, n).copy()
        d.create_ts = _arr(res.create_ts, C.c_int64, n, np.int64).copy()
        d.expire_ts = _arr(res.expire_ts, C.c_int64, n, np.int64).copy()
        d.bad_block = _arr(res.bad_block, C.c_uint32, min(sm.num_bad_blocks, nb + 1), np.uint32).copy()
        return d

    def close(self):
        if self._h:
            lib().sdb_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------
# Device-resident batched entry point (bench / multi-SST pipelines)
# ------------------------------------------------------------------------------------------------
class DeviceSstOutput:
    """Caller-owned device outputs + workspace for sdb_encode_sst (allocated once, reused)."""

    def __init__(self, n, total_key_bytes, total_val_bytes, prm, device="cuda", workspace=True):
        import torch
        dc, bc, fc = C.c_uint64(), C.c_uint64(), C.c_uint64()
        st = lib().sdb_encode_bounds(n, total_key_bytes, total_val_bytes, C.byref(prm), C.byref(dc),
                                     C.byref(bc), C.byref(fc))
        if st:
            raise SdbError(st, "sdb_encode_bounds")
        self.params = prm
        self.data = torch.empty(dc.value, dtype=torch.uint8, device=device)
        self.block_off = torch.empty(bc.value + 1, dtype=torch.int64, device=device)
        self.block_first = torch.empty(bc.value + 1, dtype=torch.int32, device=device)
        self.index_key_len = torch.empty(bc.value + 1, dtype=torch.int32, device=device)
        self.block_stats = torch.empty(3 * (bc.value + 1), dtype=torch.int16, device=device)
        self.bloom = torch.empty(fc.value, dtype=torch.uint8, device=device)
        self.summary = torch.zeros(C.sizeof(_abi.SstSummary), dtype=torch.uint8, device=device)
        self.workspace = None
        if workspace:  # own scratch for sdb_encode_sst (a set shares one, see encode_ssts_device)
            ws = lib().sdb_encode_workspace_bytes(n, C.byref(prm))
            self.workspace = torch.empty(max(ws, 256), dtype=torch.uint8, device=device)
        self.out = _abi.SstOut(self.data.data_ptr(), dc.value, self.block_off.data_ptr(),
                               self.block_first.data_ptr(), self.index_key_len.data_ptr(),
                               self.block_stats.data_ptr(), bc.value, self.bloom.data_ptr(), fc.value,
                               self.summary.data_ptr())

    def summary_host(self):
        raw = self.summary.cpu().numpy().tobytes()
        return _abi.SstSummary.from_buffer_copy(raw)

    def to_host(self):
        sm = self.summary_host()
        nb = sm.num_blocks
        r = {
            "summary": sm,
            "data": self.data[:sm.data_len].cpu().numpy(),
            "block_off": self.block_off[:nb + 1].cpu().numpy().view(np.uint64),
            "block_first_entry": self.block_first[:nb + 1].cpu().numpy().view(np.uint32),
            "index_key_len": self.index_key_len[:nb].cpu().numpy().view(np.uint32),
            "block_stats": self.block_stats[:3 * nb].cpu().numpy().view(np.uint16).reshape(-1, 3),
            "bloom": self.bloom[:sm.bloom_len].cpu().numpy(),
        }
        return r


def encode_sst_device(dbatch, out, stream=None):
    """Enqueue one SST encode (device batch -> device outputs) on `stream` (torch stream or None)."""
    sp = None
    if stream is not None:
        sp = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    kb = dbatch.to_ctypes()
    st = lib().sdb_encode_sst(C.byref(kb), C.byref(out.params), C.byref(out.out), out.workspace.data_ptr(),
                              out.workspace.numel(), sp)
    if st:
        raise SdbError(st, "sdb_encode_sst")


def ssts_workspace(dbatches, prm, device="cuda"):
    """Scratch for sdb_encode_ssts over these device batches (sdb_encode_ssts_workspace_bytes)."""
    import torch
    kbs = (_abi.KvBatch * max(len(dbatches), 1))(*[b.to_ctypes() for b in dbatches])
    n = lib().sdb_encode_ssts_workspace_bytes(len(dbatches), kbs, C.byref(prm))
    return torch.empty(max(n, 256), dtype=torch.uint8, device=device)


def encode_ssts_device(dbatches, outs, prm, workspace, stream=None):
    """Enqueue the encode of several independent SSTs (same params) as ONE launch sequence
    (sdb_encode_ssts): outs[i] receives batches[i]."""
    assert len(dbatches) == len(outs)
    sp = None
    if stream is not None:
        sp = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    kbs = (_abi.KvBatch * max(len(dbatches), 1))(*[b.to_ctypes() for b in dbatches])
    os_ = (_abi.SstOut * max(len(outs), 1))(*[o.out for o in outs])
    st = lib().sdb_encode_ssts(len(dbatches), kbs, C.byref(prm), os_, workspace.data_ptr(), workspace.numel(), sp)
    if st:
        raise SdbError(st, "sdb_encode_ssts")


class DeviceDecodeOutput:
    """Caller-owned device outputs + workspace for sdb_decode_blocks / sdb_decode_blocks_at."""

    def __init__(self, nblocks, cap_entries, key_cap, device="cuda"):
        import torch
        o = lambda n, dt: torch.empty(max(n, 1), dtype=dt, device=device)
        self.nblocks = nblocks
        self.block_entry_start = o(nblocks + 1, torch.int64)
        self.key_arena = o(key_cap + 16, torch.uint8)
        self.key_off = o(cap_entries + 1, torch.int64)
        self.val_off = o(cap_entries, torch.int64)
        self.val_len = o(cap_entries, torch.int32)
        self.seq = o(cap_entries, torch.int64)
        self.flags = o(cap_entries, torch.uint8)
        self.create_ts = o(cap_entries, torch.int64)
        self.expire_ts = o(cap_entries, torch.int64)
        self.bad_block = o(nblocks + 1, torch.int32)
        self.summary = torch.zeros(64, dtype=torch.uint8, device=device)
        self.out = _abi.DecodedOut(self.block_entry_start.data_ptr(), self.key_arena.data_ptr(), key_cap,
                                   self.key_off.data_ptr(), self.val_off.data_ptr(), self.val_len.data_ptr(),
                                   self.seq.data_ptr(), self.flags.data_ptr(), self.create_ts.data_ptr(),
                                   self.expire_ts.data_ptr(), cap_entries, self.bad_block.data_ptr(),
                                   nblocks + 1, self.summary.data_ptr())
        wsb = lib().sdb_decode_workspace_bytes(nblocks)
        self.workspace = torch.empty(max(wsb, 256), dtype=torch.uint8, device=device)

    def summary_host(self):
        return _abi.DecodeSummary.from_buffer_copy(self.summary.cpu().numpy().tobytes()[:C.sizeof(_abi.DecodeSummary)])

    def to_host(self):
        """A Decoded with the same fields as Decoder.decode (numpy)."""
        sm = self.summary_host()
        d = Decoded()
        d.status = sm.status
        d.summary = {f: getattr(sm, f) for f, _ in _abi.DecodeSummary._fields_}
        n = sm.num_entries if sm.status in (0, 3, 4, 9) else 0
        d.n = n
        v = lambda t, k, dt: t[:k].cpu().numpy().view(dt)
        d.block_entry_start = v(self.block_entry_start, self.nblocks + 1, np.uint64)
        d.key_off = v(self.key_off, n + 1, np.uint64)
        d.key_arena = v(self.key_arena, sm.key_bytes, np.uint8)
        d.val_off = v(self.val_off, n, np.uint64)
        d.val_len = v(self.val_len, n, np.uint32)
        d.seq = v(self.seq, n, np.uint64)
        d.flags = v(self.flags, n, np.uint8)
        d.create_ts = v(self.create_ts, n, np.int64)
        d.expire_ts = v(self.expire_ts, n, np.int64)
        d.bad_block = v(self.bad_block, min(sm.num_bad_blocks, self.nblocks + 1), np.uint32)
        return d


def decode_blocks_at_device(arena, block_start, block_end, nblocks, out, sst_version=2, stream=None):
    """Enqueue sdb_decode_blocks_at: blocks at arbitrary places of one device arena (torch tensors)."""
    sp = None
    if stream is not None:
        sp = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    st = lib().sdb_decode_blocks_at(arena.data_ptr(), block_start.data_ptr(), block_end.data_ptr(), nblocks,
                                    sst_version, C.byref(out.out), out.workspace.data_ptr(), out.workspace.numel(), sp)
    if st:
        raise SdbError(st, "sdb_decode_blocks_at")


def decode_blocks_ex_device(arena, block_start, block_end, nblocks, out, sst_version=2, descending=False, stream=None,
                            fail_fast=False):
    """Enqueue sdb_decode_blocks_ex (block_end None: contiguous blocks, block_start has nblocks + 1 entries).
    fail_fast: read_blocks semantics (SDB_DECODE_FAIL_FAST: columns unspecified when the call fails)."""
    flags = (_abi.DECODE_DESCENDING if descending else 0) | (_abi.DECODE_FAIL_FAST if fail_fast else 0)
    st = lib().sdb_decode_blocks_ex(arena.data_ptr(), block_start.data_ptr(),
                                    None if block_end is None else block_end.data_ptr(), nblocks, sst_version, flags,
                                    C.byref(out.out), out.workspace.data_ptr(), out.workspace.numel(), _sp(stream))
    if st:
        raise SdbError(st, "sdb_decode_blocks_ex")


def decompress_blocks_device(codec, blocks, block_off, stream=None):
    """Compressed blocks -> a plain block run (sdb_decompress_plan + sdb_decompress_blocks; the first half
    of decode_block, format/sst.rs:980-999).  blocks: device u8 tensor, block_off: device int64 tensor of
    nblocks + 1.  Synchronises once to size the output.  Returns (out, out_start, out_end, err) device
    tensors (err: block << 8 | status of the first failing block, ~0 none) — decode them with
    decode_blocks_at_device(out, out_start, out_end, ...)."""
    import torch
    dev = blocks.device
    nb = block_off.numel() - 1
    sp = _sp(stream)
    ws = torch.empty(int(lib().sdb_decompress_workspace_bytes(nb)), dtype=torch.uint8, device=dev)
    out_start = torch.empty(nb + 1, dtype=torch.int64, device=dev)
    st = lib().sdb_decompress_plan(codec, blocks.data_ptr(), block_off.data_ptr(), nb, out_start.data_ptr(),
                                   ws.data_ptr(), ws.numel(), sp)
    if st:
        raise SdbError(st, "sdb_decompress_plan")
    if stream is not None and hasattr(stream, "synchronize"):
        stream.synchronize()
    else:
        torch.cuda.synchronize(dev)
    total = int(out_start[nb].item())
    out = torch.empty(max(total, 1) + 16, dtype=torch.uint8, device=dev)
    out_end = torch.empty(max(nb, 1), dtype=torch.int64, device=dev)
    err = torch.empty(1, dtype=torch.int64, device=dev)
    st = lib().sdb_decompress_blocks(codec, blocks.data_ptr(), block_off.data_ptr(), nb, out.data_ptr(), total,
                                     out_start.data_ptr(), out_end.data_ptr(), err.data_ptr(), sp)
    if st:
        raise SdbError(st, "sdb_decompress_blocks")
    return out, out_start, out_end[:nb], err


def decompress_blocks_once_device(codec, blocks, block_off, slot_bytes, out_cap=None, stream=None, out=None):
    """sdb_decompress_blocks_once: decompress_blocks_device without the host synchronisation between the plan
    and the run.  Zlib inflates every block once into a slot of slot_bytes and re-plans only the blocks that
    overflowed theirs (packed after the slots; out_start then is not monotone, out_start[nblocks] = the bytes
    used); the other codecs run plan + run back to back.  out_cap defaults to nblocks * slot_bytes plus the
    compressed section's length * 8 for overflows.  Returns (out, out_start, out_end, err) as
    decompress_blocks_device."""
    import torch
    dev = blocks.device
    nb = block_off.numel() - 1
    if out_cap is None:
        out_cap = nb * slot_bytes + 8 * int(blocks.numel()) + 64
    ws = torch.empty(int(lib().sdb_decompress_once_workspace_bytes(nb)), dtype=torch.uint8, device=dev)
    if out is None:
        out = torch.empty(max(out_cap, 1) + 16, dtype=torch.uint8, device=dev)
    out_start = torch.empty(nb + 1, dtype=torch.int64, device=dev)
    out_end = torch.empty(max(nb, 1), dtype=torch.int64, device=dev)
    err = torch.empty(1, dtype=torch.int64, device=dev)
    st = lib().sdb_decompress_blocks_once(codec, blocks.data_ptr(), block_off.data_ptr(), nb, slot_bytes,
                                          out.data_ptr(), out_cap, out_start.data_ptr(), out_end.data_ptr(),
                                          err.data_ptr(), ws.data_ptr(), ws.numel(), _sp(stream))
    if st:
        raise SdbError(st, "sdb_decompress_blocks_once")
    return out, out_start, out_end[:nb], err


def compress_blocks_device(codec, blocks, block_off, in_bytes=None, out_cap=None, stream=None):
    """An encoded data section -> the same blocks compressed (sdb_compress_blocks; compress_and_transform,
    format/sst.rs:525-594).  blocks: device u8 tensor, block_off: device int64 tensor of nblocks + 1.
    Returns (out, out_off, err) device tensors; out_off[nblocks] = the compressed section's length."""
    import torch
    dev = blocks.device
    nb = block_off.numel() - 1
    if in_bytes is None:
        in_bytes = int(block_off[nb].item() - block_off[0].item()) if nb else 0
    if out_cap is None:
        out_cap = in_bytes + in_bytes // 8 + 64 * (nb + 1)
    ws = torch.empty(int(lib().sdb_compress_workspace_bytes(nb, in_bytes)), dtype=torch.uint8, device=dev)
    out = torch.empty(max(out_cap, 1) + 16, dtype=torch.uint8, device=dev)
    out_off = torch.empty(nb + 1, dtype=torch.int64, device=dev)
    err = torch.empty(1, dtype=torch.int64, device=dev)
    st = lib().sdb_compress_blocks(codec, blocks.data_ptr(), block_off.data_ptr(), nb, in_bytes, out.data_ptr(), out_cap,
                                   out_off.data_ptr(), err.data_ptr(), ws.data_ptr(), ws.numel(), _sp(stream))
    if st:
        raise SdbError(st, "sdb_compress_blocks")
    return out, out_off, err


LOOKUP_FIELDS = (("state", "uint8"), ("status", "int32"), ("block", "int32"), ("entry", "int32"),
                 ("key_len", "int32"), ("val_off", "int64"), ("val_len", "int32"), ("seq", "int64"),
                 ("flags", "uint8"), ("create_ts", "int64"), ("expire_ts", "int64"))


def sst_lookup_device(view_tensors, key_bytes, key_off, nkeys, descending=False, stream=None):
    """sdb_sst_lookup over device tensors.  view_tensors: dict with data, block_off, index_keys,
    index_key_off (torch device tensors), num_blocks, sst_version and optionally bloom (device
    tensor) + num_probes.  Returns a dict of device result tensors (LOOKUP_FIELDS)."""
    import torch
    dev = key_bytes.device
    vt = view_tensors
    bloom = vt.get("bloom")
    v = _abi.SstView(vt["data"].data_ptr(), vt["block_off"].data_ptr(), vt["num_blocks"],
                     vt["index_keys"].data_ptr(), vt["index_key_off"].data_ptr(),
                     bloom.data_ptr() if bloom is not None else None,
                     int(vt.get("bloom_len", 0)) if bloom is not None else 0, int(vt.get("num_probes", 0)),
                     int(vt.get("sst_version", 2)), 0)
    res = {f: torch.zeros(max(nkeys, 1), dtype=getattr(torch, dt), device=dev) for f, dt in LOOKUP_FIELDS}
    out = _abi.LookupOut(*[res[f].data_ptr() for f, _ in LOOKUP_FIELDS])
    wsb = lib().sdb_sst_lookup_workspace_bytes(vt["num_blocks"], nkeys)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    sp = None
    if stream is not None:
        sp = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
    st = lib().sdb_sst_lookup(C.byref(v), key_bytes.data_ptr(), key_off.data_ptr(), nkeys, int(bool(descending)),
                              C.byref(out), ws.data_ptr(), wsb, sp)
    if st:
        raise SdbError(st, "sdb_sst_lookup")
    res["_ws"] = ws
    return res


SCAN_COLUMNS = (("val_off", "int64"), ("val_len", "int32"), ("seq", "int64"), ("flags", "uint8"),
                ("create_ts", "int64"), ("expire_ts", "int64"))


def scan_ranges_columnar(ranges):
    """[(start, start_kind, end, end_kind), ...] (keys: bytes or None, kinds: _abi.BOUND_*) -> the host
    arrays of sdb_scan_ranges: dict of start_bytes, start_off, start_kind, end_bytes, end_off, end_kind."""
    n = len(ranges)
    out = {}
    for side, ki, kk in (("start", 0, 1), ("end", 2, 3)):
        keys = [bytes(r[ki] or b"") for r in ranges]
        off = np.zeros(n + 1, np.uint64)
        if n:
            off[1:] = np.cumsum([len(k) for k in keys])
        out[side + "_bytes"] = np.frombuffer(b"".join(keys) or b"\0", np.uint8).copy()
        out[side + "_off"] = off
        out[side + "_kind"] = np.array([int(r[kk]) for r in ranges] or [0], np.uint8)
    return out


def sst_scan_device(view_tensors, ranges, descending=False, stream=None, cap_entries=None, key_cap=None):
    """sdb_sst_scan over device tensors.  view_tensors: as sst_lookup_device.  ranges: a list of (start,
    start_kind, end, end_kind), or a dict of device tensors named as scan_ranges_columnar's arrays plus
    "n".  Returns a dict of device tensors: range_entry_start (n + 1), range_block (2 n), range_status,
    key_arena, key_off, the SCAN_COLUMNS and summary (the sdb_scan_summary words: num_entries, key_bytes,
    num_failed_ranges, blocks_read, status).  With cap_entries / key_cap None the call runs once with
    empty columns, reads the summary (a host synchronisation), allocates exactly and runs again."""
    import torch
    vt = view_tensors
    dev = vt["data"].device
    if isinstance(ranges, dict):
        rt, n = ranges, int(ranges["n"])
    else:
        n = len(ranges)
        rt = {}
        for k, a in scan_ranges_columnar(ranges).items():
            rt[k] = torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
    v = _abi.SstView(vt["data"].data_ptr(), vt["block_off"].data_ptr(), vt["num_blocks"],
                     vt["index_keys"].data_ptr(), vt["index_key_off"].data_ptr(), None, 0, 0,
                     int(vt.get("sst_version", 2)), 0)
    rg = _abi.ScanRanges(n, rt["start_bytes"].data_ptr(), rt["start_off"].data_ptr(), rt["start_kind"].data_ptr(),
                         rt["end_bytes"].data_ptr(), rt["end_off"].data_ptr(), rt["end_kind"].data_ptr())
    res = {"range_entry_start": torch.zeros(n + 1, dtype=torch.int64, device=dev),
           "range_block": torch.zeros(max(2 * n, 1), dtype=torch.int32, device=dev),
           "range_status": torch.zeros(max(n, 1), dtype=torch.int32, device=dev),
           "summary": torch.zeros(5, dtype=torch.int64, device=dev)}
    wsb = lib().sdb_sst_scan_workspace_bytes(vt["num_blocks"], n)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)

    def run(ce, kc):
        res["key_arena"] = torch.zeros(max(kc, 1), dtype=torch.uint8, device=dev)
        res["key_off"] = torch.zeros(ce + 1, dtype=torch.int64, device=dev)
        for f, dt in SCAN_COLUMNS:
            res[f] = torch.zeros(max(ce, 1), dtype=getattr(torch, dt), device=dev)
        out = _abi.ScanOut(res["range_entry_start"].data_ptr(), res["range_block"].data_ptr(),
                           res["range_status"].data_ptr(), res["key_arena"].data_ptr(), kc,
                           res["key_off"].data_ptr(), *[res[f].data_ptr() for f, _ in SCAN_COLUMNS], ce,
                           res["summary"].data_ptr())
        st = lib().sdb_sst_scan(C.byref(v), C.byref(rg), int(bool(descending)), C.byref(out), ws.data_ptr(), wsb,
                                _sp(stream))
        if st:
            raise SdbError(st, "sdb_sst_scan")

    if cap_entries is None or key_cap is None:
        run(0 if cap_entries is None else cap_entries, 0 if key_cap is None else key_cap)
        _sync(stream, dev)
        sm = res["summary"].cpu().numpy()
        if int(sm[4]) & 0xFFFFFFFF == _abi.SDB_LIMIT_EXCEEDED:
            run(max(int(sm[0]), cap_entries or 0), max(int(sm[1]), key_cap or 0))
    else:
        run(cap_entries, key_cap)
    res["_ws"], res["_ranges"] = ws, rt
    return res


GET_FIELDS = (("state", "uint8"), ("status", "int32"), ("sst", "int32"), ("block", "int32"), ("val_off", "int64"),
              ("val_len", "int32"), ("seq", "int64"), ("flags", "uint8"), ("create_ts", "int64"),
              ("expire_ts", "int64"), ("ssts_read", "int32"), ("ssts_filtered", "int32"))
GET_SUMMARY = ("num_found", "num_deleted", "num_not_found", "num_merge", "num_failed", "blocks_checked", "status")


def keys_columnar(keys):
    """[bytes, ...] -> (key_bytes uint8, key_off uint64) host arrays."""
    off = np.zeros(len(keys) + 1, np.uint64)
    if keys:
        off[1:] = np.cumsum([len(k) for k in keys])
    return np.frombuffer(b"".join(keys) or b"\0", np.uint8).copy(), off


def _to_dev(array, dev):
    """A host array as a tensor on dev; uint64 goes as int64, bit for bit (torch has no uint64 to speak of)."""
    import torch
    return torch.from_numpy(array.view(np.int64) if array.dtype == np.uint64 else array).to(dev)


def lsm_tree_device(views, runs, device=None):
    """The device-resident sdb_lsm_view of a tree.  views: per-SST tensor dicts in search order, as
    sst_lookup_device takes them plus first_key / last_key (bytes: SsTableInfo.first_entry / last_entry;
    absent or None for an SST without entries) and optionally policy: (prefix_kind, prefix_arg, no_whole_key),
    what the SST's filter was built with (absent: the plain whole-key policy), which the filtered reads
    (lsm_scan_filtered_device, lsm_get_filtered_device) take as "_policies" (None when no view has one).  runs:
    the number of SSTs of each run, newest run first (an L0 SST is a run of one).  Returns a dict: "lsm" (the
    _abi.LsmView), num_ssts, num_runs, total_blocks and, under "_"-prefixed keys, the device arrays it points
    into."""
    import torch
    ns = len(views)
    assert sum(runs) == ns and all(r >= 0 for r in runs), "runs must partition the views"
    dev = device if device is not None else (views[0]["data"].device if ns else "cuda")
    arr = (_abi.SstView * max(ns, 1))()
    for i, vt in enumerate(views):
        bloom = vt.get("bloom")
        arr[i] = _abi.SstView(vt["data"].data_ptr(), vt["block_off"].data_ptr(), vt["num_blocks"],
                              vt["index_keys"].data_ptr(), vt["index_key_off"].data_ptr(),
                              bloom.data_ptr() if bloom is not None else None,
                              int(vt.get("bloom_len", 0)) if bloom is not None else 0, int(vt.get("num_probes", 0)),
                              int(vt.get("sst_version", 2)), 0)
    dv = lambda a: _to_dev(a, dev)  # noqa: E731
    fkb, fko = keys_columnar([bytes(vt.get("first_key") or b"") for vt in views])
    lkb, lko = keys_columnar([bytes(vt.get("last_key") or b"") for vt in views])
    t = {"_views": views,
         "_ssts": dv(np.frombuffer(bytes(arr), np.uint8).copy()),
         "_run_start": dv(np.concatenate([[0], np.cumsum(runs)]).astype(np.int32)),
         "_first_key_bytes": dv(fkb), "_first_key_off": dv(fko), "_last_key_bytes": dv(lkb), "_last_key_off": dv(lko),
         "_block_base": dv(np.concatenate([[0], np.cumsum([int(vt["num_blocks"]) for vt in views])]).astype(np.uint64))}
    total = sum(int(vt["num_blocks"]) for vt in views)
    t["lsm"] = _abi.LsmView(t["_ssts"].data_ptr(), ns, len(runs), t["_run_start"].data_ptr(),
                            t["_first_key_bytes"].data_ptr(), t["_first_key_off"].data_ptr(),
                            t["_last_key_bytes"].data_ptr(), t["_last_key_off"].data_ptr(),
                            t["_block_base"].data_ptr(), total)
    t["_policies"] = None
    if any(vt.get("policy") is not None for vt in views):
        pol = np.zeros((ns, 4), np.uint32)
        for i, vt in enumerate(views):
            pol[i, :3] = vt.get("policy") or (0, 0, 0)
        t["_policies"] = dv(pol.view(np.int32).reshape(-1))
    t.update(num_ssts=ns, num_runs=len(runs), total_blocks=total, device=dev)
    return t


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _limit_exceeded(summary, word):
    return int(summary.cpu().numpy()[word]) & 0xFFFFFFFF == _abi.SDB_LIMIT_EXCEEDED


def projections_columnar(visible):
    """[SsTableView.visible_range per SST: None (the whole SST) or (start, start_kind, end, end_kind)] -> the host
    arrays of the sdb_scan_ranges that the projected reads take as `proj`, as scan_ranges_columnar names them;
    None becomes (UNBOUNDED, UNBOUNDED)."""
    return scan_ranges_columnar([v if v is not None else (None, _abi.BOUND_UNBOUNDED, None, _abi.BOUND_UNBOUNDED)
                                 for v in visible])


def _projections(projections, tree):
    """The `proj` argument of a projected read: None, one visible range (or None) per SST of the tree, or a dict of
    device tensors named as projections_columnar's arrays plus "n" -> (the tensors kept alive, the _abi.ScanRanges
    or None)."""
    if projections is None:
        return None, None
    if isinstance(projections, dict):
        pt, n = projections, int(projections["n"])
    else:
        assert len(projections) == tree["num_ssts"], "one visible range (or None) per SST"
        n = len(projections)
        pt = {k: _to_dev(a, tree["device"]) for k, a in projections_columnar(projections).items()}
    return pt, _abi.ScanRanges(n, _ptr(pt["start_bytes"]), _ptr(pt["start_off"]), _ptr(pt["start_kind"]),
                               _ptr(pt["end_bytes"]), _ptr(pt["end_off"]), _ptr(pt["end_kind"]))


# The ten tree reads: symbol -> (the entry point's arguments, its sizer's), in C order, each under the name _lsm_get and
# _lsm_scan marshal it by; every entry point ends with (workspace, workspace_bytes, stream).  What a symbol takes is
# what its tuple names: policies and probe_len / prefixes and fout from _filtered on, proj from _projected on, mem,
# mout and mchain for _mem; a sizer takes merge where the entry point's chain is optional.
_TREE, _CAND, _KEYS = ("total_blocks", "num_ssts", "num_runs", "n"), ("ce", "ckb"), ("key_bytes", "key_off", "n")
_SCAN = ("max_seq", "descending") + _CAND + ("out",)
READ_CALLS = {
    "sdb_lsm_get": (("lsm",) + _KEYS + ("max_seq", "out"), _TREE),
    "sdb_lsm_get_merge": (("lsm",) + _KEYS + ("max_seq", "out", "chain"), _TREE),
    "sdb_lsm_get_filtered": (("lsm", "policies") + _KEYS + ("probe_len", "max_seq", "out", "chain"), _TREE + ("merge",)),
    "sdb_lsm_get_projected": (("lsm", "proj", "policies") + _KEYS + ("probe_len", "max_seq", "out", "chain"),
                              _TREE + ("merge",)),
    "sdb_lsm_get_mem": (("mem", "lsm", "proj", "policies") + _KEYS + ("probe_len", "max_seq", "out", "mout", "chain", "mchain"),
                        ("num_tables",) + _TREE + ("merge",)),
    "sdb_lsm_scan": (("lsm", "ranges") + _SCAN, _TREE + _CAND),
    "sdb_lsm_scan_merge": (("lsm", "ranges") + _SCAN + ("chain",), _TREE + _CAND),
    "sdb_lsm_scan_filtered": (("lsm", "policies", "ranges", "prefixes") + _SCAN + ("chain", "fout"), _TREE + _CAND + ("merge",)),
    "sdb_lsm_scan_projected": (("lsm", "proj", "policies", "ranges", "prefixes") + _SCAN + ("chain", "fout"),
                               _TREE + _CAND + ("merge",)),
    "sdb_lsm_scan_mem": (("mem", "lsm", "proj", "policies", "ranges", "prefixes") + _SCAN + ("mout", "chain", "mchain", "fout"),
                         ("num_tables",) + _TREE + _CAND + ("merge",)),
}
# The read that is no get and no merging scan, marshalled by _lsm_scan like them: limit and rout are its own.
RECENCY_CALLS = {
    "sdb_lsm_scan_recency": (("mem", "lsm", "proj", "policies", "ranges", "prefixes", "max_seq", "limit", "descending") + _CAND +
                             ("out", "mout", "fout", "rout"), ("num_tables",) + _TREE + _CAND),
}


def _read_args(entry):
    return READ_CALLS[entry] if entry in READ_CALLS else RECENCY_CALLS[entry]


def _read_workspace_bytes(entry, v):
    """What entry's sizer answers for the marshalled values v."""
    return getattr(lib(), entry + "_workspace_bytes")(*[v[a] for a in _read_args(entry)[1]])


def _read_call(entry, v, ws, wsb, stream):
    """The C call of a tree read over the marshalled values v; raises SdbError on a status."""
    st = getattr(lib(), entry)(*[v[a] for a in _read_args(entry)[0]], ws.data_ptr(), wsb, _sp(stream))
    if st:
        raise SdbError(st, entry)


def _byref(struct):
    return C.byref(struct) if struct is not None else None


def _read_values(tree, mem, pj, merge):
    """What both families marshal alike: the tables (mem_tables_device's, or None), the tree and its shape, the
    projections (_projections' struct, or None), the policies and the sizers' merge."""
    return {"mem": _byref(mem["mem"] if mem else None), "num_tables": mem["num_tables"] if mem else 0,
            "lsm": C.byref(tree["lsm"]), "total_blocks": tree["total_blocks"], "num_ssts": tree["num_ssts"],
            "num_runs": tree["num_runs"], "proj": _byref(pj), "policies": _ptr(tree.get("_policies")),
            "merge": int(bool(merge))}


def read_workspace_bytes(entry, tree, n, cand=(0, 0), merge=False, tables=None):
    """What entry + "_workspace_bytes" answers for a call of the tree read `entry` (a key of READ_CALLS or
    RECENCY_CALLS) over tree (what lsm_tree_device built) with n keys or ranges; for a scan cand = (cand_entries,
    cand_key_bytes); merge: the call has a chain; tables: what mem_tables_device returned, or None.  A sizer takes
    of these what its tuple names."""
    v = _read_values(tree, tables, None, merge)
    v.update(n=n, ce=cand[0], ckb=cand[1])
    return _read_workspace_bytes(entry, v)


def _read_output(dev, name, count, dtype, fill):
    """Where every output of a tree read comes from, and the contract of the eleven lsm_*_device wrappers' alloc=:
    alloc(name, count, dtype, fill) -> a 1-D tensor of dtype on the tree's device with at least count elements.
    name: the output's key in the result dict ("range_status", "key_arena", "chain_seq", "table", "summary", ...;
    "_ws": a workspace the call allocates itself).  count: its logical element count (n + 1, cap_entries,
    key_arena_cap, cap_links, the summary's words, ...), which may be 0.  fill: the byte every element starts as: 0,
    the caller's fill= for the link columns, 0xFF for a scan's table (rows that no call writes name no table), or
    None where the call writes every element it later reads.  A call that retries asks again for what it sizes anew.
    The C call gets the pointers and the capacities it was asked for, so what lies beyond count is never written:
    an allocator may hand out slices of a pool of its own, or arrays inside guard bytes.  This one, the default,
    returns a fresh tensor of max(count, 1) elements."""
    import torch
    if fill is None:
        return torch.empty(max(count, 1), dtype=dtype, device=dev)
    if fill == 0:
        return torch.zeros(max(count, 1), dtype=dtype, device=dev)
    return torch.full((max(count, 1) * dtype.itemsize,), fill, dtype=torch.uint8, device=dev).view(dtype)


def _lsm_get(entry, views, runs, keys, max_seq, stream, workspace, merge=False, cap_links=None, fill=0, probe_len=None,
             projections=None, mem=None, alloc=None):
    """The tree gets.  entry: the C entry point, a key of READ_CALLS, which names what it takes: the filtered ones
    the policies, probe_len and an optional chain, the projected ones the projections too; merge: the
    call has a chain.  Marshals the tree, the keys, the bounds and probe_len as device tensors, the result dict with
    the GET_FIELDS and the summary; a caller's workspace must hold the call; with merge and cap_links None the links
    are sized at nkeys first and, when they did not fit, at the reported num_links in a second call.  mem: for
    sdb_lsm_get_mem: None (a NULL sdb_mem_view) or what mem_tables_device returned; the result then has table and
    row (MEM_FIELDS) and, with a chain, chain_table and chain_row.  alloc: see _read_output."""
    import torch
    takes = READ_CALLS[entry][0]
    tree = views if isinstance(views, dict) else lsm_tree_device(views, runs)
    dev = tree["device"]
    new = alloc or functools.partial(_read_output, dev)
    if isinstance(keys, (tuple, list)) and len(keys) == 3 and hasattr(keys[0], "data_ptr"):
        kb, ko, n = keys
    else:
        n = len(keys)
        kb, ko = (_to_dev(a, dev) for a in keys_columnar([bytes(k) for k in keys]))
    if max_seq is not None and not hasattr(max_seq, "data_ptr"):
        max_seq = _to_dev(np.asarray(max_seq, np.uint64).copy(), dev)
    if probe_len is not None and not hasattr(probe_len, "data_ptr"):
        probe_len = _to_dev(np.asarray(list(probe_len) or [0], np.int32), dev)
    res = {f: new(f, n, getattr(torch, dt), 0) for f, dt in GET_FIELDS}
    res["summary"] = new("summary", len(GET_SUMMARY), torch.int64, 0)
    pjt, pj = _projections(projections, tree)
    v = _read_values(tree, mem, pj, merge)
    v.update(key_bytes=kb.data_ptr(), key_off=ko.data_ptr(), n=n, probe_len=_ptr(probe_len), max_seq=_ptr(max_seq),
             out=C.byref(_abi.GetOut(*[res[f].data_ptr() for f, _ in GET_FIELDS], res["summary"].data_ptr())))
    if "mout" in takes:
        for f, dt in MEM_FIELDS:  # (every call writes all n of them: no fill)
            res[f] = new(f, n, getattr(torch, dt), None)
        v["mout"] = C.byref(_abi.MemGetOut(*[res[f].data_ptr() for f, _ in MEM_FIELDS]))
    wsb = read_workspace_bytes(entry, tree, n, merge=merge, tables=mem)
    ws = workspace if workspace is not None else new("_ws", wsb, torch.uint8, None)
    assert ws.numel() >= wsb, "workspace too small"

    def run(cap):
        v["chain"] = C.byref(_chain_out(res, n, cap, new, fill)) if merge else None
        v["mchain"] = C.byref(_mem_chain_out(res, cap, new, fill)) if merge and "mchain" in takes else None
        _read_call(entry, v, ws, wsb, stream)

    if merge and cap_links is None:
        run(n)  # one link per query is the least a tree of values needs
        _sync(stream, dev)
        if _limit_exceeded(res["chain_summary"], 2):
            run(int(res["chain_summary"][0].item()))
    else:
        run(cap_links or 0)
    res.update(_ws=ws, _tree=tree, _keys=(kb, ko), _max_seq=max_seq, _probe_len=probe_len, _projections=pjt, _mem=mem)
    return res


def lsm_get_device(views, runs, keys, max_seq=None, stream=None, workspace=None, alloc=None):
    """sdb_lsm_get: a batch of Db::get over a device-resident tree.  views, runs: as lsm_tree_device, or
    views = a tree lsm_tree_device built (runs is then ignored).  keys: a list of bytes, or device tensors
    (key_bytes, key_off, nkeys).  max_seq: None (no bound), a list / array of nkeys bounds, or a device
    int64 tensor.  workspace: a device uint8 tensor to use (and reuse) instead of a fresh one.  With device
    tensors and a prebuilt tree the call copies nothing from the host, so it can be captured into a graph.  Returns a dict of device tensors (GET_FIELDS, and summary: the
    sdb_get_summary words in GET_SUMMARY order); what the call allocated stays alive under "_" keys.  alloc: where
    the outputs come from (see _read_output); None: fresh tensors."""
    return _lsm_get("sdb_lsm_get", views, runs, keys, max_seq, stream, workspace, alloc=alloc)


LSM_SCAN_COLUMNS = (("sst", "int32"),) + SCAN_COLUMNS
LSM_SCAN_SUMMARY = ("num_entries", "key_bytes", "num_candidates", "candidate_key_bytes", "num_failed_ranges",
                    "blocks_checked", "status")


def _lsm_scan_out(res, cap_e, cap_k, new):
    """Fresh row columns for cap_e rows and cap_k key bytes in res, and the sdb_lsm_scan_out over res."""
    import torch
    res["key_arena"] = new("key_arena", cap_k, torch.uint8, 0)
    res["key_off"] = new("key_off", cap_e + 1, torch.int64, 0)
    for f, dt in LSM_SCAN_COLUMNS:
        res[f] = new(f, cap_e, getattr(torch, dt), 0)
    out = _abi.LsmScanOut(res["range_entry_start"].data_ptr(), res["range_status"].data_ptr(),
                          res["range_ssts"].data_ptr(), res["key_arena"].data_ptr(), cap_k,
                          res["key_off"].data_ptr(), *[res[f].data_ptr() for f, _ in LSM_SCAN_COLUMNS], cap_e,
                          res["summary"].data_ptr())
    return out


def _lsm_scan(entry, tree, ranges, max_seq, descending, stream, workspace, cand, cap, merge=False, cap_links=None, fill=0,
              prefixes=None, probe_len=None, projections=None, mem=None, limit=None, alloc=None):
    """The tree scans.  entry: the C entry point, a key of READ_CALLS, which names what it takes: the filtered ones
    the policies, the prefixes, an optional chain and the filter outputs, the projected ones the projections too; merge:
    the call has a chain.  Marshals the ranges, the bounds, the prefixes and the projections as device tensors and the
    result dict; a caller's workspace that is too small is replaced by a fresh one, unless cand was given.
    With a capacity None (cap_links counts only with merge) the call runs once, and on SDB_LIMIT_EXCEEDED again
    with the staging at max(given, reported), cap like the staging and cap_links like cand_entries where those
    were None.  mem: for sdb_lsm_scan_mem: None (a NULL sdb_mem_view) or what mem_tables_device returned; the
    result then has table and row per output row (MEM_FIELDS), range_tables and, with a chain, chain_table and
    chain_row.  limit: for sdb_lsm_scan_recency: None, a list / array of n row limits, or a device int64 tensor; the
    result then has range_sources_read and range_visible.  alloc: see _read_output."""
    import torch
    takes = _read_args(entry)[0]
    dev = tree["device"]
    new = alloc or functools.partial(_read_output, dev)
    if isinstance(ranges, dict):
        rt, n = ranges, int(ranges["n"])
    else:
        n = len(ranges)
        rt = {k: _to_dev(a, dev) for k, a in scan_ranges_columnar(ranges).items()}
    if max_seq is not None and not hasattr(max_seq, "data_ptr"):
        max_seq = _to_dev(np.asarray(list(max_seq) or [0], np.uint64), dev)
    rg = _abi.ScanRanges(n, rt["start_bytes"].data_ptr(), rt["start_off"].data_ptr(), rt["start_kind"].data_ptr(),
                         rt["end_bytes"].data_ptr(), rt["end_off"].data_ptr(), rt["end_kind"].data_ptr())
    res = {"range_entry_start": new("range_entry_start", n + 1, torch.int64, 0),
           "range_status": new("range_status", n, torch.int32, 0), "range_ssts": new("range_ssts", n, torch.int32, 0),
           "summary": new("summary", len(LSM_SCAN_SUMMARY), torch.int64, 0)}
    pjt, pj = _projections(projections, tree)
    v = _read_values(tree, mem, pj, merge)
    v.update(ranges=C.byref(rg), n=n, max_seq=_ptr(max_seq), descending=int(bool(descending)))
    pt = prefixes
    if "prefixes" in takes:
        if prefixes is not None and not isinstance(prefixes, dict):
            assert len(prefixes) == n, "one prefix (or None) per range"
            pt = {k: None if a is None else _to_dev(a, dev) for k, a in scan_prefixes_columnar(prefixes, probe_len).items()}
        v["prefixes"] = _byref(None if pt is None else _abi.ScanPrefixes(
            _ptr(pt["prefix_bytes"]), _ptr(pt["prefix_off"]), _ptr(pt["has_prefix"]), _ptr(pt.get("probe_len"))))
    if "fout" in takes:
        res["range_filtered"] = new("range_filtered", n, torch.int32, 0)
        res["num_filtered"] = new("num_filtered", 1, torch.int64, 0)
        v["fout"] = C.byref(_abi.ScanFilterOut(res["range_filtered"].data_ptr(), res["num_filtered"].data_ptr()))
    if "mout" in takes:
        res["range_tables"] = new("range_tables", n, torch.int32, 0)
    if "rout" in takes:
        if limit is not None and not hasattr(limit, "data_ptr"):
            limit = _to_dev(np.asarray(list(limit) or [0], np.uint64), dev)
        res["range_sources_read"] = new("range_sources_read", n, torch.int32, 0)
        res["range_visible"] = new("range_visible", n, torch.int64, 0)
        v.update(limit=_ptr(limit),
                 rout=C.byref(_abi.RecencyOut(res["range_sources_read"].data_ptr(), res["range_visible"].data_ptr())))

    def run(ce, ckb, cap_e, cap_k, cap_l):
        v.update(ce=ce, ckb=ckb)
        wsb = read_workspace_bytes(entry, tree, n, (ce, ckb), merge, mem)
        ws = workspace if workspace is not None and workspace.numel() >= wsb else None
        if ws is None:
            assert workspace is None or cand is None, "workspace too small"
            ws = new("_ws", wsb, torch.uint8, None)
        v["out"] = C.byref(_lsm_scan_out(res, cap_e, cap_k, new))
        v["chain"] = C.byref(_chain_out(res, cap_e, cap_l, new, fill)) if merge else None
        if "mout" in takes:  # (rows that no call writes name no table)
            res["table"] = new("table", cap_e, torch.int32, 0xFF)
            res["row"] = new("row", cap_e, torch.int64, 0)
            v["mout"] = C.byref(_abi.MemScanOut(res["table"].data_ptr(), res["row"].data_ptr(), res["range_tables"].data_ptr()))
        v["mchain"] = C.byref(_mem_chain_out(res, cap_l, new, fill)) if merge and "mchain" in takes else None
        _read_call(entry, v, ws, wsb, stream)
        res["_ws"] = ws

    if cand is None or cap is None or (merge and cap_links is None):
        ce, ckb = cand if cand is not None else (0, 0)
        run(ce, ckb, *(cap if cap is not None else (0, 0)), cap_links or 0)
        _sync(stream, dev)
        if _limit_exceeded(res["summary"], 6) or (merge and _limit_exceeded(res["chain_summary"], 2)):
            sm = res["summary"].cpu().numpy()
            ce, ckb = max(ce, int(sm[2])), max(ckb, int(sm[3]))
            run(ce, ckb, *(cap if cap is not None else (ce, ckb)), cap_links if cap_links is not None else ce)
    else:
        run(cand[0], cand[1], cap[0], cap[1], cap_links or 0)
    res.update(_tree=tree, _ranges=rt, _max_seq=max_seq, _prefixes=pt, _projections=pjt, _mem=mem, _limit=limit)
    return res


def lsm_scan_device(tree, ranges, max_seq=None, descending=False, stream=None, workspace=None, cand=None, cap=None,
                    alloc=None):
    """sdb_lsm_scan: a batch of Db::scan over a device-resident tree.  tree: what lsm_tree_device built.
    ranges: a list of (start, start_kind, end, end_kind), or a dict of device tensors named as
    scan_ranges_columnar's arrays plus "n".  max_seq: None (no bound), a list / array of n bounds, or a device
    int64 tensor.  cand: (cand_entries, cand_key_bytes), the staging capacity; cap: (cap_entries, key_arena_cap),
    the column capacity.  With either None the call first runs without staging room, reads the candidate totals
    (a host synchronisation), sizes both like the staging (num_entries <= num_candidates) and runs again; with
    both given, device tensors for ranges and max_seq and a workspace it copies nothing from the host, so it can
    be captured into a graph.  Returns a dict of device tensors: range_entry_start (n + 1), range_status,
    range_ssts, key_arena, key_off, the LSM_SCAN_COLUMNS and summary (the sdb_lsm_scan_summary words in
    LSM_SCAN_SUMMARY order); what the call allocated stays alive under "_" keys.  alloc: where the outputs come from
    (see _read_output); None: fresh tensors."""
    return _lsm_scan("sdb_lsm_scan", tree, ranges, max_seq, descending, stream, workspace, cand, cap, alloc=alloc)


CHAIN_COLUMNS = (("sst", "int32"), ("block", "int32"), ("val_off", "int64"), ("val_len", "int32"), ("seq", "int64"),
                 ("flags", "uint8"), ("create_ts", "int64"), ("expire_ts", "int64"))
CHAIN_SUMMARY = ("num_links", "max_chain_len", "status")


def _chain_out(res, items, cap_links, new, fill=0):
    """The sdb_chain_out of a call over `items` queries or rows with room for cap_links links; its tensors go
    into res as chain_start, chain_<column> and chain_summary."""
    import torch
    res["chain_start"] = new("chain_start", items + 1, torch.int64, 0)
    for f, dt in CHAIN_COLUMNS:  # every byte of the link columns starts as `fill`
        res["chain_" + f] = new("chain_" + f, cap_links, getattr(torch, dt), fill)
    res["chain_summary"] = new("chain_summary", len(CHAIN_SUMMARY), torch.int64, 0)
    return _abi.ChainOut(res["chain_start"].data_ptr(), *[res["chain_" + f].data_ptr() for f, _ in CHAIN_COLUMNS],
                         cap_links, res["chain_summary"].data_ptr())


def lsm_get_merge_device(views, runs, keys, max_seq=None, stream=None, workspace=None, cap_links=None, fill=0, alloc=None):
    """sdb_lsm_get_merge: lsm_get_device for a store with a merge operator.  Besides the GET_FIELDS and the
    summary the result holds the operand chains: chain_start (nkeys + 1), chain_<CHAIN_COLUMNS> per link and
    chain_summary (CHAIN_SUMMARY order).  cap_links: room for the links; None sizes it from a first call (a host
    synchronisation) and calls again when the links did not fit.  With cap_links given, device tensors and a
    workspace the call copies nothing from the host, so it can be captured into a graph.  fill: what the link
    columns hold before the call, byte by byte.  alloc: as lsm_get_device's."""
    return _lsm_get("sdb_lsm_get_merge", views, runs, keys, max_seq, stream, workspace, merge=True, cap_links=cap_links,
                    fill=fill, alloc=alloc)


def lsm_scan_merge_device(tree, ranges, max_seq=None, descending=False, stream=None, workspace=None, cand=None,
                          cap=None, cap_links=None, fill=0, alloc=None):
    """sdb_lsm_scan_merge: lsm_scan_device for a store with a merge operator; arguments as there.  Besides its
    tensors the result holds the rows' operand chains: chain_start (cap_entries + 1, indexed by output row),
    chain_<CHAIN_COLUMNS> per link and chain_summary (CHAIN_SUMMARY order).  cap_links: room for the links; None
    sizes it like the staging (every link is a candidate).  With cand, cap or cap_links None the call retries
    once on SDB_LIMIT_EXCEEDED, after a host synchronisation, as lsm_scan_device does.  alloc: as lsm_scan_device's."""
    return _lsm_scan("sdb_lsm_scan_merge", tree, ranges, max_seq, descending, stream, workspace, cand, cap, merge=True,
                     cap_links=cap_links, fill=fill, alloc=alloc)


def scan_prefixes_columnar(prefixes, probe_len=None):
    """[prefix bytes or None per range] (None: a plain Db::scan, no prefix query) and optionally the
    SDB_PREFIX_LENGTHS answers per range -> the host arrays of sdb_scan_prefixes: dict of prefix_bytes,
    prefix_off, has_prefix and probe_len (None when not given)."""
    kb, ko = keys_columnar([bytes(p or b"") for p in prefixes])
    return {"prefix_bytes": kb, "prefix_off": ko,
            "has_prefix": np.array([p is not None for p in prefixes] or [0], np.uint8),
            "probe_len": None if probe_len is None else np.array(list(probe_len) or [0], np.int32)}


def lsm_scan_filtered_device(tree, ranges, prefixes=None, probe_len=None, max_seq=None, descending=False, stream=None,
                             workspace=None, cand=None, cap=None, cap_links=None, fill=0, merge=False, alloc=None):
    """sdb_lsm_scan_filtered: lsm_scan_device (merge=False) or lsm_scan_merge_device (merge=True) with the SSTs'
    filters consulted under the tree's policies (lsm_tree_device's per-view policy).  prefixes: None (no range has
    a prefix), a list with the scan prefix of every range (bytes: Db::scan_prefix, None: Db::scan), or a dict of
    device tensors named as scan_prefixes_columnar's arrays; probe_len: with a list of prefixes, the per-range
    lengths for SDB_PREFIX_LENGTHS SSTs.  The other arguments, the retry once on SDB_LIMIT_EXCEEDED and the result
    are the unfiltered call's, plus range_filtered (n) and num_filtered (one element).  alloc: as lsm_scan_device's."""
    return _lsm_scan("sdb_lsm_scan_filtered", tree, ranges, max_seq, descending, stream, workspace, cand, cap,
                     merge=bool(merge), cap_links=cap_links, fill=fill, prefixes=prefixes, probe_len=probe_len, alloc=alloc)


def lsm_get_filtered_device(views, runs, keys, probe_len=None, max_seq=None, stream=None, workspace=None, cap_links=None,
                            fill=0, merge=False, alloc=None):
    """sdb_lsm_get_filtered: lsm_get_device (merge=False) or lsm_get_merge_device (merge=True) with every SST's
    filter probed under its policy (lsm_tree_device's per-view policy), so trees written with a prefix extractor or
    without whole-key hashes are served.  probe_len: None, a list / array of nkeys lengths for SDB_PREFIX_LENGTHS
    SSTs (-1: None), or a device int32 tensor.  The other arguments, the retry on links that do not fit and the
    result are the unfiltered call's.  alloc: as lsm_get_device's."""
    return _lsm_get("sdb_lsm_get_filtered", views, runs, keys, max_seq, stream, workspace, merge=bool(merge),
                    cap_links=cap_links, fill=fill, probe_len=probe_len, alloc=alloc)


def lsm_scan_projected_device(tree, projections, ranges, prefixes=None, probe_len=None, max_seq=None, descending=False,
                              stream=None, workspace=None, cand=None, cap=None, cap_links=None, fill=0, merge=False,
                              alloc=None):
    """sdb_lsm_scan_projected: lsm_scan_filtered_device over projected SST views.  projections: None (no SST is
    projected: exactly the filtered call), a list with SsTableView.visible_range of every SST of the tree (None: the
    whole SST, else (start, start_kind, end, end_kind)), or a dict of device tensors named as projections_columnar's
    arrays plus "n".  The other arguments (alloc among them) and the result are the filtered call's."""
    return _lsm_scan("sdb_lsm_scan_projected", tree, ranges, max_seq, descending, stream, workspace, cand, cap,
                     merge=bool(merge), cap_links=cap_links, fill=fill, prefixes=prefixes,
                     probe_len=probe_len, projections=projections, alloc=alloc)


def lsm_get_projected_device(views, runs, projections, keys, probe_len=None, max_seq=None, stream=None, workspace=None,
                             cap_links=None, fill=0, merge=False, alloc=None):
    """sdb_lsm_get_projected: lsm_get_filtered_device over projected SST views; projections as
    lsm_scan_projected_device takes them.  The other arguments (alloc among them) and the result are the filtered
    call's."""
    return _lsm_get("sdb_lsm_get_projected", views, runs, keys, max_seq, stream, workspace, merge=bool(merge),
                    cap_links=cap_links, fill=fill, probe_len=probe_len, projections=projections, alloc=alloc)


MEM_FIELDS = (("table", "int32"), ("row", "int64"))


def _mem_chain_out(res, cap_links, new, fill=0):
    """The sdb_mem_chain_out beside _chain_out's link columns: chain_table and chain_row."""
    import torch
    for f, dt in MEM_FIELDS:
        res["chain_" + f] = new("chain_" + f, cap_links, getattr(torch, dt), fill)
    return _abi.MemChainOut(*[res["chain_" + f].data_ptr() for f, _ in MEM_FIELDS])


def mem_tables_device(runs, device="cuda"):
    """The device-resident sdb_mem_view of memtables in search order (the active one, then the immutable ones front
    first).  runs: DeviceRuns, for example ReplayedTable.as_run(), or _abi.Run structs whose pointers the caller
    keeps alive.  Returns a dict: "mem" (the _abi.MemView), num_tables and, under "_"-prefixed keys, what it points
    into."""
    arr = (_abi.Run * max(len(runs), 1))()
    for i, r in enumerate(runs):
        arr[i] = r.to_ctypes() if hasattr(r, "to_ctypes") else r
    if runs and hasattr(runs[0], "t"):
        device = runs[0].t[0].device
    tabs = _to_dev(np.frombuffer(bytes(arr), np.uint8).copy(), device)
    return {"mem": _abi.MemView(tabs.data_ptr(), len(runs), 0), "num_tables": len(runs), "_tables": tabs, "_runs": runs}


def lsm_get_mem_device(tables, views, runs, keys, max_seq=None, projections=None, probe_len=None, cap_links=None,
                       merge=False, stream=None, workspace=None, fill=0, alloc=None):
    """sdb_lsm_get_mem: lsm_get_projected_device with device memtables searched ahead of the tree.  tables: None
    (a NULL sdb_mem_view), a list of DeviceRuns in search order, or what mem_tables_device returned; views, runs: as
    lsm_tree_device (a tree without SSTs is searched too: the tables alone).  The other arguments (alloc among them),
    the retry on links that do not fit and the result are lsm_get_projected_device's, plus table and row per query
    (table -1: the tree decided, or nothing) and, with merge, chain_table and chain_row per link."""
    mem = tables if tables is None or isinstance(tables, dict) else mem_tables_device(tables)
    return _lsm_get("sdb_lsm_get_mem", views, runs, keys, max_seq, stream, workspace, merge=bool(merge),
                    cap_links=cap_links, fill=fill, probe_len=probe_len, projections=projections, mem=mem, alloc=alloc)


def lsm_scan_mem_device(tables, tree, ranges, projections=None, prefixes=None, probe_len=None, max_seq=None,
                        descending=False, stream=None, workspace=None, cand=None, cap=None, cap_links=None, fill=0,
                        merge=False, alloc=None):
    """sdb_lsm_scan_mem: lsm_scan_projected_device with device memtables merged ahead of the tree.  tables: None (a
    NULL sdb_mem_view), a list of DeviceRuns in search order, or what mem_tables_device returned; tree: what
    lsm_tree_device built (a tree without SSTs is scanned too: the tables alone).  The other arguments (alloc among
    them), the retry once on SDB_LIMIT_EXCEEDED and the result are lsm_scan_projected_device's, plus table and row per
    output row (table -1: an SST holds the row), range_tables (n) and, with merge, chain_table and chain_row per link."""
    mem = tables if tables is None or isinstance(tables, dict) else mem_tables_device(tables, tree["device"])
    return _lsm_scan("sdb_lsm_scan_mem", tree, ranges, max_seq, descending, stream, workspace, cand, cap,
                     merge=bool(merge), cap_links=cap_links, fill=fill, prefixes=prefixes,
                     probe_len=probe_len, projections=projections, mem=mem, alloc=alloc)


def lsm_scan_recency_device(tables, tree, ranges, projections=None, prefixes=None, probe_len=None, max_seq=None, limit=None,
                            descending=False, stream=None, workspace=None, cand=None, cap=None, alloc=None):
    """sdb_lsm_scan_recency: a batch of Db::scan_prefix_by_recency over device memtables and the tree: the sources
    drained one after another, newest first, every visible version a row, tombstones and merge operands included.
    ranges: the prefixes' ranges (prefix_range); prefixes: the prefixes themselves, for the filters.  limit: None
    (every source is drained), a list / array of n row limits (0: drain), or a device int64 tensor.  The other
    arguments (alloc among them), the retry once on SDB_LIMIT_EXCEEDED and the result are lsm_scan_mem_device's without
    the chain, plus range_sources_read and range_visible (n)."""
    mem = tables if tables is None or isinstance(tables, dict) else mem_tables_device(tables, tree["device"])
    return _lsm_scan("sdb_lsm_scan_recency", tree, ranges, max_seq, descending, stream, workspace, cand, cap,
                     prefixes=prefixes, probe_len=probe_len, projections=projections, mem=mem, limit=limit, alloc=alloc)


def prefix_range(prefix):
    """BytesRange::from_prefix: (start, kind, end, kind) of the keys that start with prefix: [prefix, the prefix with
    its last byte below 0xFF incremented and what follows it dropped), unbounded above when every byte is 0xFF."""
    p = bytes(prefix)
    if not p:
        return (None, 0, None, 0)
    end = p.rstrip(b"\xff")
    return (p, 1, end[:-1] + bytes([end[-1] + 1]), 2) if end else (p, 1, None, 0)


# ------------------------------------------------------------------------------------------------
# Compaction (sdb_merge_runs / sdb_sst_cuts / sdb_compactor_*)
# ------------------------------------------------------------------------------------------------
def _sync(stream, dev):
    """Wait for work queued on `stream` (a torch stream, a raw handle or None) before a host read."""
    import torch
    if stream is not None and hasattr(stream, "synchronize"):
        stream.synchronize()
    else:
        torch.cuda.synchronize(dev)  # device-wide: covers a raw stream handle too


def _sp(stream):
    if stream is None:
        return None
    return stream.cuda_stream if hasattr(stream, "cuda_stream") else stream


_hip = None


def _d2h(ptr, nbytes):
    """Copy nbytes at a raw device pointer to a host numpy uint8 array (hipMemcpy D2H)."""
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    out = np.empty(max(nbytes, 1), np.uint8)
    if nbytes:
        st = _hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2)
        if st:
            raise SdbError(_abi.SDB_DEVICE_ERROR, "hipMemcpy D2H")
    return out[:nbytes]


class DeviceRun:
    """A sorted run on the device in the sdb_run layout (torch tensors)."""

    def __init__(self, n, key_arena, key_off, val_base, val_off, val_len, seq, flags, create_ts, expire_ts,
                 key_bytes, val_bytes):
        self.n = n
        self.t = (key_arena, key_off, val_base, val_off, val_len, seq, flags, create_ts, expire_ts)
        self.key_bytes, self.val_bytes = key_bytes, val_bytes

    @classmethod
    def from_host(cls, run, device="cuda"):
        import torch
        up = lambda a: torch.from_numpy(np.concatenate([np.ascontiguousarray(a).view(np.uint8),
                                                        np.zeros(16, np.uint8)])).to(device)
        return cls(run.n, up(run.key_arena), up(run.key_off), up(run.val_base), up(run.val_off), up(run.val_len),
                   up(run.seq), up(run.flags), up(run.create_ts), up(run.expire_ts),
                   int(run.key_off[-1]) if run.n else 0, int(run.val_len.sum()))

    @classmethod
    def from_decoded(cls, dout, blocks, n):
        """A DeviceDecodeOutput of `n` entries whose values live in the `blocks` device tensor."""
        sm = dout.summary_host()
        vb = int(dout.val_len[:n].to(dtype=__import__("torch").int64).sum().item()) if n else 0
        return cls(n, dout.key_arena, dout.key_off, blocks, dout.val_off, dout.val_len, dout.seq, dout.flags,
                   dout.create_ts, dout.expire_ts, int(sm.key_bytes), vb)

    def to_ctypes(self):
        return _abi.Run(self.n, *[t.data_ptr() for t in self.t])


def merge_runs_device(druns, ret, stream=None):
    """sdb_merge_runs over DeviceRuns -> (dict of device tensors of the merged batch, MergeSummary)."""
    import torch
    dev = druns[0].t[0].device if druns else "cuda"
    total = sum(r.n for r in druns)
    kcap = sum(r.key_bytes for r in druns)
    vcap = sum(r.val_bytes for r in druns)
    e = lambda k, dt: torch.empty(max(k, 1), dtype=dt, device=dev)
    o = {"key_bytes": e(kcap + 16, torch.uint8), "key_off": e(total + 1, torch.int64),
         "val_bytes": e(vcap + 16, torch.uint8), "val_off": e(total + 1, torch.int64),
         "kind": e(total, torch.uint8), "seq": e(total, torch.int64), "create_ts": e(total, torch.int64),
         "expire_ts": e(total, torch.int64), "ts_mask": e(total, torch.uint8),
         "summary": torch.zeros(C.sizeof(_abi.MergeSummary), dtype=torch.uint8, device=dev)}
    out = _abi.MergedOut(o["key_bytes"].data_ptr(), kcap, o["key_off"].data_ptr(), o["val_bytes"].data_ptr(), vcap,
                         o["val_off"].data_ptr(), o["kind"].data_ptr(), o["seq"].data_ptr(), o["create_ts"].data_ptr(),
                         o["expire_ts"].data_ptr(), o["ts_mask"].data_ptr(), total, o["summary"].data_ptr())
    cr = (_abi.Run * max(len(druns), 1))(*[r.to_ctypes() for r in druns])
    wsb = lib().sdb_merge_runs_workspace_bytes(cr, len(druns))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
    st = lib().sdb_merge_runs(cr, len(druns), C.byref(ret), C.byref(out), ws.data_ptr(), ws.numel(), _sp(stream))
    if st:
        raise SdbError(st, "sdb_merge_runs")
    _sync(stream, dev)
    sm = _abi.MergeSummary.from_buffer_copy(o["summary"].cpu().numpy().tobytes())
    o["_ws"] = ws
    return o, sm


def merged_to_host(o, sm):
    from .batch import Batch
    n = sm.num_out
    v = lambda k, m, dt: o[k][:m].cpu().numpy().view(dt)
    return Batch(v("key_bytes", sm.key_bytes, np.uint8), v("key_off", n + 1, np.uint64),
                 v("val_bytes", sm.val_bytes, np.uint8), v("val_off", n + 1, np.uint64), v("kind", n, np.uint8),
                 v("seq", n, np.uint64), v("create_ts", n, np.int64), v("expire_ts", n, np.int64),
                 v("ts_mask", n, np.uint8))


def sst_cuts_device(dbatch, prm, max_sst_size, stream=None):
    """sdb_sst_cuts over a device batch -> list of SST start entries + [n] (synchronises)."""
    import torch
    n = dbatch.n
    dev = dbatch.key_bytes.device if hasattr(dbatch, "key_bytes") else "cuda"
    cut = torch.zeros(n + 2, dtype=torch.int64, device=dev)
    num = torch.zeros(1, dtype=torch.int64, device=dev)
    wsb = lib().sdb_sst_cuts_workspace_bytes(n, C.byref(prm))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=dev)
    kb = dbatch.to_ctypes()
    st = lib().sdb_sst_cuts(C.byref(kb), C.byref(prm), max_sst_size, cut.data_ptr(), n + 1, num.data_ptr(),
                            ws.data_ptr(), ws.numel(), _sp(stream))
    if st:
        raise SdbError(st, "sdb_sst_cuts")
    _sync(stream, dev)
    ns = int(num.item())
    return [int(x) for x in cut[:ns + 1].cpu().numpy()] if ns else []


class Compactor:
    """sdb_compactor_*: one compaction job (merge + retention + cuts + encode) per run()."""

    _PLAIN = object()  # `operator` of a job without one

    def __init__(self, device=0):
        require_device()
        self.h = lib().sdb_compactor_create(device)
        if not self.h:
            raise SdbError(_abi.SDB_DEVICE_ERROR, "sdb_compactor_create")

    def _job(self, symbol, head, ret, operator, prm, max_sst_size, stream, flt=None, resume=None):
        """One job entry point: the inputs `head`, then ret, (with an operator) its callback and a NULL context,
        (the filtered symbols) the filter and the cursor, params, max_sst_size, stream, num_ssts.  The ranged and the
        filtered symbols always take the callback pair: NULL without an operator."""
        filtered = symbol.endswith("_filtered")
        op = (_abi.MERGE_BATCH_FN(), None) if symbol.endswith("_ranged") or filtered else ()
        if operator is not self._PLAIN:
            cb, self.operator_state = self._operator_callback(operator)
            op = (cb, None)
        if filtered:
            from . import compaction_filter as CF
            cf, self.filter_state = (None, None) if flt is None else CF.callbacks(flt)
            # (key, seq), or an sdb_resume_cursor the caller built itself, which passes through as it is
            cur, keep = (None, None) if resume is None else \
                (resume, None) if isinstance(resume, _abi.ResumeCursor) else CF.cursor(*resume)
            op += (None if cf is None else C.byref(cf), None if cur is None else C.byref(cur))
        ns = C.c_uint32(0)
        st = getattr(lib(), symbol)(self.h, *head, C.byref(ret), *op, C.byref(prm), max_sst_size, _sp(stream), C.byref(ns))
        self.status = st
        return st, ns.value

    def _run(self, druns, ret, operator, prm, max_sst_size, stream):
        cr = (_abi.Run * max(len(druns), 1))(*[r.to_ctypes() for r in druns])
        return self._job("sdb_compactor_run" + ("_merge" if operator is not self._PLAIN else ""), (cr, len(druns)), ret,
                         operator, prm, max_sst_size, stream)

    @staticmethod
    def _inputs(inputs, views=False):
        """The sdb_compaction_input array of a job's inputs; `views`: the sdb_compaction_view array (+ index keys)."""
        ci = [_abi.CompactionInput(x.data.data_ptr(), x.block_off.data_ptr(), x.block_off.numel() - 1, x.num_entries,
                                   x.key_bytes, x.val_bytes) for x in inputs]
        if not views:
            return (_abi.CompactionInput * max(len(ci), 1))(*ci)
        return (_abi.CompactionView * max(len(ci), 1))(*[
            _abi.CompactionView(c, x.index_keys.data_ptr(), x.index_key_off.data_ptr()) for c, x in zip(ci, inputs)])

    @staticmethod
    def _run_shape(run_start, ninputs):
        """(run_start, nruns) as the jobs over encoded inputs take them: without run_start every input is a run."""
        if run_start is None:
            return None, ninputs
        return (C.c_uint32 * len(run_start))(*run_start), len(run_start) - 1

    def _run_ssts(self, inputs, ret, operator, prm, max_sst_size, input_version, run_start, stream):
        return self._job("sdb_compactor_run_ssts" + ("_merge" if operator is not self._PLAIN else ""),
                         (self._inputs(inputs), len(inputs), *self._run_shape(run_start, len(inputs)), input_version),
                         ret, operator, prm, max_sst_size, stream)

    def run(self, druns, ret, prm, max_sst_size, stream=None):
        return self._run(druns, ret, self._PLAIN, prm, max_sst_size, stream)

    def run_ssts(self, inputs, ret, prm, max_sst_size, input_version=2, run_start=None, stream=None):
        """sdb_compactor_run_ssts: the job from encoded input SSTs (decode included).  inputs: objects with
        .data / .block_off (device tensors: the data section, block_off u64[num_blocks + 1]) and the
        SstStats counts .num_entries / .key_bytes / .val_bytes; run_start: inputs of each sorted run."""
        return self._run_ssts(inputs, ret, self._PLAIN, prm, max_sst_size, input_version, run_start, stream)

    @staticmethod
    def _operator_callback(operator):
        """`operator` (merge_batch(key, existing, operands) -> bytes, slatedb_amd/merge.py) as an sdb_merge_batch_fn.
        The result of a call stays alive, in `keep`, until the next one; an exception in the operator becomes a
        non-zero return (the job fails with SDB_MERGE_OPERATOR_ERROR) and is kept in keep["error"]."""
        keep = {"result": None, "error": None}

        def call(ctx, key, key_len, existing, existing_len, operands, operand_len, n, result, result_len):
            try:
                k = C.string_at(key, key_len) if key_len else b""
                ex = None if not existing else C.string_at(existing, existing_len)
                ops = [C.string_at(operands[i], operand_len[i]) if operand_len[i] else b"" for i in range(n)]
                r = bytes(operator.merge_batch(k, ex, ops))
                buf = (C.c_uint8 * max(len(r), 1)).from_buffer_copy(r or b"\0")
                keep["result"] = buf
                result[0] = C.cast(buf, _abi.u8p)
                result_len[0] = len(r)
                return 0
            except Exception as e:  # never unwind through the C frames
                keep["error"] = e
                return 1
        return _abi.MERGE_BATCH_FN(call), keep

    def run_merge(self, druns, ret, operator, prm, max_sst_size, stream=None):
        """sdb_compactor_run_merge: run() with the store's merge operator (an object with
        merge_batch(key, existing, operands), slatedb_amd/merge.py) between the merge and retention."""
        return self._run(druns, ret, operator, prm, max_sst_size, stream)

    def run_ssts_merge(self, inputs, ret, operator, prm, max_sst_size, input_version=2, run_start=None, stream=None):
        """sdb_compactor_run_ssts_merge: run_ssts() with the store's merge operator."""
        return self._run_ssts(inputs, ret, operator, prm, max_sst_size, input_version, run_start, stream)

    def _ranged_job(self, symbol, inputs, ret, prm, max_sst_size, job_range, projections, operator, input_version,
                    run_start, stream, *filtered):
        """The ranged and the filtered job over encoded inputs: the views, the run shape, the job range and the
        projections (uploaded when they are host arrays, kept until the job's work is done), then _job."""
        dev = inputs[0].data.device if inputs else "cuda"
        keep = []  # the range tensors: until the job's work is done

        def ranges(arrays):  # the arrays of an sdb_scan_ranges (host, or already on the device) -> the struct
            t = {k: a if hasattr(a, "data_ptr") else _to_dev(a, dev) for k, a in arrays.items() if k != "n"}
            keep.append(t)
            return C.byref(_abi.ScanRanges(len(t["start_off"]) - 1, _ptr(t["start_bytes"]), _ptr(t["start_off"]),
                                           _ptr(t["start_kind"]), _ptr(t["end_bytes"]), _ptr(t["end_off"]),
                                           _ptr(t["end_kind"])))
        columnar = lambda x, f: x if isinstance(x, dict) else f(x)  # noqa: E731  (a dict: the host arrays themselves)
        jr = None if job_range is None else ranges(columnar(job_range, lambda r: scan_ranges_columnar([r])))
        pj = None if projections is None else ranges(columnar(projections, projections_columnar))
        res = self._job(symbol, (self._inputs(inputs, views=True), len(inputs), *self._run_shape(run_start, len(inputs)),
                                 input_version, jr, pj), ret, self._PLAIN if operator is None else operator, prm, max_sst_size,
                        stream, *filtered)
        _sync(stream, dev)  # the range tensors are released on return
        return res

    def run_ssts_ranged(self, inputs, ret, prm, max_sst_size, job_range=None, projections=None, operator=None,
                        input_version=2, run_start=None, stream=None):
        """sdb_compactor_run_ssts_ranged: run_ssts() (with `operator`: run_ssts_merge()) over one job range and a
        visible range per input.  inputs: as run_ssts, plus .index_keys / .index_key_off (device tensors: each
        block's index key).  job_range: (start, start_kind, end, end_kind) as scan_ranges_columnar takes it, or
        None = unbounded; projections: one such tuple or None (the whole SST) per input, as projections_columnar
        takes them, or None; either may also be the dict of arrays those functions return (host arrays, or device
        tensors the caller keeps)."""
        return self._ranged_job("sdb_compactor_run_ssts_ranged", inputs, ret, prm, max_sst_size, job_range, projections,
                                operator, input_version, run_start, stream)

    def run_filtered(self, druns, ret, prm, max_sst_size, flt=None, resume=None, operator=None, stream=None):
        """sdb_compactor_run_filtered: run() (with `operator`: run_merge()) with a compaction filter (a
        slatedb_amd.compaction_filter BatchFilter, or an object with filter(entry)) and / or a resume cursor
        (key, seq) = the last row the interrupted job wrote.  filter_state["error"] keeps a filter's exception."""
        cr = (_abi.Run * max(len(druns), 1))(*[r.to_ctypes() for r in druns])
        return self._job("sdb_compactor_run_filtered", (cr, len(druns)), ret, self._PLAIN if operator is None else operator,
                         prm, max_sst_size, stream, flt, resume)

    def run_ssts_filtered(self, inputs, ret, prm, max_sst_size, flt=None, resume=None, job_range=None, projections=None,
                          operator=None, input_version=2, run_start=None, stream=None):
        """sdb_compactor_run_ssts_filtered: run_ssts_ranged() with a compaction filter and / or a resume cursor."""
        return self._ranged_job("sdb_compactor_run_ssts_filtered", inputs, ret, prm, max_sst_size, job_range, projections,
                                operator, input_version, run_start, stream, flt, resume)

    def filter_stats(self):
        """sdb_filter_stats of the last job (zeros after a job without a filter and without a cursor)."""
        fs = _abi.FilterStats()
        st = lib().sdb_compactor_filter_stats(self.h, C.byref(fs))
        if st:
            raise SdbError(st, "sdb_compactor_filter_stats")
        return fs

    def range_stats(self):
        """sdb_range_job_stats of the last run_ssts_ranged job (zeros after any other)."""
        rs = _abi.RangeJobStats()
        st = lib().sdb_compactor_range_stats(self.h, C.byref(rs))
        if st:
            raise SdbError(st, "sdb_compactor_range_stats")
        return rs

    def merge_stats(self):
        """sdb_merge_op_stats of the last job (zeros after a job without an operator)."""
        ms = _abi.MergeOpStats()
        st = lib().sdb_compactor_merge_stats(self.h, C.byref(ms))
        if st:
            raise SdbError(st, "sdb_compactor_merge_stats")
        return ms

    def merged(self):
        kb, sm = _abi.KvBatch(), _abi.MergeSummary()
        st = lib().sdb_compactor_merged(self.h, C.byref(kb), C.byref(sm))
        if st:
            raise SdbError(st, "sdb_compactor_merged")
        from .batch import Batch
        n = kb.n
        if not n:
            return Batch(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint8), np.zeros(1, np.uint64),
                         np.zeros(0, np.uint8), np.zeros(0, np.uint64), np.zeros(0, np.int64), np.zeros(0, np.int64),
                         np.zeros(0, np.uint8)), sm
        g = lambda p, k, dt: _d2h(p, k * np.dtype(dt).itemsize).view(dt)
        ko, vo = g(kb.key_off, n + 1, np.uint64), g(kb.val_off, n + 1, np.uint64)
        # the arenas end at the last offsets (the summary's byte counts stay retention's under a filter or a cursor)
        return Batch(g(kb.key_bytes, int(ko[n]), np.uint8), ko,
                     g(kb.val_bytes, int(vo[n]), np.uint8), vo, g(kb.kind, n, np.uint8),
                     g(kb.seq, n, np.uint64), g(kb.create_ts, n, np.int64), g(kb.expire_ts, n, np.int64),
                     g(kb.ts_mask, n, np.uint8)), sm

    def sst(self, i):
        """SST i of the last run as host arrays (the fields of DeviceSstOutput.to_host) + entry range."""
        v = _abi.CompactedSst()
        st = lib().sdb_compactor_sst(self.h, i, C.byref(v))
        if st:
            raise SdbError(st, "sdb_compactor_sst")
        sm = v.summary
        nb = sm.num_blocks
        g = lambda p, k, dt: _d2h(p, k * np.dtype(dt).itemsize).view(dt)
        return {"summary": sm, "entry_start": v.entry_start, "entry_end": v.entry_end,
                "data": g(v.data, sm.data_len, np.uint8), "block_off": g(v.block_off, nb + 1, np.uint64),
                "block_first_entry": g(v.block_first_entry, nb + 1, np.uint32),
                "index_key_len": g(v.index_key_len, nb, np.uint32),
                "block_stats": g(v.block_stats, 3 * nb, np.uint16).reshape(-1, 3),
                "bloom": g(v.bloom, sm.bloom_len, np.uint8)}

    def close(self):
        if getattr(self, "h", None):
            lib().sdb_compactor_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------
# WAL replay / device memtable (sdb_wal_replay_sort, sdb_wal_replay_emit)
# ------------------------------------------------------------------------------------------------
class ReplayedTable:
    """One replayed memtable: rows [lo, hi) of the replay's output stream (device tensors shared by every table
    of the call) and its W7 metadata (replay.table_metadata)."""

    def __init__(self, cols, lo, hi, meta):
        self.cols, self.lo, self.hi, self.meta = cols, lo, hi, meta
        self.n = hi - lo

    def _p(self, name, width):
        return self.cols[name].data_ptr() + self.lo * width

    def to_ctypes(self):
        """The table as an sdb_kv_batch: offsets index the shared arenas, as a compactor's cut SST views the
        merged stream."""
        c = self.cols
        return _abi.KvBatch(self.n, c["key_bytes"].data_ptr(), self._p("key_off", 8), c["val_bytes"].data_ptr(),
                            self._p("val_off", 8), self._p("kind", 1), self._p("seq", 8), self._p("create_ts", 8),
                            self._p("expire_ts", 8), self._p("ts_mask", 1), None)

    def as_run(self):
        """The table as the one sorted run of its flush (sdb_compactor_run, flush.rs:186-236)."""
        import torch
        c, lo, hi = self.cols, self.lo, self.hi
        koff, voff = c["key_off"][lo:hi + 1], c["val_off"][lo:hi + 1]
        kind, mask = c["kind"][lo:hi], c["ts_mask"][lo:hi]
        flags = (torch.where(kind == _abi.KIND_TOMBSTONE, _abi.FLAG_TOMBSTONE, 0) |
                 torch.where(kind == _abi.KIND_MERGE, _abi.FLAG_MERGE_OPERAND, 0) |
                 torch.where((mask & _abi.TS_CREATE) != 0, _abi.FLAG_HAS_CREATE_TS, 0) |
                 torch.where((mask & _abi.TS_EXPIRE) != 0, _abi.FLAG_HAS_EXPIRE_TS, 0)).to(torch.uint8)
        vlen = (voff[1:] - voff[:-1]).to(torch.int32)
        pad = lambda t: torch.cat([t.contiguous().view(torch.uint8), torch.zeros(16, dtype=torch.uint8, device=t.device)])
        kb = int((koff[-1] - koff[0]).item()) if self.n else 0
        vb = int((voff[-1] - voff[0]).item()) if self.n else 0
        return DeviceRun(self.n, c["key_bytes"], pad(koff), c["val_bytes"], pad(voff[:-1]), pad(vlen), pad(c["seq"][lo:hi]),
                         pad(flags), pad(c["create_ts"][lo:hi]), pad(c["expire_ts"][lo:hi]), kb, vb)

    def to_host(self):
        lo, hi = self.lo, self.hi
        v = lambda k, dt: self.cols[k][lo:hi].cpu().numpy().view(dt)
        ko = self.cols["key_off"][lo:hi + 1].cpu().numpy().view(np.uint64)
        vo = self.cols["val_off"][lo:hi + 1].cpu().numpy().view(np.uint64)
        kb = self.cols["key_bytes"][int(ko[0]):int(ko[-1])].cpu().numpy()
        vb = self.cols["val_bytes"][int(vo[0]):int(vo[-1])].cpu().numpy()
        return Batch(kb, ko - ko[0], vb, vo - vo[0], v("kind", np.uint8), v("seq", np.uint64), v("create_ts", np.int64),
                     v("expire_ts", np.int64), v("ts_mask", np.uint8))


class WalReplay:
    """The two device calls of a replay over one DeviceRun, with the host step between them left to the caller:
    sort() -> (facts, summary); emit(cuts) -> (columns, table_row_start, summary)."""

    def __init__(self, drun, batch_start, workspace=None, fill=None):
        import torch
        self.drun, self.dev = drun, drun.t[0].device
        self.nb = len(batch_start) - 1
        self.bs = torch.tensor([int(x) for x in batch_start], dtype=torch.int64, device=self.dev)
        self.wsb = lib().sdb_wal_replay_workspace_bytes(drun.n, self.nb)
        self.ws = workspace if workspace is not None else torch.empty(max(self.wsb, 256), dtype=torch.uint8, device=self.dev)
        self.fill = fill
        self.run = drun.to_ctypes()

    def _new(self, count, dt):
        import torch
        nbytes = max(count, 1) * torch.empty(0, dtype=dt).element_size()
        return torch.full((nbytes,), self.fill or 0, dtype=torch.uint8, device=self.dev).view(dt)  # fill: the tests' canary

    def sort(self, min_seq=None, stream=None, ws_ptr=None, ws_bytes=None):
        import torch
        self.facts_t = self._new(self.nb * C.sizeof(_abi.WalBatchFacts), torch.uint8)
        self.summary_t = self._new(C.sizeof(_abi.WalReplaySummary), torch.uint8)
        st = lib().sdb_wal_replay_sort(C.byref(self.run), self.bs.data_ptr(), self.nb, 0 if min_seq is None else min_seq,
                                       0 if min_seq is None else 1, self.facts_t.data_ptr(), self.summary_t.data_ptr(),
                                       self.ws.data_ptr() if ws_ptr is None else ws_ptr,
                                       self.ws.numel() if ws_bytes is None else ws_bytes, _sp(stream))
        if st:
            raise SdbError(st, "sdb_wal_replay_sort")
        _sync(stream, self.dev)
        raw = self.facts_t.cpu().numpy().tobytes()
        sz = C.sizeof(_abi.WalBatchFacts)
        facts = [_abi.WalBatchFacts.from_buffer_copy(raw[b * sz:(b + 1) * sz]) for b in range(self.nb)]
        return facts, _abi.WalReplaySummary.from_buffer_copy(self.summary_t.cpu().numpy().tobytes())

    def emit(self, cuts, cap_entries=None, key_cap=None, val_cap=None, stream=None, ws_ptr=None, ws_bytes=None, extra=0):
        """extra: elements allocated behind every capacity (the tests' canaries)."""
        import torch
        r = self.drun
        ce = r.n if cap_entries is None else cap_entries
        kc = r.key_bytes if key_cap is None else key_cap
        vc = r.val_bytes if val_cap is None else val_cap
        nt = len(cuts) - 1
        tbs = torch.tensor([int(x) for x in cuts], dtype=torch.int64, device=self.dev)
        x = extra
        o = {"key_bytes": self._new(kc + 16 + x, torch.uint8), "key_off": self._new(ce + 1 + x, torch.int64),
             "val_bytes": self._new(vc + 16 + x, torch.uint8), "val_off": self._new(ce + 1 + x, torch.int64),
             "kind": self._new(ce + x, torch.uint8), "seq": self._new(ce + x, torch.int64),
             "create_ts": self._new(ce + x, torch.int64), "expire_ts": self._new(ce + x, torch.int64),
             "ts_mask": self._new(ce + x, torch.uint8),
             "table_row_start": self._new(nt + 1, torch.int64),
             "summary": self._new(C.sizeof(_abi.WalReplaySummary), torch.uint8)}
        out = _abi.WalTablesOut(o["key_bytes"].data_ptr(), kc, o["key_off"].data_ptr(), o["val_bytes"].data_ptr(), vc,
                                o["val_off"].data_ptr(), o["kind"].data_ptr(), o["seq"].data_ptr(),
                                o["create_ts"].data_ptr(), o["expire_ts"].data_ptr(), o["ts_mask"].data_ptr(), ce,
                                o["table_row_start"].data_ptr(), o["summary"].data_ptr())
        st = lib().sdb_wal_replay_emit(C.byref(self.run), self.bs.data_ptr(), self.nb, tbs.data_ptr(), nt, C.byref(out),
                                       self.ws.data_ptr() if ws_ptr is None else ws_ptr,
                                       self.ws.numel() if ws_bytes is None else ws_bytes, _sp(stream))
        if st:
            raise SdbError(st, "sdb_wal_replay_emit")
        _sync(stream, self.dev)
        sm = _abi.WalReplaySummary.from_buffer_copy(o["summary"].cpu().numpy().tobytes())
        return o, sm


def wal_replay_device(drun, batch_start, min_seq, prm, max_memtable_bytes, last_l0_seq=0, last_l0_clock_tick=-(1 << 63),
                      wal_ids=None, stream=None):
    """WalReplayIterator over decoded WAL rows (wal_replay.rs:111-184): drun holds the rows of every batch in
    arrival order, batch b = rows [batch_start[b], batch_start[b + 1]); min_seq None = no filter.  Runs
    sdb_wal_replay_sort, reads the per-batch facts, splits the tables on the host (replay.split_tables) and runs
    sdb_wal_replay_emit.  Returns the ReplayedTables in order (all of them views of one device output)."""
    from . import replay
    w = WalReplay(drun, batch_start)
    facts, sm = w.sort(min_seq, stream)
    if sm.status:
        raise SdbError(sm.status, "sdb_wal_replay_sort: batch %d" % sm.first_error_entry)
    cuts = replay.split_tables(facts, prm, max_memtable_bytes)
    if len(cuts) < 2:
        return []
    o, sm = w.emit(cuts, stream=stream)
    if sm.status:
        raise SdbError(sm.status, "sdb_wal_replay_emit")
    trs = [int(x) for x in o["table_row_start"].cpu().numpy()]
    meta = replay.table_metadata(facts, cuts, last_l0_seq, last_l0_clock_tick, wal_ids)
    return [ReplayedTable(o, trs[t], trs[t + 1], meta[t]) for t in range(len(cuts) - 1)]
