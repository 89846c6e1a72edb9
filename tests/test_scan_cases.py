"""CPU checks for the range scans (sdb_sst_scan): the expectation helpers of tests/scan_cases.py against
the point-lookup oracle and the reference's descending order, and the host side of the C ABI."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from slatedb_amd import _abi

from .scan_cases import EXC, INC, U, Sst
from .test_lookup_oracle import dup_batch


@pytest.fixture(scope="module")
def lib():
    from slatedb_amd import runtime
    return runtime.lib()


@pytest.mark.parametrize("version,bs", [(2, 256), (1, 512)])
def test_point_range_starts_at_the_lookup_entry(version, bs):
    """[k, k] ascending begins with the entry Db::get positions on: O.sst_lookup's FOUND entry."""
    b = dup_batch()
    sst = Sst(b, version, bs)
    keys = [b.key(i) for i in range(0, b.n, 7)]
    r = O.sst_lookup(sst.data, sst.block_off, sst.ik_bytes, sst.ik_off, keys, sst_version=version)
    for q, k in enumerate(keys):
        assert r.state[q] == _abi.LOOKUP_FOUND
        (bs_, be_), idx = sst.expect_idx((k, INC, k, INC))
        assert bs_ <= r.block[q] < be_
        assert idx[0] == sst.bes[int(r.block[q])] + int(r.entry[q])
        key, vo, vl, seq, fl, cts, ets = sst.rows[int(idx[0])]
        assert (key, vo, vl, seq, fl) == (k, int(r.val_off[q]), int(r.val_len[q]), int(r.seq[q]), int(r.flags[q]))
        assert cts == (int(r.create_ts[q]) if fl & _abi.FLAG_HAS_CREATE_TS else None)
        assert ets == (int(r.expire_ts[q]) if fl & _abi.FLAG_HAS_EXPIRE_TS else None)
        assert all(sst.keys[i] == k for i in idx.tolist())


def test_descending_keeps_versions_newest_first():
    """A key whose versions straddle a block boundary: descending lists its seqs newest first, and the
    keys around it in descending order (fill_descending_buffer, sst_iter.rs:567-651)."""
    sst = Sst(dup_batch(), 2, 256)
    key, a, z = sst.straddling_key()
    assert z - a >= 2 and any(a < e <= z for e in sst.bes)
    _, rows = sst.expect((key, INC, key, INC), descending=True)
    seqs = [r[3] for r in rows]
    assert len(seqs) == z - a + 1 and seqs == sorted(seqs, reverse=True)
    lo, hi = sst.keys[a - 1], sst.keys[z + 1]
    _, rows = sst.expect((lo, INC, hi, INC), descending=True)
    ks = [r[0] for r in rows]
    assert ks[0] == hi and ks[-1] == lo and ks == sorted(ks, reverse=True)
    mine = [r[3] for r in rows if r[0] == key]
    assert mine == seqs
    _, asc = sst.expect((lo, INC, hi, INC))
    assert sorted(asc) == sorted(rows) and asc != rows[::-1]  # not the plain reverse


def test_block_range_edges():
    sst = Sst(dup_batch(), 2, 256)
    ikeys = sst.index_keys
    k = next(j for j in range(sst.nb // 2, sst.nb - 1) if ikeys[j - 1] < ikeys[j] < ikeys[j + 1])
    ik = ikeys[k]
    assert sst.index_keys[0] == b"" and ik
    assert sst.expect_idx((None, U, ik, EXC))[0] == (0, k)       # Excluded(index key): block k is out
    assert sst.expect_idx((None, U, ik, INC))[0] == (0, k + 1)
    assert sst.expect_idx((None, U, None, U))[0] == (0, sst.nb)
    assert len(sst.expect_idx((None, U, None, U))[1]) == len(sst.keys)


# ------------------------------------------------------------------------------------------------
# C ABI, host side
# ------------------------------------------------------------------------------------------------
class HostCall:
    """A well-formed sdb_sst_scan call over host arrays (never reaches a kernel without a device)."""

    def __init__(self, lib, kinds=(INC, INC)):
        self.keep = []
        sst = Sst(dup_batch(n=300), 2, 256)
        a = lambda x: self.keep.append(np.ascontiguousarray(x)) or self.keep[-1].ctypes.data  # noqa: E731
        self.view = _abi.SstView(a(sst.data), a(sst.block_off), sst.nb, a(sst.ik_bytes), a(sst.ik_off), None, 0, 0, 2, 0)
        n = 2
        off = np.array([0, 3, 6], np.uint64)
        kb = np.frombuffer(b"k00k01", np.uint8)
        self.ranges = _abi.ScanRanges(n, a(kb), a(off), a(np.array([kinds[0], INC], np.uint8)), a(kb), a(off),
                                      a(np.array([INC, kinds[1]], np.uint8)))
        cap = 64
        self.summary = _abi.ScanSummary()
        self.out = _abi.ScanOut(a(np.zeros(n + 1, np.uint64)), a(np.zeros(2 * n, np.uint32)), a(np.zeros(n, np.int32)),
                                a(np.zeros(4096, np.uint8)), 4096, a(np.zeros(cap + 1, np.uint64)),
                                a(np.zeros(cap, np.uint64)), a(np.zeros(cap, np.uint32)), a(np.zeros(cap, np.uint64)),
                                a(np.zeros(cap, np.uint8)), a(np.zeros(cap, np.int64)), a(np.zeros(cap, np.int64)),
                                cap, C.addressof(self.summary))
        self.wsb = lib.sdb_sst_scan_workspace_bytes(sst.nb, n)
        self.ws = np.zeros(self.wsb, np.uint8)

    def call(self, lib, out=True, wsb=None):
        return lib.sdb_sst_scan(C.byref(self.view), C.byref(self.ranges), 0, C.byref(self.out) if out else None,
                                self.ws.ctypes.data, self.wsb if wsb is None else wsb, None)


def test_scan_symbols_and_workspace(lib):
    assert lib.sdb_sst_scan and lib.sdb_sst_scan_workspace_bytes
    assert lib.sdb_abi_version() == 2
    w = lib.sdb_sst_scan_workspace_bytes
    assert w(0, 0) > 0
    for nb in (0, 1, 1000, 10**6):
        for n in (0, 1, 4096, 10**6):
            assert w(nb + 1, n) >= w(nb, n) and w(nb, n + 1) >= w(nb, n)
            assert w(2 * nb + 1024, n) > w(nb, n) and w(nb, 2 * n + 1024) > w(nb, n)


def test_scan_argument_checks(lib):
    c = HostCall(lib)
    assert c.call(lib, out=False) == _abi.SDB_INVALID_ARGUMENT
    assert c.call(lib, wsb=c.wsb - 1) == _abi.SDB_INVALID_ARGUMENT
    assert lib.sdb_sst_scan(None, C.byref(c.ranges), 0, C.byref(c.out), c.ws.ctypes.data, c.wsb, None) == _abi.SDB_INVALID_ARGUMENT
    c.out.summary = None
    assert c.call(lib) == _abi.SDB_INVALID_ARGUMENT


def test_scan_no_device_fails_loudly(lib):
    if lib.sdb_device_count() > 0:
        pytest.skip("a HIP device is visible")
    assert HostCall(lib, kinds=(3, INC)).call(lib) == _abi.SDB_INVALID_ARGUMENT
    assert HostCall(lib, kinds=(EXC, 3)).call(lib) == _abi.SDB_INVALID_ARGUMENT
    assert HostCall(lib).call(lib) == _abi.SDB_DEVICE_ERROR
    assert HostCall(lib, kinds=(U, EXC)).call(lib) == _abi.SDB_DEVICE_ERROR
