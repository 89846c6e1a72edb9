"""Expected results of sdb_sst_scan, computed from the oracle's ascending block decode.

A range (start, start_kind, end, end_kind) over one encoded SST yields
  * the block range partitions_covering_range(index, start, end) (partitioned_keyspace.rs:87-110, called
    from sst_iter.rs:548-552), restated literally below over the index keys;
  * every entry of those blocks whose key the range contains (SstView::contains, sst_iter.rs:97-121);
  * descending: the key groups in reverse, each group's versions in their physical (newest first) order
    (fill_descending_buffer, sst_iter.rs:567-651).
"""
import bisect

import numpy as np

from oracle import oracle as O
from slatedb_amd import _abi

U, INC, EXC = _abi.BOUND_UNBOUNDED, _abi.BOUND_INCLUDED, _abi.BOUND_EXCLUDED


def partition_point(keys, pred):
    """partitioned_keyspace.rs:16-39."""
    if not keys:
        return 0
    low, high, pp = 0, len(keys) - 1, 0
    while low <= high:
        mid = low + (high - low) // 2
        if pred(keys[mid]):
            low = mid + 1
            pp = mid + 1
        elif mid > low:
            high = mid - 1
        else:
            break
    return pp


def first_partition_including_or_after_key(keys, k):
    """partitioned_keyspace.rs:43-68: None of first_partition_including_key becomes 0."""
    pp = partition_point(keys, lambda f: f < k)
    return pp - 1 if pp > 0 else 0


def last_partition_including_key(keys, k):
    """partitioned_keyspace.rs:72-83."""
    pp = partition_point(keys, lambda f: f <= k)
    return None if pp == 0 else pp - 1


def partitions_covering_range(keys, s, sk, e, ek):
    """partitioned_keyspace.rs:87-110 -> (start_idx, end_idx_exclusive); end may be below start."""
    start = 0 if sk == U else first_partition_including_or_after_key(keys, s)
    if ek == U:
        end = len(keys)
    else:
        p = last_partition_including_key(keys, e)
        if p is None:
            end = start
        elif ek == EXC and e == keys[p]:
            end = p
        else:
            end = p + 1
    return start, end


def contains(key, s, sk, e, ek):
    """BytesRange::contains over the two bounds."""
    if sk == INC and key < s or sk == EXC and key <= s:
        return False
    if ek == INC and key > e or ek == EXC and key >= e:
        return False
    return True


def empty_as_set(s, sk, e, ek):
    return sk != U and ek != U and (s > e or (s == e and (sk == EXC or ek == EXC)))


def row_tuples(d, n=None):
    """(key, val_off, val_len, seq, flags, cts, ets) per entry of decoded columns, timestamps masked by
    the flags (as tests/test_descending.py rows)."""
    n = d.n if n is None else n
    ko = np.asarray(d.key_off[:n + 1]).astype(np.int64).tolist()
    ka = np.asarray(d.key_arena).tobytes()
    fl = np.asarray(d.flags[:n]).astype(np.int64)
    cts = np.where(fl & _abi.FLAG_HAS_CREATE_TS, np.asarray(d.create_ts[:n]).astype(np.int64), -1).tolist()
    ets = np.where(fl & _abi.FLAG_HAS_EXPIRE_TS, np.asarray(d.expire_ts[:n]).astype(np.int64), -1).tolist()
    has_c = (fl & _abi.FLAG_HAS_CREATE_TS != 0).tolist()
    has_e = (fl & _abi.FLAG_HAS_EXPIRE_TS != 0).tolist()
    vo = np.asarray(d.val_off[:n]).astype(np.int64).tolist()
    vl = np.asarray(d.val_len[:n]).astype(np.int64).tolist()
    sq = np.asarray(d.seq[:n]).astype(np.uint64).tolist()
    fl = fl.tolist()
    return [(ka[ko[i]:ko[i + 1]], vo[i], vl[i], sq[i], fl[i], cts[i] if has_c[i] else None,
             ets[i] if has_e[i] else None) for i in range(n)]


class Sst:
    """One oracle-encoded SST with its ascending decode: the source of every expectation."""

    def __init__(self, batch, version, block_size, restart_interval=16, data=None):
        self.version = version
        self.enc = O.encode_sst(batch, O.params(block_size=block_size, sst_version=version,
                                                restart_interval=restart_interval))
        assert self.enc.status == 0
        self.data = self.enc.data if data is None else data
        self.block_off = self.enc.block_off
        self.nb = len(self.block_off) - 1
        self.ik_bytes, self.ik_off = O.sst_index_keys(batch, self.enc)
        ikb = self.ik_bytes.tobytes()
        self.index_keys = [ikb[int(self.ik_off[k]):int(self.ik_off[k + 1])] for k in range(self.nb)]
        dec = O.decode_blocks(self.enc.data, self.block_off, version)
        assert dec.status == 0 and dec.n == batch.n
        self.rows = row_tuples(dec)
        self.keys = [r[0] for r in self.rows]
        self.bes = np.asarray(dec.block_entry_start).astype(np.int64).tolist()
        self.dec = dec
        newkey = np.array([i == 0 or self.keys[i] != self.keys[i - 1] for i in range(len(self.keys))], np.int64)
        self.gid = np.cumsum(newkey)  # key group of every entry

    def expect_idx(self, rng_, descending=False):
        """((start block, end block), indices into the ascending decode) of one range."""
        s, sk, e, ek = rng_
        s, e = s or b"", e or b""
        bs, be = partitions_covering_range(self.index_keys, s, sk, e, ek)
        none = np.zeros(0, np.int64)
        if empty_as_set(s, sk, e, ek) or be <= bs:
            return (bs, be), none
        i0 = 0 if sk == U else (bisect.bisect_left if sk == INC else bisect.bisect_right)(self.keys, s)
        i1 = len(self.keys) if ek == U else (bisect.bisect_right if ek == INC else bisect.bisect_left)(self.keys, e)
        i0, i1 = max(i0, self.bes[bs]), min(i1, self.bes[be])  # only entries of the covering blocks
        if i1 <= i0:
            return (bs, be), none
        for i in {i0, i1 - 1}:
            assert contains(self.keys[i], s, sk, e, ek)
        for i in {i0 - 1, i1} & set(range(self.bes[bs], self.bes[be])):
            assert not contains(self.keys[i], s, sk, e, ek)
        idx = np.arange(i0, i1, dtype=np.int64)
        if descending:  # key groups in reverse, each group's versions in physical order
            idx = idx[np.lexsort((idx, -self.gid[i0:i1]))]
        return (bs, be), idx

    def expect(self, rng_, descending=False):
        """((start block, end block), rows) of one range."""
        blocks, idx = self.expect_idx(rng_, descending)
        return blocks, [self.rows[i] for i in idx.tolist()]

    def straddling_key(self, min_versions=3):
        """(key, first entry, last entry) of a key whose versions lie in more than one block."""
        for k in range(1, self.nb):
            i = self.bes[k]
            if 0 < i < len(self.keys) and self.keys[i - 1] == self.keys[i]:
                key = self.keys[i]
                a, b = bisect.bisect_left(self.keys, key), bisect.bisect_right(self.keys, key)
                if b - a >= min_versions:
                    return key, a, b - 1
        return None


def absent_near(key):
    return key + b"\x00"


def range_list(sst, seed):
    """The ranges every device case scans (built once per case)."""
    keys, nb = sst.keys, sst.nb
    n = len(keys)
    mid, late = keys[n // 3], keys[2 * n // 3]
    out = [(None, U, None, U)]
    out += [(mid, INC, None, U), (mid, EXC, None, U), (None, U, late, INC), (None, U, late, EXC)]
    for k in (keys[0], keys[n // 2], keys[n - 1]):  # points: present
        out.append((k, INC, k, INC))
    for k in (absent_near(keys[n // 2]), keys[5][:-1], b"zzzz", b"\x00"):  # points: absent
        out.append((k, INC, k, INC))
    kb = min(max(1, nb // 2), nb - 1)
    k2 = min(nb - 1, kb + 2)
    for lo_key, hi_key in ((sst.index_keys[kb], sst.index_keys[k2]), (keys[sst.bes[kb]], keys[sst.bes[k2]]),
                           (sst.index_keys[kb], keys[sst.bes[k2]]), (keys[sst.bes[kb]], sst.index_keys[kb])):
        for sk in (INC, EXC):
            for ek in (INC, EXC):
                out.append((lo_key, sk, hi_key, ek))
                out.append((mid if mid < hi_key else keys[0], sk, lo_key, ek))  # the block key as the end bound
    i = sst.bes[kb] + 1  # inside one restart region (and one block)
    out.append((keys[i], INC, keys[max(i, min(i + 2, sst.bes[kb + 1] - 1))], INC))
    st = sst.straddling_key()
    if st:
        out += [(st[0], INC, st[0], INC), (keys[max(st[1] - 1, 0)], EXC, keys[min(st[2] + 1, n - 1)], EXC)]
    first, last = keys[0], keys[-1]
    out += [(None, U, first, EXC), (b"", EXC, first[:-1], INC), (last + b"\xff", INC, None, U), (last, EXC, None, U)]
    out += [(b"", INC, mid, INC), (b"", INC, None, U)]
    out += [(late, INC, mid, INC), (late, EXC, mid, EXC)]  # start above end
    out += [(mid, EXC, mid, INC), (mid, INC, mid, EXC), (mid, EXC, mid, EXC)]  # equal keys, a side excluded
    rng = np.random.default_rng(seed)

    def pick():
        k = keys[int(rng.integers(0, n))]
        c = int(rng.integers(0, 4))
        return k if c < 2 else (absent_near(k) if c == 2 else k[:max(1, len(k) - 1)])

    for _ in range(300):
        a, b = pick(), pick()
        if rng.random() < 0.8 and a > b:
            a, b = b, a
        out.append((a, int(rng.integers(0, 3)), b, int(rng.integers(0, 3))))
    return out
