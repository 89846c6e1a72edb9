"""Blocks that are malformed inside a valid CRC: a block surgeon, a literal walker and a named catalogue.

Three parts, shared by tests/test_malformed_blocks.py (CPU) and tests/test_gpu_malformed_blocks.py:

  * the surgeon edits the CRC-stripped payload of one block of an oracle-encoded SST, recomputes the CRC and
    rebuilds block_off when the size changes (`Shape.sst_with`), or lays payloads out back to back behind a
    lead pad so that a chosen block starts at a chosen `s & 15` (`arena`);
  * `walk(payload, version, descending)` is the second model of a block decode, written from the reference's
    text and not from oracle/sdb_oracle.c (the role brute_force plays for the WAL replay);
  * `v2_catalogue()` / `v1_catalogue()` name every mutation with the status it must produce alone, ascending and descending.

Statuses: what the reference returns as Err(InvalidRowFlags) is SDB_INVALID_ROW_FLAGS; where it would panic
(a Buf read past the end, a slice out of range, an assert, a shift overflow) the C ABI says
SDB_CORRUPT_BLOCK (include/slatedb_amd.h).
"""
import functools
import struct
import zlib

import numpy as np

from oracle import oracle as O
from slatedb_amd import _abi
from slatedb_amd.batch import Batch

from .decode_cases import piece_cuts

CORRUPT, FLAGS = _abi.SDB_CORRUPT_BLOCK, _abi.SDB_INVALID_ROW_FLAGS
TOMB, EXPIRE, CREATE, MERGE = (_abi.FLAG_TOMBSTONE, _abi.FLAG_HAS_EXPIRE_TS, _abi.FLAG_HAS_CREATE_TS,
                               _abi.FLAG_MERGE_OPERAND)
TAIL_PAD = 4096  # zero bytes behind the data of every device arena


# ----------------------------------------------------------------------------------------------------
# The literal walker
# ----------------------------------------------------------------------------------------------------
class _Panic(Exception):
    """The reference would panic here (SDB_CORRUPT_BLOCK)."""


class _BadFlags(Exception):
    """SlateDBError::InvalidRowFlags (SDB_INVALID_ROW_FLAGS)."""


class _Buf:
    """bytes::Buf over data[pos..]: Bytes::slice(pos..) panics past the end, and so does every read."""

    def __init__(self, data, pos):
        if pos > len(data):
            raise _Panic("slice start past the end")
        self.d, self.p = data, pos

    def take(self, n):
        if self.p + n > len(self.d):
            raise _Panic("read past the end")
        self.p += n
        return self.d[self.p - n:self.p]

    def uint(self, n):
        return int.from_bytes(self.take(n), "big")

    def i64(self):
        return int.from_bytes(self.take(8), "big", signed=True)


def _decode_varint(buf):
    """decode_varint (utils.rs:622-634).  `<< shift` with shift >= 32 is an arithmetic overflow (a panic with
    overflow checks on, which is how the C ABI reads it); at shift 28 the high bits of the byte fall off the
    u32 silently."""
    result, shift = 0, 0
    while True:
        byte = buf.uint(1)
        if shift >= 32:
            raise _Panic("shift overflow")
        result |= ((byte & 0x7F) << shift) & 0xFFFFFFFF
        if not byte & 0x80:
            return result
        shift += 7


def _decode_flags(f):
    """decode_flags (row_codec_v2.rs:234-249, row.rs:251-266): unknown bits, or tombstone with merge."""
    if f & ~0x0F or (f & TOMB and f & MERGE):
        raise _BadFlags(f)
    return f


def _timestamps(buf, f):
    ets = buf.i64() if f & EXPIRE else None
    cts = buf.i64() if f & CREATE else None
    return ets, cts


def _block_decode(payload):
    """Block::decode (format/block.rs:28-46)."""
    n = len(payload)
    if n < 2:
        raise _Panic("no entry count")
    count = int.from_bytes(payload[n - 2:], "big")
    data_end = n - 2 - 2 * count
    if data_end < 0:
        raise _Panic("offsets before the block")
    offsets = [int.from_bytes(payload[data_end + 2 * i:data_end + 2 * i + 2], "big") for i in range(count)]
    return payload[:data_end], offsets


def _v2_key_only(data, off):
    """SstRowCodecV2::decode_key_only (row_codec_v2.rs:224-232) of data[off..]."""
    buf = _Buf(data, off)
    shared = _decode_varint(buf)
    unshared = _decode_varint(buf)
    _decode_varint(buf)
    return shared, buf.take(unshared)


def _v2_first_key_at_restart(data, offsets, r):
    """decode_first_key_at_restart (block_iterator_v2.rs:71-78)."""
    shared, suffix = _v2_key_only(data, offsets[r])
    if shared != 0:
        raise _Panic("restart point should have shared_bytes=0")
    return suffix


def _v2_entry(data, off, current_key):
    """decode_entry_at_current_offset (block_iterator_v2.rs:95-113): SstRowCodecV2::decode
    (row_codec_v2.rs:172-220), then restore_full_key (:83-89) -> (row, new offset).  A bad flags byte is
    therefore reported before an over-long shared prefix."""
    buf = _Buf(data, off)
    shared = _decode_varint(buf)
    unshared = _decode_varint(buf)
    value_len = _decode_varint(buf)
    suffix = buf.take(unshared)
    vpos = buf.p
    if value_len > 0:
        buf.take(value_len)
    seq = buf.uint(8)
    f = _decode_flags(buf.uint(1))
    ets, cts = _timestamps(buf, f)
    if shared > len(current_key):
        raise _Panic("previous_key[..shared]")
    key = current_key[:shared] + suffix
    vl = 0 if f & TOMB else value_len
    return (key, vpos if vl else 0, vl, seq, f, cts, ets), buf.p


def _v2_ascending(data, offsets):
    """BlockIteratorV2::new (block_iterator_v2.rs:33-52) and next (:235-267): the restart table is used for
    the initial key only."""
    current = _v2_first_key_at_restart(data, offsets, 0) if offsets else b""
    off, rows = 0, []
    while off < len(data):
        row, off = _v2_entry(data, off, current)
        current = row[0]
        rows.append(row)
    return rows


def _v2_descending(data, offsets):
    """DescendingBlockIteratorV2 (block_iterator_v2.rs:318-428): new (:332-355) decodes restart 0's key,
    then the regions go last to first, each loaded ascending from its restart (load_restart_region
    :357-378, seek_to_restart :82-93) and yielded in reverse.

    THE HEADER'S RULE (include/slatedb_amd.h, SDB_DECODE_DESCENDING), not the reference's text: a region
    that does not start at its restart with shared == 0 inside the data and end exactly on the next restart
    makes the block SDB_CORRUPT_BLOCK when the iteration reaches that region -- the reference would read
    rows across regions there, or stop early on an empty one.  A row error met first, in a higher region,
    wins."""
    if not offsets:
        return []  # exhausted: num_restarts == 0
    _v2_first_key_at_restart(data, offsets, 0)
    rows = []
    for r in reversed(range(len(offsets))):
        current = _v2_first_key_at_restart(data, offsets, r)
        off = offsets[r]
        end = offsets[r + 1] if r + 1 < len(offsets) else len(data)
        if not off < end <= len(data) or (r == 0 and off != 0):
            raise _Panic("header's rule: the region is not [restart, next restart)")
        region = []
        while off < end and off < len(data):
            row, off = _v2_entry(data, off, current)
            current = row[0]
            region.append(row)
        if off != end:
            raise _Panic("header's rule: the region does not end on the next restart")
        rows += region[::-1]
    return rows


def _v1(data, offsets, descending):
    """BlockIterator::new -> decode_first_key (block_iterator.rs:196-203, 242-249), whatever the entry
    count; then load_at_current_off (:218-240) per offset, in reverse when descending, through
    SstRowCodecV0::decode (row.rs:200-249) and restore_full_key."""
    buf = _Buf(data, 0)
    if buf.uint(2) != 0:
        raise _Panic("first key overlap should be 0")
    first = buf.take(buf.uint(2))
    rows = []
    for off in (reversed(offsets) if descending else offsets):
        buf = _Buf(data, off)
        prefix = buf.uint(2)
        suffix = buf.take(buf.uint(2))
        seq = buf.uint(8)
        f = _decode_flags(buf.uint(1))
        ets, cts = _timestamps(buf, f)
        vpos = vl = 0
        if f & TOMB:
            f, ets = f & ~EXPIRE, None  # a V0 tombstone drops expire_ts (row.rs:223-231)
        else:
            vl = buf.uint(4)
            vpos = buf.p
            buf.take(vl)
        if prefix > len(first):
            raise _Panic("first_key[..prefix]")
        rows.append((first[:prefix] + suffix, vpos if vl else 0, vl, seq, f, cts, ets))
    return rows


def walk(payload, version, descending=False):
    """(status, rows) of one CRC-stripped block in iteration order.  A row is (key, value offset in the
    payload or 0 for no value, value length, seq, flags, create_ts | None, expire_ts | None); a failing
    block keeps no row."""
    payload = bytes(payload)
    try:
        data, offsets = _block_decode(payload)
        if version == 2:
            return 0, (_v2_descending if descending else _v2_ascending)(data, offsets)
        return 0, _v1(data, offsets, descending)
    except _Panic:
        return CORRUPT, []
    except _BadFlags:
        return FLAGS, []


# ----------------------------------------------------------------------------------------------------
# The surgeon
# ----------------------------------------------------------------------------------------------------
def seal(payload):
    """payload ++ CRC32 (BE): a block as the SST stores it."""
    payload = bytes(payload)
    return payload + struct.pack(">I", zlib.crc32(payload))


def arena(payloads, lead=0, break_crc=()):
    """Sealed payloads back to back behind `lead` pad bytes, with the device's zero tail -> (bytes with the
    tail, block_off).  break_crc: blocks whose stored CRC gets one bit flipped."""
    parts, off = [b"\xAA" * lead], [lead]
    for k, p in enumerate(payloads):
        b = bytearray(seal(p))
        if k in break_crc:
            b[-1] ^= 1
        parts.append(bytes(b))
        off.append(off[-1] + len(b))
    data = np.frombuffer(b"".join(parts) + bytes(TAIL_PAD), np.uint8).copy()
    return data, np.asarray(off, np.uint64)


def lead_for(payloads, k, want):
    """The lead pad that makes block k of arena(payloads) start at s & 15 == want."""
    before = sum(len(p) + 4 for p in payloads[:k])
    return (want - before) % 16


def _varint(d, p):
    v = sh = 0
    while True:
        b = d[p]
        p += 1
        v |= (b & 0x7F) << sh
        if not b & 0x80:
            return v, p
        sh += 7


def _enc_varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


class Layout:
    """Where the fields of a well-formed block's rows lie.  A row: pos, and for V2 p_un / p_vl (the second and
    third varint), for V1 nothing more; suf (key suffix), val (value bytes; V1: the u32 length), tail (seq),
    end, sh, un, vl, flags, klen, region and its index `ri` inside the region."""

    def __init__(self, payload, version):
        self.payload, self.version = bytes(payload), version
        d = self.payload
        self.count = struct.unpack(">H", d[-2:])[0]
        self.data_end = len(d) - 2 - 2 * self.count
        self.offs = [struct.unpack(">H", d[self.data_end + 2 * i:self.data_end + 2 * i + 2])[0]
                     for i in range(self.count)]
        self.rows = []
        if version == 2:
            p, prev, region, ri = 0, 0, -1, 0
            while p < self.data_end:
                if region + 1 < self.count and self.offs[region + 1] == p:
                    region, ri = region + 1, 0
                r = {"pos": p, "region": region, "ri": ri}
                r["sh"], r["p_un"] = _varint(d, p)
                r["un"], r["p_vl"] = _varint(d, r["p_un"])
                r["vl"], r["suf"] = _varint(d, r["p_vl"])
                r["val"] = r["suf"] + r["un"]
                r["tail"] = r["val"] + r["vl"]
                r["flags"] = d[r["tail"] + 8]
                r["end"] = r["tail"] + 9 + (8 if r["flags"] & EXPIRE else 0) + (8 if r["flags"] & CREATE else 0)
                r["prevlen"], r["klen"] = prev, r["sh"] + r["un"]
                prev, p, ri = r["klen"], r["end"], ri + 1
                self.rows.append(r)
            assert p == self.data_end and region == self.count - 1
        else:
            self.fk = struct.unpack(">H", d[2:4])[0]
            for i, p in enumerate(self.offs):
                r = {"pos": p, "region": 0, "ri": i}
                r["sh"], r["un"] = struct.unpack(">HH", d[p:p + 4])
                r["suf"] = p + 4
                r["tail"] = r["suf"] + r["un"]
                r["flags"] = d[r["tail"] + 8]
                q = r["tail"] + 9 + (8 if r["flags"] & EXPIRE else 0) + (8 if r["flags"] & CREATE else 0)
                r["val"], r["vl"] = q, 0
                if not r["flags"] & TOMB:
                    r["vl"] = struct.unpack(">I", d[q:q + 4])[0]
                    q += 4 + r["vl"]
                r["end"] = q
                self.rows.append(r)
            assert [r["pos"] for r in self.rows] == sorted(r["pos"] for r in self.rows)
            assert self.rows[-1]["end"] == self.data_end

    def region_rows(self, q):
        return [i for i, r in enumerate(self.rows) if r["region"] == q]

    def build(self, edits=(), offs=None, count=None):
        """The payload after `edits` [(pos, bytes removed, bytes put)] to the rows; offsets past an edit move
        with the bytes they point to.  offs / count replace the table / the stored count."""
        d = bytearray(self.payload[:self.data_end])
        table = list(self.offs)
        for pos, cut, put in sorted(edits, reverse=True):
            d[pos:pos + cut] = put
            table = [o + len(put) - cut if o > pos else o for o in table]
        table = table if offs is None else offs
        return bytes(d) + b"".join(struct.pack(">H", o & 0xFFFF) for o in table) + \
            struct.pack(">H", len(table) if count is None else count)

    def poke(self, pos, put):
        return self.build([(pos, len(put), bytes(put))])


class Mutation:
    """name; fn(layout, row) -> payload (row None for a whole-block mutation); asc / desc: the status it must
    produce alone; desc_from: "oracle" (the reference's text, restated by the oracle too) or "header" (the
    descending rule of include/slatedb_amd.h, which the oracle does not return); rows: which rows it can be
    placed on ("any", "inner": not the first of a region, "restart": the first of a region q > 0, "last": the
    block's last, None: whole block)."""

    def __init__(self, name, fn, asc, desc, rows=None, desc_from="oracle", huge=False):
        self.name, self.fn, self.asc, self.desc, self.rows = name, fn, asc, desc, rows
        self.desc_from, self.huge = desc_from, huge

    def status(self, descending):
        return self.desc if descending else self.asc


def _six(field):
    def fn(L, i):  # six continuation bytes in place: the sixth shifts by 35
        r = L.rows[i]
        return L.poke({"sh": r["pos"], "un": r["p_un"], "vl": r["p_vl"]}[field], b"\x80" * 6)
    return fn


def _noncanon(field):
    def fn(L, i):  # a one-byte varint as two bytes: the same value, one byte longer
        r = L.rows[i]
        p = {"sh": r["pos"], "un": r["p_un"], "vl": r["p_vl"]}[field]
        assert L.payload[p] < 0x80
        return L.build([(p, 1, bytes([L.payload[p] | 0x80, 0]))])
    return fn


def _wrap32(L, i):  # unshared + value length == the clean sum modulo 2^32
    r = L.rows[i]
    un = 0xFFFFFFF0
    vl = (r["un"] + r["vl"] - un) & 0xFFFFFFFF
    return L.build([(r["p_un"], r["suf"] - r["p_un"], _enc_varint(un) + _enc_varint(vl))])


def _flags(value):
    def fn(L, i):
        return L.poke(L.rows[i]["tail"] + 8, bytes([value]))
    return fn


def _flags_0e(L, i):  # merge operand with both timestamps: the valid extreme
    r = L.rows[i]
    assert not r["flags"] & (EXPIRE | CREATE)
    return L.build([(r["tail"] + 8, 1, bytes([0x0E]) + struct.pack(">qq", -5, 1 << 62))])


def _last_only(fn):
    def g(L, i):
        assert i == len(L.rows) - 1
        return fn(L, L.rows[i])
    return g


def _byte_add(L, p, d):
    assert 0 <= L.payload[p] + d < 0x80
    return bytes([L.payload[p] + d])


_v2_un_exact = _last_only(lambda L, r: L.build([(r["p_un"], 1, _byte_add(L, r["p_un"], 1)),
                                                 (r["p_vl"], 1, _byte_add(L, r["p_vl"], -1))]))
_v2_un_over = _last_only(lambda L, r: L.poke(r["p_un"], _byte_add(L, r["p_un"], 1)))
_v2_vl_exact = _last_only(lambda L, r: L.build([(r["p_un"], 1, _byte_add(L, r["p_un"], -1)),
                                                 (r["p_vl"], 1, _byte_add(L, r["p_vl"], 1))]))
_v2_vl_over = _last_only(lambda L, r: L.poke(r["p_vl"], _byte_add(L, r["p_vl"], 1)))
_v2_ts_at_end = _last_only(lambda L, r: L.poke(r["tail"] + 8, bytes([r["flags"] | EXPIRE])))
# the data ends inside the last row's first varint
_v2_varint_cut = _last_only(lambda L, r: L.build([(r["pos"], r["end"] - r["pos"], b"\x80")]))


def _shared(delta):
    def fn(L, i):  # shared = the previous key's length + delta, in place
        r = L.rows[i]
        return L.poke(r["pos"], _byte_add(L, r["pos"], r["prevlen"] + delta - r["sh"]))
    return fn


def _shared_restart(L, i):  # shared = 1 at a restart (the previous key is longer than that)
    r = L.rows[i]
    assert r["ri"] == 0 and r["sh"] == 0
    return L.poke(r["pos"], b"\x01")


def _table(change):
    def fn(L, _):
        offs, count = change(L, list(L.offs))
        return L.build(offs=offs, count=count)
    return fn


def _swap12(L, o):
    o[1], o[2] = o[2], o[1]
    return o, None


def _set(idx, value):
    def change(L, o):
        o[idx] = value(L)
        return o, None
    return change


def _count_fill(L, _):  # the table fills the block: no data byte left (one when the length is odd)
    n = len(L.payload)
    return L.payload[:n - 2] + struct.pack(">H", (n - 2) // 2)


def _count_over(L, _):  # one offset more than fits
    n = len(L.payload)
    return L.payload[:n - 2] + struct.pack(">H", (n - 2) // 2 + 1)


def v2_catalogue():
    C, F = CORRUPT, FLAGS
    M = Mutation
    out = [M("varint-cut-at-data-end", _v2_varint_cut, C, C, "last")]
    out += [M("varint6-" + f, _six(f), C, C, "any") for f in ("sh", "un", "vl")]
    out += [M("noncanon-" + f, _noncanon(f), 0, 0, "any") for f in ("sh", "un", "vl")]
    out += [M("wrap32-un-vl", _wrap32, C, C, "any", huge=True)]
    out += [M("un-ends-at-end-9", _v2_un_exact, 0, 0, "last"), M("un-ends-1-past-end-9", _v2_un_over, C, C, "last"),
            M("vl-ends-at-end-9", _v2_vl_exact, 0, 0, "last"), M("vl-ends-1-past-end-9", _v2_vl_over, C, C, "last"),
            M("ts-flag-at-data-end", _v2_ts_at_end, C, C, "last")]
    out += [M("flags-%02x" % v, _flags(v), F, F, "any") for v in (0x10, 0x80, 0x09, 0xFF)]
    out += [M("flags-0e-valid", _flags_0e, 0, 0, "any")]
    out += [M("shared-eq-prev", _shared(0), 0, 0, "inner"), M("shared-over-prev", _shared(1), C, C, "inner"),
            M("shared-at-restart-0", _shared_restart, C, C, "first"),
            # ascending the walk never looks at restart q > 0; descending seek_to_restart asserts
            M("shared-at-restart-q", _shared_restart, 0, C, "restart")]
    H = "header"
    out += [M("count-0-with-rows", _table(lambda L, o: ([], None)), 0, 0),
            M("count-1-past-fit", _count_over, C, C), M("count-fills-block", _count_fill, C, C),
            M("offset-eq-data-end", _table(_set(-1, lambda L: L.data_end)), 0, C),
            M("offset-gt-data-end", _table(_set(-1, lambda L: L.data_end + 5)), 0, C),
            M("offsets-decreasing", _table(_swap12), 0, C, desc_from=H),
            M("offsets-duplicate", _table(_set(2, lambda L: L.offs[1])), 0, C, desc_from=H),
            M("offset-mid-row", _table(_set(1, lambda L: L.offs[1] + 1)), 0, C),
            # restart 0 on the second row (shared != 0 there): decode_first_key_at_restart(0) asserts
            M("restart0-on-row-1", _table(_set(0, lambda L: L.rows[1]["pos"])), C, C),
            # restart 0 on restart 1's row: a fine initial key, but region 0 no longer starts the block
            M("restart0-eq-restart1", _table(_set(0, lambda L: L.offs[1])), 0, C, desc_from=H)]
    return out


def _v1_put16(at, value):
    def fn(L, i):
        return L.poke(at(L, i), struct.pack(">H", value(L, i)))
    return fn


def _v1_vlen_over(L, i):
    r = L.rows[i]
    assert i == len(L.rows) - 1 and not r["flags"] & TOMB
    return L.poke(r["val"], struct.pack(">I", r["vl"] + 1))


def _v1_suffix_over(L, i):  # the suffix and the nine bytes behind it end one byte past the data
    r = L.rows[i]
    assert i == len(L.rows) - 1
    return L.poke(r["pos"] + 2, struct.pack(">H", L.data_end - r["suf"] - 9 + 1))


def _v1_tomb_expire(L, i):  # a tombstone that carries expire_ts: decoded, the timestamp dropped
    r = L.rows[i]
    assert not r["flags"] & (EXPIRE | CREATE)
    return L.build([(r["tail"] + 8, r["end"] - r["tail"] - 8, bytes([TOMB | EXPIRE]) + struct.pack(">q", 77))])


def v1_catalogue():
    C, F = CORRUPT, FLAGS
    M = Mutation
    first = lambda L, i: L.rows[i]["pos"]  # (row 0's prefix is the overlap word: the prefix mutations skip it)
    return [M("v1-overlap-nonzero", lambda L, _: L.poke(0, b"\x00\x01"), C, C),
            M("v1-first-key-past-end", lambda L, _: L.poke(2, struct.pack(">H", L.data_end - 4 + 1)), C, C),
            M("v1-offset+4-past-end", _table(_set(-1, lambda L: L.data_end - 3)), C, C),
            M("v1-suffix-1-past-end", _v1_suffix_over, C, C, "last"),
            M("v1-value-1-past-end", _v1_vlen_over, C, C, "last"),
            M("v1-prefix-eq-first-key", _v1_put16(first, lambda L, i: L.fk), 0, 0, "inner"),
            M("v1-prefix-over-first-key", _v1_put16(first, lambda L, i: L.fk + 1), C, C, "inner"),
            M("v1-tombstone-with-expire", _v1_tomb_expire, 0, 0, "any"),
            M("v1-count-0", _table(lambda L, o: ([], None)), 0, 0),
            M("v1-flags-10", _flags(0x10), F, F, "any"), M("v1-flags-09", _flags(0x09), F, F, "any")]


# whole blocks of 4 - 7 bytes (the CRC included): (name, payload, {version: (asc, desc)})
TINY = [("tiny-4", b"", {1: (CORRUPT, CORRUPT), 2: (CORRUPT, CORRUPT)}),
        ("tiny-5", b"\x00", {1: (CORRUPT, CORRUPT), 2: (CORRUPT, CORRUPT)}),
        # count 0, no data.  V1: BlockIterator::new reads the first key of any block (it panics here)
        ("tiny-6-count0", b"\x00\x00", {1: (CORRUPT, CORRUPT), 2: (0, 0)}),
        ("tiny-6-count1", b"\x00\x01", {1: (CORRUPT, CORRUPT), 2: (CORRUPT, CORRUPT)}),
        # count 0, one data byte: a V2 row starts there ascending; descending without restarts yields nothing
        ("tiny-7-count0", b"\x00\x00\x00", {1: (CORRUPT, CORRUPT), 2: (CORRUPT, 0)})]


# ----------------------------------------------------------------------------------------------------
# Shapes: the smallest SSTs that reach each count-pass path (sdb_decode.hip k_dec_count / k_dec_count_big)
# ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch(n, vmin, vmax):
    rng = np.random.default_rng(n + vmin)
    return Batch.from_entries([(b"key%05d/%06d" % (i // 7, i), 0,
                                bytes(rng.integers(0, 256, int(rng.integers(vmin, vmax)), dtype=np.uint8)),
                                100000 - i, None, None) for i in range(n)])


class Shape:
    """An oracle-encoded SST of >= 3 blocks; block 1 is the one the surgeon works on."""

    def __init__(self, name, version, block_size, restart_interval, n, vlen=(8, 40)):
        self.name, self.version, self.target = name, version, 1
        self.block_size, self.restart_interval = block_size, restart_interval
        self.batch = _batch(n, *vlen)
        self.enc = O.encode_sst(self.batch, O.params(block_size=block_size, sst_version=version,
                                                     restart_interval=restart_interval, bloom_bits_per_key=0))
        assert self.enc.status == 0
        off = [int(x) for x in self.enc.block_off]
        assert len(off) >= 4, name
        raw = self.enc.data.tobytes()
        self.payloads = [raw[off[k]:off[k + 1] - 4] for k in range(len(off) - 1)]
        self.layout = Layout(self.payloads[self.target], version)
        self.index_keys, self.index_key_off = O.sst_index_keys(self.batch, self.enc)

    def placements(self, kind):
        """{placement name: row} for a mutation's row kind."""
        L = self.layout
        n, mid = len(L.rows), max(L.count // 2, 0)
        midrows = L.region_rows(mid) if self.version == 2 else [n // 2]
        if self.version == 2 and L.count == 1:
            midrows = [n // 2 - 1, n // 2]
        cand = {"first-of-block": 0, "first-of-mid-region": midrows[0], "last-of-mid-region": midrows[-1],
                "last-of-block": n - 1}
        if self.version == 2 and L.count > 1:
            cuts = piece_cuts(L.offs, L.data_end)
            if len(cuts) > 1:  # the rows on both sides of a piece cut (for_each_piece)
                cand["before-piece-cut"] = L.region_rows(cuts[1] - 1)[-1]
                cand["after-piece-cut"] = L.region_rows(cuts[1])[0]
        ok = {"any": lambda i: True, "last": lambda i: i == n - 1, "first": lambda i: i == 0,
              "inner": lambda i: L.rows[i]["ri"] > 0,
              "restart": lambda i: L.rows[i]["ri"] == 0 and i > 0}[kind]
        if kind == "inner" and self.version == 2:  # the last row of a region is inner when regions have > 1 row
            cand["second-of-block"] = 1
        out = {}
        for k, i in cand.items():
            if ok(i) and i not in out.values():
                out[k] = i
        return out

    def sst_with(self, payload):
        """The SST with block `target` replaced -> (data with the zero tail, block_off)."""
        p = list(self.payloads)
        p[self.target] = payload
        return arena(p)


SHAPES = {
    # name: (version, block size, restart interval, entries, value lengths) -- the path a fault in block 1 takes
    "v2-spec-4regions-1k": (2, 1024, 8, 90),              # <= 4 regions: tally_v2_spec, then the exact walk
    "v2-fast-25regions-4k": (2, 4096, 4, 330),            # 5 - 64 regions: tally_v2_fast, then the exact walk
    "v2-lanes-113regions-4k": (2, 4096, 1, 560, (4, 12)),  # > 64 regions: tally_v2's lane loop wraps
    "v2-pieces-8k": (2, 8192, 16, 640),                   # over one image: k_dec_count_big, tally_v2_pieces
    "v2-pieces-16k": (2, 16384, 16, 1250),                # ... of several pieces
    "v2-hbm-1region-8k": (2, 8192, 1000, 640),            # a region over 3968 bytes: parse_v2 on HBM windows
    "v1-small-1k": (1, 1024, 16, 90),                     # tally_v1 from LDS
    "v1-big-8k": (1, 8192, 16, 640),                      # tally_v1 from HBM
}


@functools.lru_cache(maxsize=None)
def shape(name):
    return Shape(name, *SHAPES[name])


class Variant:
    """One mutated block 1 of a shape: id, payload, the declared statuses (asc, desc) and where they come from."""

    def __init__(self, vid, payload, asc, desc, desc_from="oracle", row=None, huge=False, parts=()):
        self.id, self.payload, self.asc, self.desc, self.desc_from = vid, payload, asc, desc, desc_from
        self.row, self.huge, self.parts = row, huge, parts

    def status(self, descending):
        return self.desc if descending else self.asc


@functools.lru_cache(maxsize=None)
def singles(shape_name):
    """Every catalogue mutation at every placement it fits, for one shape."""
    S = shape(shape_name)
    out = []
    for m in (v2_catalogue() if S.version == 2 else v1_catalogue()):
        if m.rows is None:
            if S.version == 2 and S.layout.count < 3 and m.name.startswith(("offset", "restart0-eq")):
                continue  # the table mutations need three regions; a one-region block has no such table
            if m.name == "restart0-on-row-1" and S.layout.rows[1]["sh"] == 0:
                continue  # one-row regions: row 1 is a restart itself
            out.append(Variant(m.name, m.fn(S.layout, None), m.asc, m.desc, m.desc_from))
            continue
        for where, i in S.placements(m.rows).items():
            out.append(Variant("%s@%s" % (m.name, where), m.fn(S.layout, i), m.asc, m.desc, m.desc_from, i, m.huge))
    return out


def _both(L, fa, ia, fb, ib):
    """Two in-place row mutations in one block."""
    a, b = fa(L, ia), fb(L, ib)
    base = L.payload
    assert len(a) == len(b) == len(base)
    out = bytearray(base)
    for x in (a, b):
        for p in range(len(base)):
            if x[p] != base[p]:
                out[p] = x[p]
    return bytes(out)


@functools.lru_cache(maxsize=None)
def doubles(shape_name):
    """Two faults of different statuses in one block, in both orders.  The expected status is the walker's
    (the first fault in iteration order); each variant carries its two single-fault payloads in `parts`."""
    S = shape(shape_name)
    L = S.layout
    n = len(L.rows)
    fl = _flags(0x10)
    out = []

    def add(name, ia, ib, corrupt_a=None, corrupt_b=None):
        """The flags fault on row ia with a corrupt row ib, and the other way round."""
        ca, cb = corrupt_a or six, corrupt_b or six
        for tag, (f1, f2) in (("flags-first", (fl, cb)), ("corrupt-first", (ca, fl))):
            out.append(Variant("%s/%s" % (name, tag), _both(L, f1, ia, f2, ib), None, None,
                               parts=(f1(L, ia), f2(L, ib))))

    if S.version == 1:
        pre = _v1_put16(lambda L, i: L.rows[i]["pos"], lambda L, i: L.fk + 1)
        add("v1-rows-2-and-count-2", 2, n - 2, pre, pre)
        out.append(Variant("v1-one-row-flags-and-prefix", _both(L, fl, n // 2, pre, n // 2), None, None,
                           parts=(fl(L, n // 2), pre(L, n // 2))))
        return out
    six = _six("vl")
    mid = L.region_rows(L.count // 2)
    if len(mid) > 1:  # (one-row regions have no second row to fault)
        add("same-region", mid[0], mid[-1])
    if L.count > 1:
        add("different-regions", L.region_rows(1)[0], L.region_rows(L.count - 1)[-1])
    else:
        add("far-rows", 1, n - 2)
    add("first-and-last-row", 0, n - 1, corrupt_b=_v2_vl_over)  # the one-byte overrun of the block's last row
    if L.count > 64 + 5:
        # region q and q + 64 are walked by the same lane; region 5 is lane 5 and region 68 lane 4, so lane
        # order is not row order
        add("same-lane-3-and-67", L.region_rows(3)[0], L.region_rows(67)[0])
        add("lane-order-5-and-68", L.region_rows(5)[0], L.region_rows(68)[0])
        last = L.count - 1
        assert last % 64 < 63
        add("lane-order-overrun-last", L.region_rows(last % 64 + 1)[0], n - 1, corrupt_b=_v2_vl_over)
    if L.count > 1:
        # restart 0's key is decoded by both iterators' constructors, before any row of any region
        out.append(Variant("restart0-shared-and-last-row-flags", _both(L, _shared_restart, 0, fl, n - 1), None, None,
                           parts=(_shared_restart(L, 0), fl(L, n - 1))))
    return out


def variants(shape_name):
    return singles(shape_name) + doubles(shape_name)


def expected(S, v, descending):
    """The status of variant v: the walker's, which for a single fault is also the declared one."""
    return walk(v.payload, S.version, descending)[0]


def lookup_keys(S, v):
    """The point queries of variant v: for a row fault the key of a row before it (in an earlier restart region
    where there is one), its own and the next row's (or the next block's first key); for a table fault the
    block's first, middle and last key."""
    clean = walk(S.layout.payload, S.version)[1]
    nxt = walk(S.payloads[2], S.version)[1][0][0]
    if v.row is None or v.row == 0:
        return [clean[0][0], clean[len(clean) // 2][0], clean[-1][0]]
    L = S.layout
    earlier = [i for i in range(v.row) if L.rows[i]["region"] < L.rows[v.row]["region"]] if S.version == 2 else []
    before = earlier[-1] if earlier else v.row - 1
    after = clean[v.row + 1][0] if v.row + 1 < len(clean) else nxt
    return [clean[before][0], clean[v.row][0], after]


def thin_faults(payload, version):
    """Three in-place faults on any well-formed block, for the entry points that only pass a block's status
    through: a bad flags byte, a one-byte overrun of the last row, a prefix longer than the key it shares
    with -> [(name, payload, status)] or None when the block's last row does not serve (timestamps, a V1
    tombstone)."""
    L = Layout(payload, version)
    n = len(L.rows)
    last = L.rows[-1]
    if last["flags"] & (EXPIRE | CREATE) or (version == 1 and last["flags"] & TOMB) or n < 4:
        return None
    if version == 2:
        inner = [i for i in range(1, n) if L.rows[i]["ri"] > 0 and L.payload[L.rows[i]["pos"]] < 0x7F]
        if not inner or L.payload[last["p_vl"]] >= 0x7F:
            return None
        out = [("bad-flags", _flags(0x10)(L, n // 2), FLAGS), ("overrun-by-1", _v2_vl_over(L, n - 1), CORRUPT),
               ("shared-over-prev", _shared(1)(L, inner[len(inner) // 2]), CORRUPT)]
    else:
        pre = _v1_put16(lambda L, i: L.rows[i]["pos"], lambda L, i: L.fk + 1)
        out = [("bad-flags", _flags(0x10)(L, n // 2), FLAGS), ("overrun-by-1", _v1_vlen_over(L, n - 1), CORRUPT),
               ("prefix-over-first-key", pre(L, n // 2), CORRUPT)]
    for name, p, st in out:
        assert len(p) == len(payload) and walk(p, version)[0] == st == walk(p, version, True)[0], name
    return out


def reseal(data, block_off, k, payload):
    """data (a numpy u8 array, changed in place) with block k replaced by a payload of the same length."""
    s, e = int(block_off[k]), int(block_off[k + 1])
    assert e - s - 4 == len(payload)
    data[s:e] = np.frombuffer(seal(payload), np.uint8)
