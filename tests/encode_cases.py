"""Hand-shaped batches for the encoder's compiled-in limits (sdb_encode.hip), with a CPU restatement of
the route each block takes (`route`) so that every case can prove on the oracle that it sits where it
claims.  Four families:

  R  one routing clause of emit_fast / the piece limits / the chunk-wide `huge` flag at a time, on
     either side of its limit;
  T  tombstones whose val_off range is not empty (the ABI ignores those bytes) and batches whose first
     offsets are not zero;
  F  chosen (prev_len, len, lcp) key pairs at k_facts' lane, round and workgroup edges, short keys at
     the end of the batch, chunk-sized batches, reference errors at workgroup edges;
  C  the longest candidate block on either side of k_anchor's lookahead (table composition vs the
     serial walk).

Batches are built from explicit arrays (never Batch.from_entries, which strips tombstone values and
starts every offset at zero).  A case is a `Case`: its batch, the encode parameters and what it expects."""
import functools

import numpy as np

from oracle import oracle as O
from slatedb_amd import _abi, datasets
from slatedb_amd.batch import Batch

# sdb_encode.h
CHUNK = 2048
IMG_CAP = 4096 + 64
STAGE_CAP = 4096
KEY_STAGE_CAP = 1024
PIECE_ROW_MAX, PIECE_KEY_MAX, PIECE_VAL_MAX = 4000, 960, 3968
SEG_LOOK = 1024

FORMATS = ((2, 1), (2, 16), (1, 1))  # (sst_version, restart_interval); set_header forces 1 for V1
TOMB = _abi.KIND_TOMBSTONE


class Case:
    def __init__(self, name, batch, expect=None, **kw):
        self.name = name
        self.batch = batch
        self.kw = kw            # O.params / runtime.params keywords
        self.expect = expect or {}

    def __repr__(self):
        return "Case(%s)" % self.name

    @property
    def version(self):
        return self.kw.get("sst_version", 2)

    @property
    def restart_interval(self):
        return self.kw.get("restart_interval", 16) if self.version == 2 else 1

    def ref(self):
        return O.encode_sst(self.batch, O.params(**self.kw))

    def routes(self, ref=None):
        return route(self.batch, ref or self.ref(), self.restart_interval, self.version)


# ------------------------------------------------------------------------------------------------
# batches from explicit arrays
# ------------------------------------------------------------------------------------------------
def make_batch(rows, k0=0, v0=0):
    """rows: (key, kind, value, seq[, create_ts, expire_ts]).  A tombstone KEEPS its value bytes in
    val_bytes; key_off[0] = k0 and val_off[0] = v0 (the bytes in front are filler)."""
    n = len(rows)
    keys = [bytes(r[0]) for r in rows]
    vals = [bytes(r[2]) for r in rows]
    key_off = np.full(n + 1, k0, np.uint64)
    val_off = np.full(n + 1, v0, np.uint64)
    if n:
        key_off[1:] += np.cumsum([len(k) for k in keys], dtype=np.uint64)
        val_off[1:] += np.cumsum([len(v) for v in vals], dtype=np.uint64)
    kb = np.frombuffer(b"\xEE" * k0 + b"".join(keys), np.uint8).copy()
    vb = np.frombuffer(b"\xDD" * v0 + b"".join(vals), np.uint8).copy()
    ts = lambda r, i: r[i] if len(r) > i and r[i] is not None else None
    cts = np.array([ts(r, 4) or 0 for r in rows], np.int64)
    ets = np.array([ts(r, 5) or 0 for r in rows], np.int64)
    mask = np.array([(ts(r, 4) is not None) * _abi.TS_CREATE + (ts(r, 5) is not None) * _abi.TS_EXPIRE
                     for r in rows], np.uint8)
    return Batch(kb, key_off, vb, val_off, np.array([r[1] for r in rows], np.uint8),
                 np.array([r[3] for r in rows], np.uint64), cts, ets, mask)


def stripped(b):
    """The same entries with every tombstone's bytes removed and both offsets starting at zero."""
    rows = []
    for i in range(b.n):
        m = int(b.ts_mask[i])
        rows.append((b.key(i), int(b.kind[i]), b"" if b.kind[i] == TOMB else b.value(i), int(b.seq[i]),
                     int(b.create_ts[i]) if m & _abi.TS_CREATE else None,
                     int(b.expire_ts[i]) if m & _abi.TS_EXPIRE else None))
    return make_batch(rows)


def _pat(n, salt=0):
    """n deterministic bytes."""
    return ((np.arange(n, dtype=np.uint32) * 131 + salt * 29 + 7) % 251).astype(np.uint8).tobytes()


def _small(i, vlen=20):
    return (b"key%08d" % i, 0, _pat(vlen, i), 100000 - i)


# ------------------------------------------------------------------------------------------------
# the restatement: k_facts' row facts and k_blocks' routing
# ------------------------------------------------------------------------------------------------
def _varint_len(v):
    v = np.asarray(v, np.uint64)
    return 1 + (v >= 1 << 7).astype(np.int64) + (v >= 1 << 14) + (v >= 1 << 21) + (v >= 1 << 28)


def facts(b, version=2):
    """k_facts' per-entry facts: klen, vlen (0 for a tombstone whatever its val_off range), lcp with the
    previous key, restart-row size s_r and non-restart size s_nr."""
    klen = np.diff(b.key_off).astype(np.int64)
    vraw = np.diff(b.val_off).astype(np.int64)
    kind = b.kind if b.kind is not None else np.zeros(b.n, np.uint8)
    mask = b.ts_mask if b.ts_mask is not None else np.zeros(b.n, np.uint8)
    tomb = kind == TOMB
    vlen = np.where(tomb, 0, vraw)
    lcp = np.zeros(b.n, np.int64)
    prev = None
    for i in range(b.n):
        k = b.key(i)
        if prev is not None:
            m = min(len(k), len(prev))
            j = 0
            while j < m and k[j] == prev[j]:
                j += 1
            lcp[i] = j
        prev = k
    ts8 = 8 * (((mask & _abi.TS_CREATE) != 0).astype(np.int64) + ((mask & _abi.TS_EXPIRE) != 0))
    if version == 2:
        suf = klen - lcp
        s_nr = _varint_len(lcp) + _varint_len(suf) + _varint_len(vlen) + suf + vlen + 9 + ts8
        s_r = 1 + _varint_len(klen) + _varint_len(vlen) + klen + vlen + 9 + ts8
    else:
        s_r = 4 + klen + 9 + ts8 + np.where(tomb, 0, 4 + vlen)
        s_nr = s_r
    return dict(klen=klen, vlen=vlen, vraw=vraw, tomb=tomb, lcp=lcp, s_r=s_r, s_nr=s_nr)


def chunk_flags(b, version=2):
    """Per chunk of 2048 entries, what k_facts leaves in huge_part: a row the piece path cannot stage
    (restart size over 4000, key over 960, value over 3968, a tombstone's value counting as empty), or
    a tombstone whose ignored val_off range is not empty (the LDS stages cannot skip those bytes)."""
    f = facts(b, version)
    row = (f["s_r"] > PIECE_ROW_MAX) | (f["klen"] > PIECE_KEY_MAX) | (f["vlen"] > PIECE_VAL_MAX)
    carry = f["tomb"] & (f["vraw"] > 0)
    nc = (b.n + CHUNK - 1) // CHUNK
    return ([bool(row[c * CHUNK:(c + 1) * CHUNK].any()) for c in range(nc)],
            [bool(carry[c * CHUNK:(c + 1) * CHUNK].any()) for c in range(nc)])


def route(b, ref, restart_interval, version=2):
    """Per block of the oracle's SST `ref`: ne, bb, nv16, nk16 (emit_fast's four quantities, from the
    batch's raw offsets), the chunk-wide flags over chunks s/2048 .. (e-1)/2048, and the assembler the
    device picks: "image" (k_emit's per-wave LDS image), "pieces" (k_emit_big) or "workgroup"."""
    huge_c, carry_c = chunk_flags(b, version)
    out = []
    nb = len(ref.block_off) - 1
    for k in range(nb):
        s, e = int(ref.block_first_entry[k]), int(ref.block_first_entry[k + 1])
        vs, ve, ks, ke = int(b.val_off[s]), int(b.val_off[e]), int(b.key_off[s]), int(b.key_off[e])
        ne, bb = e - s, int(ref.block_off[k + 1] - ref.block_off[k])
        nv16 = (ve - (vs & ~15) + 15) >> 4 if ve > vs else 0
        nk16 = (ke - (ks & ~15) + 15) >> 4
        cs = range(s // CHUNK, (e - 1) // CHUNK + 1)
        huge, carry = any(huge_c[c] for c in cs), any(carry_c[c] for c in cs)
        fast = ne <= 64 and bb + 64 <= IMG_CAP and nv16 <= STAGE_CAP // 16 and nk16 <= KEY_STAGE_CAP // 16
        r = "image" if fast and not carry else "workgroup" if huge or carry else "pieces"
        out.append(dict(s=s, e=e, ne=ne, bb=bb, nv16=nv16, nk16=nk16, huge=huge, carry=carry, route=r,
                        restart_interval=restart_interval))
    return out


def counts(routes):
    """(image, pieces, workgroup) block counts: the device's big_count and slow_count are the last two."""
    rs = [r["route"] for r in routes]
    return rs.count("image"), rs.count("pieces"), rs.count("workgroup")


# ------------------------------------------------------------------------------------------------
# R: routing, one factor at a time
# ------------------------------------------------------------------------------------------------
def _fmt_kw(version, ri, block_size, bloom=10):
    return dict(sst_version=version, restart_interval=ri, block_size=block_size, bloom_bits_per_key=bloom)


def _framed(rows, block_size, key_pad=16):
    """[a row that fills a block alone] rows [another]: the rows between them are one block (block 1)
    if they fit the block size, since neither neighbour can share a block with anything."""
    lead = (b"a" * key_pad, 0, _pat(block_size, 1), 200000)
    term = (b"z" * key_pad, 0, _pat(block_size, 2), 1)
    return [lead] + list(rows) + [term]


def _r_case(name, rows, version, ri, block_size, clause, value, want, twin, k0=0, v0=0, framed=True, block=1):
    rows = _framed(rows, block_size) if framed else list(rows)
    return Case("R/%s/v%d-ri%d" % (name, version, ri), make_batch(rows, k0, v0),
                dict(block=block, clause=clause, value=value, route=want, twin="R/%s/v%d-ri%d" % (twin, version, ri)),
                **_fmt_kw(version, ri, block_size))


def _sized_rows(target, block_size, version, ri):
    """39 rows whose framed block encodes to exactly `target` bytes (CRC included): the value length of
    all rows sets the size roughly, the last row's value length byte for byte (a one-byte varint)."""
    prm = O.params(**_fmt_kw(version, ri, block_size, 0))

    def rows(vl, last):
        return [(b"key%08d" % i, 0, _pat(vl if i < 38 else last, i), 1000 - i) for i in range(39)]

    for vl in range(70, 127):
        b = make_batch(_framed(rows(vl, 0), block_size))
        e = O.encode_sst(b, prm)
        if len(e.block_off) - 1 != 3:
            continue
        need = target - int(e.block_off[2] - e.block_off[1])
        if 0 <= need < 128:
            return rows(vl, need)
    raise AssertionError("no block of %d bytes" % target)


def r_cases():
    out = []
    for v, ri in FORMATS:
        # rows per block: 64 fit the image's lanes, 65 do not
        for ne, want, twin in ((64, "image", 65), (65, "workgroup", 64)):
            out.append(_r_case("rows-%d" % ne, [_small(i) for i in range(ne)], v, ri, 4096, "ne", ne, want,
                               "rows-%d" % twin))
        # block bytes: bb + 64 <= 4160
        for bb, bs, want, twin in ((4095, 4096, "image", None), (4096, 4096, "image", 4097),
                                   (4097, 8192, "workgroup", 4096), (4100, 8192, "workgroup", None)):
            c = _r_case("bytes-%d" % bb, _sized_rows(bb, bs, v, ri), v, ri, bs, "bb", bb, want, "bytes-%s" % twin)
            if twin is None:
                c.expect["twin"] = None
            out.append(c)
        # staged key bytes: 64 granules of 16 bytes
        k128 = [(b"k%0127d" % i, 0, _pat(10, i), 500 - i) for i in range(8)]
        k129 = [(b"k%0128d" % i, 0, _pat(10, i), 500 - i) for i in range(8)]
        out.append(_r_case("keys-128-at-0", k128, v, ri, 4096, "nk16", 64, "image", "keys-128-at-1"))
        out.append(_r_case("keys-128-at-1", k128, v, ri, 4096, "nk16", 65, "workgroup", "keys-128-at-0", k0=1))
        out.append(_r_case("keys-129-at-0", k129, v, ri, 4096, "nk16", 65, "workgroup", "keys-128-at-0"))
        # staged value bytes: one row of 4066 / 4067 bytes never spans more than 256 granules
        for vl in (4066, 4067):
            for v0 in (0, 1, 15):
                nv = (v0 + vl + 15) >> 4
                out.append(_r_case("value-%d-at-%d" % (vl, v0), [(b"k", 0, _pat(vl, v0), 7)], v, ri, 4096, "nv16", nv,
                                   "image", None, v0=v0))
                out[-1].expect["twin"] = None
        # the piece limits, inside 16 KiB blocks of small rows (no framing rows: those are huge themselves)
        hdr = 13 if v == 2 else 17  # s_r - klen - vlen for a two-byte value varint / the V1 row
        limits = (("s_r", PIECE_ROW_MAX, 100, PIECE_ROW_MAX - hdr - 100), ("klen", PIECE_KEY_MAX, PIECE_KEY_MAX, 10),
                  ("vlen", PIECE_VAL_MAX, 12, PIECE_VAL_MAX))
        for fact, limit, kl, vl in limits:
            for d, want in ((0, "pieces"), (1, "workgroup")):
                kl2, vl2 = (kl + d, vl) if fact == "klen" else (kl, vl + d)
                rows = [_small(i) for i in range(600)]
                rows[150] = (b"key%08d" % 150 + b"x" * (kl2 - 11), 0, _pat(vl2, 3), 77)
                c = _r_case("piece-%s-%d" % (fact, limit + d), rows, v, ri, 16384, fact, limit + d, want,
                            "piece-%s-%d" % (fact, limit + 1 - d), framed=False, block=0)
                c.expect.update(row=150, all_routes=want)  # the flag is chunk-wide: the SST's other block follows
                out.append(c)
        # the flag is per chunk of 2048 entries, not per block
        big = lambda i: (b"key%08d" % i, 0, _pat(5000, i), 9)
        rows = [_small(i) for i in range(1400)]
        rows[1300] = big(1300)
        c = _r_case("huge-neighbour", rows, v, ri, 16384, "huge", True, "workgroup", "huge-none", framed=False, block=0)
        c.expect["all_routes"] = "workgroup"
        out.append(c)
        c = _r_case("huge-none", [_small(i) for i in range(1400)], v, ri, 16384, "huge", False, "pieces",
                    "huge-neighbour", framed=False, block=0)
        c.expect["all_routes"] = "pieces"
        out.append(c)
        # a block that ends at entry 2047 is not flagged by a huge row at entry 2048 ...
        rows = [_small(i) for i in range(2048)] + [(b"key%08d" % 2048, 0, _pat(16384, 5), 9)] + \
               [_small(i) for i in range(2049, 2060)]
        c = _r_case("huge-next-chunk", rows, v, ri, 16384, "huge", False, "pieces", "huge-straddle", framed=False,
                    block="ends-at-2048")
        out.append(c)
        # ... and one that straddles entry 2048 is, by a huge row anywhere in the second chunk
        rows = [_small(i) for i in range(2200)]
        rows[2150] = big(2150)
        c = _r_case("huge-straddle", rows, v, ri, 16384, "huge", True, "workgroup", "huge-next-chunk", framed=False,
                    block="straddles-2048")
        out.append(c)
    return out


def target_block(case, routes):
    """The index of the block a case's expectation speaks of."""
    b = case.expect["block"]
    if b == "ends-at-2048":
        return next(i for i, r in enumerate(routes) if r["e"] == CHUNK)
    if b == "straddles-2048":
        return next(i for i, r in enumerate(routes) if r["s"] < CHUNK < r["e"])
    return b


# ------------------------------------------------------------------------------------------------
# T: tombstones carrying ignored bytes, non-zero first offsets
# ------------------------------------------------------------------------------------------------
T_PAYLOADS = (1, 100, 4097)
T_POSITIONS = ("first", "middle", "last")
T_OFFSETS = (0, 1, 15, 16)
T_N = 500
# Values k_emit copies through its span table, not from registers (over 108 bytes: batches of spans up to
# 128 bytes, longer ones row by row), behind a tombstone whose ignored bytes push them up the value stage:
# the stage overlaps the block image, and only a staged byte at or below its image position is safe there.
T_SPAN_VLENS = (120, 200)
T_SPAN_PAYLOAD = 1000


def _t_rows(tomb, fat, pad, carrier=None, payload=0, vlen=100):
    """T_N rows of vlen-byte values; the rows in `tomb` are tombstones (`carrier` with `payload` ignored
    bytes), row `fat` has a 3000-byte value and row pad[0] one of vlen + pad[1] bytes."""
    rows = []
    for i in range(T_N):
        if i in tomb:
            rows.append((b"key%08d" % i, TOMB, _pat(payload if i == carrier else 0, i), 100000 - i))
        else:
            vl = 3000 if i == fat else vlen + pad[1] if i == pad[0] else vlen
            rows.append((b"key%08d" % i, 0, _pat(vl, i), 100000 - i))
    return rows


@functools.lru_cache(maxsize=None)
def _t_layout(version, block_size, vlen=100):
    """Tombstones at the first, a middle and the last row of block 1 (about 35 rows per 4 KiB at 100 bytes).  A
    tombstone is a short row: block 0's last value is padded until the first one no longer fits behind
    it, and the row after the last one is too fat to follow it into block 1."""
    prm = O.params(**_fmt_kw(version, 16, block_size, 0))
    firsts = lambda tomb, fat, pad: [int(x) for x in
                                     O.encode_sst(make_batch(_t_rows(tomb, fat, pad, vlen=vlen)), prm).block_first_entry[1:3]]
    s = firsts((), None, (None, 0))[0]
    for extra in range(140):
        pad = (s - 1, extra)
        if firsts((s, s + 5), None, pad)[0] == s:
            t = firsts((s, s + 5), None, pad)[1]
            tomb = (s, s + 5, t - 1)
            assert firsts(tomb, t, pad) == [s, t]
            return dict(zip(T_POSITIONS, tomb)), t, pad
    raise AssertionError("block 0 cannot be filled")


def t_batch(version, block_size, payload, position, off, vlen=100):
    """The T layout with `payload` ignored bytes on the tombstone at `position` (None: on none of them) and
    both first offsets at `off`."""
    pos, fat, pad = _t_layout(version, block_size, vlen)
    carrier = None if position is None else pos[position]
    return make_batch(_t_rows(set(pos.values()), fat, pad, carrier, payload, vlen), off, off)


def t_cases(block_sizes=(4096, 16384), versions=(2, 1), blooms=(10, 0)):
    out = []
    for bs in block_sizes:
        for v in versions:
            for bloom in blooms:
                kw = _fmt_kw(v, 16, bs, bloom)
                for off in T_OFFSETS:
                    if off:  # non-zero first offsets alone
                        out.append(Case("T/plain/bs%d-v%d-f%d-off%d" % (bs, v, bloom, off),
                                        t_batch(v, bs, 0, None, off), dict(payload=0, position=None), **kw))
                    for payload in T_PAYLOADS:
                        for position in T_POSITIONS:
                            out.append(Case("T/%d-%s/bs%d-v%d-f%d-off%d" % (payload, position, bs, v, bloom, off),
                                            t_batch(v, bs, payload, position, off),
                                            dict(payload=payload, position=position), **kw))
                for vlen in T_SPAN_VLENS:
                    for position in T_POSITIONS[:2]:
                        out.append(Case("T/spans%d-%s/bs%d-v%d-f%d" % (vlen, position, bs, v, bloom),
                                        t_batch(v, bs, T_SPAN_PAYLOAD, position, 0, vlen),
                                        dict(payload=T_SPAN_PAYLOAD, position=position), **kw))
    return out


# ------------------------------------------------------------------------------------------------
# F: the k_facts lattice
# ------------------------------------------------------------------------------------------------
F_LCPS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 127, 128)
F_N = 4097
F_ROTATIONS = (0, 1, 2)


def f_specs():
    """(prev_len, len, lcp) triples: differing keys, equal keys (lcp == len == prev_len), extensions
    (lcp == prev_len < len), lengths that are no multiple of 16, keys of 1 to 3 bytes."""
    specs = []
    for c in F_LCPS:
        specs.append((c + 3, c + 5, c))
        specs.append((c + 13, c + 1, c))
        if c:
            specs.append((c, c, c))
            specs.append((c, c + 2, c))
    specs += [(1, 1, 0), (1, 1, 1), (1, 2, 1), (2, 3, 2), (3, 3, 0), (2, 1, 0), (3, 2, 1), (3, 3, 3), (16, 16, 16)]
    assert len(specs) % 2 == 1  # a tile of 2 * len(specs) entries then visits every residue mod 64 of its parity
    return specs


def _pair(spec, u):
    """Two keys realising spec, whose first byte differs from the neighbouring pairs' (so the pair's first
    key has lcp 0 with whatever precedes it and is never a prefix of it)."""
    pl, ln, c = spec
    assert c <= min(pl, ln) and (c < ln or pl == ln)
    lead = b"cd"[u % 2:u % 2 + 1] if c else b""
    common = (lead + b"m" * c)[:c]
    prev = common + (b"p" if c == 0 else b"x") * (pl - c)
    cur = common + (b"q" if c == 0 else b"y") * (ln - c)
    return prev, cur


@functools.lru_cache(maxsize=None)
def f_tiled(rotation):
    """F_N entries: `rotation` filler entries, then the specs' pairs over and over.  Returns the batch and
    `where`: entry -> spec index for the second key of every pair."""
    specs = f_specs()
    rows, where = [], {}
    for i in range(rotation):
        rows.append((b"A%d" % i, 0, b"f", F_N))
    u = 0
    while len(rows) < F_N:
        prev, cur = _pair(specs[u % len(specs)], u)
        rows.append((prev, 0, _pat(3, u), F_N - len(rows)))
        if len(rows) < F_N:
            where[len(rows)] = u % len(specs)
            rows.append((cur, 0, _pat(5, u), F_N - len(rows)))
        u += 1
    return make_batch(rows), where


def f_lattice_cases():
    out = []
    for rot in F_ROTATIONS:
        b, _ = f_tiled(rot)
        for v in (2, 1):
            for bs in (256, 4096):
                out.append(Case("F/lattice-rot%d/v%d-bs%d" % (rot, v, bs), b, dict(rotation=rot), **_fmt_kw(v, 16, bs)))
    return out


def f_tail_cases():
    """Keys whose 16-byte window would run past key_off[n]: k_facts re-reads them byte by byte."""
    out = []
    body = lambda n: [(b"key%017d" % i, 0, _pat(9, i), 9000 - i) for i in range(n)]  # 20-byte keys
    short = [(b"zza", 0, b"1", 3), (b"zzb", 0, b"2", 2), (b"zzc", 0, b"3", 1)]
    for k in (1, 2, 3):
        out.append(("F/tail-%d-short" % k, body(70) + short[:k], k))
    for n in (1, 2, 5):
        out.append(("F/tail-n%d" % n, [(b"k%d" % i, 0, b"v", 9 - i) for i in range(n)], n))
    for n in (65, 2049):  # the last entry is a lane 0 whose previous key also lies in the last 16 bytes
        out.append(("F/tail-lane0-n%d" % n, body(n - 2) + [(b"zzzza", 0, b"1", 2), (b"zzzzb", 0, b"2", 1)], 2))
    cases = []
    for name, rows, k in out:
        for v in (2, 1):
            cases.append(Case("%s/v%d" % (name, v), make_batch(rows), dict(short=k), **_fmt_kw(v, 16, 4096)))
    return cases


F_GEOMETRY_N = (2047, 2048, 2049, 4096, 4097)


def f_geometry_cases():
    """D1 rows at block size 64 (every entry its own block: 2048 blocks in a chunk, the n + 1-sized lists
    full) and at 4096."""
    return [Case("F/geometry-n%d/bs%d" % (n, bs), datasets.d1(n=n), dict(n=n), **_fmt_kw(2, 16, bs))
            for n in F_GEOMETRY_N for bs in (64, 4096)]


F_ERR_N = 4100


def _err_rows(errors):
    """F_ERR_N rows of 12-byte keys with `errors` = {entry: what} planted."""
    rows = [(b"key%09d" % i, 0, b"v", F_ERR_N - i) for i in range(F_ERR_N)]
    for i, what in errors.items():
        k, kind, val, seq = rows[i]
        if what == "empty":
            rows[i] = (b"", kind, val, seq)
        elif what == "prefix":  # a proper prefix of its predecessor
            rows[i] = (rows[i - 1][0][:-1], kind, val, seq)
        elif what == "kind":
            rows[i] = (k, 7, val, seq)
        elif what == "v1-long-key":
            rows[i] = (k + b"k" * 70000, kind, val, seq)
        else:
            raise KeyError(what)
    return rows


F_ERRORS = (("empty", 2, _abi.SDB_EMPTY_KEY), ("prefix", 2, _abi.SDB_INVALID_ARGUMENT),
            ("kind", 2, _abi.SDB_INVALID_ARGUMENT), ("v1-long-key", 1, _abi.SDB_LIMIT_EXCEEDED))


def f_error_cases():
    out = []
    for what, v, status in F_ERRORS:
        for at in (2047, 2048, 2049):
            out.append(Case("F/error-%s-at-%d" % (what, at), make_batch(_err_rows({at: what})),
                            dict(status=status, entry=at), **_fmt_kw(v, 16, 4096)))
    # two errors in two k_facts workgroups: the earlier entry's wins
    out.append(Case("F/error-two", make_batch(_err_rows({3000: "empty", 100: "kind"})),
                    dict(status=_abi.SDB_INVALID_ARGUMENT, entry=100), **_fmt_kw(2, 16, 4096)))
    out.append(Case("F/error-two-swapped", make_batch(_err_rows({3000: "kind", 100: "empty"})),
                    dict(status=_abi.SDB_EMPTY_KEY, entry=100), **_fmt_kw(2, 16, 4096)))
    # a WAL SST has no index keys: a key that is a prefix of its predecessor is fine
    for at in (2047, 2048):
        out.append(Case("F/wal-prefix-at-%d" % at, make_batch(_err_rows({at: "prefix"})), dict(status=0, entry=None),
                        sst_type=_abi.SST_WAL, **_fmt_kw(2, 16, 4096)))
    return out


# ------------------------------------------------------------------------------------------------
# C: chain mode (k_anchor: table composition when the longest candidate block fits the lookahead)
# ------------------------------------------------------------------------------------------------
C_N = 2600


def tiny_rows(n=C_N):
    keys = np.arange(n, dtype=">u4").view(np.uint8).copy()  # consecutive keys share 3 bytes: 13-byte V2 rows
    return Batch(keys, np.arange(n + 1, dtype=np.uint64) * np.uint64(4), np.zeros(0, np.uint8),
                 np.zeros(n + 1, np.uint64), np.zeros(n, np.uint8), np.arange(n, dtype=np.uint64),
                 np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.uint8))


def seg_look(block_size):
    """set_header's lookahead: a block holds at most block_size / 12 + 2 entries, staged up to 1024."""
    return min(block_size // 12 + 2, SEG_LOOK)


def longest_candidate(b, version, block_size, ri):
    """The longest block that would start at any entry (BlockBuilder::would_fit from every start, cut at
    the batch's end): k_seg's wmax.  V1 prefixes are against the candidate's first key, so V1 is restated
    for 4-byte keys only (tiny_rows)."""
    n = b.n
    if version == 2:
        f = facts(b, 2)
        best = 0
        for rho in range(ri):  # candidates starting at entries = rho mod ri share their restart rows
            cost = np.where((np.arange(n) - rho) % ri == 0, f["s_r"] + 2, f["s_nr"])
            cum = np.concatenate([[0], np.cumsum(cost)])
            s = np.arange(rho, n, ri)
            # entries s .. s + m - 1 fit while 2 + cum[s + m] - cum[s] <= block_size; the first always does
            m = np.searchsorted(cum, cum[s] + block_size - 2, side="right") - 1 - s
            best = max(best, int(np.maximum(m, 1).max()))
        return best
    assert (np.diff(b.key_off) == 4).all() and not b.val_off[-1]
    keys = b.key_bytes.view(">u4").astype(np.int64)
    best = 0
    span = block_size // 13 + 2
    for s in range(n):
        w = keys[s:s + span]
        x = w ^ w[0]
        pre = np.where(x == 0, 4, np.where(x < 1 << 8, 3, np.where(x < 1 << 16, 2, np.where(x < 1 << 24, 1, 0))))
        pre[0] = 0  # the first key is written whole
        row = 4 + (4 - pre) + 9 + 4  # V0 row of a value of 0 bytes
        before = 2 + np.concatenate([[0], np.cumsum(row + 2)[:-1]])  # Block::size before entry j
        fits = before + row <= block_size
        fits[0] = True
        bad = np.nonzero(~fits)[0]
        best = max(best, int(bad[0]) if bad.size else len(w))
    return best


@functools.lru_cache(maxsize=None)
def tiny_wmax(version, block_size):
    return longest_candidate(tiny_rows(), version, block_size, 16 if version == 2 else 1)


C_SERIAL_BS = {2: 16384, 1: 32768}  # tiny_rows' blocks are longer than the lookahead and shorter than a chunk


@functools.lru_cache(maxsize=None)
def c_threshold(version):
    """The smallest block size at which tiny_rows' longest candidate block exceeds the lookahead of 1024."""
    lo, hi = 12276, C_SERIAL_BS[version]  # seg_look is 1024 from 12264 on
    assert tiny_wmax(version, hi) > SEG_LOOK >= tiny_wmax(version, lo)
    while lo + 1 < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if tiny_wmax(version, mid) > SEG_LOOK else (mid, hi)
    return hi


def c_block_sizes(version):
    # 12252 / 12264: the lookahead itself just under and at its cap of 1024
    t = c_threshold(version)
    return sorted({8192, 12252, 12264, 16384, t - 1, t, C_SERIAL_BS[version]})


def c_cases():
    out = []
    for v in (2, 1):
        for bs in c_block_sizes(v):
            w = tiny_wmax(v, bs)
            out.append(Case("C/v%d-bs%d" % (v, bs), tiny_rows(),
                            dict(wmax=w, mode=1 if 1 <= w <= seg_look(bs) else 0),
                            **_fmt_kw(v, 16 if v == 2 else 1, bs)))
    return out


# ------------------------------------------------------------------------------------------------
# P: which table path a chain takes (k_anchor: tables in LDS, streamed per wave, HBM; k_group for the
# compactor's cuts: LDS or HBM compose), the kernels' predicates restated for the host (sdb_encode.hip: kAnchorLds,
# kAnchorThreads / 64, kGroupLds and the layouts in k_anchor / k_group -- a change there is repeated here, or the
# P shapes below silently stop reaching their paths)
# ------------------------------------------------------------------------------------------------
ANCHOR_LDS, GROUP_LDS, ANCHOR_WAVES = 148 * 1024, 96 * 1024, 16


def _al16(x):
    return (x + 15) & ~15


def chain_geometry(n):
    """(chunks, chunks per group, groups) as plan_slot sizes them."""
    k, g = (n + CHUNK - 1) // CHUNK, 16
    while g * g < k:
        g += 1
    return k, g, (k + g - 1) // g


def anchor_path(n, w, block_size):
    """k_anchor's path for n entries whose longest candidate block is w entries."""
    k, g, ng = chain_geometry(n)
    if not 1 <= w <= seg_look(block_size):
        return "mode0"
    if 2 * _al16(2 * k * w) + 8 * k * w + 16 * ng * w + 16 * ng <= ANCHOR_LDS:
        return "lds"
    for gs in range(g, 0, -1):  # group tables + a buffer of gs chunk tables per wave
        ngs = (k + gs - 1) // gs
        tables = _al16(2 * _al16(4 * ngs * w) + 8 * ngs * w + 16 * ngs)
        if tables + ANCHOR_WAVES * _al16(12 * gs * w) <= ANCHOR_LDS:
            return "streamed"
    return "hbm"


def group_paths(n, w, block_size):
    """k_group's compose path of every group (the last group may be shorter, and fit)."""
    k, g, ng = chain_geometry(n)
    if not 1 <= w <= seg_look(block_size):
        return {"mode0"}
    return {"lds" if min(g, k - q * g) * w * 14 + 64 <= GROUP_LDS else "hbm" for q in range(ng)}


# 101 chunks of 13-byte rows, ~120 / ~127 candidates per chunk: the chunk tables outgrow k_anchor's LDS while
# the group tables and a buffer per wave still fit (the smallest chunk count with such a window is 77)
P_STREAMED_N, P_STREAMED_BS = 100 * CHUNK + 700, (1600, 1700)
# 34 chunks, ~615 candidates: the 16 chunk tables of groups 0 and 1 outgrow k_group's LDS, the last group's 2 fit.
# The cut sizes: under one group's bytes (~442 KB: the walk takes no group table), group 0 taken and the cut
# right behind it / further into group 1, groups 0 and 1 taken (group 1 entered at candidate 389) and the cut
# inside group 2, and one SST.
P_CUTS_N, P_CUTS_BS = 33 * CHUNK + 100, 8192
P_CUTS_MAX_SST = (30000, 450000, 600000, 880000, 10 ** 12)


def all_cases():
    return (r_cases() + t_cases() + f_lattice_cases() + f_tail_cases() + f_geometry_cases() + f_error_cases() +
            c_cases())
