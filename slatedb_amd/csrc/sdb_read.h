// sdb_read.h — the one reader of an encoded block, shared by the point lookups (sdb_lookup.hip), the range
// scans (sdb_scan.hip), the tree gets (sdb_get.hip) and the tree scans (sdb_lsm_scan.hip): the incremental key
// comparators, Block::decode of a checked block, the entry-header and row parsers, the seeks, the row walker and
// the row -> column writer, the index partition_point, the bounds + CRC pass over marked blocks and the
// consistency check of a tree's index arrays.  Everything takes what it reads (an
// sdb_sst_view, a Blk), never a kernel's argument struct.  What reads a key range (the bounds, the covering block
// range, the lowest failing block, the clip of a block, the restored key) is in sdb_range.h, on top of this header, for the two scans.
#pragma once
#include "sdb_bloom.h"
#include "sdb_crc.h"
#include "sdb_device.h"
#include "sdb_filter.h"
#include "sdb_reads.h"

namespace sdb {

SDB_DEV uint64_t be_at(const uint8_t *p, int n) {
    uint64_t v = 0;
    for (int i = 0; i < n; i++) v = (v << 8) | p[i];
    return v;
}

// Order of a and b (<[u8] as Ord>) and their common prefix, from global memory.
struct Cmp {
    uint32_t m;  // common prefix of key and target
    int c;       // sign(key cmp target)
    uint32_t len;
};
SDB_DEV Cmp cmp_bytes(const uint8_t *a, uint32_t na, const uint8_t *t, uint32_t nt, uint32_t base) {
    // a is the key from byte `base` on; t the whole target
    Cmp r;
    const uint32_t rest = nt > base ? nt - base : 0;
    const uint32_t l = lcp_bytes(a, na, t + base, rest);
    r.m = base + l;
    r.len = base + na;
    if (l < na && l < rest) r.c = a[l] < t[base + l] ? -1 : 1;
    else r.c = na < rest ? -1 : (na > rest ? 1 : 0);
    return r;
}
// The key K' = K[..sh] ++ S given K's state s against the target.
SDB_DEV Cmp cmp_next(Cmp s, uint32_t sh, const uint8_t *S, uint32_t un, const uint8_t *t, uint32_t nt) {
    if (sh > s.m) {  // K' agrees with K on [0, m]: same order; T a proper prefix of K' when m == |T|
        Cmp r;
        r.m = s.m;
        r.len = sh + un;
        r.c = s.m < nt ? s.c : 1;
        return r;
    }
    return cmp_bytes(S, un, t, nt, sh);  // K'[0, sh) == T[0, sh)
}

struct Blk {  // Block::decode of a checked block
    const uint8_t *d;
    uint32_t data_end, count;
    const uint8_t *offs;
    uint64_t base;
};
SDB_DEV int blk_open(const sdb_sst_view &v, uint64_t k, Blk &b) {
    const uint64_t s = v.block_off[k], e = v.block_off[k + 1];
    if (e < s || e - s < 6) return SDB_CORRUPT_BLOCK;
    const uint32_t blen = (uint32_t)(e - s - 4);
    b.d = v.data + s;
    b.base = s;
    b.count = (uint32_t)be_at(b.d + blen - 2, 2);
    if (2 + 2 * (uint64_t)b.count > blen) return SDB_CORRUPT_BLOCK;
    b.data_end = blen - 2 - 2 * b.count;
    b.offs = b.d + b.data_end;
    return 0;
}
SDB_DEV uint32_t boff(const Blk &b, uint32_t i) { return (uint32_t)be_at(b.offs + 2 * i, 2); }

SDB_DEV bool rdv(const uint8_t *d, uint32_t end, uint32_t &pos, uint32_t &v) {  // decode_varint
    uint32_t r = 0;
    for (int sh = 0; sh <= 28; sh += 7) {
        if (pos >= end) return false;
        const uint8_t x = d[pos++];
        r |= (uint32_t)(x & 0x7F) << sh;
        if (!(x & 0x80)) {
            v = r;
            return true;
        }
    }
    return false;
}
SDB_DEV bool flags_valid(uint8_t f) { return !(f & ~0x0Fu) && !((f & SDB_FLAG_TOMBSTONE) && (f & SDB_FLAG_MERGE_OPERAND)); }

struct Row {
    uint32_t sh, un, vl, suf, vpos, next;
    uint64_t seq;
    int64_t cts, ets;
    uint8_t flags;
};
// The V2 entry header at byte p: the varints shared, unshared and value length (row_codec_v2.rs:172-186), with
// shared <= max_sh (what the caller knows of the previous key) and the key suffix d[suf, suf + un) inside the
// data.  !ok: corrupt.
struct V2Hdr {
    bool ok;
    uint32_t sh, un, vl, suf;
};
SDB_DEV V2Hdr v2_hdr(const Blk &b, uint32_t p, uint32_t max_sh) {
    V2Hdr h{};
    if (!rdv(b.d, b.data_end, p, h.sh) || !rdv(b.d, b.data_end, p, h.un) || !rdv(b.d, b.data_end, p, h.vl) ||
        h.sh > max_sh || (uint64_t)p + h.un > b.data_end)
        return h;
    h.ok = true;
    h.suf = p;
    return h;
}
// The row tail at byte p, its first nine bytes inside the data: seq, flags, then expire_ts and create_ts where
// flagged.  p moves past it.
SDB_DEV int row_tail(const Blk &b, uint32_t &p, Row &r) {
    r.seq = be_at(b.d + p, 8);
    r.flags = b.d[p + 8];
    p += 9;
    if (!flags_valid(r.flags)) return SDB_INVALID_ROW_FLAGS;
    const uint32_t need = ((r.flags & SDB_FLAG_HAS_EXPIRE_TS) ? 8 : 0) + ((r.flags & SDB_FLAG_HAS_CREATE_TS) ? 8 : 0);
    if ((uint64_t)p + need > b.data_end) return SDB_CORRUPT_BLOCK;
    r.ets = r.cts = 0;
    if (r.flags & SDB_FLAG_HAS_EXPIRE_TS) {
        r.ets = (int64_t)be_at(b.d + p, 8);
        p += 8;
    }
    if (r.flags & SDB_FLAG_HAS_CREATE_TS) {
        r.cts = (int64_t)be_at(b.d + p, 8);
        p += 8;
    }
    return 0;
}
SDB_DEV int v2_row(const Blk &b, uint32_t pos, Row &r) {  // SstRowCodecV2::decode (row_codec_v2.rs:172-220)
    const V2Hdr h = v2_hdr(b, pos, ~0u);
    if (!h.ok || (uint64_t)h.suf + h.un + h.vl + 9 > b.data_end) return SDB_CORRUPT_BLOCK;
    r.sh = h.sh;
    r.un = h.un;
    r.vl = h.vl;
    r.suf = h.suf;
    r.vpos = r.suf + r.un;
    pos = r.vpos + r.vl;
    if (int st = row_tail(b, pos, r)) return st;
    r.next = pos;
    return 0;
}
// decode_first_key_at_restart (block_iterator_v2.rs:73-80): key = d[*kp, *kp + *kn), shared == 0
SDB_DEV int v2_restart_key(const Blk &b, uint32_t ri, uint32_t &kp, uint32_t &kn) {
    const V2Hdr h = v2_hdr(b, boff(b, ri), 0);  // an offset past the data has no first varint
    if (!h.ok) return SDB_CORRUPT_BLOCK;
    kp = h.suf;
    kn = h.un;
    return 0;
}
SDB_DEV uint32_t region_end(const Blk &b, uint32_t ri) { return ri + 1 < b.count ? boff(b, ri + 1) : b.data_end; }

struct Pos {
    bool ok;         // positioned
    uint32_t at;     // V2: byte offset of the entry; V1: its index
    Cmp key;         // the entry's key against the target
};

// binary_search_restarts (block_iterator_v2.rs:138-154)
SDB_DEV int v2_bsearch(const Blk &b, const uint8_t *t, uint32_t nt, uint32_t &low) {
    uint32_t lo = 0, hi = b.count;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        uint32_t kp, kn;
        if (int st = v2_restart_key(b, mid, kp, kn)) return st;
        if (cmp_bytes(b.d + kp, kn, t, nt, 0).c < 0) lo = mid + 1;
        else hi = mid;
    }
    low = lo;
    return 0;
}

// BlockIteratorV2::seek ascending (block_iterator_v2.rs:157-176, 269-313)
SDB_DEV int v2_seek_asc(const Blk &b, const uint8_t *t, uint32_t nt, Pos &P) {
    P.ok = false;
    if (b.count == 0) return 0;
    uint32_t low;
    if (int st = v2_bsearch(b, t, nt, low)) return st;
    for (uint32_t ri = low ? low - 1 : 0; ri < b.count; ri++) {  // find_restart_for_key_ascending
        uint32_t kp, kn;
        if (int st = v2_restart_key(b, ri, kp, kn)) return st;
        uint32_t off = boff(b, ri);
        const Cmp rk = cmp_bytes(b.d + kp, kn, t, nt, 0);  // seek_to_restart
        if (off >= b.data_end) return 0;                   // exhausted
        if (rk.c >= 0) {
            P.ok = true;
            P.at = off;
            P.key = rk;
            return 0;
        }
        const uint32_t rend = region_end(b, ri);
        Cmp prev = rk;
        while (off < rend && off < b.data_end) {
            const V2Hdr h = v2_hdr(b, off, prev.len);  // decode_key_at_offset (:115-126)
            if (!h.ok) return SDB_CORRUPT_BLOCK;
            const Cmp cur = cmp_next(prev, h.sh, b.d + h.suf, h.un, t, nt);
            if (cur.c >= 0) {
                P.ok = true;
                P.at = off;
                P.key = cur;
                return 0;
            }
            Row r;  // advance_past_current_entry
            if (int st = v2_row(b, off, r)) return st;
            off = r.next;
            prev = cur;
        }
    }
    return 0;
}

// DescendingBlockIteratorV2::seek (block_iterator_v2.rs:178-208, 430-469)
SDB_DEV int v2_seek_desc(const Blk &b, const uint8_t *t, uint32_t nt, Pos &P) {
    P.ok = false;
    if (b.count == 0) return 0;
    uint32_t low;
    if (int st = v2_bsearch(b, t, nt, low)) return st;
    uint32_t start = low ? low - 1 : 0;
    if (low < b.count) {  // find_restart_for_key_descending
        uint32_t kp, kn;
        if (int st = v2_restart_key(b, low, kp, kn)) return st;
        if (cmp_bytes(b.d + kp, kn, t, nt, 0).c == 0) {
            uint32_t last = low;
            while (last + 1 < b.count) {
                if (int st = v2_restart_key(b, last + 1, kp, kn)) return st;
                if (cmp_bytes(b.d + kp, kn, t, nt, 0).c != 0) break;
                last++;
            }
            start = last;
        }
    }
    for (uint32_t ri = start + 1; ri-- > 0;) {
        uint32_t kp, kn;
        if (int st = v2_restart_key(b, ri, kp, kn)) return st;
        Cmp cur{0, 0, kn};
        cur = cmp_bytes(b.d + kp, kn, t, nt, 0);
        uint32_t off = boff(b, ri);
        const uint32_t rend = region_end(b, ri);
        bool have = false;
        while (off < rend && off < b.data_end) {  // load_restart_region (:375-394)
            Row r;
            if (int st = v2_row(b, off, r)) return st;
            if (r.sh > cur.len) return SDB_CORRUPT_BLOCK;
            cur = cmp_next(cur, r.sh, b.d + r.suf, r.un, t, nt);
            if (cur.c > 0) break;  // the last entry before the first key > target
            have = true;
            P.at = off;
            P.key = cur;
            off = r.next;
        }
        if (have) {
            P.ok = true;
            return 0;
        }
    }
    return 0;
}

// V1 key i = first_key[..prefix] ++ suffix (decode_key_at_index, block_iterator.rs:249-265)
SDB_DEV int v1_cmp(const Blk &b, uint32_t i, const uint8_t *t, uint32_t nt, Cmp &c) {
    if (b.data_end < 4 || be_at(b.d, 2) != 0) return SDB_CORRUPT_BLOCK;  // decode_first_key
    const uint32_t fk = (uint32_t)be_at(b.d + 2, 2);
    if (4 + fk > b.data_end) return SDB_CORRUPT_BLOCK;
    const uint32_t p = boff(b, i);
    if (p + 4 > b.data_end) return SDB_CORRUPT_BLOCK;
    const uint32_t pre = (uint32_t)be_at(b.d + p, 2), sl = (uint32_t)be_at(b.d + p + 2, 2);
    if (pre > fk || p + 4 + sl > b.data_end) return SDB_CORRUPT_BLOCK;
    Cmp f = cmp_bytes(b.d + 4, pre, t, nt, 0);  // the prefix part
    if (f.m < pre) {
        f.len = pre + sl;
        c = f;
        return 0;
    }
    c = cmp_bytes(b.d + p + 4, sl, t, nt, pre);
    return 0;
}
// SstRowCodecV0::decode of entry i (row.rs:200-249): key = first_key[..r.sh] ++ d[r.suf, r.suf + r.un);
// the flags as the iterator returns them (a V0 tombstone drops expire_ts, row.rs:223-231)
SDB_DEV int v1_row(const Blk &b, uint32_t i, Row &r) {
    if (b.data_end < 4 || be_at(b.d, 2) != 0) return SDB_CORRUPT_BLOCK;
    const uint32_t fk = (uint32_t)be_at(b.d + 2, 2);
    uint32_t p = boff(b, i);
    if (4 + fk > b.data_end || p + 4 > b.data_end) return SDB_CORRUPT_BLOCK;
    r.sh = (uint32_t)be_at(b.d + p, 2);
    r.un = (uint32_t)be_at(b.d + p + 2, 2);
    p += 4;
    if ((uint64_t)p + r.un + 9 > b.data_end) return SDB_CORRUPT_BLOCK;
    r.suf = p;
    p += r.un;
    if (int st = row_tail(b, p, r)) return st;
    r.vl = 0;
    r.vpos = 0;
    if (r.flags & SDB_FLAG_TOMBSTONE) {
        r.flags = (uint8_t)(r.flags & ~SDB_FLAG_HAS_EXPIRE_TS);
    } else {
        if ((uint64_t)p + 4 > b.data_end) return SDB_CORRUPT_BLOCK;
        r.vl = (uint32_t)be_at(b.d + p, 4);
        p += 4;
        if ((uint64_t)p + r.vl > b.data_end) return SDB_CORRUPT_BLOCK;
        r.vpos = p;
        p += r.vl;
    }
    // restore_full_key slices first_key[..prefix] after the decode returned the row: a bad flags byte or a value
    // past the data is reported before an over-long prefix, as sdb_decode_blocks reports them
    if (r.sh > fk) return SDB_CORRUPT_BLOCK;
    r.next = p;
    return 0;
}

// BlockIterator::seek (block_iterator.rs:130-190)
SDB_DEV int v1_seek(const Blk &b, const uint8_t *t, uint32_t nt, bool desc, Pos &P) {
    P.ok = false;
    uint32_t lo = 0, hi = b.count;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        Cmp c;
        if (int st = v1_cmp(b, mid, t, nt, c)) return st;
        if (desc ? c.c <= 0 : c.c < 0) lo = mid + 1;
        else hi = mid;
    }
    if (!desc && lo < b.count) {
        P.ok = true;
        P.at = lo;
    }
    if (desc && lo > 0) {
        P.ok = true;
        P.at = lo - 1;
    }
    if (P.ok) return v1_cmp(b, P.at, t, nt, P.key);
    return 0;
}

// partition_point (partitioned_keyspace.rs:16-39); le: first_key <= key, else first_key < key
SDB_DEV uint64_t partition_point(const sdb_sst_view &v, const uint8_t *t, uint32_t nt, bool le) {
    const uint64_t n = v.num_blocks;
    if (n == 0) return 0;
    uint64_t lo = 0, hi = n - 1, pp = 0;
    while (lo <= hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const uint64_t f0 = v.index_key_off[mid], f1 = v.index_key_off[mid + 1];
        const int c = cmp_bytes(v.index_keys + f0, (uint32_t)(f1 - f0), t, nt, 0).c;
        if (le ? c <= 0 : c < 0) {
            lo = mid + 1;
            pp = mid + 1;
        } else if (mid > lo) {
            hi = mid - 1;
        } else {
            break;
        }
    }
    return pp;
}
// partitions_covering_range(Included(key), Included(key)) (partitioned_keyspace.rs:87-110): the blocks
// [start, end) that can hold the key; end == start: none.
SDB_DEV void point_block_range(const sdb_sst_view &v, const uint8_t *t, uint32_t nt, uint32_t &start, uint32_t &end) {
    const uint64_t lt = partition_point(v, t, nt, false), le = partition_point(v, t, nt, true);
    start = (uint32_t)(lt > 0 ? lt - 1 : 0);
    end = (uint32_t)(le > 0 ? le : start);
}

// A fresh block iterator on entry 0 of a block with count > 0 (BlockIteratorV2::new, block_iterator_v2.rs:33-57:
// byte 0 under restart 0's key; BlockIterator::new, V1: index 0).  !P.ok: the block holds no entry.
SDB_DEV int first_entry(bool v2, const Blk &b, const uint8_t *t, uint32_t nt, Pos &P) {
    P.at = 0;
    P.ok = !v2 || b.data_end > 0;
    if (!v2) return v1_cmp(b, 0, t, nt, P.key);
    uint32_t kp, kn;
    if (int st = v2_restart_key(b, 0, kp, kn)) return st;
    P.key = cmp_bytes(b.d + kp, kn, t, nt, 0);
    return 0;
}
// The entry after the one at P, whose row is r, with its key's order carried over from P's.  !P.ok: r was the
// block's last.
SDB_DEV int next_entry(bool v2, const Blk &b, const Row &r, const uint8_t *t, uint32_t nt, Pos &P) {
    if (!v2) {
        P.ok = ++P.at < b.count;
        return P.ok ? v1_cmp(b, P.at, t, nt, P.key) : 0;
    }
    P.ok = r.next < b.data_end;
    if (!P.ok) return 0;
    const V2Hdr h = v2_hdr(b, r.next, P.key.len);
    if (!h.ok) return SDB_CORRUPT_BLOCK;
    P.at = r.next;  // before the key, as the V1 branch: with the key first the optimiser keeps P in scratch memory
    P.key = cmp_next(P.key, h.sh, b.d + h.suf, h.un, t, nt);
    return 0;
}

// Every row of a checked block parsed, in physical order: visit(row index, byte position, row).  The status is
// what a full parse reports: the restart-0 key of a V2 block with restarts, shared <= the previous key's length,
// and every v2_row / v1_row status; the rows before a failing one have been visited.
template <typename F>
SDB_DEV int for_each_row(uint32_t version, const Blk &b, F &&visit) {
    int st = 0;
    if (version == 2) {
        uint32_t kp, kn, curlen = 0, pos = 0;
        if (b.count > 0) st = v2_restart_key(b, 0, kp, kn);  // decode_first_key_at_restart(0)
        for (uint32_t i = 0; !st && pos < b.data_end; i++) {
            Row r;
            if ((st = v2_row(b, pos, r))) break;
            if (r.sh > curlen) {
                st = SDB_CORRUPT_BLOCK;
                break;
            }
            visit(i, pos, r);
            curlen = r.sh + r.un;
            pos = r.next;
        }
    } else {
        // BlockIterator::new reads the first key of every block, one without entries included
        if (b.data_end < 4 || be_at(b.d, 2) != 0 || 4 + (uint32_t)be_at(b.d + 2, 2) > b.data_end) st = SDB_CORRUPT_BLOCK;
        for (uint32_t i = 0; !st && i < b.count; i++) {
            Row r;
            if ((st = v1_row(b, i, r))) break;
            visit(i, boff(b, i), r);
        }
    }
    return st;
}

// The status of a block for_each_row failed on (or found irregular) as descending iteration reports it: the first
// error in that order.  V2 (DescendingBlockIteratorV2, block_iterator_v2.rs:318-428): new() decodes restart 0's key,
// then the regions go last to first, each decoded ascending from its restart, so the highest failing region
// decides and inside it its first failing row; a region that does not start at its restart with shared == 0 and
// end on the next one fails with SDB_CORRUPT_BLOCK (the descending decode's rule).  V1 (BlockIterator Descending,
// block_iterator.rs:218-227): the first key, then the highest failing entry.  0: the block is sound.
SDB_DEV int desc_status(uint32_t version, const Blk &b) {
    if (version != 2) {
        if (b.data_end < 4 || be_at(b.d, 2) != 0 || 4 + (uint32_t)be_at(b.d + 2, 2) > b.data_end) return SDB_CORRUPT_BLOCK;
        for (uint32_t i = b.count; i-- > 0;) {
            Row r;
            if (int st = v1_row(b, i, r)) return st;
        }
        return 0;
    }
    if (b.count == 0) return 0;
    uint32_t kp, kn;
    if (v2_restart_key(b, 0, kp, kn)) return SDB_CORRUPT_BLOCK;
    for (uint32_t ri = b.count; ri-- > 0;) {
        if (v2_restart_key(b, ri, kp, kn)) return SDB_CORRUPT_BLOCK;  // seek_to_restart
        uint32_t pos = boff(b, ri), curlen = 0;
        const uint32_t end = region_end(b, ri);
        if (end <= pos || end > b.data_end || (ri == 0 && pos != 0)) return SDB_CORRUPT_BLOCK;
        while (pos < end) {
            Row r;
            if (int st = v2_row(b, pos, r)) return st;
            if (r.sh > curlen) return SDB_CORRUPT_BLOCK;  // (0 at the restart)
            curlen = r.sh + r.un;
            pos = r.next;
        }
        if (pos != end) return SDB_CORRUPT_BLOCK;
    }
    return 0;
}

// A row's value reference, seq, flags and timestamps into slot i of an out struct (sdb_lookup_out, sdb_scan_out,
// sdb_get_out).  A value offset is relative to the SST data (base = the block's); an empty value has offset 0; a
// tombstone has no value (a V2 row still carries a length); a timestamp shows only under its flag.
template <typename Out>
SDB_DEV void put_row(const Out &o, uint64_t i, uint64_t base, const Row &r) {
    const uint32_t vl = (r.flags & SDB_FLAG_TOMBSTONE) ? 0 : r.vl;
    o.val_off[i] = vl ? base + r.vpos : 0;
    o.val_len[i] = vl;
    o.seq[i] = r.seq;
    o.flags[i] = r.flags;
    o.create_ts[i] = (r.flags & SDB_FLAG_HAS_CREATE_TS) ? r.cts : 0;
    o.expire_ts[i] = (r.flags & SDB_FLAG_HAS_EXPIRE_TS) ? r.ets : 0;
}

// Block::decode bounds + CRC of the block data[s, e) by one wave (lane l), over the wave's LDS image
// (kLkImg bytes, 64 zeroed bytes before it): the body of k_check.
constexpr uint32_t kLkThreads = 256;
constexpr uint32_t kLkImg = 4096 + 32;
constexpr uint32_t kLkLds = kCrcTablesLds + (kLkThreads / 64) * (kLkImg + 64);
SDB_DEV lu8 *lk_wave_image(uint8_t *smem, uint32_t wave, uint32_t l) {
    lu8 *img = (lu8 *)smem + kCrcTablesLds + wave * (kLkImg + 64) + 64;
    if (l < 16) ((lu32 *)(img - 64))[l] = 0;  // zero lead-in of the right-aligned CRC segments
    return img;
}
SDB_DEV int lk_check_block(const uint8_t *data, uint64_t s, uint64_t e, lu8 *img, uint32_t l) {
    if (e < s || e - s < 6) return SDB_CORRUPT_BLOCK;
    const uint32_t blen = (uint32_t)(e - s - 4);
    uint32_t crc;
    if (blen + 16 <= 4096 && blen >= 4) {
        const uint32_t p0 = (uint32_t)(s & 15), Lc = p0 + blen;
        const uint64_t a0 = s & ~15ull;
        const uint32_t ng = (uint32_t)((((s + blen + 15) & ~15ull) - a0) >> 4);
        for (uint32_t g = l; g < ng; g += 64) {
            const uint4 v = ((const uint4 *)(data + a0))[g];
            u32x4 w;
            w.x = v.x;
            w.y = v.y;
            w.z = v.z;
            w.w = v.w;
            ((lu128 *)img)[g] = w;
        }
        __builtin_amdgcn_wave_barrier();
        if (l < p0) img[l] = 0;
        if (l < 4) img[p0 + l] ^= 0xFF;  // crc32fast's init
        __builtin_amdgcn_wave_barrier();
        crc = wave_crc_image_ra(img, Lc);
        __builtin_amdgcn_wave_barrier();
    } else {  // large blocks: one lane, byte-wise
        uint32_t x = 0xFFFFFFFFu;
        if (l == 0)
            for (uint32_t i = 0; i < blen; i++) x = c_crc.t[0][(x ^ data[s + i]) & 0xFF] ^ (x >> 8);
        crc = (uint32_t)__builtin_amdgcn_readfirstlane((int)(x ^ 0xFFFFFFFFu));
    }
    return crc != (uint32_t)be_at(data + s + blen, 4) ? SDB_CHECKSUM_MISMATCH : 0;
}

// The SST of tree block k: the last i with block_base[i] <= k.
SDB_DEV uint32_t sst_of_block(const sdb_lsm_view &t, uint64_t k) {
    uint32_t lo = 0, hi = t.num_ssts;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (t.block_base[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The consistency of a tree's index arrays, by one workgroup (every thread calls it): block_base against the views'
// num_blocks and total_blocks, run_start monotone from 0 to num_ssts, first / last key offsets that do not
// descend; sstat[i] = 0, SDB_INVALID_VERSION or SDB_INVALID_ARGUMENT (blocks and a NULL array) of SST i.
// -> nonzero in every thread: the tree is malformed and nothing may be read through its arrays.
SDB_DEV int lsm_validate(const sdb_lsm_view &t, int32_t *sstat) {
    const uint32_t ns = t.num_ssts, nr = t.num_runs;
    int bad = 0;
    for (uint32_t i = threadIdx.x; i < ns; i += blockDim.x) {
        const sdb_sst_view v = t.ssts[i];
        const uint64_t b0 = t.block_base[i], b1 = t.block_base[i + 1];
        if (b1 < b0 || b1 - b0 != v.num_blocks || v.num_blocks >= 0xFFFFFFFFull || b1 > t.total_blocks) bad = 1;
        if (i == 0 && b0 != 0) bad = 1;
        if (i == ns - 1 && b1 != t.total_blocks) bad = 1;
        if (t.first_key_off[i + 1] < t.first_key_off[i] || t.last_key_off[i + 1] < t.last_key_off[i]) bad = 1;
        int st = 0;
        if (v.sst_version != 1 && v.sst_version != 2) st = SDB_INVALID_VERSION;
        else if (v.num_blocks && (!v.data || !v.block_off || !v.index_keys || !v.index_key_off)) st = SDB_INVALID_ARGUMENT;
        sstat[i] = st;
    }
    for (uint32_t r = threadIdx.x; r < nr; r += blockDim.x) {
        const uint32_t r0 = t.run_start[r], r1 = t.run_start[r + 1];
        if (r1 < r0 || r1 > ns) bad = 1;
        if (r == 0 && r0 != 0) bad = 1;
        if (r == nr - 1 && r1 != ns) bad = 1;
    }
    return __syncthreads_or(bad);
}

// The block-check pass k_check (sdb_lookup.hip), one wave per marked block: Block::decode bounds + CRC -> bstat;
// clears the marks.  The blocks are those of one SST (bad == nullptr: v), or of a tree's SSTs end to end (t, block
// k at t.block_base[sst] + block; nothing is read through t when *bad).
struct CheckArgs {
    sdb_sst_view v;
    sdb_lsm_view t;
    const uint32_t *bad;
    uint64_t num_blocks;
    uint8_t *mark;
    int32_t *bstat;
};
hipError_t launch_check(const CheckArgs &a, hipStream_t st);

}  // namespace sdb
