// sdb_lookup.h — device helpers shared by the point lookups (sdb_lookup.hip) and the range scans
// (sdb_scan.hip): the incremental key comparators, Block::decode of a checked block, the row parsers
// and the index partition_point.
#pragma once
#include "sdb_bloom.h"
#include "sdb_crc.h"
#include "sdb_device.h"

namespace sdb {

struct LookupArgs {
    sdb_sst_view v;
    const uint8_t *key_bytes;
    const uint64_t *key_off;
    uint64_t nkeys;
    uint32_t desc;
    sdb_lookup_out out;
    uint32_t *qrange;     // per query: start, end (block range; end == start: empty)
    uint8_t *mark;        // per block: 1 = a seek reads it
    int32_t *bstat;       // per block: sdb_status of Block::decode + CRC
};

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
SDB_DEV int blk_open(const LookupArgs &a, uint64_t k, Blk &b) {
    const uint64_t s = a.v.block_off[k], e = a.v.block_off[k + 1];
    if (e < s || e - s < 6) return SDB_CORRUPT_BLOCK;
    const uint32_t blen = (uint32_t)(e - s - 4);
    b.d = a.v.data + s;
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
SDB_DEV int v2_row(const Blk &b, uint32_t pos, Row &r) {  // SstRowCodecV2::decode (row_codec_v2.rs:172-220)
    if (!rdv(b.d, b.data_end, pos, r.sh) || !rdv(b.d, b.data_end, pos, r.un) || !rdv(b.d, b.data_end, pos, r.vl))
        return SDB_CORRUPT_BLOCK;
    if ((uint64_t)pos + r.un + r.vl + 9 > b.data_end) return SDB_CORRUPT_BLOCK;
    r.suf = pos;
    pos += r.un;
    r.vpos = pos;
    pos += r.vl;
    r.seq = be_at(b.d + pos, 8);
    pos += 8;
    r.flags = b.d[pos++];
    if (!flags_valid(r.flags)) return SDB_INVALID_ROW_FLAGS;
    const uint32_t need = ((r.flags & SDB_FLAG_HAS_EXPIRE_TS) ? 8 : 0) + ((r.flags & SDB_FLAG_HAS_CREATE_TS) ? 8 : 0);
    if ((uint64_t)pos + need > b.data_end) return SDB_CORRUPT_BLOCK;
    r.ets = r.cts = 0;
    if (r.flags & SDB_FLAG_HAS_EXPIRE_TS) {
        r.ets = (int64_t)be_at(b.d + pos, 8);
        pos += 8;
    }
    if (r.flags & SDB_FLAG_HAS_CREATE_TS) {
        r.cts = (int64_t)be_at(b.d + pos, 8);
        pos += 8;
    }
    r.next = pos;
    return 0;
}
// decode_first_key_at_restart (block_iterator_v2.rs:73-80): key = d[*kp, *kp + *kn), shared == 0
SDB_DEV int v2_restart_key(const Blk &b, uint32_t ri, uint32_t &kp, uint32_t &kn) {
    uint32_t p = boff(b, ri), sh, un, vl;
    if (p > b.data_end || !rdv(b.d, b.data_end, p, sh) || !rdv(b.d, b.data_end, p, un) || !rdv(b.d, b.data_end, p, vl) ||
        sh != 0 || (uint64_t)p + un > b.data_end)
        return SDB_CORRUPT_BLOCK;
    kp = p;
    kn = un;
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
            uint32_t p = off, sh, un, vl;  // decode_key_at_offset (:115-126)
            if (!rdv(b.d, b.data_end, p, sh) || !rdv(b.d, b.data_end, p, un) || !rdv(b.d, b.data_end, p, vl) ||
                sh > prev.len || (uint64_t)p + un > b.data_end)
                return SDB_CORRUPT_BLOCK;
            const Cmp cur = cmp_next(prev, sh, b.d + p, un, t, nt);
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
    if (r.sh > fk || (uint64_t)p + r.un + 9 > b.data_end) return SDB_CORRUPT_BLOCK;
    r.suf = p;
    p += r.un;
    r.seq = be_at(b.d + p, 8);
    p += 8;
    uint8_t f = b.d[p++];
    if (!flags_valid(f)) return SDB_INVALID_ROW_FLAGS;
    const uint32_t need = ((f & SDB_FLAG_HAS_EXPIRE_TS) ? 8 : 0) + ((f & SDB_FLAG_HAS_CREATE_TS) ? 8 : 0);
    if ((uint64_t)p + need > b.data_end) return SDB_CORRUPT_BLOCK;
    r.ets = r.cts = 0;
    if (f & SDB_FLAG_HAS_EXPIRE_TS) {
        r.ets = (int64_t)be_at(b.d + p, 8);
        p += 8;
    }
    if (f & SDB_FLAG_HAS_CREATE_TS) {
        r.cts = (int64_t)be_at(b.d + p, 8);
        p += 8;
    }
    r.vl = 0;
    r.vpos = 0;
    if (f & SDB_FLAG_TOMBSTONE) {
        f = (uint8_t)(f & ~SDB_FLAG_HAS_EXPIRE_TS);
    } else {
        if ((uint64_t)p + 4 > b.data_end) return SDB_CORRUPT_BLOCK;
        r.vl = (uint32_t)be_at(b.d + p, 4);
        p += 4;
        if ((uint64_t)p + r.vl > b.data_end) return SDB_CORRUPT_BLOCK;
        r.vpos = p;
        p += r.vl;
    }
    r.flags = f;
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
SDB_DEV uint64_t partition_point(const LookupArgs &a, const uint8_t *t, uint32_t nt, bool le) {
    const uint64_t n = a.v.num_blocks;
    if (n == 0) return 0;
    uint64_t lo = 0, hi = n - 1, pp = 0;
    while (lo <= hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const uint64_t f0 = a.v.index_key_off[mid], f1 = a.v.index_key_off[mid + 1];
        const int c = cmp_bytes(a.v.index_keys + f0, (uint32_t)(f1 - f0), t, nt, 0).c;
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

// might_contain (filter.rs:124-136) for the filter hash h; an empty bitmap answers false.
SDB_DEV bool bloom_might_contain(const uint8_t *bloom, uint64_t bloom_len, uint32_t num_probes, uint64_t h) {
    const uint32_t m = (uint32_t)(bloom_len * 8);
    if (!m) return false;
    uint32_t hh = (uint32_t)h % m, d = (uint32_t)(h >> 32) % m;
    for (uint32_t i = 0; i < num_probes; i++) {
        d = (uint32_t)(((uint64_t)d + i) % m);
        if (!((bloom[hh >> 3] >> (hh & 7)) & 1)) return false;
        hh = (uint32_t)(((uint64_t)hh + d) % m);
    }
    return true;
}

// Block::decode bounds + CRC of the block data[s, e) by one wave (lane l), over the wave's LDS image
// (kLkImg bytes, 64 zeroed bytes before it): the body of k_lk_check and of the multi-SST k_get_check.
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

// One wave per marked block: Block::decode bounds + CRC -> bstat; clears the marks (sdb_lookup.hip).
hipError_t launch_lk_check(LookupArgs a, hipStream_t st);

}  // namespace sdb
