// sdb_mem.h — a device memtable as the tree reads see it, shared by the get (sdb_get.hip, sdb_lsm_get_mem) and the
// scan (sdb_lsm_scan.hip, sdb_lsm_scan_mem): a table is a sorted run in the sdb_run layout, key ascending, seq
// descending (mem_table.rs:38-44).  As sdb_read.h: everything takes what it reads, never a kernel's argument struct.
#pragma once
#include "sdb_read.h"

namespace sdb {

struct Key {
    const uint8_t *t;
    uint32_t nt;
};

// M9 / S9: a table with rows needs its columns, and fewer than 2^31 rows; else the call is malformed and nothing may
// be read through the tables.
SDB_DEV int tab_malformed(const sdb_run T) {
    int bad = 0;
    if (T.n >= (1ull << 31)) bad = 1;
    if (T.n && (!T.key_arena || !T.key_off || !T.val_off || !T.val_len || !T.seq || !T.flags)) bad = 1;
    return bad;
}

// Row i of a memtable as the walks see an SST row: vl, seq, flags and the timestamps; the value starts at vbase.
SDB_DEV Row tab_row(const sdb_run &T, uint64_t i, uint64_t &vbase) {
    Row r{};
    const uint8_t no = (uint8_t)((T.create_ts ? 0 : SDB_FLAG_HAS_CREATE_TS) | (T.expire_ts ? 0 : SDB_FLAG_HAS_EXPIRE_TS));
    r.flags = (uint8_t)(T.flags[i] & ~no);
    r.seq = T.seq[i];
    r.vl = T.val_len[i];
    r.cts = T.create_ts ? T.create_ts[i] : 0;
    r.ets = T.expire_ts ? T.expire_ts[i] : 0;
    vbase = T.val_off[i];
    return r;
}

SDB_DEV int tab_cmp(const sdb_run &T, uint64_t i, const Key &k) {  // sign(key of row i cmp k)
    const uint64_t o = T.key_off[i];
    return cmp_bytes(T.key_arena + o, (uint32_t)(T.key_off[i + 1] - o), k.t, k.nt, 0).c;
}
// The first row that does not precede (k, bound) in the table's order: key > k, or key == k and seq <= bound.
SDB_DEV uint64_t tab_seek(const sdb_run &T, const Key &k, uint64_t bound) {
    uint64_t lo = 0, hi = T.n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const int c = tab_cmp(T, mid, k);
        if (c < 0 || (c == 0 && T.seq[mid] > bound)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace sdb
