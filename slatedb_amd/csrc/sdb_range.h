// sdb_range.h — the one reader of a key range, shared by the range scans (sdb_scan.hip) and the tree scans
// (sdb_lsm_scan.hip): a range's bounds and BytesRange::contains, partitions_covering_range, the lowest failing
// block of a block range, the clip of a checked block against two bounds, the restored key of a row, and the
// search and the byte copy that place it.  As sdb_read.h: everything takes what it reads (an sdb_scan_ranges, an
// sdb_sst_view, a Blk, a Bound), never a kernel's argument struct.
#pragma once
#include "sdb_read.h"

namespace sdb {

struct Bound {
    const uint8_t *t;
    uint32_t n, kind;  // kind 0 (SDB_BOUND_UNBOUNDED): that side is open
};
SDB_DEV Bound range_start(const sdb_scan_ranges &g, uint64_t r) {
    return Bound{g.start_bytes + g.start_off[r], (uint32_t)(g.start_off[r + 1] - g.start_off[r]), g.start_kind[r]};
}
SDB_DEV Bound range_end(const sdb_scan_ranges &g, uint64_t r) {
    return Bound{g.end_bytes + g.end_off[r], (uint32_t)(g.end_off[r + 1] - g.end_off[r]), g.end_kind[r]};
}
// key_precedes / key_exceeds (BytesRange::contains, sst_iter.rs:104-120) from sign(key cmp bound)
SDB_DEV bool precedes(const Bound &s, int c) { return s.kind == SDB_BOUND_INCLUDED ? c < 0 : (s.kind == SDB_BOUND_EXCLUDED && c <= 0); }
SDB_DEV bool exceeds(const Bound &e, int c) { return e.kind == SDB_BOUND_INCLUDED ? c > 0 : (e.kind == SDB_BOUND_EXCLUDED && c >= 0); }
SDB_DEV bool bad_kind(const Bound &s, const Bound &e) { return s.kind > SDB_BOUND_EXCLUDED || e.kind > SDB_BOUND_EXCLUDED; }
// No key lies between the bounds: start after end, or equal with a side excluded.
SDB_DEV bool empty_as_set(const Bound &s, const Bound &e) {
    if (!s.kind || !e.kind) return false;
    const int c = cmp_bytes(s.t, s.n, e.t, e.n, 0).c;
    return c > 0 || (c == 0 && (s.kind == SDB_BOUND_EXCLUDED || e.kind == SDB_BOUND_EXCLUDED));
}
// BytesRange::intersect (comparable_range.rs:224-236) a bound at a time: the tighter of two start bounds (Unbounded <
// Included(a) < Excluded(a)) and the tighter of two end bounds (Excluded(a) < Included(a) < Unbounded).  The
// intersection is empty exactly when empty_as_set of the two results says so (non_empty, :265-274).
// (a bound is picked field by field: a pick between two structs goes through scratch memory)
SDB_DEV Bound pick_bound(bool first, const Bound &x, const Bound &y) {
    return Bound{first ? x.t : y.t, first ? x.n : y.n, first ? x.kind : y.kind};
}
SDB_DEV Bound tighter_start(const Bound &x, const Bound &y) {
    bool first = x.kind != 0;
    if (x.kind && y.kind) {
        const int c = cmp_bytes(x.t, x.n, y.t, y.n, 0).c;
        first = c > 0 || (c == 0 && x.kind == SDB_BOUND_EXCLUDED);
    }
    return pick_bound(first, x, y);
}
SDB_DEV Bound tighter_end(const Bound &x, const Bound &y) {
    bool first = x.kind != 0;
    if (x.kind && y.kind) {
        const int c = cmp_bytes(x.t, x.n, y.t, y.n, 0).c;
        first = c < 0 || (c == 0 && x.kind == SDB_BOUND_EXCLUDED);
    }
    return pick_bound(first, x, y);
}
// Included(k)..=Included(k): SstView::point_key (sst_iter.rs:82-87)
SDB_DEV bool is_point(const Bound &s, const Bound &e) {
    return s.kind == SDB_BOUND_INCLUDED && e.kind == SDB_BOUND_INCLUDED && s.n == e.n && cmp_bytes(s.t, s.n, e.t, e.n, 0).c == 0;
}
// Projection i (SsTableView.visible_range) of an sdb_scan_ranges is malformed: a start other than Unbounded or Included
// (new_projected's assert, db_state.rs:126-130), an end that is no std::ops::Bound, or offsets that descend.
SDB_DEV bool bad_projection(const sdb_scan_ranges &g, uint64_t i) {
    return g.start_kind[i] > SDB_BOUND_INCLUDED || g.end_kind[i] > SDB_BOUND_EXCLUDED || g.start_off[i + 1] < g.start_off[i] ||
           g.end_off[i + 1] < g.end_off[i];
}

// partitions_covering_range(index, start, end) (partitioned_keyspace.rs:87-110) over v's index keys: the blocks
// [start, end), as the reference returns them: end may be below start.
struct BlockRange {
    uint64_t start, end;
};
SDB_DEV BlockRange covering_blocks(const sdb_sst_view &v, const Bound &s, const Bound &e) {
    BlockRange g{0, v.num_blocks};
    if (s.kind) {  // first_partition_including_or_after_key (:43-68)
        const uint64_t lt = partition_point(v, s.t, s.n, false);
        g.start = lt > 0 ? lt - 1 : 0;
    }
    if (e.kind) {  // last_partition_including_key (:72-83), then :98-106
        const uint64_t le = partition_point(v, e.t, e.n, true);
        if (le == 0) {
            g.end = g.start;
        } else if (e.kind == SDB_BOUND_INCLUDED) {
            g.end = le;
        } else {  // an excluded end that equals block p's index key leaves p out
            const uint64_t p = le - 1, f0 = v.index_key_off[p], f1 = v.index_key_off[p + 1];
            g.end = cmp_bytes(v.index_keys + f0, (uint32_t)(f1 - f0), e.t, e.n, 0).c == 0 ? p : p + 1;
        }
    }
    return g;
}

// The status of the lowest failing block of [bs, be), bs < be, whose blocks stand at base + block in the
// exclusive scan pb of the failed-block flags and in bstat; 0: none fails.
SDB_DEV int lowest_failure(const uint64_t *pb, const int32_t *bstat, uint64_t base, uint64_t bs, uint64_t be) {
    if (pb[base + be] == pb[base + bs]) return 0;
    uint64_t x = bs, y = be - 1;
    while (x < y) {
        const uint64_t m = x + (y - x) / 2;
        if (pb[base + m + 1] > pb[base + bs]) y = m;
        else x = m + 1;
    }
    return bstat[base + x];
}

// The rows of a checked block in physical order until visit(row index, row) returns false (for_each_row of
// sdb_read.h visits every row and reports the parse status; this walk may stop, and ends at a row that does not
// parse).
template <typename F>
SDB_DEV void walk_rows(bool v2, const Blk &b, F &&visit) {
    if (v2) {
        uint32_t pos = 0;
        for (uint32_t i = 0; pos < b.data_end; i++) {
            Row r;
            if (v2_row(b, pos, r) || !visit(i, r)) break;
            pos = r.next;
        }
    } else {
        for (uint32_t i = 0; i < b.count; i++) {
            Row r;
            if (v1_row(b, i, r) || !visit(i, r)) break;
        }
    }
}
// The rows [lo, hi) of a checked block that lie between two bounds, by the incremental comparators (no key is
// materialised): lo = the first row that does not precede s, hi = the first row from lo on that exceeds e (the
// walk stops there), each the block's row count where there is none; kb_before / kb = the restored-key bytes of
// the rows before lo / of [lo, hi).
struct Clip {
    uint32_t lo, hi;
    uint64_t kb_before, kb;
};
SDB_DEV Clip clip_block(uint32_t version, const Blk &b, const Bound &s, const Bound &e) {
    const bool v2 = version == 2;
    uint32_t lo = 0, hi = 0;
    uint64_t kbb = 0, kb = 0;
    bool in = false;
    Cmp cs{0, 0, 0}, ce{0, 0, 0};
    walk_rows(v2, b, [&](uint32_t i, const Row &r) {
        if (v2) {
            if (s.kind) cs = i == 0 ? cmp_bytes(b.d + r.suf, r.un, s.t, s.n, 0) : cmp_next(cs, r.sh, b.d + r.suf, r.un, s.t, s.n);
            if (e.kind) ce = i == 0 ? cmp_bytes(b.d + r.suf, r.un, e.t, e.n, 0) : cmp_next(ce, r.sh, b.d + r.suf, r.un, e.t, e.n);
        } else {
            if (s.kind && v1_cmp(b, i, s.t, s.n, cs)) return false;
            if (e.kind && v1_cmp(b, i, e.t, e.n, ce)) return false;
        }
        if (!in && !precedes(s, cs.c)) {
            in = true;
            lo = i;
        }
        if (in && exceeds(e, ce.c)) return false;
        kb += in ? r.sh + r.un : 0;  // two sums: one sum into either of them by a branch goes through scratch memory
        kbb += in ? 0 : r.sh + r.un;
        hi = i + 1;
        return true;
    });
    return Clip{in ? lo : hi, hi, kbb, kb};
}

SDB_DEV void copy_bytes(uint8_t *dst, const uint8_t *src, uint32_t n) {  // dst after src when they overlap: never
    typedef uint64_t u64u __attribute__((aligned(1)));
    uint32_t j = 0;
    for (; j + 8 <= n; j += 8) *(u64u *)(dst + j) = *(const u64u *)(src + j);
    for (; j < n; j++) dst[j] = src[j];
}

// The key of row x (r) of block b, its r.sh + r.un bytes written at dst.  V1: first_key[..sh] ++ suffix.  V2:
// prev[..sh] ++ suffix with prev the restored key of row x - 1, or, without it, by chaining from the block's
// first row: row y sets key[y.sh, y.sh + y.un).
SDB_DEV void restore_key(bool v2, const Blk &b, uint32_t x, const Row &r, const uint8_t *prev, uint8_t *dst) {
    if (!v2) {
        copy_bytes(dst, b.d + 4, r.sh);
    } else if (prev) {
        copy_bytes(dst, prev, r.sh);
    } else if (r.sh) {
        uint32_t rp = 0;
        for (uint32_t y = 0; y < x; y++) {
            Row q;
            if (v2_row(b, rp, q)) break;
            for (uint32_t j = q.sh; j < q.sh + q.un && j < r.sh; j++) dst[j] = b.d[q.suf + j - q.sh];
            rp = q.next;
        }
    }
    copy_bytes(dst + r.sh, b.d + r.suf, r.un);
}

// The last x in [0, n) with s[x * stride] <= v (s ascends, s[0] <= v).
SDB_DEV uint64_t last_le(const uint64_t *s, uint64_t n, uint64_t stride, uint64_t v) {
    uint64_t x = 0, y = n;
    while (y - x > 1) {
        const uint64_t m = x + (y - x) / 2;
        if (s[m * stride] <= v) x = m;
        else y = m;
    }
    return x;
}

// Workgroups of `threads` for `items` work items, at least one; the kernels stride past the cap.
static uint32_t scan_grid(uint64_t items, uint32_t threads) {
    const uint64_t g = (items + threads - 1) / threads;
    return (uint32_t)(g > 32768 ? 32768 : (g < 1 ? 1 : g));
}

}  // namespace sdb
