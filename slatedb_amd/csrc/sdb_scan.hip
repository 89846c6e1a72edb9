// sdb_scan.hip — batched range scans on one encoded SST for gfx950.
//
// Replaces an SstIterator built over a BytesRange (SstView, sst_iter.rs:64-121), drained:
//   blocks      partitions_covering_range(index, start, end)            partitioned_keyspace.rs:87-110,
//                                                                        sst_iter.rs:548-552
//   entries     every entry of those blocks with SstView::contains(key)  sst_iter.rs:97-121, 655-673
//   order       ascending: physical; descending: keys descend, the versions of one key stay newest
//               first (fill_descending_buffer re-reverses each key group)  sst_iter.rs:567-651
//   checksum    every block of the block range is CRC-checked            format/sst.rs:1029-1038
//
// What depends only on the block is computed once per block and shared by every range that touches it;
// what depends on the range is two clipped blocks (its first and its last).  No per-(range, block) state is
// stored, so the workspace is O(blocks + ranges) however much the ranges overlap.  The bounds, the block range,
// the clip of a block and the restored key are those of sdb_range.h, shared with sdb_lsm_scan.hip:
//   k_sc_locate  thread per range: block range (covering_blocks), empty-set test
//   k_sc_mark    workgroup per range: marks the blocks it reads
//   k_check      wave per marked block: bounds + CRC (sdb_lookup.hip, shared)
//   k_sc_block   thread per read block: every row parsed (for_each_row of sdb_read.h: the status), entries,
//                restored-key bytes, the runs of equal keys at its head and tail, and whether its last key
//                equals the next block's first
//   scans        entries / key bytes / failed / read over blocks
//   k_sc_edge    thread per range: status (lowest_failure), the clips [lo, hi) of its first and last block
//                (clip_block: the incremental comparators, keys are not materialised), totals
//   scans        entries / key bytes / items / failed over ranges -> range_entry_start
//   k_sc_final   summary, capacity check
//   k_sc_emit    thread per work item (range, block), found by binary search in the item scan (last_le):
//                restores keys (restore_key) and writes rows [lo, hi).
//                Descending: entry p of the range's N, in the key group [gs, ge), lands at
//                N - ge + (p - gs); a group's extent past the item's block comes from the per-block
//                head / tail runs and joins, never from a pass over the output.
#include "sdb_range.h"
#include "sdb_decode.h"

namespace sdb {

struct ScanArgs {
    sdb_sst_view v;
    sdb_scan_ranges r;
    sdb_scan_out out;
    uint32_t desc, pad;
    // per block
    uint8_t *mark;                    // 1 = some range reads it (cleared by k_check)
    int32_t *bstat;                   // -1 = not read, else the block's sdb_status
    uint64_t *cnt, *kb, *bad, *rd;    // entries, restored-key bytes, failed, read
    uint64_t *pc, *pk, *pb, *pr;      // their exclusive scans (num_blocks + 1)
    uint32_t *head, *tail;            // entries equal to the block's first / last key at its head / tail
    uint8_t *join;                    // the block's last key == the next block's first key
    // per range
    uint8_t *rempty;                  // the range is empty as a set
    uint32_t *lo_f;                   // first block: first row in range
    uint32_t *efb, *elb;              // the first and last block that keep a row
    uint64_t *nf, *kbf, *nl, *kbl;    // first / last block: rows in range, their key bytes
    uint64_t *rn, *rkb, *ritems, *rfail;
    uint64_t *rks, *ris, *rfs;        // exclusive scans (n + 1); rn scans into out.range_entry_start
    uint64_t *tx, *ty;                // scan tiles
    unsigned long long *firstbad;     // range << 8 | status of the lowest failing range
    uint32_t *go;                     // 1 = the outputs fit: emit runs
};

// Block::decode of block k.  A V2 block without restarts yields nothing descending (the existing
// descending decode's rule, block_iterator_v2.rs:318-430).
SDB_DEV int sc_open(const ScanArgs &a, uint64_t k, Blk &b) {
    if (int st = blk_open(a.v, k, b)) return st;
    if (a.v.sst_version == 2 && a.desc && b.count == 0) b.data_end = 0;
    return 0;
}

__global__ __launch_bounds__(256) void k_sc_locate(ScanArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.r.n) return;
    const Bound s = range_start(a.r, r), e = range_end(a.r, r);
    if (bad_kind(s, e)) {  // reported by k_sc_edge
        a.out.range_block[2 * r] = a.out.range_block[2 * r + 1] = 0;
        a.rempty[r] = 2;
        return;
    }
    const BlockRange g = covering_blocks(a.v, s, e);
    a.out.range_block[2 * r] = (uint32_t)g.start;
    a.out.range_block[2 * r + 1] = (uint32_t)g.end;
    a.rempty[r] = empty_as_set(s, e) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_sc_mark(ScanArgs a) {
    for (uint64_t r = blockIdx.x; r < a.r.n; r += gridDim.x) {
        if (a.rempty[r]) continue;
        const uint64_t start = a.out.range_block[2 * r], end = a.out.range_block[2 * r + 1];
        for (uint64_t b = start + threadIdx.x; b < end; b += blockDim.x) a.mark[b] = 1;
    }
}

// Row i of an open block: V2 at byte `pos` (the walk's cursor), V1 by its offset.
SDB_DEV int sc_row(const ScanArgs &a, const Blk &b, uint32_t i, uint32_t pos, Row &r) {
    return a.v.sst_version == 2 ? v2_row(b, pos, r) : v1_row(b, i, r);
}
// V1: row x has the key of row p; a key is first_key[..sh] ++ suffix (row 0 holds the first key as its suffix).
SDB_DEV bool sc_same(const ScanArgs &a, const Blk &b, const Row &x, const Row &p, uint32_t L) {
    if (x.sh + x.un != p.sh + p.un) return false;
    const uint32_t lo = x.sh < p.sh ? x.sh : p.sh;  // both are the first key below lo
    for (uint32_t j = lo; j < x.sh + x.un; j++) {
        const uint8_t cx = j < x.sh ? b.d[4 + j] : b.d[x.suf + j - x.sh], cp = j < p.sh ? b.d[4 + j] : b.d[p.suf + j - p.sh];
        if (cx != cp) return false;
    }
    return true;
}

// V2: what a walk keeps of the key of the last row it took, to tell whether the next row repeats it.  A
// repeat inside a restart region is shared == len, unshared == 0; at a restart the key comes again in
// full (shared == 0), so its bytes are compared: K[ls_sh, len) is the suffix at ls_suf, and what lies
// before ls_sh is compared by the incremental comparator from the last row that holds its key in full.
struct KeyTrack {
    uint32_t len, ls_sh, ls_un, ls_suf, f_pos;
    bool any;
};
SDB_DEV void kt_take(KeyTrack &T, const Row &r, uint32_t pos) {
    if (r.un > 0) {
        T.ls_sh = r.sh;
        T.ls_un = r.un;
        T.ls_suf = r.suf;
    } else if (r.sh < T.ls_sh) {
        T.ls_sh = r.sh;
        T.ls_un = 0;
    } else {
        T.ls_un = r.sh - T.ls_sh;
    }
    if (r.sh == 0) T.f_pos = pos;
    T.len = r.sh + r.un;
    T.any = true;
}
SDB_DEV bool sc_bytes_eq(const uint8_t *x, const uint8_t *y, uint32_t n) {
    for (uint32_t j = 0; j < n; j++)
        if (x[j] != y[j]) return false;
    return true;
}
// Row r at byte pos has the tracked key.  (0 < shared < ls_sh with unshared > 0 is taken as a new key:
// prefix compression shares all it can, so such a row differs at its first unshared byte.)
SDB_DEV bool kt_same(const Blk &b, const KeyTrack &T, const Row &r, uint32_t pos) {
    if (!T.any || r.sh + r.un != T.len) return false;
    if (r.un == 0) return true;
    if (r.sh >= T.ls_sh) return sc_bytes_eq(b.d + r.suf, b.d + T.ls_suf + (r.sh - T.ls_sh), r.un);
    if (r.sh != 0 || !sc_bytes_eq(b.d + r.suf + T.ls_sh, b.d + T.ls_suf, T.ls_un)) return false;
    const uint8_t *t = b.d + r.suf;  // r's key in full: compare the tracked key's chain with it
    Cmp c{0, 0, 0};
    for (uint32_t p = T.f_pos; p < pos;) {
        Row q;
        if (v2_row(b, p, q)) return false;
        c = p == T.f_pos ? cmp_bytes(b.d + q.suf, q.un, t, r.un, 0) : cmp_next(c, q.sh, b.d + q.suf, q.un, t, r.un);
        p = q.next;
    }
    return c.c == 0;
}

// The first key of block k as bytes in place (a V2 restart row / the V1 first_key); false: none.
SDB_DEV bool sc_first_key(const ScanArgs &a, uint64_t k, const uint8_t *&t, uint32_t &nt) {
    Blk b;
    if (sc_open(a, k, b)) return false;
    if (a.v.sst_version == 2) {
        const V2Hdr h = v2_hdr(b, 0, 0);  // an empty block has no first varint
        if (!h.ok) return false;
        t = b.d + h.suf;
        nt = h.un;
        return true;
    }
    if (b.count == 0 || b.data_end < 4) return false;
    nt = (uint32_t)be_at(b.d + 2, 2);
    if (4 + nt > b.data_end) return false;
    t = b.d + 4;
    return true;
}

__global__ __launch_bounds__(256) void k_sc_block(ScanArgs a) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.v.num_blocks) return;
    int st = a.bstat[k];
    uint64_t cnt = 0, kb = 0;
    uint32_t head = 0, tail = 0;
    bool join = false;
    const bool read = st != -1;
    Blk b;
    if (read && st == 0) st = sc_open(a, k, b);
    if (read && st == 0) {
        const uint8_t *t = nullptr;
        uint32_t nt = 0;
        // the runs of equal keys and the join with the next block place key groups: descending only
        const bool have_t = a.desc && k + 1 < a.v.num_blocks && sc_first_key(a, k + 1, t, nt);
        auto count = [&](uint32_t i, const Row &r, bool same) {  // same: row i repeats the key of row i - 1
            tail = same ? tail + 1 : 1;
            if (same && head == i) head++;
            if (i == 0) head = 1;
            cnt = i + 1;
            kb += r.sh + r.un;
        };
        Cmp c{0, 0, 0};
        if (a.v.sst_version == 2) {
            uint32_t ri = 0;
            bool regular = b.count == 0 || boff(b, 0) == 0;
            KeyTrack T{};
            st = for_each_row(2, b, [&](uint32_t i, uint32_t pos, const Row &r) {
                if (ri < b.count && boff(b, ri) == pos) {  // regions start at restarts with shared == 0, in order
                    if (r.sh != 0) regular = false;
                    ri++;
                } else if (ri < b.count && boff(b, ri) < pos) {
                    regular = false;
                }
                const bool same = a.desc && kt_same(b, T, r, pos);
                if (a.desc) kt_take(T, r, pos);
                count(i, r, same);
                if (have_t) c = i == 0 ? cmp_bytes(b.d + r.suf, r.un, t, nt, 0) : cmp_next(c, r.sh, b.d + r.suf, r.un, t, nt);
            });
            // the descending decode's rule and its order of errors: the first one descending iteration meets
            if (a.desc && b.count && (st || ri != b.count || !regular)) {
                const int ds = desc_status(2, b);
                st = ds ? ds : SDB_CORRUPT_BLOCK;
            }
            join = have_t && cnt > 0 && c.c == 0;
        } else {
            Row p{};
            st = for_each_row(1, b, [&](uint32_t i, uint32_t, const Row &r) {
                count(i, r, a.desc && i > 0 && sc_same(a, b, r, p, 0));
                p = r;
            });
            if (st && a.desc) st = desc_status(1, b);  // descending: the highest failing entry decides
            if (!st && have_t && cnt > 0) join = v1_cmp(b, b.count - 1, t, nt, c) == 0 && c.c == 0;
        }
    }
    if (st > 0) cnt = kb = head = tail = 0;
    a.bstat[k] = st;
    a.cnt[k] = cnt;
    a.kb[k] = kb;
    a.bad[k] = read && st != 0;
    a.rd[k] = read;
    a.head[k] = head;
    a.tail[k] = tail;
    a.join[k] = join && st == 0;
}

// clip_block of block k.  With both sides open there is nothing to clip: the block pass walked the same rows.
SDB_DEV Clip sc_clip(const ScanArgs &a, uint64_t k, const Bound &s, const Bound &e) {
    if (!s.kind && !e.kind) return Clip{0, (uint32_t)a.cnt[k], 0, a.kb[k]};
    Blk b;
    if (sc_open(a, k, b)) return Clip{0, 0, 0, 0};
    return clip_block(a.v.sst_version, b, s, e);
}

__global__ __launch_bounds__(256) void k_sc_edge(ScanArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.r.n) return;
    const uint64_t start = a.out.range_block[2 * r], end = a.out.range_block[2 * r + 1];
    uint64_t items = !a.rempty[r] && end > start ? end - start : 0, fb = 0, lb = 0;
    int st = a.rempty[r] == 2 ? SDB_INVALID_ARGUMENT : 0;
    uint64_t n = 0, kb = 0, nf = 0, kbf = 0, nl = 0, kbl = 0;
    uint32_t lo = 0;
    if (items && !(st = lowest_failure(a.pb, a.bstat, 0, start, end))) {
        // Interior blocks hold only keys of the range, except where a bound's key fills whole blocks (a
        // long run of versions under an excluded bound): the first and last block move inwards past
        // blocks that keep nothing, so [fb, lb] starts and ends with a kept row.
        const Bound s = range_start(a.r, r), e = range_end(a.r, r), open{nullptr, 0, 0};
        Clip f, l{0, 0, 0, 0};
        fb = start;
        lb = end - 1;
        for (;; fb++) {
            f = sc_clip(a, fb, s, fb == lb ? e : open);
            if (f.hi > f.lo || fb == lb) break;
        }
        for (; lb > fb; lb--) {
            l = sc_clip(a, lb, open, e);
            if (l.hi > 0) break;
        }
        if (lb == fb && fb != end - 1) f = sc_clip(a, fb, s, e);  // the last block came down to the first
        lo = f.lo;
        n = nf = f.hi - f.lo;
        kb = kbf = f.kb;
        if (lb > fb) {
            nl = l.hi;
            kbl = l.kb;
            n += nl + (a.pc[lb] - a.pc[fb + 1]);
            kb += kbl + (a.pk[lb] - a.pk[fb + 1]);
        }
        items = n ? lb - fb + 1 : 0;
    }
    a.out.range_status[r] = st;
    if (st) atomicMin(a.firstbad, (unsigned long long)(r << 8 | (uint64_t)st));
    a.lo_f[r] = lo;
    a.efb[r] = (uint32_t)fb;
    a.elb[r] = (uint32_t)lb;
    a.nf[r] = nf;
    a.kbf[r] = kbf;
    a.nl[r] = nl;
    a.kbl[r] = kbl;
    a.rn[r] = n;
    a.rkb[r] = kb;
    a.ritems[r] = st ? 0 : items;
    a.rfail[r] = st != 0;
}

__global__ void k_sc_init(ScanArgs a) {
    if (threadIdx.x == 0) {
        *a.firstbad = ~0ull;
        *a.go = 0;
    }
}

__global__ void k_sc_final(ScanArgs a) {
    if (threadIdx.x != 0) return;
    const uint64_t n = a.r.n;
    sdb_scan_summary s{};
    s.num_entries = a.out.range_entry_start[n];
    s.key_bytes = a.rks[n];
    s.num_failed_ranges = a.rfs[n];
    s.blocks_read = a.pr[a.v.num_blocks];
    s.status = *a.firstbad == ~0ull ? 0 : (int32_t)(*a.firstbad & 0xFF);
    const bool fits = s.num_entries <= a.out.cap_entries && s.key_bytes <= a.out.key_arena_cap;
    if (!fits) s.status = SDB_LIMIT_EXCEEDED;
    else a.out.key_off[s.num_entries] = s.key_bytes;
    *a.out.summary = s;
    *a.go = fits ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_sc_emit(ScanArgs a) {
    if (!*a.go) return;
    const uint64_t nr = a.r.n, total = a.ris[nr];
    for (uint64_t it = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = last_le(a.ris, nr, 1, it), start = a.efb[r], end = (uint64_t)a.elb[r] + 1;  // the blocks that keep rows
        const uint64_t k = start + (it - a.ris[r]);
        const uint64_t E0 = a.out.range_entry_start[r], N = a.out.range_entry_start[r + 1] - E0;
        const uint64_t K0 = a.rks[r], KB = a.rks[r + 1] - K0;
        const uint64_t nf = a.nf[r], nl = a.nl[r];
        const bool first = k == start, last = k == end - 1;
        const uint32_t lo = first ? a.lo_f[r] : 0;
        const uint32_t hi = first ? lo + (uint32_t)nf : (last ? (uint32_t)nl : (uint32_t)a.cnt[k]);
        if (hi <= lo) continue;
        const uint64_t eb = first ? 0 : nf + (a.pc[k] - a.pc[start + 1]);   // the item's first entry in the range
        const uint64_t kbb = first ? 0 : a.kbf[r] + (a.pk[k] - a.pk[start + 1]);
        // descending: how far the item's first / last key group reaches into the blocks before / after
        uint64_t ci = 0, co = 0;
        if (a.desc) {
            for (uint64_t j = k; j > start && lo == 0 && a.join[j - 1];) {
                j--;
                const uint64_t nj = j == start ? nf : a.cnt[j], tj = a.tail[j] < nj ? a.tail[j] : nj;
                ci += tj;
                if (tj < nj || nj == 0) break;
            }
            for (uint64_t j = k; j + 1 < end && hi == a.cnt[k] && a.join[j];) {
                j++;
                const uint64_t nj = j == end - 1 ? nl : a.cnt[j], hj = a.head[j] < nj ? a.head[j] : nj;
                co += hj;
                if (hj < nj || nj == 0) break;
            }
        }
        Blk b;
        if (sc_open(a, k, b)) continue;
        const bool v2 = a.v.sst_version == 2;
        uint32_t i = 0, pos = 0;
        KeyTrack T{};
        for (; v2 && i < lo; i++) {  // V2: the byte position of row lo
            Row q;
            if (v2_row(b, pos, q)) break;
            if (a.desc) kt_take(T, q, pos);
            pos = q.next;
        }
        if (i < lo && v2) continue;
        i = lo;
        const uint8_t *prevkey = nullptr;  // the previous row's restored key (V2 chains from it)
        uint64_t kcur = 0;
        while (i < hi) {
            Row lead;
            if (sc_row(a, b, i, pos, lead)) break;
            const uint32_t L = lead.sh + lead.un;
            uint32_t g = 1, p2 = lead.next;  // the run of rows with this key inside the item
            if (v2 && a.desc) kt_take(T, lead, pos);
            while (a.desc && i + g < hi) {  // ascending needs no groups: every row is placed by its index
                Row q;
                if (sc_row(a, b, i + g, p2, q) || !(v2 ? kt_same(b, T, q, p2) : sc_same(a, b, q, lead, L))) break;
                if (v2) kt_take(T, q, p2);
                g++;
                p2 = q.next;
            }
            const uint64_t P = eb + (i - lo);
            const uint64_t gs = P - (i == lo ? ci : 0), ge = P + g + (i + g == hi ? co : 0);
            const uint8_t *leadkey = nullptr;
            uint32_t mp = pos;
            for (uint32_t m = 0; m < g; m++) {
                Row q = lead;
                if (m && sc_row(a, b, i + m, mp, q)) break;
                mp = q.next;
                const uint64_t Pm = P + m, ko = kbb + kcur + (uint64_t)m * L;
                uint64_t di = Pm, dk = ko;
                if (a.desc) {
                    di = N - ge + (Pm - gs);
                    dk = KB - (ko + (ge - Pm) * L) + (Pm - gs) * L;
                }
                if (di >= N || dk > KB || L > KB - dk) continue;  // rows that are not sorted: never out of the range's slots
                uint8_t *dst = a.out.key_arena + K0 + dk;
                if (leadkey) {
                    copy_bytes(dst, leadkey, L);
                } else {
                    restore_key(v2, b, i, lead, prevkey, dst);
                    leadkey = dst;
                }
                a.out.key_off[E0 + di] = K0 + dk;
                put_row(a.out, E0 + di, b.base, q);
            }
            prevkey = leadkey;
            kcur += (uint64_t)g * L;
            i += g;
            pos = p2;
        }
    }
}

// The workspace arrays of a scan of a.r.n ranges over a.v.num_blocks blocks, bound into a from w; -> their size.
static uint64_t scan_bind(ScanArgs &a, uint8_t *w) {
    const uint64_t nb = a.v.num_blocks, n = a.r.n, nt = ((nb > n ? nb : n) + 1023) / 1024 + 2;  // nt: scan tiles
    Carver c{w, 0};
    c.take(a.mark, nb + 1);
    c.take(a.bstat, nb + 1);
    c.take(a.cnt, nb + 1);
    c.take(a.kb, nb + 1);
    c.take(a.bad, nb + 1);
    c.take(a.rd, nb + 1);
    c.take(a.pc, nb + 2);
    c.take(a.pk, nb + 2);
    c.take(a.pb, nb + 2);
    c.take(a.pr, nb + 2);
    c.take(a.head, nb + 1);
    c.take(a.tail, nb + 1);
    c.take(a.join, nb + 1);
    c.take(a.rempty, n + 1);
    c.take(a.lo_f, n + 1);
    c.take(a.efb, n + 1);
    c.take(a.elb, n + 1);
    c.take(a.nf, n + 1);
    c.take(a.kbf, n + 1);
    c.take(a.nl, n + 1);
    c.take(a.kbl, n + 1);
    c.take(a.rn, n + 1);
    c.take(a.rkb, n + 1);
    c.take(a.ritems, n + 1);
    c.take(a.rfail, n + 1);
    c.take(a.rks, n + 2);
    c.take(a.ris, n + 2);
    c.take(a.rfs, n + 2);
    c.take(a.tx, nt);
    c.take(a.ty, nt);
    c.take(a.firstbad, 8);  // 64 bytes: the word, then go
    if (w) a.go = (uint32_t *)(a.firstbad + 1);
    return c.off;
}

uint64_t scan_workspace_bytes(uint64_t num_blocks, uint64_t nranges) {
    ScanArgs a{};
    a.v.num_blocks = num_blocks;
    a.r.n = nranges;
    return scan_bind(a, nullptr);
}

hipError_t launch_scan(const sdb_sst_view &v, const sdb_scan_ranges &r, uint32_t desc, const sdb_scan_out &out, uint8_t *w,
                       hipStream_t st) {
    const uint64_t nb = v.num_blocks, n = r.n;
    ScanArgs a{};
    a.v = v;
    a.r = r;
    a.out = out;
    a.desc = desc;
    scan_bind(a, w);
    hipError_t e;
    if (n == 0 || nb == 0) {  // every range is empty
        if ((e = hipMemsetAsync(out.summary, 0, sizeof(sdb_scan_summary), st)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(out.range_entry_start, 0, 8 * (n + 1), st)) != hipSuccess) return e;
        if (n && (e = hipMemsetAsync(out.range_block, 0, 8 * n, st)) != hipSuccess) return e;
        if (n && (e = hipMemsetAsync(out.range_status, 0, 4 * n, st)) != hipSuccess) return e;
        if (out.key_off) e = hipMemsetAsync(out.key_off, 0, 8, st);
        return e;
    }
    if ((e = hipMemsetAsync(a.mark, 0, nb, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.bstat, 0xFF, 4 * nb, st)) != hipSuccess) return e;
    // the per-block and per-item walks are latency-bound threads: one wave per workgroup spreads them over the CUs
    const uint32_t rb = (uint32_t)((n + 255) / 256), rw = (uint32_t)((n + 63) / 64), bw = (uint32_t)((nb + 63) / 64);
    hipLaunchKernelGGL(k_sc_init, dim3(1), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_sc_locate, dim3(rb), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_sc_mark, dim3((uint32_t)(n < 4096 ? n : 4096)), dim3(256), 0, st, a);
    if ((e = launch_check(CheckArgs{v, {}, nullptr, nb, a.mark, a.bstat}, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_sc_block, dim3(bw), dim3(64), 0, st, a);
    if ((e = launch_excl_scan2(a.cnt, a.kb, nb, a.tx, a.ty, a.pc, a.pk, st)) != hipSuccess) return e;
    if ((e = launch_excl_scan2(a.bad, a.rd, nb, a.tx, a.ty, a.pb, a.pr, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_sc_edge, dim3(rw), dim3(64), 0, st, a);
    if ((e = launch_excl_scan2(a.rn, a.rkb, n, a.tx, a.ty, out.range_entry_start, a.rks, st)) != hipSuccess) return e;
    if ((e = launch_excl_scan2(a.ritems, a.rfail, n, a.tx, a.ty, a.ris, a.rfs, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_sc_final, dim3(1), dim3(64), 0, st, a);
    const uint32_t eg = n > (1ull << 40) / nb ? 32768 : scan_grid(n * nb, 64);  // n * nb: upper bound of the work items
    hipLaunchKernelGGL(k_sc_emit, dim3(eg), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace sdb
