// sdb_replay.hip — WAL replay on the device: decoded rows in arrival order -> the replayed memtables as
// sorted runs (include/slatedb_amd.h, "WAL replay / device memtable"; rules W1-W7).
//
// sdb_wal_replay_sort
//   k_rp_init       one workgroup: batch_start runs from 0 to n; the per-batch accumulators, err and L0 reset
//   k_rp_facts      per row (arrival order): its batch, keep or skip (W1), min / max seq of all rows and of the
//                   kept rows, max create_ts per batch (batch_acc: wave reductions, one atomic per word and
//                   workgroup inside a batch); L0 = min over rows of lcp(key, row 0's key)
//   k_rp_order      one wave: W2 over the batches (running max of the earlier non-empty batches)
//   k_rp_tile_sort  per kReplayTile rows: 8-byte prefixes behind L0, (prefix, seq, row) records in LDS, a
//                   bitonic network; the order is kept rows first, key asc, seq desc, arrival desc
//   k_rp_merge      log2(tiles) passes: one workgroup per kReplayTile outputs finds its two merge-path splits
//                   by diagonal searches, loads both segments' records to LDS and ranks every element in the
//                   other segment; only the 4-byte permutation moves
//   k_rp_mark       per sorted position: an equal (key, seq) predecessor arrived later -> replaced (W4)
//   k_rp_count      per row (arrival order): rows / bytes / replaced per batch (W5)
//   k_rp_finish     one workgroup: the facts, the summary, the survivors before each batch
// sdb_wal_replay_emit
//   k_rp_tables     one workgroup: table_batch_start runs from 0 to nbatches; each batch's table, each table's
//                   first output row; capacities; the summary
//   k_rp_tcount, k_rp_tscan, k_rp_tscatter   a stable partition of the sorted survivors by table,
//                   kReplayBuckets tables per pass: per workgroup and table counts, their scan over the
//                   workgroups, the scatter -> output row -> input row
//   k_rp_sizes, k_rp_escan   key / value bytes per kReplayBlock output rows, their exclusive offsets
//   k_rp_gather     per kReplayBlock output rows: the columns, then key and value bytes by the merge emit's
//                   wave copies (sdb_copy.h: eight lanes per row, 16 bytes per lane and step)
//
// Every kernel after k_rp_init returns at once when err is set, so nothing is read through a bad batch_start.
// The work is integer and byte movement; the sort's passes gather 16 bytes per row through the permutation.
#include <hip/hip_runtime.h>

#include "sdb_copy.h"
#include "sdb_device.h"
#include "sdb_replay.h"

namespace sdb {

namespace {

constexpr unsigned long long kNoErr = ~0ull;

SDB_DEV uint64_t wave_max64(uint64_t v) {
    return wave_readlane(wave_incl_scan_op(v, [](uint64_t x, uint64_t y) { return x > y ? x : y; }), 63);
}

// A workgroup's rows into words [F0, F0 + N) of their batches' accumulators (sums when ADD, else maxima).  A wave
// whose rows share a batch reduces first; its result goes through LDS, where thread f joins word f of the
// neighbouring waves with the same batch: a workgroup inside one batch issues one atomic per word.  The lanes of
// a wave that straddles batches issue their own.  A maximum that would not raise the word is not sent (the word
// only grows, so a stale read is a low one).
constexpr uint32_t kBlockWaves = kReplayBlock / 64;
SDB_DEV void acc_send(unsigned long long *word, uint64_t v, bool add) {
    if (!v) return;
    if (add) atomicAdd(word, (unsigned long long)v);
    else if (v > *(volatile unsigned long long *)word) atomicMax(word, (unsigned long long)v);
}
template <int F0, int N, bool ADD>
SDB_DEV void batch_acc(const ReplayArgs &a, uint32_t b, bool valid, const uint64_t (&v)[N], uint64_t (*s_v)[N], uint32_t *s_b) {
    const uint32_t w = threadIdx.x >> 6, lane = lane_id();
    const uint32_t b0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);  // (valid lanes are a prefix of the wave)
    const bool uniform = __any(valid) && __all(!valid || b == b0);
    if (uniform) {
#pragma unroll
        for (int f = 0; f < N; f++) {
            const uint64_t r = ADD ? wave_sum(v[f]) : wave_max64(v[f]);
            if (lane == 0) s_v[w][f] = r;
        }
    } else if (valid) {
#pragma unroll
        for (int f = 0; f < N; f++) acc_send((unsigned long long *)(a.acc + b) + F0 + f, v[f], ADD);
    }
    if (lane == 0) s_b[w] = uniform ? b0 : ~0u;
    __syncthreads();
    if (threadIdx.x >= N) return;
    const uint32_t f = threadIdx.x;
    uint32_t cur = ~0u;
    uint64_t sum = 0;
    for (uint32_t q = 0; q <= kBlockWaves; q++) {
        const uint32_t bq = q < kBlockWaves ? s_b[q] : ~0u;
        if (bq != cur || q == kBlockWaves) {
            if (cur != ~0u) acc_send((unsigned long long *)(a.acc + cur) + F0 + f, sum, ADD);
            cur = bq;
            sum = 0;
        }
        if (bq != ~0u) sum = ADD ? sum + s_v[q][f] : (s_v[q][f] > sum ? s_v[q][f] : sum);
    }
}
static_assert(sizeof(ReplayBatchAcc) == 11 * 8, "batch_acc addresses the accumulators as words");

__global__ __launch_bounds__(1024) void k_rp_init(ReplayArgs a) {
    __shared__ unsigned long long s_err;
    if (threadIdx.x == 0) s_err = kNoErr;
    __syncthreads();
    uint64_t *z = (uint64_t *)a.acc;
    for (uint64_t x = threadIdx.x; x < a.nbatches * (sizeof(ReplayBatchAcc) / 8); x += blockDim.x) z[x] = 0;
    for (uint64_t b = threadIdx.x; b <= a.nbatches; b += blockDim.x) {
        const uint64_t v = a.batch_start[b];
        const bool bad = v > a.n || (b == 0 && v != 0) || (b == a.nbatches ? v != a.n : a.batch_start[b + 1] < v);
        if (bad) atomicMin(&s_err, (unsigned long long)((b << 8) | SDB_INVALID_ARGUMENT));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        *a.err = s_err;
        *a.lcp0 = ~0u;
    }
}

__global__ __launch_bounds__(kReplayBlock) void k_rp_facts(ReplayArgs a) {
    if (*a.err != kNoErr) return;
    __shared__ uint64_t s_v[kBlockWaves][6];
    __shared__ uint32_t s_b[kBlockWaves], s_lcp[kBlockWaves];
    const uint64_t g = (uint64_t)blockIdx.x * kReplayBlock + threadIdx.x;
    const bool valid = g < a.n;
    uint32_t b = 0, lcp = ~0u;
    uint64_t seq = 0, cts = 0, any = 0;
    bool keep = false;
    if (valid) {
        uint64_t lo = 0, hi = a.nbatches;  // the last batch that starts at or before g
        while (hi - lo > 1) {
            const uint64_t mid = (lo + hi) >> 1;
            if (a.batch_start[mid] <= g) lo = mid;
            else hi = mid;
        }
        b = (uint32_t)lo;
        a.row_batch[g] = b;
        seq = a.r.seq[g];
        keep = !(a.has_min_seq && seq <= a.min_seq);
        a.state[g] = keep ? 1 : 0;
        const uint8_t f = a.r.flags[g];
        if (keep && (f & SDB_FLAG_HAS_CREATE_TS) && a.r.create_ts) {
            any = 1;
            cts = (uint64_t)a.r.create_ts[g] ^ (1ull << 63);
        }
        const uint64_t k0 = a.r.key_off[g], k1 = a.r.key_off[g + 1];
        lcp = lcp_bytes(a.r.key_arena + a.r.key_off[0], (uint32_t)(a.r.key_off[1] - a.r.key_off[0]), a.r.key_arena + k0,
                        (uint32_t)(k1 - k0));
    }
    lcp = ~wave_max(~lcp);
    if (lane_id() == 0) s_lcp[threadIdx.x >> 6] = lcp;
    const uint64_t v[6] = {valid ? ~seq : 0, seq, keep ? ~seq : 0, keep ? seq : 0, cts, any};  // ReplayBatchAcc's first words
    batch_acc<0, 6, false>(a, b, valid, v, s_v, s_b);  // (synchronises)
    if (threadIdx.x == 6) {
        uint32_t m = ~0u;
        for (uint32_t q = 0; q < kBlockWaves; q++) m = s_lcp[q] < m ? s_lcp[q] : m;
        if (m < *(volatile uint32_t *)a.lcp0) atomicMin(a.lcp0, m);  // (it only shrinks: a stale read is a high one)
    }
}

// W2: the smallest seq of a non-empty batch exceeds the largest seq of every earlier batch.
__global__ __launch_bounds__(64) void k_rp_order(ReplayArgs a) {
    if (*a.err != kNoErr) return;
    uint64_t carry_max = 0, carry_has = 0;
    for (uint64_t base = 0; base < a.nbatches; base += 64) {
        const uint64_t b = base + lane_id();
        const bool in = b < a.nbatches;
        const bool full = in && a.batch_start[b + 1] > a.batch_start[b];
        const uint64_t mx = full ? a.acc[b].all_max : 0, mn = full ? ~a.acc[b].all_min_inv : 0;
        const uint64_t imax = wave_incl_scan_op(mx, [](uint64_t x, uint64_t y) { return x > y ? x : y; });
        const uint64_t ihas = wave_incl_scan_op((uint64_t)full, [](uint64_t x, uint64_t y) { return x | y; });
        uint64_t emax = wave_prev_lane(imax), ehas = wave_prev_lane(ihas) | carry_has;
        emax = emax > carry_max ? emax : carry_max;
        const uint64_t bad = __ballot(full && ehas && mn <= emax);
        if (bad) {
            if (lane_id() == 0) *a.err = ((base + (uint64_t)(__ffsll((long long)bad) - 1)) << 8) | SDB_INVALID_ARGUMENT;
            return;
        }
        const uint64_t tmax = wave_readlane(imax, 63);
        carry_max = tmax > carry_max ? tmax : carry_max;
        carry_has |= wave_readlane(ihas, 63);
    }
}

// ---- the order: kept rows first; key ascending, seq descending, arrival descending (the survivor of an equal
// (key, seq) group comes first); skipped rows and the padding of the last tile behind them by index ----
struct Rec {
    uint64_t pfx, seq;
    uint32_t idx;  // row | kReplaySkip
};
SDB_DEV bool rec_less(const ReplayArgs &a, uint32_t L0, const Rec &x, const Rec &y) {
    const uint32_t sx = x.idx & kReplaySkip, sy = y.idx & kReplaySkip;
    if (sx | sy) return sx == sy ? x.idx < y.idx : sy != 0;
    if (x.pfx != y.pfx) return x.pfx < y.pfx;
    const uint64_t x0 = a.r.key_off[x.idx], x1 = a.r.key_off[x.idx + 1];
    const uint64_t y0 = a.r.key_off[y.idx], y1 = a.r.key_off[y.idx + 1];
    const int c = cmp_key(x.pfx, a.r.key_arena + x0, (uint32_t)(x1 - x0), y.pfx, a.r.key_arena + y0, (uint32_t)(y1 - y0), L0);
    if (c) return c < 0;
    if (x.seq != y.seq) return x.seq > y.seq;
    return x.idx > y.idx;
}
SDB_DEV Rec rec_at(const ReplayArgs &a, const uint32_t *perm, uint64_t p) {
    const uint32_t idx = perm[p], row = idx & ~kReplaySkip;
    return Rec{a.pfx[row], a.r.seq[row], idx};
}

__global__ __launch_bounds__(kReplayThreads) void k_rp_tile_sort(ReplayArgs a) {
    if (*a.err != kNoErr) return;
    __shared__ uint64_t s_pfx[kReplayTile], s_seq[kReplayTile];
    __shared__ uint32_t s_idx[kReplayTile];
    const uint32_t L0 = *a.lcp0, tid = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * kReplayTile;
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
        const uint32_t e = tid + u * kReplayThreads;
        const uint64_t g = base + e;
        uint64_t pf = 0, sq = 0;
        uint32_t idx = ~0u;
        if (g < a.n) {
            const uint64_t k0 = a.r.key_off[g], k1 = a.r.key_off[g + 1];
            pf = key_prefix(a.r.key_arena + k0 + L0, (uint32_t)(k1 - k0) - L0);  // every key has L0 bytes
            a.pfx[g] = pf;
            sq = a.r.seq[g];
            idx = (uint32_t)g | (a.state[g] ? 0u : kReplaySkip);
        }
        s_pfx[e] = pf;
        s_seq[e] = sq;
        s_idx[e] = idx;
    }
    __syncthreads();
    for (uint32_t k = 2; k <= kReplayTile; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), p = i | j;
            const Rec x{s_pfx[i], s_seq[i], s_idx[i]}, y{s_pfx[p], s_seq[p], s_idx[p]};
            const bool up = (i & k) == 0;
            if (up ? rec_less(a, L0, y, x) : rec_less(a, L0, x, y)) {
                s_pfx[i] = y.pfx, s_seq[i] = y.seq, s_idx[i] = y.idx;
                s_pfx[p] = x.pfx, s_seq[p] = x.seq, s_idx[p] = x.idx;
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
        const uint32_t e = tid + u * kReplayThreads;
        if (base + e < a.n) a.perm[0][base + e] = s_idx[e];  // (the padding sorted behind every row)
    }
}

// The rows of A = src[pa, pa + na) among the first d of merge(A, B), B = src[pb, pb + nb).
SDB_DEV uint64_t merge_split(const ReplayArgs &a, uint32_t L0, const uint32_t *src, uint64_t pa, uint64_t na, uint64_t pb,
                             uint64_t nb, uint64_t d) {
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (rec_less(a, L0, rec_at(a, src, pa + mid), rec_at(a, src, pb + d - 1 - mid))) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// One pass: sorted runs of `run` rows merge in pairs; workgroup c writes outputs [c, c + 1) * kReplayTile.
__global__ __launch_bounds__(kReplayThreads) void k_rp_merge(ReplayArgs a, uint64_t run, const uint32_t *src, uint32_t *dst) {
    if (*a.err != kNoErr) return;
    __shared__ uint64_t s_pfx[kReplayTile], s_seq[kReplayTile];
    __shared__ uint32_t s_idx[kReplayTile];
    __shared__ uint64_t s_split[2];
    const uint32_t L0 = *a.lcp0, tid = threadIdx.x;
    const uint64_t o0 = (uint64_t)blockIdx.x * kReplayTile, o1 = o0 + kReplayTile < a.n ? o0 + kReplayTile : a.n;
    const uint64_t pa = o0 / (2 * run) * (2 * run);
    const uint64_t pb = pa + run < a.n ? pa + run : a.n, pe = pa + 2 * run < a.n ? pa + 2 * run : a.n;
    const uint64_t na = pb - pa, nb = pe - pb;
    if (tid == 0) s_split[0] = merge_split(a, L0, src, pa, na, pb, nb, o0 - pa);
    if (tid == 64) s_split[1] = merge_split(a, L0, src, pa, na, pb, nb, o1 - pa);
    __syncthreads();
    const uint64_t i0 = s_split[0], i1 = s_split[1], j0 = (o0 - pa) - i0;
    const uint32_t ca = (uint32_t)(i1 - i0), cn = (uint32_t)(o1 - o0);  // A's share, then B's: cn - ca
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
        const uint32_t e = tid + u * kReplayThreads;
        if (e < cn) {
            const Rec x = rec_at(a, src, e < ca ? pa + i0 + e : pb + j0 + (e - ca));
            s_pfx[e] = x.pfx, s_seq[e] = x.seq, s_idx[e] = x.idx;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < 2; u++) {
        const uint32_t e = tid + u * kReplayThreads;
        if (e >= cn) continue;
        const Rec x{s_pfx[e], s_seq[e], s_idx[e]};
        const bool in_a = e < ca;
        const uint32_t q0 = in_a ? ca : 0;  // the other segment
        uint32_t lo = 0, hi = in_a ? cn - ca : ca;
        while (lo < hi) {  // its elements before x (no two elements are equal)
            const uint32_t mid = (lo + hi) >> 1, q = q0 + mid;
            if (rec_less(a, L0, Rec{s_pfx[q], s_seq[q], s_idx[q]}, x)) lo = mid + 1;
            else hi = mid;
        }
        dst[o0 + (in_a ? e : e - ca) + lo] = x.idx;
    }
}

__global__ __launch_bounds__(kReplayBlock) void k_rp_mark(ReplayArgs a) {
    if (*a.err != kNoErr) return;
    const uint64_t p = (uint64_t)blockIdx.x * kReplayBlock + threadIdx.x;
    if (p == 0 || p >= a.n) return;
    const uint32_t i = a.sorted[p], h = a.sorted[p - 1];
    if ((i | h) & kReplaySkip) return;
    if (a.r.seq[i] != a.r.seq[h] || a.pfx[i] != a.pfx[h]) return;
    const uint64_t x0 = a.r.key_off[i], x1 = a.r.key_off[i + 1], y0 = a.r.key_off[h], y1 = a.r.key_off[h + 1];
    if (cmp_key(0, a.r.key_arena + x0, (uint32_t)(x1 - x0), 0, a.r.key_arena + y0, (uint32_t)(y1 - y0), *a.lcp0) == 0)
        a.state[i] = 2;  // h arrived later (arrival descending) and replaces it
}

SDB_DEV uint32_t row_val_bytes(const ReplayArgs &a, uint32_t row, uint8_t f) {
    return (f & SDB_FLAG_TOMBSTONE) ? 0u : a.r.val_len[row];
}

__global__ __launch_bounds__(kReplayBlock) void k_rp_count(ReplayArgs a) {
    if (*a.err != kNoErr) return;
    __shared__ uint64_t s_v[kBlockWaves][5];
    __shared__ uint32_t s_b[kBlockWaves];
    const uint64_t g = (uint64_t)blockIdx.x * kReplayBlock + threadIdx.x;
    const bool valid = g < a.n;
    uint32_t b = 0;
    uint64_t rows = 0, bytes = 0, rep = 0, kb = 0, vb = 0;
    if (valid) {
        b = a.row_batch[g];
        const uint8_t s = a.state[g];
        if (s == 1) {
            const uint8_t f = a.r.flags[g];
            rows = 1;
            kb = a.r.key_off[g + 1] - a.r.key_off[g];
            vb = row_val_bytes(a, (uint32_t)g, f);
            bytes = kb + vb + 8 + (((f & SDB_FLAG_HAS_CREATE_TS) && a.r.create_ts) ? 8 : 0) +
                    (((f & SDB_FLAG_HAS_EXPIRE_TS) && a.r.expire_ts) ? 8 : 0);
        } else if (s == 2) {
            rep = 1;
        }
    }
    const uint64_t v[5] = {rows, bytes, rep, kb, vb};  // ReplayBatchAcc's last words
    batch_acc<6, 5, true>(a, b, valid, v, s_v, s_b);
}

__global__ __launch_bounds__(kReplayBlock) void k_rp_finish(ReplayArgs a) {
    __shared__ uint64_t s_w[17];
    const unsigned long long e = *a.err;
    sdb_wal_replay_summary *sm = a.summary;
    if (e != kNoErr) {
        if (threadIdx.x) return;
        *sm = sdb_wal_replay_summary{a.n, 0, 0, 0, 0, 0, (int32_t)(e & 0xFF), 0, (uint64_t)(e >> 8)};
        a.word[kRpStatus] = e & 0xFF;
        return;
    }
    uint64_t tot[5] = {0, 0, 0, 0, 0};  // rows, replaced, key bytes, value bytes, rows past W1
    for (uint64_t base = 0; base < a.nbatches; base += kReplayBlock) {
        const uint64_t b = base + threadIdx.x;
        const bool in = b < a.nbatches;
        ReplayBatchAcc A{};
        if (in) {
            A = a.acc[b];
            const bool some = A.rows != 0;
            a.facts[b] = sdb_wal_batch_facts{A.rows, A.bytes, A.replaced, some ? ~A.min_inv : 0, some ? A.max : 0,
                                             A.any ? (int64_t)(A.cts ^ (1ull << 63)) : 0, (uint32_t)A.any, 0};
        }
        const uint64_t v[5] = {A.rows, A.replaced, A.key_bytes, A.val_bytes, A.rows + A.replaced};
#pragma unroll
        for (int f = 0; f < 5; f++) {
            uint64_t t;
            const uint64_t ex = block_excl_scan_u64(v[f], s_w, &t);
            if (f == 0 && in) a.batch_pre[b] = tot[0] + ex;
            tot[f] += t;
        }
    }
    if (threadIdx.x) return;
    a.batch_pre[a.nbatches] = tot[0];
    *sm = sdb_wal_replay_summary{a.n, a.n - tot[4], tot[1], tot[0], tot[2], tot[3], SDB_OK, 0, ~0ull};
    a.word[kRpStatus] = SDB_OK;
    a.word[kRpRowsOut] = tot[0];
    a.word[kRpKeyBytes] = tot[2];
    a.word[kRpValBytes] = tot[3];
    a.word[kRpKept] = tot[4];
    a.word[kRpReplaced] = tot[1];
}

// n == 0 or nbatches == 0: zeroed facts and summary, and the words _emit reads.  With batches, batch_start still
// has to run from 0 to n: every element 0.
__global__ __launch_bounds__(kReplayBlock) void k_rp_zero(ReplayArgs a) {
    __shared__ unsigned long long s_err;
    if (threadIdx.x == 0) s_err = kNoErr;
    __syncthreads();
    if (a.n == 0 && a.nbatches)
        for (uint64_t b = threadIdx.x; b <= a.nbatches; b += blockDim.x)
            if (a.batch_start[b]) atomicMin(&s_err, (unsigned long long)((b << 8) | SDB_INVALID_ARGUMENT));
    __syncthreads();
    const unsigned long long e = s_err;
    if (e == kNoErr)
        for (uint64_t b = threadIdx.x; b < a.nbatches; b += blockDim.x) {
            a.facts[b] = sdb_wal_batch_facts{};
            a.batch_pre[b] = 0;
        }
    if (threadIdx.x) return;
    a.batch_pre[a.nbatches] = 0;
    *a.err = e;
    for (int w = 0; w < kRpWords; w++) a.word[w] = 0;
    a.word[kRpStatus] = e == kNoErr ? (uint64_t)SDB_OK : (e & 0xFF);
    *a.summary = sdb_wal_replay_summary{0, 0, 0, 0, 0, 0, (int32_t)a.word[kRpStatus], 0, e == kNoErr ? ~0ull : (uint64_t)(e >> 8)};
}

// ---- emit ----
__global__ __launch_bounds__(kReplayBlock) void k_rp_tables(ReplayArgs a) {
    __shared__ unsigned long long s_err;
    if (threadIdx.x == 0) s_err = kNoErr;
    __syncthreads();
    const sdb_wal_tables_out &o = a.out;
    int32_t st = (int32_t)a.word[kRpStatus];
    uint64_t first = st ? (uint64_t)(*a.err >> 8) : ~0ull;
    if (!st) {
        for (uint64_t t = threadIdx.x; t <= a.ntables; t += blockDim.x) {
            const uint64_t v = a.table_batch_start[t];
            const bool bad = v > a.nbatches || (t == 0 && v != 0) ||
                             (t == a.ntables ? v != a.nbatches : a.table_batch_start[t + 1] < v);
            if (bad) atomicMin(&s_err, (unsigned long long)t);
        }
        __syncthreads();
        if (s_err != kNoErr) {
            st = SDB_INVALID_ARGUMENT;
            first = s_err;
        } else if (a.word[kRpRowsOut] > o.cap_entries || a.word[kRpKeyBytes] > o.key_cap || a.word[kRpValBytes] > o.val_cap) {
            st = SDB_LIMIT_EXCEEDED;
        }
    }
    if (!st) {
        for (uint64_t t = threadIdx.x; t <= a.ntables; t += blockDim.x) {
            const uint64_t b0 = a.table_batch_start[t];
            const uint64_t pre = a.batch_pre[b0];
            a.table_pre[t] = pre;
            o.table_row_start[t] = pre;
        }
        for (uint64_t b = threadIdx.x; b < a.nbatches; b += blockDim.x) {
            uint64_t lo = 0, hi = a.ntables;  // the last table that starts at or before b
            while (hi - lo > 1) {
                const uint64_t mid = (lo + hi) >> 1;
                if (a.table_batch_start[mid] <= b) lo = mid;
                else hi = mid;
            }
            a.batch_table[b] = (uint32_t)lo;
        }
    }
    if (threadIdx.x) return;
    a.word[kRpEmitStatus] = (uint64_t)st;
    const bool sized = a.word[kRpStatus] == SDB_OK;
    *o.summary = sdb_wal_replay_summary{a.n,
                                        sized ? a.n - a.word[kRpKept] : 0,
                                        sized ? a.word[kRpReplaced] : 0,
                                        sized ? a.word[kRpRowsOut] : 0,
                                        sized ? a.word[kRpKeyBytes] : 0,
                                        sized ? a.word[kRpValBytes] : 0,
                                        st, 0, first};
}

// The table (relative to the pass's first) of sorted position p, or ~0: not a survivor, or another pass's.
SDB_DEV uint32_t pass_bucket(const ReplayArgs &a, uint64_t p, uint32_t t0, uint32_t *row) {
    if (p >= a.word[kRpKept]) return ~0u;
    const uint32_t i = a.sorted[p];  // (kept rows come first: no skip bit)
    *row = i;
    if (a.state[i] != 1) return ~0u;
    const uint32_t t = a.batch_table[a.row_batch[i]] - t0;
    return t < kReplayBuckets ? t : ~0u;
}

__global__ __launch_bounds__(kReplayBlock) void k_rp_tcount(ReplayArgs a, uint32_t t0) {
    if (a.word[kRpEmitStatus] != SDB_OK) return;
    __shared__ uint32_t s_hist[kReplayBuckets];
    if (threadIdx.x < kReplayBuckets) s_hist[threadIdx.x] = 0;
    __syncthreads();
    uint32_t row;
    const uint32_t t = pass_bucket(a, (uint64_t)blockIdx.x * kReplayBlock + threadIdx.x, t0, &row);
    if (t != ~0u) atomicAdd(&s_hist[t], 1u);
    __syncthreads();
    if (threadIdx.x < kReplayBuckets) a.count[(uint64_t)blockIdx.x * kReplayBuckets + threadIdx.x] = s_hist[threadIdx.x];
}

// workgroup b: table t0 + b's counts become exclusive over the workgroups of k_rp_tcount
__global__ __launch_bounds__(kReplayBlock) void k_rp_tscan(ReplayArgs a) {
    if (a.word[kRpEmitStatus] != SDB_OK) return;
    __shared__ uint64_t s_w[17];
    uint64_t carry = 0;
    for (uint32_t base = 0; base < a.nblocks; base += kReplayBlock) {
        const uint32_t k = base + threadIdx.x;
        uint32_t *c = a.count + (uint64_t)k * kReplayBuckets + blockIdx.x;
        uint64_t t;
        const uint64_t ex = block_excl_scan_u64(k < a.nblocks ? *c : 0, s_w, &t);
        if (k < a.nblocks) *c = (uint32_t)(carry + ex);
        carry += t;
    }
}

__global__ __launch_bounds__(kReplayBlock) void k_rp_tscatter(ReplayArgs a, uint32_t t0) {
    if (a.word[kRpEmitStatus] != SDB_OK) return;
    constexpr uint32_t kWaves = kReplayBlock / 64;
    __shared__ uint32_t s_wc[kWaves][kReplayBuckets];
    for (uint32_t x = threadIdx.x; x < kWaves * kReplayBuckets; x += kReplayBlock) (&s_wc[0][0])[x] = 0;
    __syncthreads();
    const uint32_t lane = lane_id(), w = threadIdx.x >> 6;
    uint32_t row = 0;
    const uint32_t t = pass_bucket(a, (uint64_t)blockIdx.x * kReplayBlock + threadIdx.x, t0, &row);
    uint64_t rem = __ballot(t != ~0u);
    uint32_t rank = 0;
    while (rem) {  // the lanes of one table at a time: a lane's rank among them keeps the sorted order
        const int leader = __ffsll((long long)rem) - 1;
        const uint32_t tb = (uint32_t)__shfl((int)t, leader);
        const uint64_t m = __ballot(t == tb);
        if (t == tb) rank = (uint32_t)__popcll(m & ((1ull << lane) - 1));
        if ((int)lane == leader) s_wc[w][tb] = (uint32_t)__popcll(m);
        rem &= ~m;
    }
    __syncthreads();
    if (t == ~0u) return;
    uint32_t before = 0;
    for (uint32_t q = 0; q < w; q++) before += s_wc[q][t];
    a.dst[a.table_pre[t0 + t] + a.count[(uint64_t)blockIdx.x * kReplayBuckets + t] + before + rank] = row;
}

__global__ __launch_bounds__(kReplayBlock) void k_rp_sizes(ReplayArgs a) {
    if (a.word[kRpEmitStatus] != SDB_OK) return;
    __shared__ uint64_t s_w[17];
    const uint64_t j = (uint64_t)blockIdx.x * kReplayBlock + threadIdx.x;
    uint64_t kb = 0, vb = 0, tk, tv;
    if (j < a.word[kRpRowsOut]) {
        const uint32_t i = a.dst[j];
        kb = a.r.key_off[i + 1] - a.r.key_off[i];
        vb = row_val_bytes(a, i, a.r.flags[i]);
    }
    block_excl_scan_u64(kb, s_w, &tk);
    block_excl_scan_u64(vb, s_w, &tv);
    if (threadIdx.x == 0) {
        a.tile_sum[2 * (uint64_t)blockIdx.x] = tk;
        a.tile_sum[2 * (uint64_t)blockIdx.x + 1] = tv;
    }
}

__global__ __launch_bounds__(kReplayBlock) void k_rp_escan(ReplayArgs a) {
    if (a.word[kRpEmitStatus] != SDB_OK) return;
    __shared__ uint64_t s_w[17];
    uint64_t carry[2] = {0, 0};
    for (uint32_t base = 0; base < a.nblocks; base += kReplayBlock) {
        const uint32_t k = base + threadIdx.x;
#pragma unroll
        for (int f = 0; f < 2; f++) {
            uint64_t t;
            const uint64_t ex = block_excl_scan_u64(k < a.nblocks ? a.tile_sum[2 * (uint64_t)k + f] : 0, s_w, &t);
            if (k < a.nblocks) a.tile_sum[2 * (uint64_t)k + f] = carry[f] + ex;
            carry[f] += t;
        }
    }
    if (threadIdx.x) return;
    const uint64_t m = a.word[kRpRowsOut];
    a.out.key_off[m] = a.word[kRpKeyBytes];
    a.out.val_off[m] = a.word[kRpValBytes];
}

__global__ __launch_bounds__(kReplayBlock) void k_rp_gather(ReplayArgs a) {
    if (a.word[kRpEmitStatus] != SDB_OK) return;
    __shared__ uint64_t s_w[17];
    __shared__ CopyDesc s_cd[kReplayBlock];
    const sdb_wal_tables_out &o = a.out;
    const uint64_t m = a.word[kRpRowsOut], j = (uint64_t)blockIdx.x * kReplayBlock + threadIdx.x;
    if ((uint64_t)blockIdx.x * kReplayBlock >= m) return;
    CopyDesc cd{nullptr, nullptr, nullptr, nullptr, 0, 0};
    uint32_t i = 0;
    uint8_t f = 0;
    uint64_t seq = 0;
    if (j < m) {
        i = a.dst[j];
        f = a.r.flags[i];
        seq = a.r.seq[i];
        const uint64_t k0 = a.r.key_off[i];
        cd.ks = a.r.key_arena + k0;
        cd.kb = (uint32_t)(a.r.key_off[i + 1] - k0);
        cd.vb = row_val_bytes(a, i, f);
        cd.vs = a.r.val_base + a.r.val_off[i];
    }
    uint64_t t;
    const uint64_t ko = a.tile_sum[2 * (uint64_t)blockIdx.x] + block_excl_scan_u64(cd.kb, s_w, &t);
    const uint64_t vo = a.tile_sum[2 * (uint64_t)blockIdx.x + 1] + block_excl_scan_u64(cd.vb, s_w, &t);
    if (j < m) {
        uint8_t mask = 0;
        if ((f & SDB_FLAG_HAS_CREATE_TS) && a.r.create_ts) mask |= SDB_TS_CREATE;
        if ((f & SDB_FLAG_HAS_EXPIRE_TS) && a.r.expire_ts) mask |= SDB_TS_EXPIRE;
        o.key_off[j] = ko;
        o.val_off[j] = vo;
        o.kind[j] = (f & SDB_FLAG_TOMBSTONE) ? SDB_KIND_TOMBSTONE : (f & SDB_FLAG_MERGE_OPERAND) ? SDB_KIND_MERGE : SDB_KIND_VALUE;
        o.seq[j] = seq;
        o.ts_mask[j] = mask;
        o.create_ts[j] = (mask & SDB_TS_CREATE) ? a.r.create_ts[i] : 0;
        o.expire_ts[j] = (mask & SDB_TS_EXPIRE) ? a.r.expire_ts[i] : 0;
        cd.kd = o.key_bytes + ko;
        cd.vd = o.val_bytes + vo;
    }
    s_cd[threadIdx.x] = cd;
    __syncthreads();
    copy_wave_rows(s_cd + (threadIdx.x & ~63u), lane_id());  // each wave its 64 rows (sdb_copy.h)
}

uint32_t blocks_of(uint64_t n) { return (uint32_t)((n + kReplayBlock - 1) / kReplayBlock); }

}  // namespace

hipError_t launch_replay_sort(const ReplayArgs &a, hipStream_t st) {
    if (a.n == 0 || a.nbatches == 0) {
        hipLaunchKernelGGL(k_rp_zero, dim3(1), dim3(kReplayBlock), 0, st, a);
        return hipGetLastError();
    }
    const uint32_t nb = blocks_of(a.n);
    hipLaunchKernelGGL(k_rp_init, dim3(1), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(k_rp_facts, dim3(nb), dim3(kReplayBlock), 0, st, a);
    hipLaunchKernelGGL(k_rp_order, dim3(1), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_rp_tile_sort, dim3(a.ntiles), dim3(kReplayThreads), 0, st, a);
    uint64_t run = kReplayTile;
    for (uint32_t p = 0; p < a.npass; p++, run *= 2)
        hipLaunchKernelGGL(k_rp_merge, dim3(a.ntiles), dim3(kReplayThreads), 0, st, a, run, (const uint32_t *)a.perm[p & 1],
                           a.perm[(p + 1) & 1]);
    hipLaunchKernelGGL(k_rp_mark, dim3(nb), dim3(kReplayBlock), 0, st, a);
    hipLaunchKernelGGL(k_rp_count, dim3(nb), dim3(kReplayBlock), 0, st, a);
    hipLaunchKernelGGL(k_rp_finish, dim3(1), dim3(kReplayBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_replay_emit(const ReplayArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(k_rp_tables, dim3(1), dim3(kReplayBlock), 0, st, a);
    if (a.n == 0 || a.nbatches == 0) return hipGetLastError();
    const uint32_t nb = blocks_of(a.n);
    for (uint64_t t0 = 0; t0 < a.ntables; t0 += kReplayBuckets) {
        hipLaunchKernelGGL(k_rp_tcount, dim3(nb), dim3(kReplayBlock), 0, st, a, (uint32_t)t0);
        hipLaunchKernelGGL(k_rp_tscan, dim3(kReplayBuckets), dim3(kReplayBlock), 0, st, a);
        hipLaunchKernelGGL(k_rp_tscatter, dim3(nb), dim3(kReplayBlock), 0, st, a, (uint32_t)t0);
    }
    hipLaunchKernelGGL(k_rp_sizes, dim3(nb), dim3(kReplayBlock), 0, st, a);
    hipLaunchKernelGGL(k_rp_escan, dim3(1), dim3(kReplayBlock), 0, st, a);
    hipLaunchKernelGGL(k_rp_gather, dim3(nb), dim3(kReplayBlock), 0, st, a);
    return hipGetLastError();
}

}  // namespace sdb
