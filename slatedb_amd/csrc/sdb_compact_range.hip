// sdb_compact_range.hip — the input side of sdb_compactor_run_ssts_ranged: what load_iterators does with
// job_args.range and each input's visible_range (compactor_executor.rs:327-435; calculate_view_range,
// db_state.rs:243-251) before the merge sees a row.
//   k_rx_cover    one workgroup: the ranges checked (R7), V[i] = job ∩ visible[i] (R1; with a resume cursor also
//                 ∩ [K, ..), rule S1 of sdb_compactor_run_ssts_filtered), its covering blocks
//                 (R2: covering_blocks of sdb_range.h over the input's index keys), and the scan over the inputs
//                 that closes the covered blocks up into the block list k_cx_blocks fills for the decode
//   k_rx_clip     one thread per input: the rows of its decoded blocks that V[i] contains (R3), by two bound
//                 searches over the decoded keys of its first and last rows' neighbourhood
//   k_rx_gate     one workgroup: the decode's status with the failing block renumbered among all inputs' blocks,
//                 the decoded counts against the declared ones (R6), the per-input and per-run row ranges
//   k_rx_compact  the contributed rows closed up into columns of their own (only when a row was dropped)
// These are latency-bound searches over a few hundred inputs at most; the bytes move in k_rx_compact.
#include <hip/hip_runtime.h>

#include "sdb_compact.h"
#include "sdb_range.h"

namespace sdb {
namespace {

constexpr uint32_t kRxThreads = 256;

// V[i]: the tighter start and the tighter end of the job range and input i's visible range (R1)
SDB_DEV void view_range(const RxInputs &a, uint32_t i, Bound &s, Bound &e) {
    Bound js{nullptr, 0, 0}, je{nullptr, 0, 0}, ps{nullptr, 0, 0}, pe{nullptr, 0, 0};
    if (a.has_job) {
        js = range_start(a.job, 0);
        je = range_end(a.job, 0);
    }
    if (a.has_proj) {
        ps = range_start(a.proj, i);
        pe = range_end(a.proj, i);
    }
    s = tighter_start(js, ps);
    if (a.has_resume) s = tighter_start(s, Bound{a.resume_key, a.resume_len, SDB_BOUND_INCLUDED});  // S1: seek(K)
    e = tighter_end(je, pe);
}

// Exclusive prefix of item(0..n) by the workgroup: put(i, prefix of i); the total in every thread.  Each thread
// owns a contiguous chunk; lane 0 scans the chunk sums.
template <typename G, typename P>
SDB_DEV uint64_t wg_prefix(uint32_t n, uint64_t *s_part, G &&item, P &&put) {
    const uint32_t t = threadIdx.x, per = (n + kRxThreads - 1) / kRxThreads;
    const uint32_t i0 = min(n, t * per), i1 = min(n, i0 + per);
    uint64_t sum = 0;
    for (uint32_t i = i0; i < i1; i++) sum += item(i);
    s_part[t] = sum;
    __syncthreads();
    if (t == 0) {
        uint64_t run = 0;
        for (uint32_t k = 0; k < kRxThreads; k++) {
            const uint64_t v = s_part[k];
            s_part[k] = run;
            run += v;
        }
        s_part[kRxThreads] = run;
    }
    __syncthreads();
    uint64_t run = s_part[t];
    for (uint32_t i = i0; i < i1; i++) {
        put(i, run);
        run += item(i);
    }
    const uint64_t total = s_part[kRxThreads];
    __syncthreads();
    return total;
}

// the last x in [0, n) with first[x] <= k (first ascends, first[0] <= k): the input that holds item k
SDB_DEV uint32_t input_of(const uint64_t *first, uint32_t n, uint64_t k) {
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (first[mid] <= k) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kRxThreads) void k_rx_cover(RxInputs a) {
    __shared__ uint64_t s_part[kRxThreads + 1];
    __shared__ int s_bad;
    const uint32_t t = threadIdx.x;
    if (t == 0) s_bad = 0;
    __syncthreads();
    // R7: kinds and offsets only; nothing is read through them when one is malformed
    bool bad = false;
    if (t == 0 && a.has_job)
        bad = a.job.start_kind[0] > SDB_BOUND_EXCLUDED || a.job.end_kind[0] > SDB_BOUND_EXCLUDED ||
              a.job.start_off[1] < a.job.start_off[0] || a.job.end_off[1] < a.job.end_off[0];
    if (a.has_proj)
        for (uint32_t i = t; i < a.n; i += kRxThreads) bad |= bad_projection(a.proj, i);
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    const bool fail = s_bad != 0;
    for (uint32_t i = t; i < a.n; i += kRxThreads) {
        BlockRange g{0, 0};
        bool clipped = false;
        if (!fail) {
            Bound s, e;
            view_range(a, i, s, e);
            clipped = s.kind || e.kind;
            if (!empty_as_set(s, e)) {
                sdb_sst_view v{};
                v.num_blocks = a.num_blocks[i];
                v.index_keys = a.index_keys[i];
                v.index_key_off = a.index_key_off[i];
                g = covering_blocks(v, s, e);
                if (g.end < g.start) g.end = g.start;
            }
        }
        a.cover[2 * i] = g.start;
        a.cover[2 * i + 1] = g.end;
        a.clipped[i] = clipped ? 1 : 0;
        a.cov_off[i] = a.block_off[i] + g.start;
    }
    if (t == 0) a.cover[2 * (uint64_t)a.n] = fail ? SDB_INVALID_ARGUMENT : SDB_OK;
    __syncthreads();
    const uint64_t total = wg_prefix(a.n, s_part, [&](uint32_t i) { return a.cover[2 * i + 1] - a.cover[2 * i]; },
                                     [&](uint32_t i, uint64_t p) { a.cov_first[i] = p; });
    if (t == 0) a.cov_first[a.n] = total;
}

// the decoded key of row j against a bound's key
SDB_DEV int cmp_row(const sdb_decoded_out &d, uint64_t j, const Bound &b) {
    const uint64_t k0 = d.key_off[j], k1 = d.key_off[j + 1];
    return cmp_bytes(d.key_arena + k0, (uint32_t)(k1 - k0), b.t, b.n, 0).c;
}

__global__ void k_rx_clip(RxInputs a, sdb_decoded_out d) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    uint64_t lo = 0, hi = 0;
    if (d.summary->status == SDB_OK) {  // (else the columns are unspecified: k_rx_gate fails the job)
        const uint64_t e0 = d.block_entry_start[a.cov_first[i]], e1 = d.block_entry_start[a.cov_first[i + 1]];
        lo = e0;
        hi = e1;
        if (a.clipped[i] && e0 < e1) {
            Bound s, e;
            view_range(a, i, s, e);
            if (s.kind) {  // the first row that does not precede the start
                uint64_t x = e0, y = e1;
                while (x < y) {
                    const uint64_t m = x + (y - x) / 2;
                    if (precedes(s, cmp_row(d, m, s))) x = m + 1;
                    else y = m;
                }
                lo = x;
            }
            if (e.kind) {  // the first row from there on that exceeds the end
                uint64_t x = lo, y = e1;
                while (x < y) {
                    const uint64_t m = x + (y - x) / 2;
                    if (!exceeds(e, cmp_row(d, m, e))) x = m + 1;
                    else y = m;
                }
                hi = x;
            }
        }
    }
    a.lo[i] = lo;
    a.hi[i] = hi;
}

__global__ __launch_bounds__(kRxThreads) void k_rx_gate(RxInputs a, sdb_decoded_out d, const unsigned long long *dec_err,
                                                        uint64_t decl_entries, uint64_t decl_key_bytes) {
    __shared__ uint64_t s_part[kRxThreads + 1];
    __shared__ unsigned long long s_err;
    __shared__ int s_clipped;
    const uint32_t t = threadIdx.x;
    if (t == 0) {
        s_err = ~0ull;
        s_clipped = 0;
    }
    __syncthreads();
    const sdb_decode_summary *ds = d.summary;
    const bool dec_ok = ds->status == SDB_OK;
    if (dec_ok) {  // R6: an unclipped input holds exactly its declared rows, a clipped one's cover at most
        unsigned long long e = ~0ull;
        int any = 0;
        for (uint32_t i = t; i < a.n; i += kRxThreads) {
            const uint64_t cnt = d.block_entry_start[a.cov_first[i + 1]] - d.block_entry_start[a.cov_first[i]];
            const uint64_t decl = a.num_entries[i];
            any |= a.clipped[i];
            if (a.clipped[i] ? cnt > decl : cnt != decl) {
                const unsigned long long w = ((a.gblock[i] + a.cover[2 * i]) << 8) | SDB_INVALID_ARGUMENT;
                e = w < e ? w : e;
            }
        }
        if (e != ~0ull) atomicMin(&s_err, e);
        if (any) atomicOr(&s_clipped, 1);
    } else if (t == 0) {  // the decode's lowest failing block, numbered among all inputs' blocks
        const unsigned long long e = *dec_err;
        if (e != ~0ull) {
            const uint64_t k = e >> 8;
            const uint32_t i = input_of(a.cov_first, a.n, k);
            s_err = ((a.gblock[i] + a.cover[2 * i] + (k - a.cov_first[i])) << 8) | (e & 0xFF);
        } else {
            s_err = (unsigned long long)(uint32_t)ds->status;
        }
    }
    __syncthreads();
    // no input clipped: the totals are exact, and a job whose totals disagree fails as sdb_compactor_run_ssts does
    if (t == 0 && dec_ok && !s_clipped && (ds->num_entries != decl_entries || ds->key_bytes != decl_key_bytes))
        s_err = SDB_INVALID_ARGUMENT;
    __syncthreads();
    const unsigned long long gate = s_err;
    const bool ok = gate == ~0ull;
    const uint64_t rows = wg_prefix(a.n, s_part, [&](uint32_t i) { return ok ? a.hi[i] - a.lo[i] : 0; },
                                    [&](uint32_t i, uint64_t p) { a.out_first[i] = p; });
    const uint64_t kb = wg_prefix(a.n, s_part, [&](uint32_t i) { return ok ? d.key_off[a.hi[i]] - d.key_off[a.lo[i]] : 0; },
                                  [&](uint32_t i, uint64_t p) { a.out_key[i] = p; });
    if (t == 0) {
        a.out_first[a.n] = rows;
        a.out_key[a.n] = kb;
        a.result[kRxGate] = gate;
        a.result[kRxDecoded] = dec_ok ? ds->num_entries : 0;
        a.result[kRxIn] = rows;
        a.result[kRxKeyBytes] = kb;
    }
    __syncthreads();
    for (uint32_t r = t; r <= a.nruns; r += kRxThreads) a.result[kRxResult + r] = a.out_first[a.run_start[r]];
}

__global__ void k_rx_compact(RxInputs a, sdb_decoded_out d, sdb_decoded_out o) {
    const uint64_t rows = a.out_first[a.n];
    if (blockIdx.x == 0 && threadIdx.x == 0) o.key_off[rows] = a.out_key[a.n];
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < rows; j += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t i = input_of(a.out_first, a.n, j);
        const uint64_t src = a.lo[i] + (j - a.out_first[i]);
        const uint64_t k0 = d.key_off[src], k1 = d.key_off[src + 1];
        const uint64_t ko = a.out_key[i] + (k0 - d.key_off[a.lo[i]]);
        o.key_off[j] = ko;
        copy_bytes(o.key_arena + ko, d.key_arena + k0, (uint32_t)(k1 - k0));
        o.val_off[j] = d.val_off[src];
        o.val_len[j] = d.val_len[src];
        o.seq[j] = d.seq[src];
        o.flags[j] = d.flags[src];
        o.create_ts[j] = d.create_ts[src];
        o.expire_ts[j] = d.expire_ts[src];
    }
}

}  // namespace

hipError_t launch_rx_cover(const RxInputs &a, hipStream_t st) {
    hipLaunchKernelGGL(k_rx_cover, dim3(1), dim3(kRxThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_rx_clip_gate(const RxInputs &a, const sdb_decoded_out &dec, const unsigned long long *dec_err,
                               uint64_t decl_entries, uint64_t decl_key_bytes, hipStream_t st) {
    if (a.n) hipLaunchKernelGGL(k_rx_clip, dim3((a.n + 63) / 64), dim3(64), 0, st, a, dec);
    hipLaunchKernelGGL(k_rx_gate, dim3(1), dim3(kRxThreads), 0, st, a, dec, dec_err, decl_entries, decl_key_bytes);
    return hipGetLastError();
}

hipError_t launch_rx_compact(const RxInputs &a, const sdb_decoded_out &dec, const sdb_decoded_out &out, uint64_t rows,
                             hipStream_t st) {
    const uint64_t g = (rows + 255) / 256;
    hipLaunchKernelGGL(k_rx_compact, dim3((uint32_t)(g < 1 ? 1 : (g < 4096 ? g : 4096))), dim3(256), 0, st, a, dec, out);
    return hipGetLastError();
}

}  // namespace sdb
