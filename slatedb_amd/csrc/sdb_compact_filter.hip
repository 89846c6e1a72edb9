// sdb_compact_filter.hip — the device side of the compaction filter and of the resume cursor
// (compaction_filter_iterator.rs:19-66; ResumingIterator, compactor_executor.rs:123-199), between the merge emit
// and the cuts.  The filter itself runs on the host over the gathered stream (sdb_compactor.cpp, filter_step); what
// comes back is one decision byte per row and the replacement values in row order (CfArgs, sdb_compact.h).
//   k_cf_size   per tile of kMergeTile rows: kept rows, their key bytes, the modified rows (VALUE / MERGE) and the
//               value bytes of the kept rows that keep their value
//   k_cf_scan   one workgroup: the tile sums to exclusive offsets, the totals, the stream's closing offsets.  The
//               modified-row rank maps a row to mod_off: replacement bytes before a row = mod_off[its rank]
//   k_cf_emit   one workgroup per tile: the kept rows' columns with F3 / F4 applied, then keys and values into the
//               new arenas by the chunk copies of sdb_copy.h (descriptors in LDS, eight lanes per row, 16 bytes per
//               lane per step); a value comes from the old value arena or from the uploaded one
//   k_cf_seek   S1 over decoded runs: one thread per run, the lower bound of the cursor's key
//   k_cf_drain  S2 without a filter: one workgroup, the first row at which key == K && seq >= S fails
#include <hip/hip_runtime.h>

#include "sdb_compact.h"
#include "sdb_copy.h"
#include "sdb_read.h"

namespace sdb {
namespace {

constexpr uint32_t kCfHalf = kMergeThreads;  // rows a workgroup takes at a time: a tile in kMergeTile / kCfHalf steps
static_assert(kMergeTile % kCfHalf == 0 && kCfHalf % 64 == 0 && kCfHalf <= 1024, "a tile is whole steps of whole waves");

struct CfRow {
    uint32_t kept, mod;  // mod: the value comes from the uploaded arena
    uint32_t kb, vb;     // key bytes; value bytes when the row keeps its value (0: tombstoned or replaced)
    uint8_t d;
};
SDB_DEV CfRow cf_row(const CfArgs &a, uint64_t i) {
    CfRow r{0, 0, 0, 0, SDB_CF_DROP};
    if (i >= a.n) return r;
    r.d = a.decision[i];
    if (r.d == SDB_CF_DROP) return r;
    r.kept = 1;
    r.kb = (uint32_t)(a.in.key_off[i + 1] - a.in.key_off[i]);
    r.mod = r.d == SDB_CF_VALUE || r.d == SDB_CF_MERGE;
    r.vb = r.d == SDB_CF_KEEP ? (uint32_t)(a.in.val_off[i + 1] - a.in.val_off[i]) : 0;
    return r;
}

__global__ __launch_bounds__(kCfHalf) void k_cf_size(CfArgs a) {
    __shared__ uint64_t s_w[17];
    uint64_t sum[4] = {0, 0, 0, 0};
    for (uint32_t h = 0; h < kMergeTile; h += kCfHalf) {
        const CfRow r = cf_row(a, (uint64_t)blockIdx.x * kMergeTile + h + threadIdx.x);
        const uint64_t v[4] = {r.kept, r.kb, r.mod, r.vb};
#pragma unroll
        for (int f = 0; f < 4; f++) {
            uint64_t t;
            block_excl_scan_u64(v[f], s_w, &t);
            sum[f] += t;
        }
    }
    if (threadIdx.x == 0)
        for (int f = 0; f < 4; f++) a.tile_sum[4 * (uint64_t)blockIdx.x + f] = sum[f];
}

__global__ __launch_bounds__(kCfHalf) void k_cf_scan(CfArgs a) {
    __shared__ uint64_t s_w[17];
    uint64_t carry[4] = {0, 0, 0, 0};
    for (uint64_t base = 0; base < a.ntiles; base += kCfHalf) {
        const uint64_t k = base + threadIdx.x;
#pragma unroll
        for (int f = 0; f < 4; f++) {
            uint64_t t;
            const uint64_t ex = block_excl_scan_u64(k < a.ntiles ? a.tile_sum[4 * k + f] : 0, s_w, &t);
            if (k < a.ntiles) a.tile_sum[4 * k + f] = carry[f] + ex;
            carry[f] += t;
        }
    }
    if (threadIdx.x) return;
    for (int f = 0; f < 4; f++) a.tile_sum[4 * a.ntiles + f] = carry[f];
    if (carry[0] <= a.out.cap_entries) {  // (the host sized the stream from the same decisions)
        a.out.key_off[carry[0]] = carry[1];
        a.out.val_off[carry[0]] = carry[3] + a.mod_off[carry[2]];
    }
}

__global__ __launch_bounds__(kCfHalf) void k_cf_emit(CfArgs a) {
    __shared__ uint64_t s_w[17];
    __shared__ CopyDesc s_cd[kCfHalf];
    const sdb_merged_out &o = a.out;
    uint64_t base[4];
    for (int f = 0; f < 4; f++) base[f] = a.tile_sum[4 * (uint64_t)blockIdx.x + f];
    for (uint32_t h = 0; h < kMergeTile; h += kCfHalf) {
        const uint64_t i = (uint64_t)blockIdx.x * kMergeTile + h + threadIdx.x;
        const CfRow r = cf_row(a, i);
        const uint64_t v[4] = {r.kept, r.kb, r.mod, r.vb};
        uint64_t ex[4], tot[4];
#pragma unroll
        for (int f = 0; f < 4; f++) ex[f] = block_excl_scan_u64(v[f], s_w, &tot[f]);
        CopyDesc cd{nullptr, nullptr, nullptr, nullptr, 0, 0};
        const uint64_t j = base[0] + ex[0];
        if (r.kept && j < o.cap_entries) {
            const uint64_t rank = base[2] + ex[2];             // modified rows before this one
            const uint64_t m0 = a.mod_off[rank];               // their replacement bytes
            const uint64_t ko = base[1] + ex[1], vo = base[3] + ex[3] + m0;
            uint8_t kind = a.in.kind[i], mask = a.in.ts_mask[i];
            int64_t expire = a.in.expire_ts[i];
            cd.vb = r.vb;
            cd.vs = a.in.val_bytes + a.in.val_off[i];
            if (r.d == SDB_CF_TOMBSTONE) {  // F3: no value, no expire_ts
                kind = SDB_KIND_TOMBSTONE;
                mask &= (uint8_t)~SDB_TS_EXPIRE;
                expire = 0;
            } else if (r.mod) {             // F4: the kind and the value change, the timestamps stay
                kind = r.d == SDB_CF_VALUE ? SDB_KIND_VALUE : SDB_KIND_MERGE;
                cd.vb = (uint32_t)(a.mod_off[rank + 1] - m0);
                cd.vs = a.arena + m0;
            }
            o.key_off[j] = ko;
            o.val_off[j] = vo;
            o.kind[j] = kind;
            o.seq[j] = a.in.seq[i];
            o.create_ts[j] = a.in.create_ts[i];
            o.expire_ts[j] = expire;
            o.ts_mask[j] = mask;
            cd.ks = a.in.key_bytes + a.in.key_off[i];
            cd.kb = r.kb;
            cd.kd = o.key_bytes + ko;
            cd.vd = o.val_bytes + vo;
            if (ko + cd.kb > o.key_cap || vo + cd.vb > o.val_cap) cd.kb = cd.vb = 0;  // never past the sized arenas
        }
        s_cd[threadIdx.x] = cd;
        __syncthreads();
        copy_wave_rows(s_cd + (threadIdx.x & ~63u), lane_id());  // each wave its 64 rows
        __syncthreads();
        for (int f = 0; f < 4; f++) base[f] += tot[f];
    }
}

__global__ void k_cf_seek(const CfSeekRun *runs, uint32_t nruns, const uint8_t *key, uint32_t key_len, uint64_t *lb) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nruns) return;
    const CfSeekRun R = runs[r];
    uint64_t x = 0, y = R.n;
    while (x < y) {  // the first row whose key does not precede K
        const uint64_t m = x + (y - x) / 2;
        const uint64_t k0 = R.key_off[m];
        if (cmp_bytes(R.key_arena + k0, (uint32_t)(R.key_off[m + 1] - k0), key, key_len, 0).c < 0) x = m + 1;
        else y = m;
    }
    lb[r] = x;
}

constexpr uint32_t kCfDrain = 256;
__global__ __launch_bounds__(kCfDrain) void k_cf_drain(sdb_kv_batch m, const uint8_t *key, uint32_t key_len, uint64_t seq,
                                                       uint64_t *drained) {
    __shared__ unsigned long long s_first;
    if (threadIdx.x == 0) s_first = ~0ull;
    __syncthreads();
    for (uint64_t base = 0; base < m.n; base += kCfDrain) {  // (a key has few versions: one step as a rule)
        const uint64_t i = base + threadIdx.x;
        if (i < m.n) {
            const uint64_t k0 = m.key_off[i];
            const bool same = cmp_bytes(m.key_bytes + k0, (uint32_t)(m.key_off[i + 1] - k0), key, key_len, 0).c == 0;
            if (!(same && m.seq[i] >= seq)) atomicMin(&s_first, (unsigned long long)i);
        }
        __syncthreads();
        const bool found = s_first != ~0ull;
        __syncthreads();  // (every thread has read it before the next step's atomics)
        if (found) break;
    }
    if (threadIdx.x == 0) *drained = s_first == ~0ull ? m.n : s_first;
}

}  // namespace

hipError_t launch_cf_apply(const CfArgs &a, hipStream_t st) {
    if (!a.ntiles) return hipSuccess;
    hipLaunchKernelGGL(k_cf_size, dim3((uint32_t)a.ntiles), dim3(kCfHalf), 0, st, a);
    hipLaunchKernelGGL(k_cf_scan, dim3(1), dim3(kCfHalf), 0, st, a);
    hipLaunchKernelGGL(k_cf_emit, dim3((uint32_t)a.ntiles), dim3(kCfHalf), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_cf_seek(const CfSeekRun *runs, uint32_t nruns, const uint8_t *key, uint32_t key_len, uint64_t *lb,
                          hipStream_t st) {
    if (!nruns) return hipSuccess;
    hipLaunchKernelGGL(k_cf_seek, dim3((nruns + 63) / 64), dim3(64), 0, st, runs, nruns, key, key_len, lb);
    return hipGetLastError();
}

hipError_t launch_cf_drain(const sdb_kv_batch &m, const uint8_t *key, uint32_t key_len, uint64_t seq, uint64_t *drained,
                           hipStream_t st) {
    hipLaunchKernelGGL(k_cf_drain, dim3(1), dim3(kCfDrain), 0, st, m, key, key_len, seq, drained);
    return hipGetLastError();
}

}  // namespace sdb
