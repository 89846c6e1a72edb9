// sdb_lookup.hip — batched point lookups / seeks on one encoded SST for gfx950, and the block-check pass that
// the scans (sdb_scan.hip) and the tree gets (sdb_get.hip) share with them.
//
// Replaces the read path of Db::get / an SstIterator positioned on a key:
//   filter      BloomFilter::might_contain(filter_hash(key))            filter.rs:124-136
//   blocks      partitions_covering_range([key, key]) over the index     partitioned_keyspace.rs:16-110
//   seek        BlockIteratorV2::seek asc / DescendingBlockIteratorV2    block_iterator_v2.rs:138-208,
//               ::seek; BlockIterator::seek (V1)                         269-313, 318-469;
//                                                                        block_iterator.rs:130-190
//   next block  only the first block of the range is seeked; an exhausted seek enters the next block
//               at its first (asc) / last (desc) entry                   sst_iter.rs:501-516
//   checksum    every block read is CRC-checked                          format/sst.rs:1029-1038
// Three launches: k_lk_locate (thread per query: filter + index -> the <= 2 blocks the seek can
// touch, marked), k_check (wave per marked block: the shared wave CRC), k_lk_seek (thread per
// query: the seek itself).  Keys are never materialised: a seek step compares the next key
// prev[..shared] ++ suffix with the target from the running (common prefix, order) state of the
// previous key, reading only the suffix bytes.  The block reader itself is sdb_read.h.
#include <mutex>

#include "sdb_read.h"

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

__global__ __launch_bounds__(256) void k_lk_locate(LookupArgs a) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.nkeys) return;
    const uint8_t *t = a.key_bytes + a.key_off[q];
    const uint32_t nt = (uint32_t)(a.key_off[q + 1] - a.key_off[q]);
    uint32_t start = 0, end = 0;
    bool filtered = false;
    // might_contain(filter_hash(key)) (filter.rs:124-136, 196-204)
    if (a.v.bloom) filtered = !bloom_might_contain(a.v.bloom, a.v.bloom_len, a.v.num_probes, siphash13(t, nt));
    if (!filtered) {
        point_block_range(a.v, t, nt, start, end);
        if (end > start) {  // the seeked block and the one after it in iteration order
            const uint32_t b0 = a.desc ? end - 1 : start;
            a.mark[b0] = 1;
            if (end - start >= 2) a.mark[a.desc ? end - 2 : start + 1] = 1;
        }
    }
    a.qrange[2 * q] = start;
    a.qrange[2 * q + 1] = filtered ? 0xFFFFFFFFu : end;
}

// One wave per marked block: Block::decode bounds + CRC (the shared wave CRC over an LDS image).
__global__ __launch_bounds__(kLkThreads) void k_check(CheckArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if (a.bad && *a.bad) return;
    crc_tables_to_lds((lu32 *)smem);
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6, l = (uint32_t)lane_id();
    lu8 *img = lk_wave_image(smem, wave, l);
    const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t k = (uint64_t)blockIdx.x * (blockDim.x >> 6) + wave; k < a.num_blocks; k += nw) {
        if (!a.mark[k]) continue;
        const uint8_t *data = a.v.data;
        const uint64_t *off = a.v.block_off;
        uint64_t b = k;
        if (a.bad) {
            const uint32_t i = sst_of_block(a.t, k);
            b = k - a.t.block_base[i];
            data = a.t.ssts[i].data;
            off = a.t.ssts[i].block_off;
        }
        const int st = lk_check_block(data, off[b], off[b + 1], img, l);
        if (l == 0) {
            a.bstat[k] = st;
            a.mark[k] = 0;  // ready for the next call
        }
    }
}

SDB_DEV void report(const LookupArgs &a, uint64_t q, const Blk &b, uint32_t blk, const Pos &P, int &st) {
    Row r;
    uint32_t phys = P.at;
    if (a.v.sst_version == 2) {
        if ((st = v2_row(b, P.at, r))) return;
        phys = 0;
        for (uint32_t p = 0; p < P.at; phys++) {  // the entry's index: rows before it
            Row x;
            if ((st = v2_row(b, p, x))) return;
            p = x.next;
        }
    } else if ((st = v1_row(b, P.at, r))) {
        return;
    }
    put_row(a.out, q, b.base, r);
    a.out.block[q] = blk;
    a.out.entry[q] = phys;
    a.out.key_len[q] = P.key.len;
    a.out.state[q] = P.key.c == 0 ? SDB_LOOKUP_FOUND : SDB_LOOKUP_POSITIONED;
}

__global__ __launch_bounds__(256) void k_lk_seek(LookupArgs a) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= a.nkeys) return;
    const uint8_t *t = a.key_bytes + a.key_off[q];
    const uint32_t nt = (uint32_t)(a.key_off[q + 1] - a.key_off[q]);
    const uint32_t start = a.qrange[2 * q], end = a.qrange[2 * q + 1];
    const bool v2 = a.v.sst_version == 2;
    a.out.status[q] = 0;
    a.out.state[q] = SDB_LOOKUP_EXHAUSTED;
    a.out.block[q] = a.out.entry[q] = a.out.key_len[q] = 0;
    put_row(a.out, q, 0, Row{});
    if (end == 0xFFFFFFFFu) {
        a.out.state[q] = SDB_LOOKUP_FILTERED;
        return;
    }
    int st = 0;
    for (uint32_t i = 0; end > start && i < 2 && i < end - start; i++) {  // seeked block, then its successor
        const uint32_t blk = a.desc ? end - 1 - i : start + i;
        Blk b;
        if ((st = a.bstat[blk]) || (st = blk_open(a.v, blk, b))) break;
        Pos P;
        P.ok = false;
        if (i == 0) {
            if (v2) st = a.desc ? v2_seek_desc(b, t, nt, P) : v2_seek_asc(b, t, nt, P);
            else st = v1_seek(b, t, nt, a.desc, P);
        } else if (b.count == 0) {  // an empty block; else a fresh block iterator: its first entry (asc) or last (desc)
        } else if (!a.desc) {
            st = first_entry(v2, b, t, nt, P);
        } else if (!v2) {
            P.ok = true;
            P.at = b.count - 1;
            st = v1_cmp(b, P.at, t, nt, P.key);
        } else {  // the last region's last entry
            uint32_t kp, kn;
            if (!(st = v2_restart_key(b, b.count - 1, kp, kn))) {
                Cmp cur = cmp_bytes(b.d + kp, kn, t, nt, 0);
                uint32_t off = boff(b, b.count - 1);
                while (!st && off < b.data_end) {
                    Row r;
                    if ((st = v2_row(b, off, r))) break;
                    if (r.sh > cur.len) {
                        st = SDB_CORRUPT_BLOCK;
                        break;
                    }
                    cur = cmp_next(cur, r.sh, b.d + r.suf, r.un, t, nt);
                    P.ok = true;
                    P.at = off;
                    P.key = cur;
                    off = r.next;
                }
            }
        }
        if (!st && P.ok) report(a, q, b, blk, P, st);
        if (st || P.ok) break;
    }
    if (st) {
        a.out.status[q] = st;
        a.out.state[q] = SDB_LOOKUP_EXHAUSTED;
    }
}

static uint64_t lookup_bind(LookupArgs &a, uint8_t *w) {
    Carver c{w, 0};
    c.take(a.qrange, 2 * (a.nkeys + 1));
    c.take(a.mark, a.v.num_blocks + 1);
    c.take(a.bstat, a.v.num_blocks + 1);
    return c.off;
}

uint64_t lookup_workspace_bytes(uint64_t num_blocks, uint64_t nkeys) {
    LookupArgs a{};
    a.v.num_blocks = num_blocks;
    a.nkeys = nkeys;
    return lookup_bind(a, nullptr);
}

hipError_t launch_check(const CheckArgs &a, hipStream_t st) {
    if (!a.num_blocks) return hipSuccess;
    static std::once_flag once;
    std::call_once(once, [] {
        (void)hipFuncSetAttribute((const void *)k_check, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLkLds);
        (void)hipGetLastError();
    });
    uint64_t wgs = (a.num_blocks + 3) / 4;
    if (wgs > 4096) wgs = 4096;
    hipLaunchKernelGGL(k_check, dim3((uint32_t)wgs), dim3(kLkThreads), kLkLds, st, a);
    return hipGetLastError();
}

hipError_t launch_lookup(const sdb_sst_view &v, const uint8_t *key_bytes, const uint64_t *key_off, uint64_t nkeys,
                         uint32_t desc, const sdb_lookup_out &out, uint8_t *w, hipStream_t st) {
    if (!nkeys) return hipSuccess;
    LookupArgs a{v, key_bytes, key_off, nkeys, desc, out, nullptr, nullptr, nullptr};
    lookup_bind(a, w);
    if (v.num_blocks) {
        hipError_t e = hipMemsetAsync(a.mark, 0, v.num_blocks, st);
        if (e != hipSuccess) return e;
    }
    const uint32_t qb = (uint32_t)((nkeys + 255) / 256);
    hipLaunchKernelGGL(k_lk_locate, dim3(qb), dim3(256), 0, st, a);
    hipError_t e = launch_check(CheckArgs{v, {}, nullptr, v.num_blocks, a.mark, a.bstat}, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lk_seek, dim3(qb), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace sdb
