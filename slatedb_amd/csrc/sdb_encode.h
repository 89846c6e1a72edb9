// sdb_encode.h — kernel arguments and LDS geometry of the SST encoder.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slatedb_amd.h"
#include "sdb_workspace.h"

namespace sdb {

constexpr uint32_t kChunk = 2048;            // entries per chunk (K3 / K5)
constexpr uint32_t kResolveLds = 96 * 1024;  // LDS budget of the resolve tables (u16 exits)
// k_emit's CRC tables: slicing-by-8 tables + x^256 byte tables + 6 combine-tree steps (36 KiB), or
// (SDB_EMIT_CRC_MFMA) the matrix-core CRC's weights + the tree steps (sdb_crc_mfma.h, 56 KiB): 43.1 vs
// 41.0 us per SST (r5) — the emit's LDS is not its bound, and 32 dependent MFMAs per block add latency
#ifndef SDB_EMIT_CRC_MFMA
#define SDB_EMIT_CRC_SLICE
#endif
#ifdef SDB_EMIT_CRC_SLICE
constexpr uint32_t kCrcLds = 36 * 1024;
#else
constexpr uint32_t kCrcLds = 56 * 1024;
#endif
constexpr uint32_t kImgCap = 4096 + 64;      // LDS block image per wave (fast path)
constexpr uint32_t kStageCap = 4096;         // value staging per wave (LDS-DMA, 1 KiB per instruction), in place
constexpr uint32_t kStageGuard = 64;         // LDS bytes before each image the value stage may use
constexpr uint32_t kKeyStageCap = 1024;      // key staging per wave
// k_emit's piece path (blocks over one image): a row it can stage with other rows' pieces
constexpr uint32_t kPieceRowMax = 4000, kPieceKeyMax = 960, kPieceValMax = 3968;
constexpr uint32_t kSegLook = 1024;           // k_seg: max lookahead entries staged past the chunk
constexpr uint32_t kSegSpan = kChunk + kSegLook;
constexpr uint32_t kSegThreads = 512;          // four workgroups per CU (kSegLds)
constexpr uint32_t kFactsThreads = 1024;      // k_facts: a chunk (= a fused bloom tile) per workgroup
constexpr uint32_t kFactsPerT = 2;            //   entries per thread
constexpr uint32_t kFactsEntries = kFactsThreads * kFactsPerT;
constexpr uint32_t kSegLds = (2 * kSegSpan + 4) * 4 + kChunk * 6;  // 36 KiB: four workgroups per CU
#ifndef SDB_EMIT_WAVES
#define SDB_EMIT_WAVES 16
#endif
// SDB_EMIT_WAVES waves per workgroup, 1 per CU: each wave assembles one block while the next one's data
// is in flight (16 waves: 128 VGPRs each, which hold it without spilling)
constexpr uint32_t kEmitThreads = 64 * SDB_EMIT_WAVES;
constexpr uint32_t kEmitWgPerCu = 1;
constexpr uint32_t kEmitWaveLds = kStageGuard + kImgCap + 16 + kKeyStageCap + 64 * 16;  // guard, image, key stage, spans
constexpr uint32_t kEmitLds = kCrcLds + 16 + (kEmitThreads / 64) * kEmitWaveLds;  // tables, ticket, waves
constexpr uint32_t kGroupThreads = 1024;
constexpr uint32_t kGroupLds = kResolveLds;         // group tables (restated in tests/encode_cases.py, group_paths)

// bloom build plan (sdb_bloom.hip): 2^sb-bit slices, T-key binning tiles
struct BloomPlan {
    uint32_t k, m;        // probes per key, bitmap bits
    uint32_t sb;          // log2 bits per slice
    uint32_t nslices, T, tiles;
    uint32_t one_pass;    // bin straight into per-slice LDS buckets of cap u16 (bloom_bin_core)
    uint32_t pad;
    uint64_t mmod;        // Lemire fastmod constant: floor((2^64 - 1) / m) + 1
};
struct BloomSlots {
    uint32_t *count;  // tiles x nslices: run length of each (tile, slice) slot (kSlotOverflow: too long)
    uint32_t *slot;   // (nslices x tiles) x cap probes, slice-major: u16 offsets in the slice when
                      // sb <= 16 (half the traffic), else u32 bit positions
    uint32_t cap;
};

struct BlockDesc {  // one per block, written by k_blocks, streamed by k_emit (56 bytes)
    uint32_t s, e;        // entries [s, e)
    uint64_t off;         // byte offset of the block in the data section
    uint64_t vs, ve, ks, ke;  // value / key byte ranges of the block
    uint32_t bb, route;   // encoded bytes incl. CRC; the assembler that takes the block (block_route)
};
enum : uint32_t { kRouteImage = 0, kRouteWorkgroup = 1, kRoutePieces = 2 };
// huge_part, per chunk: a row too large for a piece; a tombstone whose ignored val_off range is not empty
enum : uint32_t { kChunkHuge = 1, kChunkCarry = 2 };

struct EncodeArgs {
    // batch (device)
    const uint8_t *key_bytes;
    const uint64_t *key_off;
    const uint8_t *val_bytes;
    const uint64_t *val_off;
    const uint8_t *kind;
    const uint64_t *seq;
    const int64_t *create_ts;
    const int64_t *expire_ts;
    const uint8_t *ts_mask;
    uint64_t n;
    // params
    uint32_t block_size;
    uint32_t restart_interval;
    uint32_t version;
    uint32_t wal;           // WAL SST: no compute_index_key (no prefix panic), index_key_len 0
    uint32_t nchunks;
    uint32_t seg_look;      // lookahead entries staged by k_seg (covers the longest possible block)
    // workspace
    uint32_t *lcp;
    uint32_t *szr, *sznr;   // per entry (k_facts): restart-row size, non-restart size (V1: both the row size)
    uint32_t nfacts;        // k_facts workgroups (partials: stat_part / err_part are per facts workgroup)
    uint32_t *row_scratch;  // per entry: row offsets of slow-path blocks
    uint32_t *next;
    uint32_t *bbytes;
    uint32_t *tab_exit;
    uint32_t *tab_cnt;
    uint64_t *tab_bytes;
    uint32_t *anchor_e;     // nchunks+1
    uint32_t *anchor_blk;   // nchunks+1
    uint64_t *anchor_byte;  // nchunks+1
    unsigned long long *err;
    uint32_t *wmax;
    uint32_t *slow_count;
    uint32_t *slow_list;
    uint32_t *big_count;    // blocks over one k_emit image whose rows fit pieces (k_emit_big)
    uint32_t *big_list;
    BlockDesc *desc;
    uint64_t *stat_part;    // per k_facts workgroup: raw key, raw val, puts, deletes, merges
    uint32_t *huge_part;    // per k_facts workgroup (= chunk): kChunkHuge | kChunkCarry
    uint32_t *wmax_part;    // per chunk: longest candidate block (entries)
    unsigned long long *err_part;  // per k_facts workgroup: min (entry << 8 | code) of the checks (~0: none)
    uint32_t *gtab_exit;    // per group of kGroup chunks, seg_look candidates: composed transfer table
    uint32_t *gtab_cnt;
    uint64_t *gtab_bytes;
    // per chunk, per candidate entry offset into the chunk's group: the chain's state before the chunk (offset
    // into it, blocks and bytes since the group's entry), written with the group table by k_anchor
    uint32_t *pre_exit;
    uint32_t *pre_cnt;
    uint64_t *pre_bytes;
    uint32_t *anchor_arrived;  // k_anchor's group workgroups that have finished (the last one walks the chain)
    uint32_t *mode;         // chain head: 1 = k_seg's tables describe the chain, 0 = anchors by the serial walk
    uint32_t group;         // chunks per group (host: ~sqrt(nchunks))
    // bloom fused into the encode: k_facts hashes and bins each chunk (tile = chunk), k_seg fills
    uint32_t bloom_fused;
    BloomPlan bpl;
    BloomSlots bq;
    uint8_t *bloom_out;
    uint32_t *done;         // [0] k_emit workgroups finished (the last one writes the summary); [1] block ticket
    uint32_t nprep_wg;
    uint32_t seg_lds;       // k_seg's dynamic LDS bytes
    // outputs (device)
    uint8_t *out_data;
    uint64_t *out_block_off;
    uint32_t *out_block_first;
    uint32_t *out_index_key_len;
    uint16_t *out_block_stats;
    uint64_t data_cap, block_cap;
    sdb_sst_summary *summary;
    uint64_t bloom_len;
    uint32_t num_probes, filter_built;
    const uint64_t *bloom_len_dev;  // prefix-extractor filter: the device-counted length (~0: error)
};

// The workspace arrays of one SST's encode: X(EncodeArgs member, element type, elements).  n entries, nc
// chunks (k_seg / k_blocks), nf k_facts workgroups, nt = nc * kSegLook + 1 table rows (seg_look candidate entry
// points per chunk; one composed table per group, <= one per chunk; one prefix table per chunk).  This list is
// the only one: the field indices, the slot's offsets (SstSlot::wso), the size and make_args' bindings all come
// from it.  The bloom slots or the prefix filter's scratch (host-sized) follow the arrays, at wso[kWsTail].
#define SDB_ENCODE_WS(X)                                                                                      \
    X(lcp, uint32_t, n + 1)                                                                                   \
    X(szr, uint32_t, n + 1)                                                                                   \
    X(sznr, uint32_t, n + 1)                                                                                  \
    X(row_scratch, uint32_t, n + 1)                                                                           \
    X(next, uint32_t, n + 1)                                                                                  \
    X(bbytes, uint32_t, n + 1)                                                                                \
    X(tab_exit, uint32_t, nt)                                                                                 \
    X(tab_cnt, uint32_t, nt)                                                                                  \
    X(tab_bytes, uint64_t, nt)                                                                                \
    X(anchor_e, uint32_t, nc + 2)                                                                             \
    X(anchor_blk, uint32_t, nc + 2)                                                                           \
    X(anchor_byte, uint64_t, nc + 2)                                                                          \
    X(err, unsigned long long, 1)                                                                             \
    X(wmax, uint32_t, 1)                                                                                      \
    X(slow_count, uint32_t, 1)                                                                                \
    X(slow_list, uint32_t, n + 1)                                                                             \
    X(big_count, uint32_t, 1)                                                                                 \
    X(big_list, uint32_t, n + 1)                                                                              \
    X(desc, BlockDesc, n + 1)                                                                                 \
    X(stat_part, uint64_t, 5 * (nf + 1))                                                                      \
    X(huge_part, uint32_t, nf + 1)                                                                            \
    X(wmax_part, uint32_t, nc + 1)                                                                            \
    X(err_part, unsigned long long, nf + 1)                                                                   \
    X(done, uint32_t, 2)                                                                                      \
    X(gtab_exit, uint32_t, nt)                                                                                \
    X(gtab_cnt, uint32_t, nt)                                                                                 \
    X(gtab_bytes, uint64_t, nt)                                                                               \
    X(pre_exit, uint32_t, nt)                                                                                 \
    X(pre_cnt, uint32_t, nt)                                                                                  \
    X(pre_bytes, uint64_t, nt)                                                                                \
    X(anchor_arrived, uint32_t, 1)                                                                            \
    X(mode, uint32_t, 1)                                                                                      \
    X(bloom_len_dev, const uint64_t, 1)
enum WsField {
#define X(name, T, count) kWs_##name,
    SDB_ENCODE_WS(X)
#undef X
    kWsTail,
    kWsFields
};
// The arrays' offsets for n entries in 256-byte units (wso: kWsFields values, or NULL); returns their bytes,
// which is where the tail starts.
inline uint64_t encode_ws_layout(uint64_t n, uint32_t *wso) {
    const uint64_t nc = (n + kChunk - 1) / kChunk, nf = (n + kFactsEntries - 1) / kFactsEntries;
    const uint64_t nt = nc * kSegLook + 1;
    Carver c{nullptr, 0};
    uint64_t at[kWsFields];
#define X(name, T, count) at[kWs_##name] = c.bytes(sizeof(T) * (count));
    SDB_ENCODE_WS(X)
#undef X
    at[kWsTail] = c.off;
    for (int f = 0; wso && f < kWsFields; f++) wso[f] = (uint32_t)(at[f] >> 8);
    return c.off;
}
// The bloom slots (BloomSlots, sdb_bloom.hip) at w: the counts, then the slots of q.cap probes.  Returns their
// bytes (w == NULL: nothing is bound).
__host__ __device__ inline uint64_t bloom_slots_bind(BloomSlots &q, const BloomPlan &pl, uint8_t *w) {
    Carver c{w, 0};
    c.take(q.count, (uint64_t)pl.tiles * pl.nslices);
    c.take(q.slot, (uint64_t)pl.nslices * pl.tiles * q.cap);
    return c.off;
}
// The tail of an encode workspace that builds a whole-key filter / a prefix-extractor filter.
uint64_t encode_bloom_workspace_bytes(uint64_t n, uint32_t k, uint64_t bitmap_bytes);
uint64_t prefix_workspace_bytes(uint64_t n);
hipError_t launch_bloom_prefix(const uint8_t *key_bytes, const uint64_t *key_off, const int32_t *lens, uint64_t n,
                               uint32_t bpk, uint32_t kind, uint32_t arg, uint32_t whole, uint8_t *bitmap, uint64_t cap,
                               uint64_t *bloom_len, uint8_t *ws, hipStream_t st);
hipError_t launch_bloom_match(const uint8_t *bitmap, uint64_t bytes, uint32_t k, uint32_t whole, uint32_t kind,
                              uint32_t arg, const uint8_t *key_bytes, const uint64_t *key_off, const uint8_t *is_prefix,
                              const int32_t *qlens, uint64_t n, uint8_t *result, hipStream_t st);

// ------------------------------------------------------------------------------------------------
// A launch set: up to kMaxSsts independent SSTs with the same SsTableFormat knobs encoded by ONE
// launch sequence (blockIdx.y = SST for the per-SST grids; k_emit spreads every SST's blocks over one
// persistent grid).  The compaction / flush callers run several builders at once (l0_flush_parallelism,
// subcompactions: config.rs:1081, 1383-1390); batching them fills the GPU with the latency-bound
// segmentation kernels of all of them at once.  Passed by value (kernel arguments).
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kMaxSsts = 8;
struct SstSlot {
    const uint8_t *key_bytes;
    const uint64_t *key_off;
    const uint8_t *val_bytes;
    const uint64_t *val_off;
    const uint8_t *kind;
    const uint64_t *seq;
    const int64_t *create_ts;
    const int64_t *expire_ts;
    const uint8_t *ts_mask;
    uint64_t n;
    uint8_t *out_data;
    uint64_t *out_block_off;
    uint32_t *out_block_first;
    uint32_t *out_index_key_len;
    uint16_t *out_block_stats;
    uint64_t data_cap, block_cap;
    sdb_sst_summary *summary;
    uint8_t *bloom_out;
    uint64_t bloom_len;
    uint8_t *ws;              // this SST's workspace (256-byte aligned)
    uint32_t num_probes, filter_built, bloom_fused;
    uint32_t prefix_bloom;    // the filter is a prefix-extractor one: its length is device-counted
    uint32_t nchunks, nfacts, group, slot_cap;
    BloomPlan bpl;            // fused bloom plan (bloom_fused)
    // encode_ws_layout(n) in 256-byte units, filled on the host: the kernels load the offsets instead of
    // deriving the layout's 64-bit offset chain on the scalar unit
    uint32_t wso[kWsFields];
};
struct SstSet {
    uint32_t count;
    uint32_t block_size, restart_interval, version, wal, seg_look;
    uint32_t max_facts, max_chunks, max_groups, max_tiles, max_slices, pad;
    SstSlot s[kMaxSsts];
};

// EncodeArgs of SST i of a set (workspace carved from the slot's base; host and device).
__host__ __device__ inline EncodeArgs make_args(const SstSet &P, uint32_t i) {
    const SstSlot &s = P.s[i];
    EncodeArgs a{};
    a.key_bytes = s.key_bytes;
    a.key_off = s.key_off;
    a.val_bytes = s.val_bytes;
    a.val_off = s.val_off;
    a.kind = s.kind;
    a.seq = s.seq;
    a.create_ts = s.create_ts;
    a.expire_ts = s.expire_ts;
    a.ts_mask = s.ts_mask;
    a.n = s.n;
    a.block_size = P.block_size;
    a.restart_interval = P.restart_interval;
    a.version = P.version;
    a.wal = P.wal;
    a.nchunks = s.nchunks;
    a.seg_look = P.seg_look;
    a.nfacts = s.nfacts;
    // every array of SDB_ENCODE_WS at its offset: the list's element type must be the member's
#define X(name, T, count) a.name = (T *)(s.ws + ((uint64_t)s.wso[kWs_##name] << 8));
    SDB_ENCODE_WS(X)
#undef X
    if (!s.prefix_bloom) a.bloom_len_dev = nullptr;
    a.group = s.group;
    a.bloom_fused = s.bloom_fused;
    a.bpl = s.bpl;
    a.bq.cap = s.slot_cap;
    bloom_slots_bind(a.bq, s.bpl, s.ws + ((uint64_t)s.wso[kWsTail] << 8));
    a.bloom_out = s.bloom_out;
    a.nprep_wg = s.nchunks;
    a.seg_lds = kSegLds;
    a.out_data = s.out_data;
    a.out_block_off = s.out_block_off;
    a.out_block_first = s.out_block_first;
    a.out_index_key_len = s.out_index_key_len;
    a.out_block_stats = s.out_block_stats;
    a.data_cap = s.data_cap;
    a.block_cap = s.block_cap;
    a.summary = s.summary;
    a.bloom_len = s.bloom_len;
    a.num_probes = s.num_probes;
    a.filter_built = s.filter_built;
    return a;
}

// Enqueue the encode of every SST of the set on `st` (one launch sequence).
hipError_t launch_encode_set(const SstSet &P, size_t bin_lds, size_t fill_lds, hipStream_t st);
hipError_t launch_encode_empty(EncodeArgs a, hipStream_t st);
hipError_t launch_encode_prep(const SstSet &P, hipStream_t st);  // k_facts, k_seg, k_group: the cuts' chain

// stage timing (diagnostics)
enum Stage { kStBloom = 0, kStFacts, kStSeg, kStAnchor, kStBlocks, kStEmit, kStEmitBig, kStBloomFill, kNumStages };
void stage_mark(hipStream_t st, int stage, bool begin);
bool stage_timing_on();

// bloom (sdb_bloom.hip)
// tile_keys: keys per binning tile (0: the standalone build's choice; the fused encode bins per chunk)
BloomPlan bloom_plan(uint64_t n, uint32_t k, uint64_t bitmap_bytes, uint32_t tile_keys = 0);
uint64_t bloom_workspace_bytes(uint64_t n, uint32_t k, uint64_t bitmap_bytes);
// w: bloom_workspace_bytes(...) of scratch (256-byte aligned), or NULL (device-scope atomics; slow)
hipError_t launch_bloom_build(const uint8_t *key_bytes, const uint64_t *key_off, uint64_t n,
                              uint32_t num_probes, uint8_t *bitmap, uint64_t bitmap_bytes, uint8_t *w,
                              hipStream_t st);
hipError_t launch_bloom_query(const uint8_t *bitmap, uint64_t bitmap_bytes, uint32_t num_probes,
                              const uint8_t *key_bytes, const uint64_t *key_off, uint64_t n,
                              uint8_t *result, hipStream_t st);

}  // namespace sdb
static_assert(sdb::kSegSpan % sdb::kSegThreads == 0 && sdb::kChunk % 64 == 0, "k_seg geometry");
static_assert(sdb::kEmitLds <= 160 * 1024, "k_emit LDS");
static_assert(sizeof(sdb::SstSet) <= 4096, "SstSet is passed as kernel arguments");
