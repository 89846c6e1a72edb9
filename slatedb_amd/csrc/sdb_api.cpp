// sdb_api.cpp — the C ABI over device pointers (include/slatedb_amd.h): argument checks, workspace
// carving, launches; then the stage-timing diagnostics.  The handles that stage host buffers around these
// calls are in sdb_host.cpp and sdb_compactor.cpp.
//
// Host side of the drop-in for slatedb's EncodedSsTableBuilder / SsTableFormat::read_blocks
// (slatedb/src/sst_builder.rs:224-417, format/sst.rs:938-1038).  No CPU fallback: without a HIP
// device every compute entry point returns SDB_DEVICE_ERROR.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../../include/slatedb_amd.h"
#include "sdb_decode.h"
#include "sdb_bloom.h"
#include "sdb_compact.h"
#include "sdb_reads.h"
#include "sdb_replay.h"

using namespace sdb;

namespace {

inline hipStream_t S(void *s) { return reinterpret_cast<hipStream_t>(s); }

uint16_t num_probes_for(uint32_t bpk) { return (uint16_t)((float)bpk * 0.69f); }  // filter.rs:235-239

uint64_t filter_bytes_for(uint64_t n, uint32_t bpk) {  // filter.rs:65-69 (u32 arithmetic)
    uint32_t bits = (uint32_t)n * bpk;
    return bits / 8u + (bits % 8u != 0);
}

bool device_ok() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return false;
    return n > 0;
}

sdb_status check_params(const sdb_sst_params *p) {
    if (!p) return SDB_INVALID_ARGUMENT;
    if (p->sst_version != 1 && p->sst_version != 2) return SDB_INVALID_ARGUMENT;
    if (p->block_size == 0) return SDB_INVALID_ARGUMENT;
    if (p->sst_version == 2 && p->restart_interval == 0) return SDB_INVALID_ARGUMENT;
    if (p->sst_type > SDB_SST_WAL || (p->sst_type == SDB_SST_WAL && p->sst_version != 2)) return SDB_INVALID_ARGUMENT;
    if (p->prefix_kind > SDB_PREFIX_LENGTHS || (p->prefix_kind == SDB_PREFIX_DELIM && p->prefix_arg > 255))
        return SDB_INVALID_ARGUMENT;
    if (p->no_whole_key && p->prefix_kind == SDB_PREFIX_NONE) return SDB_INVALID_ARGUMENT;  // nothing to hash
    return SDB_OK;
}

}  // namespace

extern "C" {

uint32_t sdb_abi_version(void) { return SDB_ABI_VERSION; }

int sdb_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *sdb_status_name(int s) {
    switch (s) {
        case SDB_OK: return "OK";
        case SDB_EMPTY_KEY: return "EMPTY_KEY";
        case SDB_EMPTY_BLOCK: return "EMPTY_BLOCK";
        case SDB_CHECKSUM_MISMATCH: return "CHECKSUM_MISMATCH";
        case SDB_INVALID_ROW_FLAGS: return "INVALID_ROW_FLAGS";
        case SDB_INVALID_VERSION: return "INVALID_VERSION";
        case SDB_LIMIT_EXCEEDED: return "LIMIT_EXCEEDED";
        case SDB_UNSUPPORTED: return "UNSUPPORTED";
        case SDB_INVALID_ARGUMENT: return "INVALID_ARGUMENT";
        case SDB_CORRUPT_BLOCK: return "CORRUPT_BLOCK";
        case SDB_MERGE_OPERATOR_MISSING: return "MERGE_OPERATOR_MISSING";
        case SDB_DECOMPRESSION_ERROR: return "DECOMPRESSION_ERROR";
        case SDB_INVALID_SEQUENCE_ORDER: return "INVALID_SEQUENCE_ORDER";
        case SDB_MERGE_OPERATOR_ERROR: return "MERGE_OPERATOR_ERROR";
        case SDB_COMPACTION_FILTER_ERROR: return "COMPACTION_FILTER_ERROR";
        case SDB_DEVICE_ERROR: return "DEVICE_ERROR";
        default: return "UNKNOWN";
    }
}

uint64_t sdb_bloom_filter_bytes(uint64_t num_keys, uint32_t bits_per_key) {
    return filter_bytes_for(num_keys, bits_per_key);
}
uint32_t sdb_bloom_num_probes(uint32_t bits_per_key) { return num_probes_for(bits_per_key); }

sdb_status sdb_encode_bounds(uint64_t n, uint64_t total_key_bytes, uint64_t total_val_bytes,
                             const sdb_sst_params *params, uint64_t *data_cap, uint64_t *block_cap,
                             uint64_t *bloom_cap) {
    sdb_status st = check_params(params);
    if (st) return st;
    // every row <= 15 B of varints/headers + key + value + 25 B trailer; each entry may be its own
    // block (+2 offset +2 count +4 crc).  V0 rows: 4 + key + 9 + 16 + 4 + value, +2 offset.
    if (data_cap) *data_cap = total_key_bytes + total_val_bytes + 64 * n + 64;
    if (block_cap) *block_cap = n + 1;
    // a prefix-extractor filter holds up to one prefix hash per key besides the full-key hash
    const uint64_t hashes = (params->prefix_kind ? n : 0) + (params->no_whole_key ? 0 : n);
    if (bloom_cap)
        *bloom_cap = params->bloom_bits_per_key ? ((filter_bytes_for(hashes, params->bloom_bits_per_key) + 3) & ~3ull) + 16
                                                : 16;
    return SDB_OK;
}

}  // extern "C"

namespace {
// One SST's workspace region (256-byte multiple) inside a set's workspace: the encode's arrays, then the filter
// build's (the prefix filter's scratch, or the larger of the fused bloom's slots and the standalone build's).
// The 256 bytes after those are spare: they keep the public sizes what they have always been.
bool prefix_filter(const sdb_sst_params *p) { return p->prefix_kind != SDB_PREFIX_NONE || p->no_whole_key; }
uint64_t sst_ws_bytes(uint64_t n, const sdb_sst_params *p) {
    const uint64_t fixed = encode_ws_layout(n, nullptr);
    if (prefix_filter(p)) return fixed + prefix_workspace_bytes(n) + 256;
    const uint64_t fb = p->bloom_bits_per_key ? filter_bytes_for(n, p->bloom_bits_per_key) : 0;
    return fixed + (fb ? encode_bloom_workspace_bytes(n, num_probes_for(p->bloom_bits_per_key), fb) + 256 : 0);
}

sdb_status check_sst(const sdb_kv_batch *b, const sdb_sst_params *p, const sdb_sst_out *out) {
    if (!b || !out || !out->summary) return SDB_INVALID_ARGUMENT;
    const uint64_t n = b->n;
    if (n >= (1ull << 31)) return SDB_LIMIT_EXCEEDED;
    if (n && (!b->key_bytes || !b->key_off || !b->val_off)) return SDB_INVALID_ARGUMENT;
    const bool want_filter = p->sst_type != SDB_SST_WAL && p->bloom_bits_per_key > 0 && n >= p->min_filter_keys;
    const uint64_t hashes = prefix_filter(p) ? (p->prefix_kind ? n : 0) + (p->no_whole_key ? 0 : n) : n;
    const uint64_t fb = want_filter ? filter_bytes_for(hashes, p->bloom_bits_per_key) : 0;
    if (want_filter && fb && (!out->bloom || out->bloom_cap < fb)) return SDB_INVALID_ARGUMENT;
    if (want_filter && prefix_filter(p) && ((uintptr_t)out->bloom & 3)) return SDB_INVALID_ARGUMENT;
    if (want_filter && p->prefix_kind == SDB_PREFIX_LENGTHS && n && !b->prefix_len) return SDB_INVALID_ARGUMENT;
    if (n && (!out->data || !out->block_off || !out->block_first_entry || !out->index_key_len || !out->block_stats))
        return SDB_INVALID_ARGUMENT;
    return SDB_OK;
}

// The slot of one SST (no launches); *standalone_bloom: the filter needs the standalone build first.
SstSlot plan_slot(const sdb_kv_batch *b, const sdb_sst_params *p, const sdb_sst_out *out, uint8_t *ws,
                  bool *standalone_bloom) {
    const uint64_t n = b->n;
    const bool want_filter = p->sst_type != SDB_SST_WAL && p->bloom_bits_per_key > 0 && n >= p->min_filter_keys;
    const uint64_t fb = want_filter ? filter_bytes_for(n, p->bloom_bits_per_key) : 0;
    SstSlot s{};
    s.key_bytes = b->key_bytes;
    s.key_off = b->key_off;
    s.val_bytes = b->val_bytes;
    s.val_off = b->val_off;
    s.kind = b->kind;
    s.seq = b->seq;
    s.create_ts = b->create_ts;
    s.expire_ts = b->expire_ts;
    s.ts_mask = b->ts_mask;
    s.n = n;
    s.out_data = out->data;
    s.out_block_off = out->block_off;
    s.out_block_first = out->block_first_entry;
    s.out_index_key_len = out->index_key_len;
    s.out_block_stats = out->block_stats;
    s.data_cap = out->data_cap;
    s.block_cap = out->block_cap;
    s.summary = out->summary;
    s.bloom_out = out->bloom;
    s.bloom_len = fb;
    s.ws = ws;
    s.num_probes = want_filter ? num_probes_for(p->bloom_bits_per_key) : 0;
    s.filter_built = want_filter ? 1 : 0;
    s.nchunks = (uint32_t)((n + kChunk - 1) / kChunk);
    s.nfacts = (uint32_t)((n + kFactsEntries - 1) / kFactsEntries);
    encode_ws_layout(n, s.wso);
    {   // chunks per group: about sqrt(nchunks), so the chain walk (k_anchor, k_cut) takes ~2-3 sqrt(nchunks) table steps
        uint32_t g = 16;
        while ((uint64_t)g * g < s.nchunks) g++;
        s.group = g;
    }
    *standalone_bloom = false;
    if (want_filter && prefix_filter(p)) {  // device-counted size: built before the set (sdb_bloom.hip)
        s.prefix_bloom = 1;
        s.bloom_len = 0;
        *standalone_bloom = true;
    } else if (want_filter && n) {
        // the bloom is fused with the encode (k_facts hashes, binned per chunk) when the binned build
        // fits; otherwise the standalone build runs before the set
        const BloomPlan pl = bloom_plan(n, s.num_probes, fb, kChunk);
        if (bloom_plan_fits(pl)) {
            s.bloom_fused = 1;
            s.bpl = pl;
            s.slot_cap = bloom_slot_cap(pl);
        } else {
            *standalone_bloom = true;
        }
    }
    return s;
}

SstSet set_header(const sdb_sst_params *p) {
    SstSet P{};
    P.block_size = p->block_size;
    P.restart_interval = p->sst_version == 2 ? p->restart_interval : 1;
    P.version = p->sst_version;
    P.wal = p->sst_type == SDB_SST_WAL;
    // a block holds at most (block_size - 2) / 12 + 1 entries (smallest row: 12 bytes in V2, 13 in V1);
    // blocks longer than the lookahead continue from HBM inside k_seg
    const uint64_t look = (uint64_t)p->block_size / 12 + 2;
    P.seg_look = (uint32_t)(look < kSegLook ? look : kSegLook);
    return P;
}
}  // namespace

extern "C" {

uint64_t sdb_encode_workspace_bytes(uint64_t n, const sdb_sst_params *params) {
    if (!params) return 0;
    return sst_ws_bytes(n, params) + 256;
}

uint64_t sdb_encode_ssts_workspace_bytes(uint32_t count, const sdb_kv_batch *batches, const sdb_sst_params *params) {
    if (!params || (count && !batches)) return 0;
    uint64_t t = 256;
    for (uint32_t i = 0; i < count; i++) t += sst_ws_bytes(batches[i].n, params);
    return t;
}

sdb_status sdb_encode_ssts(uint32_t count, const sdb_kv_batch *batches, const sdb_sst_params *p,
                           const sdb_sst_out *outs, void *workspace, uint64_t workspace_bytes, void *stream) {
    sdb_status st = check_params(p);
    if (st) return st;
    if (count && (!batches || !outs)) return SDB_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < count; i++)
        if ((st = check_sst(&batches[i], p, &outs[i]))) return st;
    if (!device_ok()) return SDB_DEVICE_ERROR;
    if (!workspace || workspace_bytes < sdb_encode_ssts_workspace_bytes(count, batches, p)) return SDB_INVALID_ARGUMENT;
    hipStream_t s = S(stream);
    uint8_t *ws = ws_align(workspace);
    SstSet P = set_header(p);
    size_t bin_lds = 0, fill_lds = 0;
    auto flush = [&]() -> bool {
        const bool ok = launch_encode_set(P, bin_lds, fill_lds, s) == hipSuccess;
        SstSet q = set_header(p);
        P = q;
        bin_lds = fill_lds = 0;
        return ok;
    };
    for (uint32_t i = 0; i < count; i++) {
        bool standalone = false;
        const SstSlot slot = plan_slot(&batches[i], p, &outs[i], ws, &standalone);
        ws += sst_ws_bytes(batches[i].n, p);
        if (standalone) {
            SstSet one = set_header(p);
            one.count = 1;
            one.s[0] = slot;
            const EncodeArgs a = make_args(one, 0);
            stage_mark(s, kStBloom, true);
            hipError_t e;
            if (slot.prefix_bloom)
                e = launch_bloom_prefix(slot.key_bytes, slot.key_off, batches[i].prefix_len, slot.n, p->bloom_bits_per_key,
                                        p->prefix_kind, p->prefix_arg, p->no_whole_key ? 0 : 1, slot.bloom_out,
                                        outs[i].bloom_cap, (uint64_t *)a.bloom_len_dev, (uint8_t *)a.bq.count, s);
            else
                e = launch_bloom_build(slot.key_bytes, slot.key_off, slot.n, slot.num_probes, slot.bloom_out, slot.bloom_len,
                                       (uint8_t *)a.bq.count, s);
            if (e != hipSuccess) return SDB_DEVICE_ERROR;
            stage_mark(s, kStBloom, false);
        }
        if (!slot.n) {  // empty SST: summary only (a filter of an empty SST has no bytes)
            SstSet one = set_header(p);
            one.count = 1;
            one.s[0] = slot;
            if (launch_encode_empty(make_args(one, 0), s) != hipSuccess) return SDB_DEVICE_ERROR;
            continue;
        }
        P.s[P.count++] = slot;
        P.max_facts = std::max(P.max_facts, slot.nfacts);
        P.max_chunks = std::max(P.max_chunks, slot.nchunks);
        P.max_groups = std::max(P.max_groups, (slot.nchunks + slot.group - 1) / slot.group);
        if (slot.bloom_fused) {
            P.max_tiles = std::max(P.max_tiles, slot.bpl.tiles);
            P.max_slices = std::max(P.max_slices, slot.bpl.nslices);
            bin_lds = std::max(bin_lds, bloom_bin_lds(slot.bpl));
            fill_lds = std::max(fill_lds, bloom_fill_lds(slot.bpl));
        }
        if (P.count == kMaxSsts && !flush()) return SDB_DEVICE_ERROR;
    }
    if (P.count && !flush()) return SDB_DEVICE_ERROR;
    return SDB_OK;
}

uint64_t sdb_bloom_workspace_bytes(uint64_t n, uint32_t bits_per_key) {
    return bloom_workspace_bytes(n, num_probes_for(bits_per_key), filter_bytes_for(n, bits_per_key)) + 256;
}

sdb_status sdb_encode_sst(const sdb_kv_batch *b, const sdb_sst_params *p, const sdb_sst_out *out,
                          void *workspace, uint64_t workspace_bytes, void *stream) {
    if (!b || !out) return SDB_INVALID_ARGUMENT;
    return sdb_encode_ssts(1, b, p, out, workspace, workspace_bytes, stream);
}

sdb_status sdb_bloom_build(const uint8_t *key_bytes, const uint64_t *key_off, uint64_t n,
                           uint32_t bits_per_key, uint8_t *bitmap, uint64_t bitmap_bytes, void *workspace,
                           uint64_t workspace_bytes, void *stream) {
    if (!device_ok()) return SDB_DEVICE_ERROR;
    uint64_t fb = filter_bytes_for(n, bits_per_key);
    if (bitmap_bytes < fb || (fb && !bitmap) || (n && (!key_bytes || !key_off))) return SDB_INVALID_ARGUMENT;
    // the build writes 32-bit words: a 4-byte aligned bitmap, and (atomic path, no workspace) room for
    // the word that holds the last byte
    if (((uintptr_t)bitmap & 3) || (!workspace && fb && bitmap_bytes < ((fb + 3) & ~3ull))) return SDB_INVALID_ARGUMENT;
    if (workspace && workspace_bytes < sdb_bloom_workspace_bytes(n, bits_per_key)) return SDB_INVALID_ARGUMENT;
    if (launch_bloom_build(key_bytes, key_off, n, num_probes_for(bits_per_key), bitmap, fb, ws_align(workspace), S(stream)) != hipSuccess)
        return SDB_DEVICE_ERROR;
    return SDB_OK;
}

uint64_t sdb_bloom_prefix_workspace_bytes(uint64_t n) { return prefix_workspace_bytes(n) + 256; }

sdb_status sdb_bloom_build_prefix(const uint8_t *key_bytes, const uint64_t *key_off, const int32_t *prefix_len,
                                  uint64_t n, uint32_t bits_per_key, uint32_t prefix_kind, uint32_t prefix_arg,
                                  uint32_t whole_key, uint8_t *bitmap, uint64_t bitmap_cap, uint64_t *bloom_len,
                                  void *workspace, uint64_t workspace_bytes, void *stream) {
    if (!device_ok()) return SDB_DEVICE_ERROR;
    if (prefix_kind > SDB_PREFIX_LENGTHS || (prefix_kind == SDB_PREFIX_NONE && !whole_key) || !bloom_len ||
        (n && (!key_bytes || !key_off)) || (prefix_kind == SDB_PREFIX_LENGTHS && n && !prefix_len) ||
        (prefix_kind == SDB_PREFIX_DELIM && prefix_arg > 255) || !bitmap || ((uintptr_t)bitmap & 3) ||
        !workspace || workspace_bytes < sdb_bloom_prefix_workspace_bytes(n))
        return SDB_INVALID_ARGUMENT;
    if (launch_bloom_prefix(key_bytes, key_off, prefix_len, n, bits_per_key, prefix_kind, prefix_arg, whole_key ? 1 : 0,
                            bitmap, bitmap_cap, bloom_len, ws_align(workspace), S(stream)) != hipSuccess)
        return SDB_DEVICE_ERROR;
    return SDB_OK;
}

sdb_status sdb_bloom_might_match(const uint8_t *bitmap, uint64_t bitmap_bytes, uint32_t num_probes, uint32_t whole_key,
                                 uint32_t prefix_kind, uint32_t prefix_arg, const uint8_t *key_bytes,
                                 const uint64_t *key_off, const uint8_t *is_prefix, const int32_t *query_prefix_len,
                                 uint64_t n, uint8_t *result, void *stream) {
    if (!device_ok()) return SDB_DEVICE_ERROR;
    if (prefix_kind > SDB_PREFIX_LENGTHS || (n && (!key_bytes || !key_off || !result)) ||
        (prefix_kind == SDB_PREFIX_LENGTHS && n && !query_prefix_len) || (bitmap_bytes && !bitmap))
        return SDB_INVALID_ARGUMENT;
    if (launch_bloom_match(bitmap, bitmap_bytes, num_probes, whole_key ? 1 : 0, prefix_kind, prefix_arg, key_bytes, key_off,
                           is_prefix, query_prefix_len, n, result, S(stream)) != hipSuccess)
        return SDB_DEVICE_ERROR;
    return SDB_OK;
}

sdb_status sdb_bloom_might_contain(const uint8_t *bitmap, uint64_t bitmap_bytes, uint32_t num_probes,
                                   const uint8_t *key_bytes, const uint64_t *key_off, uint64_t n,
                                   uint8_t *result, void *stream) {
    if (!device_ok()) return SDB_DEVICE_ERROR;
    if (n && (!key_bytes || !key_off || !result)) return SDB_INVALID_ARGUMENT;
    if (launch_bloom_query(bitmap, bitmap_bytes, num_probes, key_bytes, key_off, n, result, S(stream)) != hipSuccess)
        return SDB_DEVICE_ERROR;
    return SDB_OK;
}

uint64_t sdb_decode_workspace_bytes(uint64_t nblocks) {
    DecodeArgs a{};
    a.nblocks = nblocks;
    return decode_bind(a, nullptr);
}

static sdb_status decode_common(const uint8_t *blocks, const uint64_t *block_off, const uint64_t *block_end,
                                uint64_t nblocks, uint16_t sst_version, const sdb_decoded_out *out, void *workspace,
                                uint64_t workspace_bytes, void *stream, uint32_t flags = 0) {
    if (!out || !out->summary || !out->block_entry_start) return SDB_INVALID_ARGUMENT;
    if (sst_version != 1 && sst_version != 2) return SDB_INVALID_VERSION;  // block_iterator.rs:60-77
    if (nblocks && (!blocks || !block_off)) return SDB_INVALID_ARGUMENT;
    if (!device_ok()) return SDB_DEVICE_ERROR;
    if (!workspace || workspace_bytes < sdb_decode_workspace_bytes(nblocks)) return SDB_INVALID_ARGUMENT;
    DecodeArgs a{};
    a.blocks = blocks;
    a.block_off = block_off;
    a.block_end = block_end;
    a.nblocks = nblocks;
    a.version = sst_version;
    a.descending = (flags & SDB_DECODE_DESCENDING) ? 1u : 0u;
    a.fail_fast = (flags & SDB_DECODE_FAIL_FAST) ? 1u : 0u;
    a.out = *out;
    decode_bind(a, ws_align(workspace));
    a.bad_block = out->bad_block;
    a.bad_cap = out->bad_cap;
    if (launch_decode(a, S(stream)) != hipSuccess) return SDB_DEVICE_ERROR;
    return SDB_OK;
}

sdb_status sdb_decode_blocks(const uint8_t *blocks, const uint64_t *block_off, uint64_t nblocks,
                             uint16_t sst_version, const sdb_decoded_out *out, void *workspace,
                             uint64_t workspace_bytes, void *stream) {
    return decode_common(blocks, block_off, nullptr, nblocks, sst_version, out, workspace, workspace_bytes, stream);
}

sdb_status sdb_decode_blocks_ex(const uint8_t *arena, const uint64_t *block_start, const uint64_t *block_end,
                                uint64_t nblocks, uint16_t sst_version, uint32_t flags, const sdb_decoded_out *out,
                                void *workspace, uint64_t workspace_bytes, void *stream) {
    if (flags & ~(uint32_t)(SDB_DECODE_DESCENDING | SDB_DECODE_FAIL_FAST)) return SDB_INVALID_ARGUMENT;
    if (block_end && nblocks && !block_start) return SDB_INVALID_ARGUMENT;
    return decode_common(arena, block_start, block_end, nblocks, sst_version, out, workspace, workspace_bytes, stream,
                         flags);
}

sdb_status sdb_decode_blocks_at(const uint8_t *arena, const uint64_t *block_start, const uint64_t *block_end,
                                uint64_t nblocks, uint16_t sst_version, const sdb_decoded_out *out,
                                void *workspace, uint64_t workspace_bytes, void *stream) {
    if (nblocks && !block_end) return SDB_INVALID_ARGUMENT;
    return decode_common(arena, block_start, block_end, nblocks, sst_version, out, workspace, workspace_bytes, stream);
}

uint64_t sdb_decompress_workspace_bytes(uint64_t nblocks) { return decompress_workspace_bytes(nblocks) + 256; }

static bool lz_codec(uint32_t codec) {  // every compressing codec of CompressionCodec (format/sst.rs:884-917)
    return codec == SDB_CODEC_LZ4 || codec == SDB_CODEC_SNAPPY || codec == SDB_CODEC_ZLIB || codec == SDB_CODEC_ZSTD;
}

sdb_status sdb_decompress_plan(uint32_t codec, const uint8_t *blocks, const uint64_t *block_off, uint64_t nblocks,
                               uint64_t *out_start, void *workspace, uint64_t workspace_bytes, void *stream) {
    if (!lz_codec(codec)) return SDB_INVALID_ARGUMENT;
    if (!out_start || (nblocks && (!blocks || !block_off))) return SDB_INVALID_ARGUMENT;
    if (!workspace || workspace_bytes < sdb_decompress_workspace_bytes(nblocks)) return SDB_INVALID_ARGUMENT;
    if (!device_ok()) return SDB_DEVICE_ERROR;
    return launch_decompress_plan(codec, blocks, block_off, nblocks, out_start, ws_align(workspace), S(stream)) == hipSuccess
               ? SDB_OK : SDB_DEVICE_ERROR;
}

sdb_status sdb_decompress_blocks(uint32_t codec, const uint8_t *blocks, const uint64_t *block_off, uint64_t nblocks,
                                 uint8_t *out, uint64_t out_cap, const uint64_t *out_start, uint64_t *out_end,
                                 uint64_t *err, void *stream) {
    if (!lz_codec(codec)) return SDB_INVALID_ARGUMENT;
    if (!err || !out_start || (nblocks && (!blocks || !block_off || !out_end || (out_cap && !out)))) return SDB_INVALID_ARGUMENT;
    if (!device_ok()) return SDB_DEVICE_ERROR;
    return launch_decompress_run(codec, blocks, block_off, nblocks, out, out_cap, out_start, out_end,
                                 (unsigned long long *)err, S(stream)) == hipSuccess ? SDB_OK : SDB_DEVICE_ERROR;
}

uint64_t sdb_decompress_once_workspace_bytes(uint64_t nblocks) { return decompress_once_workspace_bytes(nblocks) + 256; }

sdb_status sdb_decompress_blocks_once(uint32_t codec, const uint8_t *blocks, const uint64_t *block_off, uint64_t nblocks,
                                      uint64_t slot_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_start,
                                      uint64_t *out_end, uint64_t *err, void *workspace, uint64_t workspace_bytes,
                                      void *stream) {
    if (!lz_codec(codec)) return SDB_INVALID_ARGUMENT;
    if (!err || !out_start || (nblocks && (!blocks || !block_off || !out_end || (out_cap && !out)))) return SDB_INVALID_ARGUMENT;
    if (!workspace || workspace_bytes < sdb_decompress_once_workspace_bytes(nblocks)) return SDB_INVALID_ARGUMENT;
    if (codec == SDB_CODEC_ZLIB && (slot_bytes < 8 || slot_bytes > (1ull << 32) ||
                                    (nblocks && out_cap / nblocks < slot_bytes)))
        return SDB_INVALID_ARGUMENT;
    if (!device_ok()) return SDB_DEVICE_ERROR;
    return launch_decompress_once(codec, blocks, block_off, nblocks, slot_bytes, out, out_cap, out_start, out_end,
                                  (unsigned long long *)err, ws_align(workspace), S(stream)) == hipSuccess ? SDB_OK
                                                                                                 : SDB_DEVICE_ERROR;
}

uint64_t sdb_compress_workspace_bytes(uint64_t nblocks, uint64_t in_bytes) {
    return compress_workspace_bytes(nblocks, in_bytes) + 256;
}

sdb_status sdb_compress_blocks(uint32_t codec, const uint8_t *blocks, const uint64_t *block_off, uint64_t nblocks,
                               uint64_t in_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint64_t *err,
                               void *workspace, uint64_t workspace_bytes, void *stream) {
    if (!lz_codec(codec)) return SDB_INVALID_ARGUMENT;
    if (!out_off || !err || (nblocks && (!blocks || !block_off || (out_cap && !out)))) return SDB_INVALID_ARGUMENT;
    if (!workspace || workspace_bytes < sdb_compress_workspace_bytes(nblocks, in_bytes)) return SDB_INVALID_ARGUMENT;
    if (!device_ok()) return SDB_DEVICE_ERROR;
    return launch_compress(codec, blocks, block_off, nblocks, in_bytes, out, out_cap, out_off,
                           (unsigned long long *)err, ws_align(workspace), S(stream)) == hipSuccess ? SDB_OK : SDB_DEVICE_ERROR;
}

uint64_t sdb_merge_runs_workspace_bytes(const sdb_run *runs, uint32_t nruns) {
    if (nruns && !runs) return 0;
    MergeArgs a{};
    for (uint32_t r = 0; r < nruns; r++) a.total += runs[r].n;
    return merge_bind(a, nullptr) + 256;
}

sdb_status sdb_merge_runs(const sdb_run *runs, uint32_t nruns, const sdb_retention *ret, const sdb_merged_out *out,
                          void *workspace, uint64_t workspace_bytes, void *stream) {
    MergeArgs a;
    sdb_status st = build_merge_args(runs, nruns, ret, out, workspace, workspace_bytes, &a);
    if (st) return st;
    if (!device_ok()) return SDB_DEVICE_ERROR;
    if (launch_merge(a, true, S(stream)) != hipSuccess) return SDB_DEVICE_ERROR;
    return SDB_OK;
}

uint64_t sdb_sst_cuts_workspace_bytes(uint64_t n, const sdb_sst_params *params) {
    if (!params) return 0;
    sdb_sst_params p = *params;
    p.bloom_bits_per_key = 0;
    p.prefix_kind = SDB_PREFIX_NONE;
    p.no_whole_key = 0;
    return sst_ws_bytes(n, &p) + 512 + 256;
}

sdb_status sdb_sst_cuts(const sdb_kv_batch *batch, const sdb_sst_params *params, uint64_t max_sst_size,
                        uint64_t *cut_start, uint64_t cut_cap, uint64_t *num_ssts, void *workspace,
                        uint64_t workspace_bytes, void *stream) {
    return sst_cuts_padded(batch, params, max_sst_size, cut_start, cut_cap, num_ssts, workspace, workspace_bytes,
                           S(stream), nullptr);
}

}  // extern "C"

namespace sdb {
sdb_status sst_cuts_padded(const sdb_kv_batch *batch, const sdb_sst_params *params, uint64_t max_sst_size,
                           uint64_t *cut_start, uint64_t cut_cap, uint64_t *num_ssts, void *workspace,
                           uint64_t workspace_bytes, hipStream_t s, const uint64_t *n_real) {
    if (!batch || !params || !cut_start || !num_ssts) return SDB_INVALID_ARGUMENT;
    sdb_sst_params p = *params;  // the chain only: no filter
    p.bloom_bits_per_key = 0;
    p.prefix_kind = SDB_PREFIX_NONE;
    p.no_whole_key = 0;
    sdb_status st = check_params(&p);
    if (st) return st;
    const uint64_t n = batch->n;
    if (n >= (1ull << 31)) return SDB_LIMIT_EXCEEDED;
    if (cut_cap < n + 1 || (n && (!batch->key_bytes || !batch->key_off || !batch->val_off))) return SDB_INVALID_ARGUMENT;
    if (!device_ok()) return SDB_DEVICE_ERROR;
    if (!workspace || workspace_bytes < sdb_sst_cuts_workspace_bytes(n, params)) return SDB_INVALID_ARGUMENT;
    uint8_t *ws = ws_align(workspace);
    if (!n) {
        if (hipMemsetAsync(cut_start, 0, 8, s) != hipSuccess || hipMemsetAsync(num_ssts, 0, 8, s) != hipSuccess)
            return SDB_DEVICE_ERROR;
        return SDB_OK;
    }
    // the prep kernels write an SST summary: a scratch one after the encode workspace
    sdb_sst_summary *scratch = (sdb_sst_summary *)(ws + sst_ws_bytes(n, &p));
    sdb_sst_out out{};
    out.data_cap = ~0ull;
    out.block_cap = ~0ull;
    out.summary = scratch;
    bool standalone = false;
    SstSet P = set_header(&p);
    P.s[0] = plan_slot(batch, &p, &out, ws, &standalone);
    P.count = 1;
    P.max_facts = P.s[0].nfacts;
    P.max_chunks = P.s[0].nchunks;
    P.max_groups = (P.s[0].nchunks + P.s[0].group - 1) / P.s[0].group;
    if (launch_cuts(P, max_sst_size, cut_start, cut_cap, num_ssts, s, n_real) != hipSuccess) return SDB_DEVICE_ERROR;
    return SDB_OK;
}
}  // namespace sdb

namespace {
// What the read entry points check of their shared arguments (each after its own NULL checks).  A check that
// returns another status than its neighbours stays where it was in each entry point, so every combination of
// arguments gets the status it always got.
sdb_status check_view(const sdb_sst_view *sst) {
    if (sst->sst_version != 1 && sst->sst_version != 2) return SDB_INVALID_VERSION;
    if (sst->num_blocks >= 0xFFFFFFFFull) return SDB_LIMIT_EXCEEDED;
    if (sst->num_blocks && (!sst->data || !sst->block_off || !sst->index_keys || !sst->index_key_off))
        return SDB_INVALID_ARGUMENT;
    return SDB_OK;
}
sdb_status check_tree(const sdb_lsm_view *lsm) {
    if (lsm->total_blocks >= 0xFFFFFFFFull || lsm->num_ssts == 0xFFFFFFFFu) return SDB_LIMIT_EXCEEDED;
    if (lsm->num_ssts && (!lsm->ssts || !lsm->run_start || !lsm->first_key_off || !lsm->last_key_off ||
                          !lsm->block_base || !lsm->first_key_bytes || !lsm->last_key_bytes))
        return SDB_INVALID_ARGUMENT;
    return SDB_OK;
}
sdb_status check_ranges(const sdb_scan_ranges *r) {
    if (r->n && (!r->start_bytes || !r->start_off || !r->start_kind || !r->end_bytes || !r->end_off || !r->end_kind))
        return SDB_INVALID_ARGUMENT;
    return SDB_OK;
}
}  // namespace

extern "C" {

uint64_t sdb_sst_lookup_workspace_bytes(uint64_t num_blocks, uint64_t nkeys) {
    return lookup_workspace_bytes(num_blocks, nkeys) + 256;
}

sdb_status sdb_sst_lookup(const sdb_sst_view *sst, const uint8_t *key_bytes, const uint64_t *key_off,
                          uint64_t nkeys, int32_t descending, const sdb_lookup_out *out, void *workspace,
                          uint64_t workspace_bytes, void *stream) {
    if (!sst || !out) return SDB_INVALID_ARGUMENT;
    sdb_status st = check_view(sst);
    if (st) return st;
    if (nkeys && (!key_bytes || !key_off || !out->state || !out->status || !out->block || !out->entry ||
                  !out->key_len || !out->val_off || !out->val_len || !out->seq || !out->flags || !out->create_ts ||
                  !out->expire_ts))
        return SDB_INVALID_ARGUMENT;
    if (!device_ok()) return SDB_DEVICE_ERROR;
    if (!workspace || workspace_bytes < sdb_sst_lookup_workspace_bytes(sst->num_blocks, nkeys)) return SDB_INVALID_ARGUMENT;
    uint8_t *w = ws_align(workspace);
    if (launch_lookup(*sst, key_bytes, key_off, nkeys, descending ? 1u : 0u, *out, w, S(stream)) != hipSuccess)
        return SDB_DEVICE_ERROR;
    return SDB_OK;
}

uint64_t sdb_sst_scan_workspace_bytes(uint64_t num_blocks, uint64_t nranges) {
    return scan_workspace_bytes(num_blocks, nranges) + 256;
}

sdb_status sdb_sst_scan(const sdb_sst_view *sst, const sdb_scan_ranges *ranges, int32_t descending,
                        const sdb_scan_out *out, void *workspace, uint64_t workspace_bytes, void *stream) {
    if (!sst || !ranges || !out) return SDB_INVALID_ARGUMENT;
    sdb_status st = check_view(sst);
    if (st) return st;
    const uint64_t n = ranges->n;
    if (!out->summary || !out->range_entry_start || check_ranges(ranges)) return SDB_INVALID_ARGUMENT;
    if (n && (!out->range_block || !out->range_status)) return SDB_INVALID_ARGUMENT;
    if (!out->key_off || (out->key_arena_cap && !out->key_arena)) return SDB_INVALID_ARGUMENT;
    if (out->cap_entries && (!out->val_off || !out->val_len || !out->seq || !out->flags || !out->create_ts ||
                             !out->expire_ts))
        return SDB_INVALID_ARGUMENT;
    if (!workspace || workspace_bytes < sdb_sst_scan_workspace_bytes(sst->num_blocks, n)) return SDB_INVALID_ARGUMENT;
    if (!device_ok()) {  // no device: the arrays are host memory, so the kinds can be checked here
        for (uint64_t r = 0; r < n; r++)
            if (ranges->start_kind[r] > SDB_BOUND_EXCLUDED || ranges->end_kind[r] > SDB_BOUND_EXCLUDED)
                return SDB_INVALID_ARGUMENT;
        return SDB_DEVICE_ERROR;
    }
    uint8_t *w = ws_align(workspace);
    if (launch_scan(*sst, *ranges, descending ? 1u : 0u, *out, w, S(stream)) != hipSuccess) return SDB_DEVICE_ERROR;
    return SDB_OK;
}

// NULL: nothing missing.  The CSR offsets and the summary always, the link columns where there is room for a link.
static bool chain_ok(const sdb_chain_out *c) {
    if (!c || !c->chain_start || !c->summary) return false;
    return !c->cap_links || (c->sst && c->block && c->val_off && c->val_len && c->seq && c->flags && c->create_ts &&
                             c->expire_ts);
}

// The projections of a projected tree read (P5): one per SST, every array there when there is an SST.
static sdb_status check_projections(const sdb_lsm_view *lsm, const sdb_scan_ranges *proj) {
    if (!proj) return SDB_OK;
    if (proj->n != lsm->num_ssts) return SDB_INVALID_ARGUMENT;
    return check_ranges(proj);
}

// The five gets: one set of argument checks, in one order, over the descriptor its entry point filled (sdb_reads.h).
static sdb_status lsm_get_call(const GetCall &c, void *workspace, uint64_t workspace_bytes, void *stream) {
    const sdb_lsm_view *lsm = c.lsm;
    const sdb_get_out *out = c.out;
    const uint64_t nkeys = c.nkeys;
    if (!lsm || !out || (c.merge && !c.chain)) return SDB_INVALID_ARGUMENT;
    const uint32_t ntab = c.mem ? c.mem->num_tables : 0;
    if (c.layers && (!c.mout || (c.chain != nullptr) != (c.mchain != nullptr) || (ntab && !c.mem->tables)))
        return SDB_INVALID_ARGUMENT;
    // (the limits all give one status, so this one may come before the tree's)
    const uint64_t per_key = (uint64_t)lsm->num_runs + ntab;  // a byte per (query, run), a record per (query, table)
    if (per_key && nkeys > (1ull << 40) / per_key) return SDB_LIMIT_EXCEEDED;
    sdb_status st = check_tree(lsm);
    if (st) return st;
    if (check_projections(lsm, c.proj)) return SDB_INVALID_ARGUMENT;
    if (!out->summary || (c.merge && !chain_ok(c.chain))) return SDB_INVALID_ARGUMENT;
    if (nkeys && (!c.key_bytes || !c.key_off || !out->state || !out->status || !out->sst || !out->block || !out->val_off ||
                  !out->val_len || !out->seq || !out->flags || !out->create_ts || !out->expire_ts || !out->ssts_read ||
                  !out->ssts_filtered))
        return SDB_INVALID_ARGUMENT;
    if (c.layers && ((nkeys && (!c.mout->table || !c.mout->row)) ||
                     (c.merge && c.chain->cap_links && (!c.mchain->table || !c.mchain->row))))
        return SDB_INVALID_ARGUMENT;
    const uint64_t need = get_workspace_bytes({.num_tables = ntab, .total_blocks = lsm->total_blocks, .num_ssts = lsm->num_ssts,
                                               .num_runs = lsm->num_runs, .n = nkeys, .merge = c.merge});
    if (!workspace || workspace_bytes < need + 256) return SDB_INVALID_ARGUMENT;
    if (!device_ok()) return SDB_DEVICE_ERROR;
    return launch_get(c, ws_align(workspace), S(stream)) != hipSuccess ? SDB_DEVICE_ERROR : SDB_OK;
}

uint64_t sdb_lsm_get_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs, uint64_t nkeys) {
    return get_workspace_bytes({.total_blocks = total_blocks, .num_ssts = num_ssts, .num_runs = num_runs, .n = nkeys}) + 256;
}

sdb_status sdb_lsm_get(const sdb_lsm_view *lsm, const uint8_t *key_bytes, const uint64_t *key_off, uint64_t nkeys,
                       const uint64_t *max_seq, const sdb_get_out *out, void *workspace, uint64_t workspace_bytes,
                       void *stream) {
    return lsm_get_call({.lsm = lsm, .key_bytes = key_bytes, .key_off = key_off, .nkeys = nkeys, .max_seq = max_seq, .out = out},
                        workspace, workspace_bytes, stream);
}

uint64_t sdb_lsm_get_merge_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs, uint64_t nkeys) {
    return get_workspace_bytes({.total_blocks = total_blocks, .num_ssts = num_ssts, .num_runs = num_runs, .n = nkeys,
                                .merge = true}) + 256;
}

sdb_status sdb_lsm_get_merge(const sdb_lsm_view *lsm, const uint8_t *key_bytes, const uint64_t *key_off, uint64_t nkeys,
                             const uint64_t *max_seq, const sdb_get_out *out, const sdb_chain_out *chain, void *workspace,
                             uint64_t workspace_bytes, void *stream) {
    return lsm_get_call({.lsm = lsm, .key_bytes = key_bytes, .key_off = key_off, .nkeys = nkeys, .max_seq = max_seq, .out = out,
                         .chain = chain, .merge = true},
                        workspace, workspace_bytes, stream);
}

uint64_t sdb_lsm_get_filtered_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs, uint64_t nkeys,
                                              int32_t merge) {
    return get_workspace_bytes({.total_blocks = total_blocks, .num_ssts = num_ssts, .num_runs = num_runs, .n = nkeys,
                                .merge = merge != 0}) + 256;
}

sdb_status sdb_lsm_get_filtered(const sdb_lsm_view *lsm, const sdb_filter_policy *policies, const uint8_t *key_bytes,
                                const uint64_t *key_off, uint64_t nkeys, const int32_t *probe_len, const uint64_t *max_seq,
                                const sdb_get_out *out, const sdb_chain_out *chain, void *workspace, uint64_t workspace_bytes,
                                void *stream) {
    return lsm_get_call({.lsm = lsm, .pol = policies, .key_bytes = key_bytes, .key_off = key_off, .nkeys = nkeys,
                         .probe_len = probe_len, .max_seq = max_seq, .out = out, .chain = chain, .merge = chain != nullptr},
                        workspace, workspace_bytes, stream);
}

uint64_t sdb_lsm_get_projected_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs, uint64_t nkeys,
                                               int32_t merge) {
    // a projection needs no state
    return sdb_lsm_get_filtered_workspace_bytes(total_blocks, num_ssts, num_runs, nkeys, merge);
}

sdb_status sdb_lsm_get_projected(const sdb_lsm_view *lsm, const sdb_scan_ranges *proj, const sdb_filter_policy *policies,
                                 const uint8_t *key_bytes, const uint64_t *key_off, uint64_t nkeys, const int32_t *probe_len,
                                 const uint64_t *max_seq, const sdb_get_out *out, const sdb_chain_out *chain, void *workspace,
                                 uint64_t workspace_bytes, void *stream) {
    return lsm_get_call({.lsm = lsm, .proj = proj, .pol = policies, .key_bytes = key_bytes, .key_off = key_off, .nkeys = nkeys,
                         .probe_len = probe_len, .max_seq = max_seq, .out = out, .chain = chain, .merge = chain != nullptr},
                        workspace, workspace_bytes, stream);
}

uint64_t sdb_lsm_get_mem_workspace_bytes(uint32_t num_tables, uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs,
                                         uint64_t nkeys, int32_t merge) {
    return get_workspace_bytes({.num_tables = num_tables, .total_blocks = total_blocks, .num_ssts = num_ssts,
                                .num_runs = num_runs, .n = nkeys, .merge = merge != 0}) + 256;
}

sdb_status sdb_lsm_get_mem(const sdb_mem_view *mem, const sdb_lsm_view *lsm, const sdb_scan_ranges *proj,
                           const sdb_filter_policy *policies, const uint8_t *key_bytes, const uint64_t *key_off, uint64_t nkeys,
                           const int32_t *probe_len, const uint64_t *max_seq, const sdb_get_out *out,
                           const sdb_mem_get_out *mout, const sdb_chain_out *chain, const sdb_mem_chain_out *mchain,
                           void *workspace, uint64_t workspace_bytes, void *stream) {
    return lsm_get_call({.mem = mem, .lsm = lsm, .proj = proj, .pol = policies, .key_bytes = key_bytes, .key_off = key_off,
                         .nkeys = nkeys, .probe_len = probe_len, .max_seq = max_seq, .out = out, .mout = mout, .chain = chain,
                         .mchain = mchain, .merge = chain != nullptr, .layers = true},
                        workspace, workspace_bytes, stream);
}

// The six scans: one set of argument checks, in one order, over the descriptor its entry point filled (sdb_reads.h).
static sdb_status lsm_scan_call(const ScanCall &c, void *workspace, uint64_t workspace_bytes, void *stream) {
    const sdb_lsm_view *lsm = c.lsm;
    const sdb_lsm_scan_out *out = c.out;
    if (!lsm || !c.ranges || !out || (c.merge && !c.chain) || (c.filter && !c.fout)) return SDB_INVALID_ARGUMENT;
    const uint32_t ntab = c.mem ? c.mem->num_tables : 0;
    if (c.layers && (!c.mout || (c.chain != nullptr) != (c.mchain != nullptr) || (ntab && !c.mem->tables)))
        return SDB_INVALID_ARGUMENT;
    if (c.recency && !c.rout) return SDB_INVALID_ARGUMENT;
    const uint64_t n = c.ranges->n;
    // (the limits all give one status, so these may come before the tree's)
    const uint64_t per_range = (uint64_t)lsm->num_ssts + ntab;  // per (range, source) state
    if (per_range && n > (1ull << 40) / per_range) return SDB_LIMIT_EXCEEDED;
    if (c.cand_entries > (1ull << 40) || c.cand_key_bytes > (1ull << 44)) return SDB_LIMIT_EXCEEDED;
    sdb_status st = check_tree(lsm);
    if (st) return st;
    if (check_projections(lsm, c.proj)) return SDB_INVALID_ARGUMENT;
    if (!out->summary || !out->range_entry_start || !out->key_off || check_ranges(c.ranges)) return SDB_INVALID_ARGUMENT;
    if (n && (!out->range_status || !out->range_ssts)) return SDB_INVALID_ARGUMENT;
    if (out->key_arena_cap && !out->key_arena) return SDB_INVALID_ARGUMENT;
    if (out->cap_entries && (!out->sst || !out->val_off || !out->val_len || !out->seq || !out->flags ||
                             !out->create_ts || !out->expire_ts))
        return SDB_INVALID_ARGUMENT;
    if (c.merge && !chain_ok(c.chain)) return SDB_INVALID_ARGUMENT;
    if (c.filter && n && (!c.fout->range_filtered || !c.fout->num_filtered)) return SDB_INVALID_ARGUMENT;
    if (c.filter && n && c.prefixes && (!c.prefixes->prefix_bytes || !c.prefixes->prefix_off || !c.prefixes->has_prefix))
        return SDB_INVALID_ARGUMENT;
    if (c.layers && ((n && !c.mout->range_tables) || (out->cap_entries && (!c.mout->table || !c.mout->row)) ||
                     (c.merge && c.chain->cap_links && (!c.mchain->table || !c.mchain->row))))
        return SDB_INVALID_ARGUMENT;
    if (c.recency && n && (!c.rout->range_sources_read || !c.rout->range_visible)) return SDB_INVALID_ARGUMENT;
    const uint64_t need = lsm_scan_workspace_bytes({.num_tables = ntab, .total_blocks = lsm->total_blocks,
                                                    .num_ssts = lsm->num_ssts, .n = n, .cand_entries = c.cand_entries,
                                                    .cand_key_bytes = c.cand_key_bytes, .merge = c.merge, .filter = c.filter,
                                                    .recency = c.recency});
    if (!workspace || workspace_bytes < need + 256) return SDB_INVALID_ARGUMENT;
    if (!device_ok()) return SDB_DEVICE_ERROR;
    return launch_lsm_scan(c, ws_align(workspace), S(stream)) != hipSuccess ? SDB_DEVICE_ERROR : SDB_OK;
}

// (runs only fix the search order: a scan's workspace is per (range, SST), so the sizers ignore num_runs)
uint64_t sdb_lsm_scan_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs, uint64_t nranges,
                                      uint64_t cand_entries, uint64_t cand_key_bytes) {
    (void)num_runs;
    return lsm_scan_workspace_bytes({.total_blocks = total_blocks, .num_ssts = num_ssts, .n = nranges,
                                     .cand_entries = cand_entries, .cand_key_bytes = cand_key_bytes}) + 256;
}

sdb_status sdb_lsm_scan(const sdb_lsm_view *lsm, const sdb_scan_ranges *ranges, const uint64_t *max_seq,
                        int32_t descending, uint64_t cand_entries, uint64_t cand_key_bytes, const sdb_lsm_scan_out *out,
                        void *workspace, uint64_t workspace_bytes, void *stream) {
    return lsm_scan_call({.lsm = lsm, .ranges = ranges, .max_seq = max_seq, .desc = descending ? 1u : 0u,
                          .cand_entries = cand_entries, .cand_key_bytes = cand_key_bytes, .out = out},
                         workspace, workspace_bytes, stream);
}

uint64_t sdb_lsm_scan_merge_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs,
                                            uint64_t nranges, uint64_t cand_entries, uint64_t cand_key_bytes) {
    (void)num_runs;
    return lsm_scan_workspace_bytes({.total_blocks = total_blocks, .num_ssts = num_ssts, .n = nranges,
                                     .cand_entries = cand_entries, .cand_key_bytes = cand_key_bytes, .merge = true}) + 256;
}

sdb_status sdb_lsm_scan_merge(const sdb_lsm_view *lsm, const sdb_scan_ranges *ranges, const uint64_t *max_seq,
                              int32_t descending, uint64_t cand_entries, uint64_t cand_key_bytes,
                              const sdb_lsm_scan_out *out, const sdb_chain_out *chain, void *workspace,
                              uint64_t workspace_bytes, void *stream) {
    return lsm_scan_call({.lsm = lsm, .ranges = ranges, .max_seq = max_seq, .desc = descending ? 1u : 0u,
                          .cand_entries = cand_entries, .cand_key_bytes = cand_key_bytes, .out = out, .chain = chain,
                          .merge = true},
                         workspace, workspace_bytes, stream);
}

uint64_t sdb_lsm_scan_filtered_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs,
                                               uint64_t nranges, uint64_t cand_entries, uint64_t cand_key_bytes,
                                               int32_t merge) {
    (void)num_runs;
    return lsm_scan_workspace_bytes({.total_blocks = total_blocks, .num_ssts = num_ssts, .n = nranges,
                                     .cand_entries = cand_entries, .cand_key_bytes = cand_key_bytes, .merge = merge != 0,
                                     .filter = true}) + 256;
}

sdb_status sdb_lsm_scan_filtered(const sdb_lsm_view *lsm, const sdb_filter_policy *policies, const sdb_scan_ranges *ranges,
                                 const sdb_scan_prefixes *prefixes, const uint64_t *max_seq, int32_t descending,
                                 uint64_t cand_entries, uint64_t cand_key_bytes, const sdb_lsm_scan_out *out,
                                 const sdb_chain_out *chain, const sdb_scan_filter_out *fout, void *workspace,
                                 uint64_t workspace_bytes, void *stream) {
    return lsm_scan_call({.lsm = lsm, .pol = policies, .ranges = ranges, .prefixes = prefixes, .max_seq = max_seq,
                          .desc = descending ? 1u : 0u, .cand_entries = cand_entries, .cand_key_bytes = cand_key_bytes,
                          .out = out, .chain = chain, .fout = fout, .merge = chain != nullptr, .filter = true},
                         workspace, workspace_bytes, stream);
}

uint64_t sdb_lsm_scan_projected_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs,
                                                uint64_t nranges, uint64_t cand_entries, uint64_t cand_key_bytes,
                                                int32_t merge) {
    // a pair's view range is recomputed where it is read: no state beyond the filtered scan's
    return sdb_lsm_scan_filtered_workspace_bytes(total_blocks, num_ssts, num_runs, nranges, cand_entries, cand_key_bytes, merge);
}

sdb_status sdb_lsm_scan_projected(const sdb_lsm_view *lsm, const sdb_scan_ranges *proj, const sdb_filter_policy *policies,
                                  const sdb_scan_ranges *ranges, const sdb_scan_prefixes *prefixes, const uint64_t *max_seq,
                                  int32_t descending, uint64_t cand_entries, uint64_t cand_key_bytes,
                                  const sdb_lsm_scan_out *out, const sdb_chain_out *chain, const sdb_scan_filter_out *fout,
                                  void *workspace, uint64_t workspace_bytes, void *stream) {
    return lsm_scan_call({.lsm = lsm, .proj = proj, .pol = policies, .ranges = ranges, .prefixes = prefixes, .max_seq = max_seq,
                          .desc = descending ? 1u : 0u, .cand_entries = cand_entries, .cand_key_bytes = cand_key_bytes,
                          .out = out, .chain = chain, .fout = fout, .merge = chain != nullptr, .filter = true},
                         workspace, workspace_bytes, stream);
}

uint64_t sdb_lsm_scan_mem_workspace_bytes(uint32_t num_tables, uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs,
                                          uint64_t nranges, uint64_t cand_entries, uint64_t cand_key_bytes, int32_t merge) {
    (void)num_runs;
    return lsm_scan_workspace_bytes({.num_tables = num_tables, .total_blocks = total_blocks, .num_ssts = num_ssts, .n = nranges,
                                     .cand_entries = cand_entries, .cand_key_bytes = cand_key_bytes, .merge = merge != 0,
                                     .filter = true}) + 256;
}

sdb_status sdb_lsm_scan_mem(const sdb_mem_view *mem, const sdb_lsm_view *lsm, const sdb_scan_ranges *proj,
                            const sdb_filter_policy *policies, const sdb_scan_ranges *ranges,
                            const sdb_scan_prefixes *prefixes, const uint64_t *max_seq, int32_t descending,
                            uint64_t cand_entries, uint64_t cand_key_bytes, const sdb_lsm_scan_out *out,
                            const sdb_mem_scan_out *mout, const sdb_chain_out *chain, const sdb_mem_chain_out *mchain,
                            const sdb_scan_filter_out *fout, void *workspace, uint64_t workspace_bytes, void *stream) {
    return lsm_scan_call({.mem = mem, .lsm = lsm, .proj = proj, .pol = policies, .ranges = ranges, .prefixes = prefixes,
                          .max_seq = max_seq, .desc = descending ? 1u : 0u, .cand_entries = cand_entries,
                          .cand_key_bytes = cand_key_bytes, .out = out, .mout = mout, .chain = chain, .mchain = mchain,
                          .fout = fout, .merge = chain != nullptr, .filter = true, .layers = true},
                         workspace, workspace_bytes, stream);
}

uint64_t sdb_lsm_scan_recency_workspace_bytes(uint32_t num_tables, uint64_t total_blocks, uint32_t num_ssts,
                                              uint32_t num_runs, uint64_t nranges, uint64_t cand_entries,
                                              uint64_t cand_key_bytes) {
    (void)num_runs;
    return lsm_scan_workspace_bytes({.num_tables = num_tables, .total_blocks = total_blocks, .num_ssts = num_ssts, .n = nranges,
                                     .cand_entries = cand_entries, .cand_key_bytes = cand_key_bytes, .filter = true,
                                     .recency = true}) + 256;
}

sdb_status sdb_lsm_scan_recency(const sdb_mem_view *mem, const sdb_lsm_view *lsm, const sdb_scan_ranges *proj,
                                const sdb_filter_policy *policies, const sdb_scan_ranges *ranges,
                                const sdb_scan_prefixes *prefixes, const uint64_t *max_seq, const uint64_t *limit,
                                int32_t descending, uint64_t cand_entries, uint64_t cand_key_bytes,
                                const sdb_lsm_scan_out *out, const sdb_mem_scan_out *mout, const sdb_scan_filter_out *fout,
                                const sdb_recency_out *rout, void *workspace, uint64_t workspace_bytes, void *stream) {
    return lsm_scan_call({.mem = mem, .lsm = lsm, .proj = proj, .pol = policies, .ranges = ranges, .prefixes = prefixes,
                          .max_seq = max_seq, .desc = descending ? 1u : 0u, .cand_entries = cand_entries,
                          .cand_key_bytes = cand_key_bytes, .out = out, .mout = mout, .fout = fout, .filter = true,
                          .layers = true, .recency = true, .limit = limit, .rout = rout},
                         workspace, workspace_bytes, stream);
}

// ---- WAL replay / device memtable ----
uint64_t sdb_wal_replay_workspace_bytes(uint64_t n, uint64_t nbatches) {
    ReplayArgs a{};
    a.n = n;
    a.nbatches = nbatches;
    return replay_bind(a, nullptr) + 256;
}

// The checks both calls share, and the arguments they share.
static sdb_status replay_args(const sdb_run *rows, const uint64_t *batch_start, uint64_t nbatches, void *workspace,
                              uint64_t workspace_bytes, ReplayArgs *a) {
    if (!rows || !workspace) return SDB_INVALID_ARGUMENT;
    const uint64_t n = rows->n;
    if (nbatches && !batch_start) return SDB_INVALID_ARGUMENT;
    if (n && (!rows->key_arena || !rows->key_off || !rows->val_base || !rows->val_off || !rows->val_len || !rows->seq ||
              !rows->flags))
        return SDB_INVALID_ARGUMENT;
    if (n >= kReplaySkip) return SDB_LIMIT_EXCEEDED;  // the permutation is 31 bits and a flag
    *a = ReplayArgs{};
    a->n = n;
    a->nbatches = nbatches;
    a->r = *rows;
    a->batch_start = batch_start;
    if (workspace_bytes < replay_bind(*a, nullptr) + 256) return SDB_INVALID_ARGUMENT;
    replay_bind(*a, ws_align(workspace));
    a->ntiles = (uint32_t)((n + kReplayTile - 1) / kReplayTile);
    a->nblocks = (uint32_t)((n + kReplayBlock - 1) / kReplayBlock);
    for (uint64_t run = kReplayTile; run < n; run *= 2) a->npass++;
    a->sorted = a->perm[a->npass & 1];
    return SDB_OK;
}

sdb_status sdb_wal_replay_sort(const sdb_run *rows, const uint64_t *batch_start, uint64_t nbatches, uint64_t min_seq,
                               int32_t has_min_seq, sdb_wal_batch_facts *facts, sdb_wal_replay_summary *summary,
                               void *workspace, uint64_t workspace_bytes, void *stream) {
    ReplayArgs a;
    if (!summary || (nbatches && !facts)) return SDB_INVALID_ARGUMENT;
    sdb_status st = replay_args(rows, batch_start, nbatches, workspace, workspace_bytes, &a);
    if (st) return st;
    a.min_seq = min_seq;
    a.has_min_seq = has_min_seq ? 1u : 0u;
    a.facts = facts;
    a.summary = summary;
    if (!device_ok()) return SDB_DEVICE_ERROR;
    return launch_replay_sort(a, S(stream)) == hipSuccess ? SDB_OK : SDB_DEVICE_ERROR;
}

sdb_status sdb_wal_replay_emit(const sdb_run *rows, const uint64_t *batch_start, uint64_t nbatches,
                               const uint64_t *table_batch_start, uint64_t ntables, const sdb_wal_tables_out *out,
                               void *workspace, uint64_t workspace_bytes, void *stream) {
    ReplayArgs a;
    if (!out || !out->summary || !out->table_row_start || !table_batch_start || ntables > nbatches)
        return SDB_INVALID_ARGUMENT;
    sdb_status st = replay_args(rows, batch_start, nbatches, workspace, workspace_bytes, &a);
    if (st) return st;
    if (a.n && (!out->key_bytes || !out->key_off || !out->val_bytes || !out->val_off || !out->kind || !out->seq ||
                !out->create_ts || !out->expire_ts || !out->ts_mask))
        return SDB_INVALID_ARGUMENT;
    a.table_batch_start = table_batch_start;
    a.ntables = ntables;
    a.out = *out;
    if (!device_ok()) return SDB_DEVICE_ERROR;
    return launch_replay_emit(a, S(stream)) == hipSuccess ? SDB_OK : SDB_DEVICE_ERROR;
}

uint32_t sdb_diag_replay_tile(void) { return kReplayTile; }

}  // extern "C"

// =================================================================================================
// Stage timing (diagnostics)
// =================================================================================================
namespace sdb {
namespace {
std::mutex g_diag_mu;
bool g_diag_on = false;
struct StageRec {
    int stage;
    hipEvent_t a, b;
};
std::vector<StageRec> g_recs;
std::vector<hipEvent_t> g_open(kNumStages, nullptr);
uint64_t g_launches = 0;
}  // namespace
bool stage_timing_on() { return g_diag_on; }
void stage_mark(hipStream_t st, int stage, bool begin) {
    if (!g_diag_on) return;
    std::lock_guard<std::mutex> lk(g_diag_mu);
    hipEvent_t e;
    hipEventCreate(&e);
    hipEventRecord(e, st);
    if (begin) {
        g_open[stage] = e;
        if (stage == kStFacts) g_launches++;
    } else {
        g_recs.push_back({stage, g_open[stage], e});
        g_open[stage] = nullptr;
    }
}
}  // namespace sdb

extern "C" {
void sdb_diag_enable_stage_timing(int on) {
    std::lock_guard<std::mutex> lk(g_diag_mu);
    g_diag_on = on != 0;
}
int sdb_diag_stage_times(double *ms, int max_stages, uint64_t *launches) {
    std::lock_guard<std::mutex> lk(g_diag_mu);
    std::vector<double> acc(kNumStages, 0.0);
    for (auto &r : g_recs) {
        hipEventSynchronize(r.b);
        float t = 0;
        hipEventElapsedTime(&t, r.a, r.b);
        acc[r.stage] += t;
        hipEventDestroy(r.a);
        hipEventDestroy(r.b);
    }
    g_recs.clear();
    for (int i = 0; i < max_stages && i < kNumStages; i++) ms[i] = acc[i];
    if (launches) *launches = g_launches;
    g_launches = 0;
    return kNumStages;
}
}  // extern "C"

// Diagnostics: the fused bloom's slot plan inside sdb_encode_sst's workspace: byte offset of the run
// counts (tiles x nslices u32), tiles, slices and slot capacity.
extern "C" uint64_t sdb_diag_bloom_slots(uint64_t n, const sdb_sst_params *p, uint32_t *tiles, uint32_t *nslices,
                                         uint32_t *cap) {
    const uint64_t fb = p && p->bloom_bits_per_key ? filter_bytes_for(n, p->bloom_bits_per_key) : 0;
    const uint32_t k = p ? num_probes_for(p->bloom_bits_per_key) : 0;
    const BloomPlan pl = bloom_plan(n, k, fb, kChunk);
    *tiles = pl.tiles;
    *nslices = pl.nslices;
    *cap = bloom_slot_cap(pl);
    return sdb::encode_ws_layout(n, nullptr);
}

// Diagnostics: where sdb_encode_sst's workspace keeps the encode's routing state: byte offsets of the u32
// slow_count (workgroup-path blocks), big_count (piece-path blocks), wmax (longest candidate block) and
// mode (1: table composition, 0: the serial walk).  k_anchor zeroes the counters, k_blocks fills them and
// nothing resets them afterwards, so they are readable once the encode's stream is synchronised.
extern "C" void sdb_diag_encode_state(uint64_t n, uint64_t *slow_count, uint64_t *big_count, uint64_t *wmax,
                                      uint64_t *mode) {
    uint32_t wso[sdb::kWsFields];
    sdb::encode_ws_layout(n, wso);
    *slow_count = (uint64_t)wso[sdb::kWs_slow_count] << 8;
    *big_count = (uint64_t)wso[sdb::kWs_big_count] << 8;
    *wmax = (uint64_t)wso[sdb::kWs_wmax] << 8;
    *mode = (uint64_t)wso[sdb::kWs_mode] << 8;
}

// Diagnostics: where sdb_merge_runs' workspace keeps the merge's state for `total` input entries: byte offsets,
// from the workspace pointer rounded up to 256 bytes, of lcp0 (u32 L0), pfx (u64 per global entry), perm (u64 per
// merged position), dec (u8 per merged position), tile_sum (3 u64 per tile) and bound (k_mg_bounds: 2 x nruns
// u64 per 256 entries), as merge_bind carves them.  Nothing resets them after the merge, so they are readable
// once the merge's stream is synchronised.
extern "C" void sdb_diag_merge_state(uint64_t total, uint64_t *lcp0, uint64_t *pfx, uint64_t *perm, uint64_t *dec,
                                     uint64_t *tile_sum, uint64_t *bound) {
    sdb::MergeArgs a{};
    a.total = total;
    uint8_t *const base = (uint8_t *)(uintptr_t)256;  // merge_bind binds nothing at a null base
    sdb::merge_bind(a, base);
    *lcp0 = (uint64_t)((uint8_t *)a.lcp0 - base);
    *pfx = (uint64_t)((uint8_t *)a.pfx - base);
    *perm = (uint64_t)((uint8_t *)a.perm - base);
    *dec = (uint64_t)((uint8_t *)a.dec - base);
    *tile_sum = (uint64_t)((uint8_t *)a.tile_sum - base);
    *bound = (uint64_t)((uint8_t *)a.bound - base);
}
