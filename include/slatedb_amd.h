/*
 * slatedb_amd.h — C ABI of the MI355X-native SST block codec + bloom-filter builder.
 *
 * This is the drop-in boundary for slatedb's SST encode/decode hot path.  Every entry point is
 * plain C (no HIP/torch types): pointers, sizes, an opaque stream handle and a status code.
 * Citations are `path:line` relative to the slatedb reference (workspace 0.15.0).
 *
 * What each group replaces (the reference side is Rust; the binding a maintainer would add is in
 * INTEGRATION.md):
 *   - sdb_encode_sst*          -> EncodedSsTableBuilder::{add, finish_block, build}
 *                                 (slatedb/src/sst_builder.rs:224-254, 284-326, 370-417) with
 *                                 BlockBuilderV2 / BlockBuilderV1 (format/block_v2.rs:118-240,
 *                                 format/block.rs:76-218), SstRowCodecV2 / SstRowCodecV0
 *                                 (format/row_codec_v2.rs:127-169, format/row.rs:159-198), the
 *                                 per-block CRC32 of compress_and_transform (format/sst.rs:525-554)
 *                                 and BloomFilterBuilder (filter.rs:40-90).
 *   - sdb_bloom_build*         -> FilterBuilder::build for BloomFilterPolicy "_bf"
 *                                 (filter_policy.rs:170-283, filter.rs:71-90, 196-239).
 *   - sdb_bloom_might_contain  -> BloomFilter::might_contain (filter.rs:124-136).
 *   - sdb_decode_blocks*       -> SsTableFormat::read_blocks/decode_block + validate_checksum
 *                                 (format/sst.rs:938-999, 1029-1038) followed by draining
 *                                 DataBlockIterator ascending (block_iterator.rs:54-101,
 *                                 block_iterator_v2.rs:235-267) — the contract of the public
 *                                 SstFile::read_block (sst_reader.rs:287-309).
 *   - sdb_sst_scan             -> SstIterator over a BytesRange, drained (sst_iter.rs:64-121, 548-673):
 *                                 the blocks of partitions_covering_range (partitioned_keyspace.rs:
 *                                 87-110), clipped to the range, many ranges per call.
 *   - sdb_lsm_get              -> the on-disk part of Reader::get_key_value_with_options (reader.rs:203-260):
 *                                 GetIterator::from_lsm_tree (db_iter.rs:79-124) over L0 and the sorted
 *                                 runs, snapshot-aware (max_seq), many keys per call.
 *   - sdb_lsm_scan             -> the on-disk part of Reader::scan_with_options (reader.rs:275-320):
 *                                 DbIterator::new (db_iter.rs:189-257) over L0 and the sorted runs, drained:
 *                                 the newest visible version per key, many ranges per call.
 *   - sdb_lsm_get_merge,       -> the same two reads under MergeOperatorIterator (merge_operator.rs:242-485,
 *     sdb_lsm_scan_merge         db_iter.rs:234-243): every key's operand chain located on the device, the
 *                                 user's operator run on the host over the links.
 *   - sdb_lsm_get_mem          -> Reader::get_key_value_with_options from the active memtable down
 *                                 (reader.rs:133-182): device memtables (sorted runs, as sdb_wal_replay_emit
 *                                 leaves them) searched ahead of the tree, with or without operand chains.
 *   - sdb_lsm_scan_mem         -> Reader::scan_with_options from the active memtable down (reader.rs:275-320,
 *                                 db_iter.rs:145-163): the same memtables merged ahead of the tree's SSTs.
 *   - sdb_lsm_scan_recency     -> Reader::scan_prefix_by_recency_with_options (reader.rs:322-428) under
 *                                 DbRecencyIterator (db_iter.rs:376-442): the same sources drained one after
 *                                 another, newest first, up to a row limit; no merge, raw rows.
 *   - sdb_sst_builder_*        -> host-side mirror of EncodedSsTableBuilder's add()/build()/
 *                                 next_block() call order (sst_builder.rs:224-276), batching
 *                                 entries into a columnar pinned buffer and encoding on the GPU.
 *
 * Conventions
 *   - "device" entry points take device pointers and enqueue on `stream` (a hipStream_t passed as
 *     void*; NULL = the legacy default stream).  They never allocate, never synchronise, launch only
 *     on `stream` (no side streams, no cross-stream events; concurrent calls on different streams
 *     share nothing), and are safe to capture into a HIP graph.  Results that the host needs
 *     (lengths, status) are written
 *     to a device-resident summary struct the caller copies back.
 *   - "host" entry points take host pointers, manage a per-handle device arena + pinned staging and
 *     return synchronously.
 *   - Keys/values are Arrow-style columnar: entry i's key is key_bytes[key_off[i] .. key_off[i+1]).
 *     Offsets are monotone (n+1 entries, key_off[0] may be non-zero).
 *   - The library fails loudly: if no HIP device is present every compute entry point returns
 *     SDB_DEVICE_ERROR.  There is no CPU fallback.
 */
#ifndef SLATEDB_AMD_H
#define SLATEDB_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SDB_ABI_VERSION 2u

/* Status codes.  Mirrors the hot-path variants of SlateDBError (slatedb/src/error.rs:23-38,
 * 142-152, 197); the reference *panics* where SDB_LIMIT_EXCEEDED is returned. */
typedef enum sdb_status {
    SDB_OK = 0,
    SDB_EMPTY_KEY = 1,              /* SlateDBError::EmptyKey (block_v2.rs:168-170) / assert in
                                       compute_lower_bound (utils.rs:210) */
    SDB_EMPTY_BLOCK = 2,            /* SlateDBError::EmptyBlock */
    SDB_CHECKSUM_MISMATCH = 3,      /* SlateDBError::ChecksumMismatch (format/sst.rs:1029-1038) */
    SDB_INVALID_ROW_FLAGS = 4,      /* SlateDBError::InvalidRowFlags (row_codec_v2.rs:234-249) */
    SDB_INVALID_VERSION = 5,        /* SlateDBError::InvalidVersion (block_iterator.rs:60-77) */
    SDB_LIMIT_EXCEEDED = 6,         /* reference panics: u16 asserts row.rs:73-85, block_v2.rs:195 */
    SDB_UNSUPPORTED = 7,            /* compression / block transformer (not on this path) */
    SDB_INVALID_ARGUMENT = 8,       /* bad kind byte, capacity too small, NULL pointer, ... */
    SDB_CORRUPT_BLOCK = 9,          /* block bytes that the reference would panic on while parsing */
    SDB_MERGE_OPERATOR_MISSING = 10,/* SlateDBError::MergeOperatorMissing (merge_operator.rs:213-223) */
    SDB_DECOMPRESSION_ERROR = 11,   /* SlateDBError::BlockDecompressionError (format/sst.rs:884-917) */
    SDB_INVALID_SEQUENCE_ORDER = 12,/* SlateDBError::InvalidSequenceOrder (merge_operator.rs:293-299) */
    SDB_MERGE_OPERATOR_ERROR = 13,  /* SlateDBError::MergeOperatorError: the user's operator failed */
    SDB_COMPACTION_FILTER_ERROR = 14,/* CompactionFilterError::{FilterError, CompactionEndError} */
    SDB_DEVICE_ERROR = 100          /* no HIP device / launch failure */
} sdb_status;

/* Entry kinds: ValueDeletable::{Value, Merge, Tombstone} (types.rs:166-173). */
enum { SDB_KIND_VALUE = 0, SDB_KIND_MERGE = 1, SDB_KIND_TOMBSTONE = 2 };
/* Row flags, RowFlags (format/row.rs:8-16). */
enum { SDB_FLAG_TOMBSTONE = 1, SDB_FLAG_HAS_EXPIRE_TS = 2, SDB_FLAG_HAS_CREATE_TS = 4,
       SDB_FLAG_MERGE_OPERAND = 8 };
/* ts_mask bits. */
enum { SDB_TS_CREATE = 1, SDB_TS_EXPIRE = 2 };

/* A sorted run of RowEntry (types.rs:17-29), key asc / seq desc (mem_table.rs:38-44), columnar. */
typedef struct sdb_kv_batch {
    uint64_t n;
    const uint8_t *key_bytes;
    const uint64_t *key_off;    /* n+1 */
    const uint8_t *val_bytes;   /* tombstones: value bytes are ignored (treated as empty); a batch should
                                   not carry any: blocks near a tombstone whose val_off range is not
                                   empty are assembled by the general, slower path */
    const uint64_t *val_off;    /* n+1 */
    const uint8_t *kind;        /* n; NULL = all SDB_KIND_VALUE */
    const uint64_t *seq;        /* n; NULL = all 0 */
    const int64_t *create_ts;   /* n (NULL = none); used where ts_mask & SDB_TS_CREATE, any entry may be read */
    const int64_t *expire_ts;   /* n (NULL = none); used where ts_mask & SDB_TS_EXPIRE, any entry may be read */
    const uint8_t *ts_mask;     /* n; NULL = no timestamps */
    const int32_t *prefix_len;  /* n; SDB_PREFIX_LENGTHS only: PrefixExtractor::prefix_len(Point(key))
                                   computed by the caller's extractor (-1 = None); else NULL */
} sdb_kv_batch;

enum { SDB_SST_COMPACTED = 0, SDB_SST_WAL = 1 };   /* SstType (schemas/sst.fbs) */
/* Prefix extractor of BloomFilterPolicy::with_prefix_extractor (filter_policy.rs:213-224, filter.rs:
 * 40-63, prefix_extractor.rs:41-95).  The extractor is a user trait object in the reference; the
 * device evaluates the two stateless families the reference's tests use, or takes the lengths the
 * caller's own extractor returned (SDB_PREFIX_LENGTHS), which covers any extractor. */
enum { SDB_PREFIX_NONE = 0,
       SDB_PREFIX_FIXED = 1,    /* prefix_len = key.len() >= arg ? Some(arg) : None */
       SDB_PREFIX_DELIM = 2,    /* first byte == arg at i: Some(i + 1), else None */
       SDB_PREFIX_LENGTHS = 3 };/* sdb_kv_batch.prefix_len / the query lengths */

/* SsTableFormat knobs on this path (format/sst.rs:620-643, db/builder.rs:439-531). */
typedef struct sdb_sst_params {
    uint32_t block_size;         /* SstBlockSize, default 4096 (config.rs:231-267) */
    uint16_t sst_version;        /* 1 = BlockBuilderV1 + SstRowCodecV0, 2 = BlockBuilderV2 + V2 */
    uint16_t restart_interval;   /* V2 only; reference constant 16 (block_v2.rs:8) */
    uint32_t bloom_bits_per_key; /* BloomFilterPolicy::new(bpk) (filter_policy.rs:201); 0 = none */
    uint32_t min_filter_keys;    /* filter built iff num_rows >= min_filter_keys (sst_builder.rs:390) */
    uint32_t sst_type;           /* SDB_SST_COMPACTED, or SDB_SST_WAL: EncodedWalSsTableBuilder
                                    (wal/slatedb/sst_builder.rs:68-205): entries in insertion order,
                                    no compute_index_key (so no prefix panic), no filter; V2 only */
    uint32_t prefix_kind;        /* SDB_PREFIX_*: prefix hashes (deduplicated against the previous
                                    key's prefix) join the filter (filter.rs:40-58) */
    uint32_t prefix_arg;         /* FIXED: the length; DELIM: the delimiter byte */
    uint32_t no_whole_key;       /* 1 = with_whole_key_filtering(false) (filter_policy.rs:226-235):
                                    full keys are not hashed; 0 (default) = they are */
} sdb_sst_params;

/* Scalar results of one SST encode, written by the device. */
typedef struct sdb_sst_summary {
    uint64_t data_len;           /* bytes of data section (all blocks incl. CRC) */
    uint64_t num_blocks;
    uint64_t num_entries;
    uint64_t raw_key_size;       /* SstStats::raw_key_size (sst_builder.rs:225) */
    uint64_t raw_val_size;       /* SstStats::raw_val_size (sst_builder.rs:226) */
    uint64_t num_puts, num_deletes, num_merges;
    uint64_t bloom_len;          /* bitmap bytes (0 if no filter) */
    uint32_t num_probes;         /* optimal_num_probes(bpk) (filter.rs:235-239) */
    uint32_t filter_built;       /* 1 iff a filter was built */
    int32_t status;              /* sdb_status of the device-side checks */
    uint32_t max_block_entries;  /* diagnostics: longest block in entries */
    uint64_t first_error_entry;  /* entry index that raised `status` (UINT64_MAX if none) */
} sdb_sst_summary;

/* Caller-owned outputs.  For sdb_encode_sst (device) every pointer is device memory. */
typedef struct sdb_sst_out {
    uint8_t *data;               /* data section: blocks (Block::encode ++ crc32 BE), contiguous */
    uint64_t data_cap;
    uint64_t *block_off;         /* num_blocks+1 byte offsets into data (BlockMeta.offset) */
    uint32_t *block_first_entry; /* num_blocks+1 entry indices (last = n) */
    uint32_t *index_key_len;     /* per block: BlockMeta.first_key = key(first entry)[..len]
                                    (compute_index_key, utils.rs:198-226); block 0 -> 0 */
    uint16_t *block_stats;       /* 3 per block: num_puts, num_deletes, num_merges (sst_stats.rs:9-16) */
    uint64_t block_cap;          /* capacity (in blocks) of the four arrays above */
    uint8_t *bloom;              /* bloom bitmap (BloomFilter.buffer; the u16 BE num_probes header of
                                    Filter::encode is NOT included) */
    uint64_t bloom_cap;
    sdb_sst_summary *summary;    /* device-writable */
} sdb_sst_out;

/* ---------------------------------------------------------------------------------------------
 * Sizing (pure host arithmetic, no device needed)
 * ------------------------------------------------------------------------------------------- */
uint32_t sdb_abi_version(void);
/* Upper bounds on the output arrays for a batch of n entries holding the given key/value bytes. */
sdb_status sdb_encode_bounds(uint64_t n, uint64_t total_key_bytes, uint64_t total_val_bytes,
                             const sdb_sst_params *params, uint64_t *data_cap,
                             uint64_t *block_cap, uint64_t *bloom_cap);
/* Device scratch needed by sdb_encode_sst for n entries. */
uint64_t sdb_encode_workspace_bytes(uint64_t n, const sdb_sst_params *params);
/* BloomFilterBuilder::filter_size_bytes (filter.rs:65-69): ceil(u32(n*bpk)/8). */
uint64_t sdb_bloom_filter_bytes(uint64_t num_keys, uint32_t bits_per_key);
/* optimal_num_probes (filter.rs:235-239). */
uint32_t sdb_bloom_num_probes(uint32_t bits_per_key);

/* ---------------------------------------------------------------------------------------------
 * Device entry points (device pointers, async on `stream`)
 * ------------------------------------------------------------------------------------------- */
/* Encode one SST's data section + bloom bitmap from a device-resident sorted batch.  Host-side
 * argument errors are returned directly; data-dependent errors (empty key, V1 u16 overflow, bad
 * kind) are reported in out->summary->status after the stream completes. */
sdb_status sdb_encode_sst(const sdb_kv_batch *batch, const sdb_sst_params *params,
                          const sdb_sst_out *out, void *workspace, uint64_t workspace_bytes,
                          void *stream);

/* Encode `count` independent SSTs that share `params` in ONE launch sequence on `stream` (the SSTs of
 * one compaction job or of concurrent L0 flushes: l0_flush_parallelism / subcompactions,
 * config.rs:1081, 1383-1390).  Same per-SST contract as sdb_encode_sst (outs[i] for batches[i]; the
 * device checks land in outs[i].summary).  The kernels of up to 8 SSTs share each launch, so the
 * latency-bound segmentation of small grids fills the chip; larger counts run as consecutive sets.
 * workspace: sdb_encode_ssts_workspace_bytes(count, batches, params) bytes (only batches[i].n is read
 * on the host). */
uint64_t sdb_encode_ssts_workspace_bytes(uint32_t count, const sdb_kv_batch *batches,
                                         const sdb_sst_params *params);
sdb_status sdb_encode_ssts(uint32_t count, const sdb_kv_batch *batches, const sdb_sst_params *params,
                           const sdb_sst_out *outs, void *workspace, uint64_t workspace_bytes,
                           void *stream);
/* Scheduling hint: the caller keeps `builders` encode launch sequences (sdb_encode_sst / _ssts on distinct
 * streams, e.g. the concurrent SST writers of compactions and flushes) in flight on the current device.
 * The block-assembly kernel then takes 1/builders of the CUs (at least 1 workgroup), so one sequence's
 * segmentation kernels run on the CUs another sequence's assembly leaves free (1, the default: every
 * CU).  Process-wide per device; results do not depend on it.  SDB_INVALID_ARGUMENT for 0. */
sdb_status sdb_set_concurrent_builders(uint32_t builders);

/* Bloom bitmap over n keys (BloomFilterBuilder with whole-key filtering, filter.rs:40-90).
 * bitmap must hold sdb_bloom_filter_bytes(n, bpk) bytes and be 4-byte aligned (the build stores
 * 32-bit words); it is zeroed and filled on `stream`.  workspace (sdb_bloom_workspace_bytes) holds
 * the binned probes; NULL selects the slower device-scope-atomic build, which also needs
 * bitmap_bytes >= the filter size rounded up to 4.  Otherwise SDB_INVALID_ARGUMENT. */
uint64_t sdb_bloom_workspace_bytes(uint64_t num_keys, uint32_t bits_per_key);
sdb_status sdb_bloom_build(const uint8_t *key_bytes, const uint64_t *key_off, uint64_t n,
                           uint32_t bits_per_key, uint8_t *bitmap, uint64_t bitmap_bytes,
                           void *workspace, uint64_t workspace_bytes, void *stream);

/* Filter over whole keys and/or extracted prefixes (BloomFilterBuilder::add_key with a prefix
 * extractor, filter.rs:40-90): the filter's size follows the number of hashes (full keys + distinct
 * consecutive prefixes), which the device counts, so the byte length is written to *bloom_len (device
 * u64).  bitmap: 4-byte aligned, >= sdb_bloom_filter_bytes(2 n, bpk) bytes (the bound).  prefix_len:
 * per-key lengths for SDB_PREFIX_LENGTHS (else NULL).  Keys must be sorted for the prefix dedup. */
uint64_t sdb_bloom_prefix_workspace_bytes(uint64_t n);
sdb_status sdb_bloom_build_prefix(const uint8_t *key_bytes, const uint64_t *key_off, const int32_t *prefix_len,
                                  uint64_t n, uint32_t bits_per_key, uint32_t prefix_kind,
                                  uint32_t prefix_arg, uint32_t whole_key, uint8_t *bitmap,
                                  uint64_t bitmap_cap, uint64_t *bloom_len, void *workspace,
                                  uint64_t workspace_bytes, void *stream);
/* Filter::might_match (filter.rs:149-175) for FilterQuery targets: is_prefix[i] = 0 -> Point(key),
 * 1 -> Prefix(key) (a scan prefix; NULL = all points).  With whole-key filtering a point probes the
 * full key; otherwise the extracted prefix (query_prefix_len for SDB_PREFIX_LENGTHS, -1 = None); no
 * extractable prefix answers 1 (no false negative).  result[i] = 1 iff the key may be present. */
sdb_status sdb_bloom_might_match(const uint8_t *bitmap, uint64_t bitmap_bytes, uint32_t num_probes,
                                 uint32_t whole_key, uint32_t prefix_kind, uint32_t prefix_arg,
                                 const uint8_t *key_bytes, const uint64_t *key_off,
                                 const uint8_t *is_prefix, const int32_t *query_prefix_len, uint64_t n,
                                 uint8_t *result, void *stream);

/* Batched BloomFilter::might_contain(filter_hash(key)) (filter.rs:124-136, 150-175): result[i]=1
 * iff every probe bit is set.  An empty bitmap answers 0.  The bitmap may start at any byte address
 * (e.g. inside an SST's filter block); only bytes [0, bitmap_bytes) are read. */
sdb_status sdb_bloom_might_contain(const uint8_t *bitmap, uint64_t bitmap_bytes,
                                   uint32_t num_probes, const uint8_t *key_bytes,
                                   const uint64_t *key_off, uint64_t n, uint8_t *result,
                                   void *stream);

/* Decoded entries, columnar, ascending order within and across blocks. */
typedef struct sdb_decode_summary {
    uint64_t num_entries;
    uint64_t key_bytes;
    uint64_t num_bad_blocks;
    int32_t status;              /* error of the lowest-index failing block (try_join_all order) */
    uint32_t pad;
} sdb_decode_summary;

typedef struct sdb_decoded_out {
    uint64_t *block_entry_start; /* nblocks+1 */
    uint8_t *key_arena;          /* full keys restored (restore_full_key, row_codec_v2.rs:83-89) */
    uint64_t key_arena_cap;
    uint64_t *key_off;           /* cap_entries+1 */
    uint64_t *val_off;           /* byte offset of the value inside `blocks` (zero-copy, like
                                    Bytes::slice); tombstones -> 0 */
    uint32_t *val_len;
    uint64_t *seq;
    uint8_t *flags;              /* RowFlags of the row; kind = tombstone/merge/value from it */
    int64_t *create_ts;          /* valid iff flags & HAS_CREATE_TS */
    int64_t *expire_ts;          /* valid iff flags & HAS_EXPIRE_TS (V0 tombstones: never) */
    uint64_t cap_entries;
    uint32_t *bad_block;         /* indices of blocks that failed (CRC / flags / parse) */
    uint64_t bad_cap;
    sdb_decode_summary *summary; /* device-writable */
} sdb_decoded_out;

uint64_t sdb_decode_workspace_bytes(uint64_t nblocks);
/* Decode nblocks encoded blocks (each = Block::encode ++ crc32 BE) located at
 * blocks[block_off[k] .. block_off[k+1]).  sst_version 1 or 2 selects the row codec. */
sdb_status sdb_decode_blocks(const uint8_t *blocks, const uint64_t *block_off, uint64_t nblocks,
                             uint16_t sst_version, const sdb_decoded_out *out, void *workspace,
                             uint64_t workspace_bytes, void *stream);

/* Decode nblocks blocks placed anywhere in one device arena: block k = arena[block_start[k] ..
 * block_end[k]).  The read path fetches an SST's blocks as ~2 MiB ranged GETs (read_blocks,
 * format/sst.rs:919-978; bytes_to_fetch / max_fetch_tasks, config.rs:1323-1337) and splits each per
 * BlockMeta.offset; uploading many such ranges into one arena and decoding them here costs one launch
 * sequence instead of one per range.  Same output contract as sdb_decode_blocks; val_off is relative to
 * `arena`.  Workspace: sdb_decode_workspace_bytes(nblocks). */
sdb_status sdb_decode_blocks_at(const uint8_t *arena, const uint64_t *block_start, const uint64_t *block_end,
                                uint64_t nblocks, uint16_t sst_version, const sdb_decoded_out *out,
                                void *workspace, uint64_t workspace_bytes, void *stream);

/* Decode with options.  block_end == NULL: contiguous blocks (block_start has nblocks + 1 entries),
 * else as sdb_decode_blocks_at.  flags:
 *   SDB_DECODE_DESCENDING  entries in descending iteration order, as SstIterator in
 *     IterationOrder::Descending yields them (sst_iter.rs:460, 557): blocks last to first, each
 *     through DescendingBlockIteratorV2 (block_iterator_v2.rs:318-430) / BlockIterator Descending
 *     (block_iterator.rs:159-224).  Keys / columns are in that order; block_entry_start keeps the
 *     ascending prefix of the per-block counts, so block k's entries are [N - bes[k+1], N - bes[k]).
 *     A V2 block whose restart regions do not start at restarts with shared == 0 and end at the next
 *     one reports SDB_CORRUPT_BLOCK (the reference asserts there, block_iterator_v2.rs:76).
 *     Within a block the status is that of the first error in descending iteration order: restart 0's key
 *     (decoded by DescendingBlockIteratorV2::new), then the highest failing restart region and in it its first
 *     failing row; for V1 the first key, then the highest failing entry.  A V2 block without restarts yields
 *     nothing and no error.
 *   SDB_DECODE_FAIL_FAST   read_blocks semantics (format/sst.rs:938-1038, all or nothing): the status is
 *     the first failing block's, in block order, with its checksum verified before its rows as
 *     decode_block does, and every column is unspecified when the call fails (without the flag the
 *     good blocks are still decoded and the bad ones listed).  The checksums are then verified by the
 *     emit pass, which re-reads every block anyway, instead of the count pass. */
enum { SDB_DECODE_DESCENDING = 1, SDB_DECODE_FAIL_FAST = 2 };
sdb_status sdb_decode_blocks_ex(const uint8_t *arena, const uint64_t *block_start, const uint64_t *block_end,
                                uint64_t nblocks, uint16_t sst_version, uint32_t flags, const sdb_decoded_out *out,
                                void *workspace, uint64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Compressed blocks (SsTableInfo.compression_format != None): the first half of decode_block
 * (format/sst.rs:980-999) — validate_checksum over the stored bytes, then SsTableFormat::decompress
 * (format/sst.rs:884-917) — on the device, for every codec:
 *   SDB_CODEC_LZ4     lz4_flex 0.11.6 block::decompress_size_prepended (u32 LE size, then an LZ4 block;
 *                     output shorter than the declared size is kept, as lz4_flex truncates);
 *   SDB_CODEC_SNAPPY  snap 1.1.1 raw::Decoder::decompress_vec (varint size, then Snappy raw elements);
 *   SDB_CODEC_ZLIB    flate2 1.1.9 read::ZlibDecoder::read_to_end (zlib header, deflate, Adler-32; input
 *                     that ends inside the stream yields the bytes decoded so far, as flate2's read does);
 *   SDB_CODEC_ZSTD    zstd 0.13.3 stream::decode_all (zstd frames and skippable frames in sequence).
 * Two steps, so the caller can size the output:
 *   1. sdb_decompress_plan writes out_start[0..nblocks] (device): block k's output slot starts at
 *      out_start[k] and holds its decompressed length + 4 (the declared length for Lz4 / Snappy, the
 *      frames' Frame_Content_Size for Zstd — zstd::bulk::compress writes it — and a count-mode decode
 *      for Zlib and for Zstd frames without one; Adler-32 / XXH64 checksums are verified in step 2);
 *      out_start[nblocks] = the bytes `out` needs.  A header that cannot be read, a Zlib / Zstd stream
 *      that fails to decode, or more than 64 MiB gets an empty slot (that block then fails in step 2).
 *   2. sdb_decompress_blocks fills out[out_start[k] .. out_end[k]) with the uncompressed block followed
 *      by the CRC32 (BE) of those bytes — Block::encode() ++ crc, so sdb_decode_blocks_at(out,
 *      out_start, out_end, ...) decodes the run (value references then point into `out`).  *err
 *      (device u64) = block << 8 | status of the first failing block in block order (~0: none):
 *      SDB_CHECKSUM_MISMATCH, SDB_DECOMPRESSION_ERROR, SDB_CORRUPT_BLOCK (fewer than 4 bytes),
 *      SDB_LIMIT_EXCEEDED (over 64 MiB) or SDB_INVALID_ARGUMENT (slot past out_cap); a failing block's
 *      out_end[k] = out_start[k].
 * blocks / block_off (nblocks + 1) as sdb_decode_blocks.  Workspace (step 1 only):
 * sdb_decompress_workspace_bytes(nblocks). */
enum { SDB_CODEC_NONE = 0, SDB_CODEC_SNAPPY = 1, SDB_CODEC_ZLIB = 2, SDB_CODEC_LZ4 = 3, SDB_CODEC_ZSTD = 4 };
uint64_t sdb_decompress_workspace_bytes(uint64_t nblocks);
sdb_status sdb_decompress_plan(uint32_t codec, const uint8_t *blocks, const uint64_t *block_off, uint64_t nblocks,
                               uint64_t *out_start, void *workspace, uint64_t workspace_bytes, void *stream);
sdb_status sdb_decompress_blocks(uint32_t codec, const uint8_t *blocks, const uint64_t *block_off, uint64_t nblocks,
                                 uint8_t *out, uint64_t out_cap, const uint64_t *out_start, uint64_t *out_end,
                                 uint64_t *err, void *stream);
/* Both steps without a host synchronisation between them (out sized by the caller up front).  For
 * SDB_CODEC_ZLIB, whose plan is a whole inflate, each block is inflated once into a slot of slot_bytes
 * (out_start[k] = k * slot_bytes, 8 <= slot_bytes <= 4 GiB, out_cap >= nblocks * slot_bytes); the blocks
 * whose output + 4 does not fit their slot are planned and inflated again, packed from
 * nblocks * slot_bytes on, and their out_start[k] rewritten — so out_start is not monotone and
 * out_start[nblocks] = the bytes of out the call used.  A block past out_cap fails with
 * SDB_INVALID_ARGUMENT as in step 2.  Zlib streams made of fixed-code and stored deflate blocks only are
 * inflated one per lane against shared tables; a stream with a dynamic-Huffman block anywhere in it (what
 * flate2 at its default level writes, and what sdb_compress_blocks writes for every window that compresses
 * better that way; its incompressible and tiny windows are stored or fixed-code) takes the
 * per-decoder-table kernel, handed over at its first dynamic block.  The other codecs ignore
 * slot_bytes: the plan and the run back to
 * back (out_start as step 1 writes it).  out_start / out_end / *err then mean what step 2 says, and
 * sdb_decode_blocks_at(out, out_start, out_end, ...) decodes the run.  Workspace:
 * sdb_decompress_once_workspace_bytes(nblocks). */
uint64_t sdb_decompress_once_workspace_bytes(uint64_t nblocks);
sdb_status sdb_decompress_blocks_once(uint32_t codec, const uint8_t *blocks, const uint64_t *block_off, uint64_t nblocks,
                                      uint64_t slot_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_start,
                                      uint64_t *out_end, uint64_t *err, void *workspace, uint64_t workspace_bytes,
                                      void *stream);

/* The compressing write side: compress_and_transform (format/sst.rs:525-554) with SsTableFormat::compress
 * (format/sst.rs:557-594) for every block of an encoded data section (each Block::encode() ++ CRC32 BE, as
 * sdb_encode_sst writes it): block k becomes the codec's bytes of its Block::encode() followed by the CRC32
 * (BE) of those compressed bytes, at out[out_off[k], out_off[k + 1]):
 *   SDB_CODEC_LZ4     u32 LE length ++ one LZ4 block (lz4_flex block::compress_prepend_size);
 *   SDB_CODEC_SNAPPY  varint length ++ Snappy raw elements (snap raw::Encoder::compress_vec);
 *   SDB_CODEC_ZLIB    78 9C ++ deflate (a dynamic-Huffman, fixed-Huffman or stored block per 4 KiB window,
 *                     whichever is shortest) ++ Adler-32 BE (flate2 ZlibEncoder, default level 6);
 *   SDB_CODEC_ZSTD    one zstd frame with Frame_Content_Size, a compressed block per 4 KiB window (Huffman
 *                     or raw / RLE literals, sequences with predefined / RLE / FSE-compressed tables) or a
 *                     raw / RLE block when shorter (zstd::bulk::compress at level 3).
 * One wave per block: hash-chain LZ77 with lazy matching in the wave's LDS, entropy codes built by the wave
 * (compression ratio within a few per cent of the canonical libraries).  The streams are valid for their formats and
 * decode (the crates' decompressors, sdb_decompress_blocks) to the block; they are not the crates' own
 * bytes (a match finder's choices are its own).  in_bytes = block_off[nblocks] - block_off[0];
 * out_off (device, nblocks + 1) = the compressed blocks' offsets from out (BlockMeta.offset when the data
 * section starts the SST), out_off[nblocks] = the compressed data section's length.  *err (device u64) =
 * block << 8 | status of the first failing block (~0: none): SDB_CORRUPT_BLOCK (a block under 4 bytes),
 * SDB_LIMIT_EXCEEDED (the section is over out_cap: nothing is written).
 * Workspace: sdb_compress_workspace_bytes(nblocks, in_bytes). */
uint64_t sdb_compress_workspace_bytes(uint64_t nblocks, uint64_t in_bytes);
sdb_status sdb_compress_blocks(uint32_t codec, const uint8_t *blocks, const uint64_t *block_off, uint64_t nblocks,
                               uint64_t in_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint64_t *err,
                               void *workspace, uint64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Point lookups / seeks on one encoded SST (device): the read path of Db::get and of an SstIterator
 * positioned on a key:
 *   1. filter: BloomFilter::might_contain(filter_hash(key)) (filter.rs:124-136, sst_iter.rs:201-227);
 *   2. blocks: partitions_covering_range([key, key]) over BlockMeta.first_key (partitioned_keyspace.rs:
 *      16-110), i.e. [first_partition_including_or_after_key, last_partition_including_key + 1);
 *   3. the first block of that range in iteration order is seeked (sst_iter.rs:501-516):
 *      BlockIteratorV2::seek (block_iterator_v2.rs:138-208, 269-313) ascending or
 *      DescendingBlockIteratorV2::seek (:318-469); BlockIterator::seek for V1 (block_iterator.rs:
 *      130-190); when it is exhausted the next block of the range is entered at its first entry
 *      (ascending) or its last (descending);
 *   4. the entry the iterator returns next is reported, and FOUND if its key equals the query.
 * Each block read is CRC-checked first (validate_checksum, format/sst.rs:1029-1038).
 * ------------------------------------------------------------------------------------------- */
enum { SDB_LOOKUP_FILTERED = 0,     /* the bloom filter rules the key out (no block read) */
       SDB_LOOKUP_EXHAUSTED = 1,    /* no entry at or past the key in iteration order */
       SDB_LOOKUP_POSITIONED = 2,   /* positioned on an entry whose key differs from the query */
       SDB_LOOKUP_FOUND = 3 };      /* positioned on an entry with key == query (newest version) */
typedef struct sdb_sst_view {       /* device pointers into one encoded SST */
    const uint8_t *data;            /* data section (blocks ++ crc) */
    const uint64_t *block_off;      /* num_blocks + 1: BlockMeta.offset, then the data length */
    uint64_t num_blocks;
    const uint8_t *index_keys;      /* BlockMeta.first_key of block k = */
    const uint64_t *index_key_off;  /*   index_keys[index_key_off[k] .. index_key_off[k + 1]) */
    const uint8_t *bloom;           /* bitmap (filter without its u16 header); NULL = no filter */
    uint64_t bloom_len;
    uint32_t num_probes;
    uint16_t sst_version;           /* 1 or 2 */
    uint16_t pad;
} sdb_sst_view;
typedef struct sdb_lookup_out {     /* device arrays, one element per query */
    uint8_t *state;                 /* SDB_LOOKUP_* */
    int32_t *status;                /* sdb_status of the blocks read (CHECKSUM_MISMATCH, ...) */
    uint32_t *block;                /* block of the positioned entry */
    uint32_t *entry;                /* index of that entry inside its block (physical order) */
    uint32_t *key_len;              /* its key length */
    uint64_t *val_off;              /* its value: data[val_off .. val_off + val_len) (tombstone: 0, 0) */
    uint32_t *val_len;
    uint64_t *seq;
    uint8_t *flags;                 /* RowFlags as the iterator returns them */
    int64_t *create_ts;             /* valid iff flags & HAS_CREATE_TS */
    int64_t *expire_ts;             /* valid iff flags & HAS_EXPIRE_TS */
} sdb_lookup_out;
uint64_t sdb_sst_lookup_workspace_bytes(uint64_t num_blocks, uint64_t nkeys);
sdb_status sdb_sst_lookup(const sdb_sst_view *sst, const uint8_t *key_bytes, const uint64_t *key_off,
                          uint64_t nkeys, int32_t descending, const sdb_lookup_out *out,
                          void *workspace, uint64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Range scans on one encoded SST (device): an SstIterator over a BytesRange, drained.  The range is
 * the SstView's (sst_iter.rs:64-121): Db::scan builds it with new_owned(range, ..), Db::get with
 * for_key, the range key..=key.  Many ranges are scanned by one call:
 *   1. blocks: range_block = partitions_covering_range(index, start, end) over BlockMeta.first_key
 *      (partitioned_keyspace.rs:87-110, called at sst_iter.rs:548-552), the Excluded(k) end with k
 *      equal to a block's index key included (that block is not part of the range); block 0's index
 *      key is empty.  start above end gives end < start, as the reference's Range would hold it;
 *   2. entries: every entry of those blocks for which SstView::contains(key) holds (sst_iter.rs:
 *      97-121, 655-673): one contiguous physical run with every version of every key in the range.
 *      A range that is empty as a set (start above end, or equal keys with an excluded side) yields
 *      nothing and reads no block.  Overlapping ranges each get their own copy;
 *   3. order: ranges in input order.  descending == 0: physical order.  descending != 0: what
 *      SstIterator::next yields in IterationOrder::Descending (sst_iter.rs:567-651): keys descend and
 *      the versions of one key stay newest first, because fill_descending_buffer re-reverses each key
 *      group, across block boundaries too.  This is NOT the order of SDB_DECODE_DESCENDING, which is
 *      the block iterator's plain reverse (oldest version of a key first);
 *   4. errors: every block of range_block is bounds- and CRC-checked (format/sst.rs:1029-1038) and its
 *      rows parsed (flags, varints, as sdb_decode_blocks reports them) before a row is used;
 *      range_status[r] is the status of the lowest-index failing block of range r, and a failing
 *      range contributes zero entries.  That is all or nothing per range, like SDB_DECODE_FAIL_FAST;
 *      the reference would yield the entries ahead of the bad block and then fail.  Other ranges are
 *      unaffected; summary.status is the status of the lowest-numbered failing range.  A V2 block
 *      whose restart table cannot be followed is SDB_CORRUPT_BLOCK in descending mode, as in
 *      SDB_DECODE_DESCENDING (block_iterator_v2.rs:76);
 *   5. capacity: the summary always holds the totals the call needs.  When num_entries > cap_entries
 *      or key_bytes > key_arena_cap, summary.status is SDB_LIMIT_EXCEEDED and no column byte is
 *      written; range_entry_start, range_block and range_status are still valid, so the caller can
 *      size the columns and call again.
 * Host-detectable errors are returned directly (NULL pointers, a short workspace: SDB_INVALID_ARGUMENT).
 * A bound kind above 2 is SDB_INVALID_ARGUMENT too: from the call when no device is present (the
 * arrays are then host memory), otherwise as that range's range_status (the kinds live in device
 * memory, and the call does not synchronise).  n == 0 or num_blocks == 0 is SDB_OK with every range
 * empty, the summary zeroed and range_entry_start all 0.  Compressed data sections are decompressed
 * first (sdb_decompress_blocks_once).
 * ------------------------------------------------------------------------------------------- */
enum { SDB_BOUND_UNBOUNDED = 0, SDB_BOUND_INCLUDED = 1, SDB_BOUND_EXCLUDED = 2 };  /* std::ops::Bound */
typedef struct sdb_scan_ranges {    /* device pointers; range r = (start bound, end bound) */
    uint64_t n;
    const uint8_t *start_bytes;     /* start key of range r = */
    const uint64_t *start_off;      /*   start_bytes[start_off[r] .. start_off[r + 1]); ignored when UNBOUNDED */
    const uint8_t *start_kind;      /* n: SDB_BOUND_* */
    const uint8_t *end_bytes;
    const uint64_t *end_off;        /* n + 1 */
    const uint8_t *end_kind;        /* n */
} sdb_scan_ranges;
typedef struct sdb_scan_summary {
    uint64_t num_entries;           /* totals the call needs (also when they exceed the capacities) */
    uint64_t key_bytes;
    uint64_t num_failed_ranges;
    uint64_t blocks_read;           /* distinct blocks checked and parsed */
    int32_t status;
    uint32_t pad;
} sdb_scan_summary;
typedef struct sdb_scan_out {       /* device arrays */
    uint64_t *range_entry_start;    /* n + 1: range r's entries are [res[r], res[r + 1]) */
    uint32_t *range_block;          /* 2 n: start, end of range r's block range */
    int32_t *range_status;          /* n */
    uint8_t *key_arena;             /* full keys restored, as sdb_decoded_out */
    uint64_t key_arena_cap;
    uint64_t *key_off;              /* cap_entries + 1 */
    uint64_t *val_off;              /* the value: sst->data[val_off .. val_off + val_len) (tombstone: 0, 0) */
    uint32_t *val_len;
    uint64_t *seq;
    uint8_t *flags;                 /* RowFlags as the iterator returns them */
    int64_t *create_ts;             /* valid iff flags & HAS_CREATE_TS */
    int64_t *expire_ts;             /* valid iff flags & HAS_EXPIRE_TS */
    uint64_t cap_entries;
    sdb_scan_summary *summary;      /* device-writable */
} sdb_scan_out;
uint64_t sdb_sst_scan_workspace_bytes(uint64_t num_blocks, uint64_t nranges);
sdb_status sdb_sst_scan(const sdb_sst_view *sst, const sdb_scan_ranges *ranges, int32_t descending,
                        const sdb_scan_out *out, void *workspace, uint64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Batched Db::get over a tree of encoded SSTs (device): the on-disk part of
 * Reader::get_key_value_with_options (reader.rs:203-260).  For a point range the reference builds a
 * GetIterator (db_iter.rs:48-138, 219-225); over the tree that is GetIterator::from_lsm_tree
 * (db_iter.rs:79-90): a flat, lazy chain of per-SST iterators, not a merge.  Memtables and the write
 * batch stay on the host and are consulted first (memtables in device memory: sdb_lsm_get_mem).  Many keys are
 * resolved by one call:
 *   1. chain: for query q the chain is the concatenation, over the runs in order (newest first), of that
 *      run's covering SSTs: the contiguous SSTs i of the run with first_key[i] <= key <= last_key[i], in
 *      run order.  Every L0 SST is a run of one and comes first, newest first (build_l0_point_iters,
 *      segment_iterator.rs:312-330); then each sorted run contributes tables_covering_point_key(key)
 *      (build_sr_point_iters, segment_iterator.rs:332-353; db_state.rs:540-596, 662-665): the last SST
 *      whose start key is <= key if its range holds the key, and the SSTs immediately before it while
 *      their range still reaches the key (one key's versions straddling the cut between two output
 *      SSTs).  For a well-formed sorted run the two agree (point_table_idx_covering_key); for a run of
 *      one it equals searching that SST.  Here a view is a whole SST; projected views (visible_range) are
 *      read by sdb_lsm_get_projected;
 *   2. per SST of the chain: the bloom filter (bloom != NULL) may rule the SST out (sst_iter.rs:201-227);
 *      an empty bitmap rules every key out, as in sdb_sst_lookup.  Otherwise the block range is
 *      partitions_covering_range([key, key]) over the SST's index keys.  EVERY block of that range is
 *      bounds- and CRC-checked (format/sst.rs:1029-1038) and its rows parsed before a row is used; the
 *      lowest failing block's status fails the query, as in sdb_sst_scan rule 4.  Then the first entry
 *      in physical order with key == query and seq <= max_seq[q] is taken: versions above the bound are
 *      dropped before the walk sees them (FilterIterator::new_with_max_seq, filter_iterator.rs:22-48,
 *      db_iter.rs:354-372), across block boundaries and into the next covering SST of the run, so a
 *      tombstone above the bound does not stop the search.  No such entry: the walk goes on;
 *   3. decision (db_iter.rs:102-124): the first entry the first non-empty leaf yields decides the get.
 *      A value: SDB_GET_FOUND.  A tombstone: SDB_GET_DELETED with value 0, 0; older SSTs are not looked
 *      at.  A merge operand: SDB_GET_MERGE_OPERAND with status SDB_MERGE_OPERATOR_MISSING
 *      (MergeOperatorRequiredIterator, merge_operator.rs:213-223); the operand's columns are reported, so
 *      a caller with an operator knows where the chain begins (sdb_lsm_get_merge walks the chain).  An
 *      exhausted chain: SDB_GET_NOT_FOUND with sst = 0xFFFFFFFF and zeroed columns.  Expiry is NOT
 *      filtered on this path: expire_ts is returned to the caller, as in KeyValue;
 *   4. laziness of errors: a query reports a block error only from an SST that lies in its chain at or
 *      before the SST that decides it; an SST the bloom filter ruled out for that query does not count.
 *      A corrupt block in an older SST does not fail a query that a newer SST answered.  The call may
 *      check more blocks than the reference would read (it marks the whole chain before it knows which
 *      SST decides); those results never surface.  A failing query has state SDB_GET_NOT_FOUND,
 *      sst = 0xFFFFFFFF and zeroed columns; ssts_read / ssts_filtered count up to and including the SST
 *      that failed it;
 *   5. mixed formats: sst_version is per view, V1 and V2 SSTs may share a tree.  A view whose version is
 *      neither 1 nor 2 gives SDB_INVALID_VERSION to the queries that reach it (in their chain, not
 *      filtered, not decided before it);
 *   6. arguments: NULL structs, NULL arrays that a non-empty input needs and a short workspace return
 *      SDB_INVALID_ARGUMENT from the call (total_blocks or num_ssts >= 0xFFFFFFFF, or nkeys * num_runs over 2^40:
 *      SDB_LIMIT_EXCEEDED);
 *      then SDB_DEVICE_ERROR when no device is present.  What lives in device memory is checked on the
 *      device: block_base that disagrees with the views' num_blocks or with total_blocks, run_start that
 *      is not monotone from 0 to num_ssts, or key offsets that descend fail EVERY query with
 *      SDB_INVALID_ARGUMENT through status, and nothing is read through the malformed arrays.  A view
 *      with blocks and a NULL array fails the queries that reach it the same way.  nkeys == 0,
 *      num_ssts == 0 or total_blocks == 0 is SDB_OK with every query SDB_GET_NOT_FOUND and the summary
 *      zeroed (no SST was searched, so no counter moves);
 *   7. conventions: as every device entry point: no allocation, no synchronisation, launches only on
 *      `stream`, safe to capture into a HIP graph as a linear sequence; the workspace is reusable by
 *      the next call without a host-side reset.  Compressed data sections are decompressed first
 *      (sdb_decompress_blocks_once).
 * The counters num_found, num_deleted, num_not_found, num_merge and num_failed partition the queries
 * (num_not_found: exhausted chains with status SDB_OK; num_merge: merge operands, which are not failures).
 * ------------------------------------------------------------------------------------------- */
typedef struct sdb_lsm_view {        /* device pointers unless noted */
    const sdb_sst_view *ssts;        /* DEVICE array of num_ssts views, in search order */
    uint32_t num_ssts, num_runs;     /* host values */
    const uint32_t *run_start;       /* num_runs + 1: run r = ssts[run_start[r] .. run_start[r + 1]); runs newest
                                        first; an L0 SST is a run of one */
    const uint8_t *first_key_bytes;  /* SsTableInfo.first_entry of SST i = */
    const uint64_t *first_key_off;   /*   first_key_bytes[first_key_off[i] .. first_key_off[i + 1]) */
    const uint8_t *last_key_bytes;   /* SsTableInfo.last_entry, same layout */
    const uint64_t *last_key_off;
    const uint64_t *block_base;      /* num_ssts + 1: prefix sums of ssts[i].num_blocks */
    uint64_t total_blocks;           /* host value = block_base[num_ssts]; sizes the workspace and the grids */
} sdb_lsm_view;
enum { SDB_GET_NOT_FOUND = 0, SDB_GET_FOUND = 1, SDB_GET_DELETED = 2, SDB_GET_MERGE_OPERAND = 3 };
typedef struct sdb_get_summary {
    uint64_t num_found, num_deleted, num_not_found, num_merge, num_failed;
    uint64_t blocks_checked;         /* distinct blocks the call CRC-checked */
    int32_t status;                  /* status of the lowest-numbered failing query */
    uint32_t pad;
} sdb_get_summary;
typedef struct sdb_get_out {         /* device arrays, one element per query */
    uint8_t *state;                  /* SDB_GET_* */
    int32_t *status;                 /* SDB_OK, a block error, SDB_MERGE_OPERATOR_MISSING, ... */
    uint32_t *sst;                   /* index into ssts of the SST that decided the get (0xFFFFFFFF: none) */
    uint32_t *block;                 /* block of the deciding entry inside that SST */
    uint64_t *val_off;               /* ssts[sst].data[val_off .. val_off + val_len) (tombstone / none: 0, 0) */
    uint32_t *val_len;
    uint64_t *seq;
    uint8_t *flags;                  /* RowFlags as the iterator returns them */
    int64_t *create_ts;              /* valid iff flags & HAS_CREATE_TS */
    int64_t *expire_ts;              /* valid iff flags & HAS_EXPIRE_TS */
    uint32_t *ssts_read;             /* SSTs of the chain whose blocks this query consulted, up to and including
                                        the deciding one */
    uint32_t *ssts_filtered;         /* SSTs of the chain before the deciding one that the bloom filter ruled out */
    sdb_get_summary *summary;        /* device-writable */
} sdb_get_out;
uint64_t sdb_lsm_get_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs, uint64_t nkeys);
sdb_status sdb_lsm_get(const sdb_lsm_view *lsm, const uint8_t *key_bytes, const uint64_t *key_off, uint64_t nkeys,
                       const uint64_t *max_seq /* device, nkeys; NULL = no bound */, const sdb_get_out *out,
                       void *workspace, uint64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Batched Db::scan over a tree of encoded SSTs (device): the on-disk part of Reader::scan_with_options
 * (reader.rs:275-320) -> DbIterator::new (db_iter.rs:189-257), drained.  The write batch stays on the host and
 * the caller merges it on top; memtables in device memory are merged by sdb_lsm_scan_mem.  The tree is the sdb_lsm_view of sdb_lsm_get, the ranges are
 * the sdb_scan_ranges of sdb_sst_scan.  Many ranges are scanned by one call:
 *   1. SSTs of a range: SST i takes part in range r iff it has blocks and {k : first_key[i] <= k <=
 *      last_key[i]} meets the range as a set: the range is not empty as a set, last_key[i] does not precede
 *      its start bound and first_key[i] does not exceed its end bound.  This is per SST; runs only fix the
 *      search order, which is the order of `ssts`, newest first.  The reference opens every L0 SST and, per
 *      sorted run, tables_covering_range (segment_iterator.rs:355-414, db_state.rs:600-660); any SST it opens
 *      beyond this rule holds no key of the range, so the entries agree.  No bloom filter is consulted: a
 *      range has none without a prefix extractor (sdb_lsm_scan_filtered is the call that consults them).  A range
 *      that is empty as a set reads nothing.  Here a view is a whole SST; sdb_lsm_scan_projected reads projected
 *      views (visible_range).
 *      range_ssts[r] is the number of SSTs that take part;
 *   2. blocks: per participating SST, partitions_covering_range(index keys, start, end) exactly as
 *      sdb_sst_scan rule 1 (partitioned_keyspace.rs:87-110).  EVERY such block is bounds- and CRC-checked
 *      (format/sst.rs:1029-1038) and its rows are parsed before a row is used.  summary.blocks_checked is the
 *      size of the union of those blocks over all ranges, exactly: nothing here is lazy;
 *   3. rows: among all entries of the participating SSTs whose key the range contains, versions with
 *      seq > max_seq[r] are dropped first (FilterIterator::new_with_max_seq, applied before the
 *      deduplicating merge, db_iter.rs:205-217).  Per key the newest remaining version wins (MergeIterator
 *      with dedup: key ascending, seq descending, merge_iterator.rs:55-69, 180-209).  Equal (key, seq) in two
 *      SSTs, which the store never writes: the SST earlier in search order wins; within one SST the first in
 *      physical order (an SST holds its rows key ascending, seq descending, as the store writes them).  A
 *      winning tombstone yields nothing for the key (DbIterator::next_entry, db_iter.rs:280-303), a winning
 *      value yields one row.  Expiry is NOT filtered, as in sdb_lsm_get;
 *   4. merge operands: a key whose winner is a merge operand fails its range with
 *      SDB_MERGE_OPERATOR_MISSING (MergeOperatorRequiredIterator, merge_operator.rs:213-223).  An operand
 *      hidden behind a newer visible value or tombstone, or above the bound, does not.  A store with an
 *      operator calls sdb_lsm_scan_merge;
 *   5. order and errors: ranges in input order; inside a range keys ascend, or descend when descending != 0
 *      (one row per key, so both orders hold the same rows).  A failing range contributes zero entries: all
 *      or nothing, as sdb_sst_scan rule 4; the reference would yield the rows ahead of the failure first.
 *      range_status[r] is the status of the lowest failing block: lowest SST in search order, then lowest
 *      block.  A view with a version other than 1 or 2 gives SDB_INVALID_VERSION to the ranges it takes part
 *      in, a view with blocks and a NULL array SDB_INVALID_ARGUMENT, at that SST's place in the order.  A
 *      bound kind above 2 fails that range with SDB_INVALID_ARGUMENT (it takes part in nothing).  Block,
 *      version and argument errors take precedence over rule 4.  Other ranges are unaffected;
 *      summary.status is the status of the lowest-numbered failing range;
 *   6. capacity: the call stages candidates in the workspace: every entry of rule 3's set before any
 *      filtering, i.e. what sdb_sst_scan over each participating SST would yield for the range; ranges failed
 *      by a block, version or argument error contribute none.  The summary always reports num_candidates /
 *      candidate_key_bytes.  If they exceed cand_entries / cand_key_bytes: summary.status is
 *      SDB_LIMIT_EXCEEDED, num_entries = key_bytes = 0, range_entry_start is all 0, no column byte is written,
 *      and range_status (without rule 4) and range_ssts are valid.  If the candidates fit but
 *      num_entries > cap_entries or key_bytes > key_arena_cap: summary.status is SDB_LIMIT_EXCEEDED with the
 *      true totals, range_entry_start and range_status are valid and no column byte is written.
 *      num_entries <= num_candidates, so a caller who sizes the columns like the staging needs at most two
 *      calls;
 *   7. arguments and conventions, as sdb_lsm_get rules 6-7: NULL structs or arrays that a non-empty input
 *      needs, or a short workspace: SDB_INVALID_ARGUMENT from the call (total_blocks or num_ssts >=
 *      0xFFFFFFFF, n * num_ssts or cand_entries over 2^40, or cand_key_bytes over 2^44: SDB_LIMIT_EXCEEDED);
 *      then SDB_DEVICE_ERROR when no device is
 *      present.  A malformed tree (run_start, block_base, key offsets or range offsets that descend) fails
 *      EVERY range with SDB_INVALID_ARGUMENT on the device with blocks_checked 0, and nothing is read through
 *      the malformed arrays.  n == 0, num_ssts == 0 or total_blocks == 0 is SDB_OK with every range empty and
 *      the summary zeroed.  No allocation, no synchronisation, launches only on `stream`, safe to capture into
 *      a HIP graph as a linear sequence; the workspace is reusable by the next call without a host-side
 *      reset.  Compressed data sections are decompressed first (sdb_decompress_blocks_once).
 * ------------------------------------------------------------------------------------------- */
typedef struct sdb_lsm_scan_summary {
    uint64_t num_entries, key_bytes;               /* what the call yields over all ranges */
    uint64_t num_candidates, candidate_key_bytes;  /* what it stages before the merge (rule 6) */
    uint64_t num_failed_ranges;
    uint64_t blocks_checked;                       /* distinct tree blocks CRC-checked: exact (rule 2) */
    int32_t status;                                /* status of the lowest-numbered failing range, or LIMIT_EXCEEDED */
    uint32_t pad;
} sdb_lsm_scan_summary;
typedef struct sdb_lsm_scan_out {    /* device arrays */
    uint64_t *range_entry_start;     /* n + 1: range r's entries are [res[r], res[r + 1]) */
    int32_t *range_status;           /* n */
    uint32_t *range_ssts;            /* n: SSTs that took part in range r (rule 1) */
    uint8_t *key_arena;              /* full keys restored */
    uint64_t key_arena_cap;
    uint64_t *key_off;               /* cap_entries + 1 */
    uint32_t *sst;                   /* index into lsm->ssts of the SST that holds the row */
    uint64_t *val_off;               /* the value: ssts[sst].data[val_off .. val_off + val_len) */
    uint32_t *val_len;
    uint64_t *seq;
    uint8_t *flags;                  /* RowFlags as the iterator returns them */
    int64_t *create_ts;              /* valid iff flags & HAS_CREATE_TS */
    int64_t *expire_ts;              /* valid iff flags & HAS_EXPIRE_TS */
    uint64_t cap_entries;
    sdb_lsm_scan_summary *summary;   /* device-writable */
} sdb_lsm_scan_out;
uint64_t sdb_lsm_scan_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs, uint64_t nranges,
                                      uint64_t cand_entries, uint64_t cand_key_bytes);
sdb_status sdb_lsm_scan(const sdb_lsm_view *lsm, const sdb_scan_ranges *ranges,
                        const uint64_t *max_seq /* device, n; NULL = no bound */, int32_t descending,
                        uint64_t cand_entries, uint64_t cand_key_bytes, const sdb_lsm_scan_out *out,
                        void *workspace, uint64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Merge-operand chains in tree reads (device): what a store WITH a merge operator reads.  DbIterator::new
 * wraps its iterator in MergeOperatorIterator (merge_different_expire_ts = true, no snapshot barrier:
 * db_iter.rs:234-247) instead of MergeOperatorRequiredIterator.  The operator is a user trait object and
 * stays on the host; the device finds the versions of a key that form its operand chain
 * (merge_with_older_entries, merge_operator.rs:369-448) and the MergeTracker metadata (:262-303), and the
 * host calls merge_batch on bytes that are already located.
 *
 * Chains come out in CSR form over the call's items (queries of a get, output rows of a scan): links newest
 * first, the order in which merge_with_older_entries meets them.  A chain is a run of merge operands followed
 * by at most one base value; a tombstone ends a chain and is never a link.
 *
 * sdb_lsm_get_merge: sdb_lsm_get rules 1-2 and 5-7 hold (the chain of SSTs, filters, block ranges, block
 * checks, versions, arguments, conventions); rules 3-4 become:
 *   3'. versions: each SST of the chain yields EVERY entry with key == query and seq <= max_seq[q], in
 *      physical order, across blocks, into the next covering SST of the run and into the next run.  The first
 *      entry decides the state: a value: SDB_GET_FOUND, one link; a tombstone: SDB_GET_DELETED, no link,
 *      the tombstone's columns as sdb_lsm_get reports them; nothing: SDB_GET_NOT_FOUND; a merge operand:
 *      SDB_GET_MERGE_OPERAND with status SDB_OK and at least one link: the walk goes on while entries are
 *      operands; a value ends the chain as its base and last link; a tombstone ends it with no base
 *      (GetIterator returns None there, db_iter.rs:108-114, so its timestamps are NOT folded on this path);
 *      an exhausted chain of SSTs ends it with no base.
 *      Per-query columns, the entry MergeOperatorIterator returns (merge_operator.rs:437-447): sst, block,
 *      val_off, val_len and seq are the newest link's; create_ts is the maximum and expire_ts the minimum
 *      over the links that carry one; flags holds HAS_CREATE_TS / HAS_EXPIRE_TS for those aggregates and
 *      SDB_FLAG_MERGE_OPERAND iff no base was found (ValueDeletable::Merge against Value, :439-443).
 *      A link whose seq exceeds the newest link's fails the query with SDB_INVALID_SEQUENCE_ORDER
 *      (MergeTracker::update, :293-299); only a tree the store did not write holds one.  It is found per
 *      run: it takes precedence over a block error of the same run, and ssts_read / ssts_filtered then
 *      count that whole run's walk;
 *   4'. laziness of errors: a query reports a block error from any SST of its chain at or before the SST
 *      where the chain ENDED: the one holding the base or the tombstone, else the last SST of the chain; a
 *      filtered SST never counts.  A corrupt block behind the end never surfaces.  ssts_read /
 *      ssts_filtered count up to and including the ending SST.  A failing query has SDB_GET_NOT_FOUND,
 *      sst = 0xFFFFFFFF, zeroed columns and no links.
 * The summary is sdb_get_summary; num_merge counts operand winners and the five counters partition the
 * queries.  chain->summary->num_links and chain_start (nkeys + 1) are always written; when num_links >
 * cap_links the chain summary's status is SDB_LIMIT_EXCEEDED and no link column is written, while the
 * per-query columns stay valid: a caller needs at most two calls.  chain, chain_start and chain->summary must
 * not be NULL, the link columns not when cap_links > 0.
 *
 * sdb_lsm_scan_merge: sdb_lsm_scan rules 1-3 and 5-7 hold; rule 4 becomes: in the merged order of a range's
 * visible candidates (key ascending, seq descending, earlier SST first on ties) the winner of a key is its
 * first visible version.  A value winner yields a row with one link, a tombstone winner no row, an operand
 * winner a row whose links are the operands that follow for the same key up to and including the first
 * value.  A tombstone stops the chain and is not a link; HERE its create_ts / expire_ts are folded into the
 * row's aggregates and the row's flags show a base: MergeIterator hands it to merge_with_older_entries as
 * the base (merge_iterator.rs:193-206, merge_operator.rs:421-425).  Row columns as in the get variant;
 * chain_start is indexed by output row (num_entries + 1 valid elements, array sized cap_entries + 1).  With
 * descending != 0 the rows descend; a row's links stay newest first.  A point range k..=k is scanned like any
 * other: the reference routes it through GetIterator, which does not fold a tombstone base's timestamps;
 * callers who need that call sdb_lsm_get_merge.  Capacity (rule 6, extended): candidates, then rows, then
 * links.  While candidates or rows do not fit the chain summary reports SDB_LIMIT_EXCEEDED (num_links is the
 * true total once the candidates fit) and neither chain_start nor a link column is written.  When the rows
 * fit but num_links > cap_links: the chain summary reports SDB_LIMIT_EXCEEDED with the true total, chain_start
 * is valid, no link column is written and the row columns are complete.  SDB_MERGE_OPERATOR_MISSING never
 * comes out of this entry point.
 * ------------------------------------------------------------------------------------------- */
typedef struct sdb_chain_summary {
    uint64_t num_links;              /* links the call needs, also when above cap_links */
    uint64_t max_chain_len;
    int32_t status;                  /* SDB_OK | SDB_LIMIT_EXCEEDED */
    uint32_t pad;
} sdb_chain_summary;
typedef struct sdb_chain_out {       /* device arrays; CSR over the call's queries (get) or rows (scan) */
    uint64_t *chain_start;           /* count + 1: links of item i are [chain_start[i], chain_start[i + 1]) */
    uint32_t *sst;                   /* per link: index into lsm->ssts */
    uint32_t *block;
    uint64_t *val_off;               /* ssts[sst].data[val_off .. val_off + val_len) */
    uint32_t *val_len;
    uint64_t *seq;
    uint8_t *flags;                  /* RowFlags of the link's row */
    int64_t *create_ts;              /* valid iff flags & HAS_CREATE_TS */
    int64_t *expire_ts;              /* valid iff flags & HAS_EXPIRE_TS */
    uint64_t cap_links;
    sdb_chain_summary *summary;      /* device-writable */
} sdb_chain_out;
uint64_t sdb_lsm_get_merge_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs, uint64_t nkeys);
sdb_status sdb_lsm_get_merge(const sdb_lsm_view *lsm, const uint8_t *key_bytes, const uint64_t *key_off, uint64_t nkeys,
                             const uint64_t *max_seq /* device, nkeys; NULL = no bound */, const sdb_get_out *out,
                             const sdb_chain_out *chain, void *workspace, uint64_t workspace_bytes, void *stream);
uint64_t sdb_lsm_scan_merge_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs,
                                            uint64_t nranges, uint64_t cand_entries, uint64_t cand_key_bytes);
sdb_status sdb_lsm_scan_merge(const sdb_lsm_view *lsm, const sdb_scan_ranges *ranges,
                              const uint64_t *max_seq /* device, n; NULL = no bound */, int32_t descending,
                              uint64_t cand_entries, uint64_t cand_key_bytes, const sdb_lsm_scan_out *out,
                              const sdb_chain_out *chain, void *workspace, uint64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Filter policies in tree reads (device): Db::scan_prefix and gets over SSTs whose "_bf" filter was built with a
 * prefix extractor.  The reference's public Db::scan_prefix (db.rs:1071-1143) puts the prefix into
 * SstIteratorOptions.prefix (scan_with_options, reader.rs:284-293), and every per-SST iterator evaluates its
 * FilterQuery before it opens the SST (sst_iter.rs:848-862, 785-810, 201-227): a ruled-out SST is never opened,
 * its blocks are never fetched and its errors never surface.  sdb_lsm_scan_filtered is sdb_lsm_scan (chain ==
 * NULL: a winning operand fails its range) or sdb_lsm_scan_merge (chain != NULL) with that step;
 * sdb_lsm_get_filtered is sdb_lsm_get (chain == NULL) or sdb_lsm_get_merge with the filter step of rule 2 made
 * aware of the SST's policy: a tree written with no_whole_key = 1 stores no full-key hashes, so probing
 * might_contain(filter_hash(key)) there answers false for present keys.
 *   F1. the query of a pair (range r, SST i): a point range (start and end both SDB_BOUND_INCLUDED with equal
 *       keys: SstView::point_key, sst_iter.rs:82-87) asks Point(key), also when has_prefix[r] is set
 *       (sst_iter.rs:852-856); otherwise, if has_prefix[r], Prefix(p); otherwise there is no query and no filter
 *       is consulted.  prefixes == NULL: no range has a prefix.  In a get the query is always Point(key);
 *   F2. the answer is Filter::might_match exactly as sdb_bloom_might_match defines it (filter.rs:150-175): a
 *       Point under whole-key filtering (no_whole_key == 0) probes the full key; anything else probes
 *       target[..n], n from the SST's extractor: SDB_PREFIX_FIXED: len >= prefix_arg ? prefix_arg : None;
 *       SDB_PREFIX_DELIM: through the first delimiter byte, else None; SDB_PREFIX_LENGTHS: probe_len of the
 *       range / key (a NULL array or -1: None); SDB_PREFIX_NONE: None.  None answers "might match".  An empty
 *       bitmap (bloom != NULL, bloom_len == 0) answers "no" to every query that has something to probe and
 *       "might match" to a None.  bloom == NULL: the SST has no filter and takes part.  policies == NULL: every
 *       SST has {SDB_PREFIX_NONE, 0, 0}, the plain whole-key policy;
 *   F3. in the scan a ruled-out SST takes no part in that range: no block of it is marked, checked or staged
 *       for the range; it is not counted in range_ssts or num_candidates but in range_filtered[r]; its block
 *       errors, an invalid sst_version and NULL arrays do not surface for that range (the filter is evaluated
 *       first, as FilterIterator::init does and as the gets do).  blocks_checked stays the exact size of the
 *       union of the covering blocks of the pairs that take part.  Everything else of sdb_lsm_scan rules 1-7
 *       and of sdb_lsm_scan_merge's rule 4 holds unchanged: errors, the capacity protocol (range_filtered and
 *       num_filtered are valid whenever range_ssts is), ordering;
 *   F4. the caller's obligation, as in the reference (db.rs:233-236): when has_prefix[r] is set every key of
 *       range r starts with the prefix.  The device does not verify this; a violation can only lose rows of
 *       filtered SSTs and never reads out of bounds.  A probe_len above the length of the probed target counts
 *       as None;
 *   F5. in the get only rule 2's filter step changes, from might_contain(filter_hash(key)) to F2 with
 *       Point(key); ssts_filtered, ssts_read and the laziness rules are unchanged.  policies == NULL and
 *       probe_len == NULL give exactly sdb_lsm_get / sdb_lsm_get_merge;
 *   F6. arguments and conventions as the tree reads above: no allocation, no synchronisation, one stream,
 *       capturable into a HIP graph as a linear sequence, the workspace reusable without a host-side reset.  A
 *       NULL fout, or a NULL array inside it (or inside a non-NULL prefixes, probe_len aside) for n > 0, is
 *       SDB_INVALID_ARGUMENT from the call.  Prefix offsets that descend make the call malformed: every range
 *       gets SDB_INVALID_ARGUMENT, like range offsets.  A prefix_kind above SDB_PREFIX_LENGTHS in policies fails
 *       the queries and ranges that reach that SST with SDB_INVALID_ARGUMENT at that SST's place in the order;
 *       it is checked before the filter, which then rules nothing out.  With no device: SDB_DEVICE_ERROR, after
 *       the host checks.
 * The probe bytes of a query, and so their SipHash, depend on (query, policy) and not on the SST: when all
 * policies of the tree agree (the normal store) the hash is computed once per range or key, else per pair.
 * ------------------------------------------------------------------------------------------- */
/* What BloomFilter::decode is given for one SST's "_bf" filter (filter.rs:94-106), from the policy name in
 * the SST's metadata ("_bf", "_bf:p=<extractor>[:wh=0]", filter_policy.rs:237-250). */
typedef struct sdb_filter_policy {
    uint32_t prefix_kind;    /* SDB_PREFIX_NONE | _FIXED | _DELIM | _LENGTHS */
    uint32_t prefix_arg;
    uint32_t no_whole_key;   /* as sdb_sst_params.no_whole_key */
    uint32_t pad;
} sdb_filter_policy;
typedef struct sdb_scan_prefixes {      /* device pointers, one element per range */
    const uint8_t *prefix_bytes;        /* the scan prefix of range r = */
    const uint64_t *prefix_off;         /*   prefix_bytes[prefix_off[r] .. prefix_off[r + 1]); n + 1 */
    const uint8_t *has_prefix;          /* n: 1 = Db::scan_prefix, 0 = plain Db::scan (no prefix query) */
    const int32_t *probe_len;           /* n or NULL: prefix_len(Prefix(p)) of the caller's extractor (of Point(key)
                                           for a point range), -1 = None; read only for SSTs whose prefix_kind is
                                           SDB_PREFIX_LENGTHS */
} sdb_scan_prefixes;
typedef struct sdb_scan_filter_out {    /* device */
    uint32_t *range_filtered;           /* n: SSTs of rule 1 that the filter ruled out for range r */
    uint64_t *num_filtered;             /* one u64: their sum */
} sdb_scan_filter_out;
uint64_t sdb_lsm_scan_filtered_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs,
                                               uint64_t nranges, uint64_t cand_entries, uint64_t cand_key_bytes,
                                               int32_t merge /* 1: a chain is passed */);
sdb_status sdb_lsm_scan_filtered(const sdb_lsm_view *lsm, const sdb_filter_policy *policies /* device, num_ssts; or NULL */,
                                 const sdb_scan_ranges *ranges, const sdb_scan_prefixes *prefixes /* or NULL */,
                                 const uint64_t *max_seq /* device, n; NULL = no bound */, int32_t descending,
                                 uint64_t cand_entries, uint64_t cand_key_bytes, const sdb_lsm_scan_out *out,
                                 const sdb_chain_out *chain /* or NULL */, const sdb_scan_filter_out *fout,
                                 void *workspace, uint64_t workspace_bytes, void *stream);
uint64_t sdb_lsm_get_filtered_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs,
                                              uint64_t nkeys, int32_t merge /* 1: a chain is passed */);
sdb_status sdb_lsm_get_filtered(const sdb_lsm_view *lsm, const sdb_filter_policy *policies /* device, num_ssts; or NULL */,
                                const uint8_t *key_bytes, const uint64_t *key_off, uint64_t nkeys,
                                const int32_t *probe_len /* device, nkeys: prefix_len(Point(key)) for SDB_PREFIX_LENGTHS
                                                            SSTs, -1 = None; or NULL */,
                                const uint64_t *max_seq /* device, nkeys; NULL = no bound */, const sdb_get_out *out,
                                const sdb_chain_out *chain /* or NULL */, void *workspace, uint64_t workspace_bytes,
                                void *stream);

/* ---------------------------------------------------------------------------------------------
 * Tree reads over projected SST views (device).  In the reference an SST of the manifest is an SsTableView: the
 * physical handle plus an optional visible_range (db_state.rs:61-78).  Range-restricted clones and projected or
 * segmented databases produce such views (manifest/mod.rs:1039-1158), and every read path honours them
 * (effective_range and calculate_view_range, db_state.rs:116-141, 243-251; compacted_effective_start_key in the
 * sorted-run searches, :540-665; SstIterator::new_owned / for_key, sst_iter.rs:324-365).  sdb_lsm_get_projected and
 * sdb_lsm_scan_projected are sdb_lsm_get_filtered and sdb_lsm_scan_filtered (themselves the supersets of the plain
 * and _merge calls) with a visible range per SST.  `proj` is an sdb_scan_ranges with n == lsm->num_ssts: element i
 * is SsTableView.visible_range of ssts[i], (SDB_BOUND_UNBOUNDED, SDB_BOUND_UNBOUNDED) meaning None, the whole SST.
 * sdb_lsm_view and sdb_sst_view are unchanged.
 *   P1. effective range: E[i] = [first_key[i], last_key[i]] intersected with visible[i] as BytesRange::intersect
 *       does (comparable_range.rs:224-236): the tighter start, where Unbounded < Included(a) < Excluded(a), and the
 *       tighter end, where Excluded(a) < Included(a) < Unbounded.  It is empty exactly when non_empty (:265-274)
 *       says so: the start key above the end key, or equal to it with a side excluded.  An SST whose E[i] is empty
 *       takes part in nothing (try_with_visible_range, db_state.rs:169-176; the reference never builds such a view);
 *   P2. get, rule 1 under projection: SST i is in key k's chain iff E[i] holds k.  In a sorted run the covering
 *       SSTs are found as point_table_idx_covering_key finds them (db_state.rs:578-596): a partition point over the
 *       effective start keys max(first_key[i], visible start) (compacted_effective_start_key, :198-204), the last
 *       such SST if its E holds k, and the SSTs right before it while their E still holds k.  An L0 SST is a run of
 *       one (SstIterator::for_key -> calculate_view_range([k, k]) -> None).  An SST that is not in the chain is not
 *       probed, marked, checked or counted: it appears in neither ssts_read nor ssts_filtered and none of its errors
 *       surfaces; a tombstone or a newer version that the view hides shadows nothing.  Everything else of
 *       sdb_lsm_get rules 2-7, 3'/4' and F5 is unchanged;
 *   P3. scan, rules 1-3 under projection: for the pair (range r, SST i) the view range is V = range r intersected
 *       with visible[i] (calculate_view_range).  If V is empty the SST takes no part in r and is counted in neither
 *       range_ssts nor range_filtered.  Otherwise rules 1-3 hold with V in place of the range: participation is
 *       judged against [first_key, last_key], the blocks are partitions_covering_range(index, V.start, V.end), the
 *       candidates are the entries whose key V contains.  blocks_checked stays the exact size of the union of those
 *       blocks over the participating pairs; a corrupt block of an SST that no V covers never surfaces.  The
 *       capacity protocol, the ordering, sdb_lsm_scan_merge's rule 4 and the laziness rules are unchanged;
 *   P4. the filter query of a projected pair: the reference judges point_key on the view range (sst_iter.rs:82-87,
 *       849-856).  If V is Included(k)..=Included(k) the pair asks Point(k), also when the range is wide and has a
 *       prefix; otherwise Prefix(p) where has_prefix[r], else nothing, as F1.  For an SST whose projection is
 *       (UNBOUNDED, UNBOUNDED) V is the range, so F1 holds as it stands.  probe_len[r] belongs to the range's own
 *       query: a pair that is a point only through its projection has no caller-supplied length, so an
 *       SDB_PREFIX_LENGTHS SST answers None there ("might match").  The once-per-range hash of the agreeing-policies
 *       path serves the pairs whose query is the range's; a point-by-projection pair hashes for itself;
 *   P5. a malformed projection is found on the device, like a malformed run_start: a start kind other than
 *       SDB_BOUND_UNBOUNDED or SDB_BOUND_INCLUDED (new_projected's assert, db_state.rs:126-130), an end kind above
 *       SDB_BOUND_EXCLUDED, or offsets that descend fail EVERY query or range with SDB_INVALID_ARGUMENT, with
 *       blocks_checked 0, and nothing is read through the arrays.  On the host, proj->n != num_ssts, or a NULL array
 *       inside a non-NULL proj when num_ssts > 0, is SDB_INVALID_ARGUMENT from the call; SDB_DEVICE_ERROR comes
 *       after the host checks;
 *   P6. proj == NULL gives exactly the _filtered call: every column, counter and summary word; so do projections
 *       that are all (UNBOUNDED, UNBOUNDED);
 *   P7. the caller's obligation, as the manifest's projection guarantees it: within a sorted run the effective
 *       start keys ascend and neighbouring E share at most a boundary key.  The device does not verify this; a
 *       violation can lose rows but never reads out of bounds.
 * The workspace is that of the _filtered call: a pair's view range is recomputed where it is read.
 * ------------------------------------------------------------------------------------------- */
uint64_t sdb_lsm_get_projected_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs,
                                               uint64_t nkeys, int32_t merge /* 1: a chain is passed */);
sdb_status sdb_lsm_get_projected(const sdb_lsm_view *lsm, const sdb_scan_ranges *proj /* n == num_ssts; or NULL */,
                                 const sdb_filter_policy *policies /* device, num_ssts; or NULL */,
                                 const uint8_t *key_bytes, const uint64_t *key_off, uint64_t nkeys,
                                 const int32_t *probe_len /* device, nkeys; or NULL */,
                                 const uint64_t *max_seq /* device, nkeys; NULL = no bound */, const sdb_get_out *out,
                                 const sdb_chain_out *chain /* or NULL */, void *workspace, uint64_t workspace_bytes,
                                 void *stream);
uint64_t sdb_lsm_scan_projected_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs,
                                                uint64_t nranges, uint64_t cand_entries, uint64_t cand_key_bytes,
                                                int32_t merge /* 1: a chain is passed */);
sdb_status sdb_lsm_scan_projected(const sdb_lsm_view *lsm, const sdb_scan_ranges *proj /* n == num_ssts; or NULL */,
                                  const sdb_filter_policy *policies /* device, num_ssts; or NULL */,
                                  const sdb_scan_ranges *ranges, const sdb_scan_prefixes *prefixes /* or NULL */,
                                  const uint64_t *max_seq /* device, n; NULL = no bound */, int32_t descending,
                                  uint64_t cand_entries, uint64_t cand_key_bytes, const sdb_lsm_scan_out *out,
                                  const sdb_chain_out *chain /* or NULL */, const sdb_scan_filter_out *fout,
                                  void *workspace, uint64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Compaction (device): the output side of CompactionExecutor::run_subcompaction_merge
 * (compactor_executor.rs:386-410, 818-871) over decoded inputs:
 *   1. MergeIterator over the sorted runs, dedup off (merge_iterator.rs:56-69): key ascending, seq
 *      descending; equal (key, seq) pairs (which the store never writes) in run order;
 *   2. MergeOperatorRequiredIterator (merge_operator.rs:213-223): a merge operand fails the job with
 *      SDB_MERGE_OPERATOR_MISSING, unless `merge_operands` passes operands on unmerged;
 *   3. RetentionIterator (retention_iterator.rs:91-204, 381-398): per key, versions newest first,
 *      a later equal-seq version replacing an earlier one (BTreeMap::insert); expired merges are
 *      skipped, expired values / tombstones become tombstones without expire_ts; the walk stops
 *      after the first non-merge version outside both the seq and the time window; trailing
 *      tombstones are dropped when filter_tombstone;
 *   4. output SSTs cut where the bytes of the blocks the writer finished exceed max_sst_size: the
 *      entry whose add finished that block closes the SST as its one-entry tail block
 *      (compactor_executor.rs:833-858, sst_builder.rs:224-325); every SST then encodes as above.
 * sdb_merge_runs and sdb_sst_cuts are asynchronous on the caller's stream; sdb_compactor_run
 * orchestrates the whole job over decoded runs, sdb_compactor_run_ssts over encoded input SSTs.
 * ------------------------------------------------------------------------------------------- */
/* One sorted input run in the layout sdb_decode_blocks produces (a decoded SST, or a sorted run's
 * SSTs decoded into one output): value i = val_base[val_off[i] .. val_off[i] + val_len[i]). */
typedef struct sdb_run {
    uint64_t n;
    const uint8_t *key_arena;
    const uint64_t *key_off;        /* n+1 */
    const uint8_t *val_base;
    const uint64_t *val_off;        /* n */
    const uint32_t *val_len;        /* n */
    const uint64_t *seq;            /* n */
    const uint8_t *flags;           /* n: RowFlags (SDB_FLAG_*) */
    const int64_t *create_ts;       /* n: valid iff flags & HAS_CREATE_TS (NULL: none anywhere) */
    const int64_t *expire_ts;       /* n: valid iff flags & HAS_EXPIRE_TS (NULL: none anywhere) */
} sdb_run;
enum { SDB_MAX_RUNS = 32 };        /* runs of one sdb_merge_runs call; the compactor merges more in groups of
                                      this many first (up to SDB_MAX_RUNS^2 runs per job) */
typedef struct sdb_retention {
    uint64_t min_seq;               /* retention_min_seq: the walk continues past seq > min_seq
                                       (retention_iterator.rs:188-190) when has_min_seq */
    uint64_t time_seq;              /* retention_timeout resolved on the host: the walk continues past
                                       seq >= time_seq when has_time_window (create_sys_ts + timeout > now,
                                       :171-187; SequenceTracker::find_ts(.., RoundUp) is monotone in seq,
                                       so the seqs inside the window are an up-set; 0 = every seq) */
    int64_t compaction_start_ts;    /* compaction_clock_tick: expire_ts <= this has expired */
    uint8_t has_min_seq, has_time_window;
    uint8_t filter_tombstone;       /* is_dest_last_run */
    uint8_t merge_operands;         /* 0: MergeOperatorRequiredIterator; 1: operands pass unmerged */
    uint32_t pad;
} sdb_retention;
typedef struct sdb_merge_summary {
    uint64_t num_in;                /* entries of all runs */
    uint64_t num_out;               /* entries after retention */
    uint64_t key_bytes, val_bytes;  /* bytes written to the output arenas */
    uint64_t expired_values;        /* RetentionMetrics::expired_entries_purged_value */
    uint64_t expired_merges;        /* RetentionMetrics::expired_entries_purged_merge */
    int32_t status;                 /* SDB_OK | SDB_MERGE_OPERATOR_MISSING | SDB_INVALID_ARGUMENT (a run
                                       out of order: first_error_entry = its global index) */
    uint32_t pad;
    uint64_t first_error_entry;     /* merged position (or run entry) that raised status */
} sdb_merge_summary;
/* Merged, retained stream: an sdb_kv_batch (n = summary.num_out) in caller-owned device memory.
 * Capacities: cap_entries >= sum n, key_cap >= sum key bytes, val_cap >= sum value bytes. */
typedef struct sdb_merged_out {
    uint8_t *key_bytes;
    uint64_t key_cap;
    uint64_t *key_off;              /* cap_entries + 1 */
    uint8_t *val_bytes;
    uint64_t val_cap;
    uint64_t *val_off;              /* cap_entries + 1 */
    uint8_t *kind;
    uint64_t *seq;
    int64_t *create_ts;
    int64_t *expire_ts;
    uint8_t *ts_mask;
    uint64_t cap_entries;
    sdb_merge_summary *summary;     /* device-writable */
} sdb_merged_out;
uint64_t sdb_merge_runs_workspace_bytes(const sdb_run *runs, uint32_t nruns);
sdb_status sdb_merge_runs(const sdb_run *runs, uint32_t nruns, const sdb_retention *retention,
                          const sdb_merged_out *out, void *workspace, uint64_t workspace_bytes, void *stream);
/* SST boundaries of a compaction output stream: cut_start[0..*num_ssts] (device) are entry indices
 * with cut_start[0] = 0 and cut_start[*num_ssts] = n; SST i = entries [cut_start[i], cut_start[i+1]).
 * cut_cap >= n + 1 always suffices.  params: the output format (block size, restart interval). */
uint64_t sdb_sst_cuts_workspace_bytes(uint64_t n, const sdb_sst_params *params);
sdb_status sdb_sst_cuts(const sdb_kv_batch *batch, const sdb_sst_params *params, uint64_t max_sst_size,
                        uint64_t *cut_start, uint64_t cut_cap, uint64_t *num_ssts, void *workspace,
                        uint64_t workspace_bytes, void *stream);

/* A compaction job on the device: merge + retention + cuts + encode of every output SST, with the
 * outputs in the handle's device memory (valid until the next run or destroy). */
typedef struct sdb_compactor sdb_compactor;
typedef struct sdb_compacted_sst {
    uint64_t entry_start, entry_end;   /* range of the merged stream (sdb_compactor_merged) */
    const uint8_t *data;               /* device: the SST's data section */
    const uint64_t *block_off;         /* device: num_blocks + 1 */
    const uint32_t *block_first_entry; /* device: num_blocks + 1 (relative to entry_start) */
    const uint32_t *index_key_len;     /* device: num_blocks */
    const uint16_t *block_stats;       /* device: 3 per block */
    const uint8_t *bloom;              /* device: summary.bloom_len bytes */
    sdb_sst_summary summary;           /* host copy */
} sdb_compacted_sst;
sdb_compactor *sdb_compactor_create(int device);
void sdb_compactor_destroy(sdb_compactor *c);
sdb_status sdb_compactor_run(sdb_compactor *c, const sdb_run *runs, uint32_t nruns, const sdb_retention *retention,
                             const sdb_sst_params *params, uint64_t max_sst_size, void *stream, uint32_t *num_ssts);
/* The same job from the encoded input SSTs, decode included (compactor_executor.rs:327-390, load_iterators:
 * each input SST is read block by block and decoded; an L0 SST is a sorted run, a sorted run of several
 * SSTs is their concatenation).  Every input's blocks are decoded by one launch sequence (CRC check,
 * V1/V2 rows, key restore; values stay in place, like Bytes::slice), straight into the merge's runs; the
 * merged stream is sized from the inputs' SstStats, so the job synchronises with the host twice: for the
 * merged count with the cut list, and for the output SSTs' summaries.  Input i: an uncompressed data
 * section on the device and the counts its footer holds.  Runs: inputs [run_start[r], run_start[r+1]),
 * run_start == NULL: one run per input.  A failing input block fails the job with its status (lowest
 * block first; the merged summary's first_error_entry = that block's index among all inputs' blocks);
 * counts that disagree with the decoded blocks fail it with SDB_INVALID_ARGUMENT.  Any number of inputs
 * (their block tables go to device memory); more than SDB_MAX_RUNS runs are merged in groups first (one
 * more host synchronisation per group), up to SDB_MAX_RUNS^2 runs. */
typedef struct sdb_compaction_input {
    const uint8_t *data;            /* device: the data section (encoded blocks, each ++ crc32) */
    const uint64_t *block_off;      /* device: num_blocks + 1 (BlockMeta.offset of each block, then the
                                       data section length) */
    uint64_t num_blocks;
    uint64_t num_entries;           /* SstStats::num_rows() (num_puts + num_deletes + num_merges) */
    uint64_t key_bytes;             /* SstStats.raw_key_size */
    uint64_t val_bytes;             /* SstStats.raw_val_size */
} sdb_compaction_input;
sdb_status sdb_compactor_run_ssts(sdb_compactor *c, const sdb_compaction_input *inputs, uint32_t ninputs,
                                  const uint32_t *run_start, uint32_t nruns, uint16_t input_sst_version,
                                  const sdb_retention *retention, const sdb_sst_params *params,
                                  uint64_t max_sst_size, void *stream, uint32_t *num_ssts);
sdb_status sdb_compactor_sst(const sdb_compactor *c, uint32_t i, sdb_compacted_sst *out);
/* The merged stream of the last run (device batch view) and its summary (host copy). */
sdb_status sdb_compactor_merged(const sdb_compactor *c, sdb_kv_batch *batch, sdb_merge_summary *summary);

/* ---------------------------------------------------------------------------------------------
 * Compaction with a merge operator: the same two jobs with MergeOperatorIterator(op, iter,
 * merge_different_expire_ts = false, snapshot_barrier_seq = retention_min_seq) between the MergeIterator
 * and the RetentionIterator, as compaction and memtable flush build it (compactor_executor.rs:390-400,
 * flush.rs:212-222).  The device finds the operand chains in the merged order, the host runs `op` over
 * bytes the device gathered, and retention, cuts and encode run over the collapsed stream.
 *
 * The walk (merge_operator.rs:324-485) runs over the versions of one key in MergeIterator order (seq
 * descending, equal seqs in run order), before retention's equal-seq replacement, and partitions them
 * into units:
 *   - a version that is not a merge operand is a unit of its own (:474-476);
 *   - a merge operand with seq > barrier is a unit of its own (:465-469); barrier = retention->min_seq
 *     when has_min_seq, else there is none; the compare is strict;
 *   - any other merge operand opens a chain with first_expire_ts = its Option<expire_ts>.  Over the
 *     following versions of the key (:387-412): one whose Option<expire_ts> differs (None == None,
 *     Some(a) == Some(a) only; :330-335, checked before the kind) ends the chain without a base and starts
 *     the next unit; a matching value or tombstone ends the chain as its base and is consumed; a matching
 *     operand is a link.  The walk then goes on with the key's remaining versions.
 *   - a chain unit: seq = its first link's; create_ts = the maximum and expire_ts = the minimum over the
 *     links and the base that carry one (MergeTracker, :262-303); kind Value when a base was found (a
 *     tombstone base included: its value is None), else Merge (:437-441); value = the operands newest first
 *     in batches of 100 (MERGE_BATCH_SIZE), each batch reversed and merged with no existing value, the
 *     batch results reversed and merged once with the base (:341-447).  A chain of one link without a base
 *     goes through the operator twice like any other.
 * SDB_INVALID_SEQUENCE_ORDER (:293-299) cannot arise: the run-order check of the merge (SDB_INVALID_ARGUMENT)
 * already guarantees descending seqs per key.
 * Retention (retention_iterator.rs:91-204) then runs unchanged over the units: each unit's seq, kind,
 * expire_ts and value length.  An expired Merge unit is skipped and counts once in expired_merges.
 * retention->merge_operands is ignored: operands that reach retention are legitimate here.
 *
 * The operator.  Operands arrive oldest first; existing == NULL: no existing value.  *result must stay
 * valid until the next call with the same ctx; the library copies it at once.  A non-zero return fails the
 * job with SDB_MERGE_OPERATOR_ERROR, first_error_entry = the merged position of the chain's first link; no
 * output SST is valid.  op == NULL: SDB_INVALID_ARGUMENT.
 *
 * Host synchronisations: those of sdb_compactor_run / sdb_compactor_run_ssts, plus, between the merge order
 * and retention, one for the chain summary (groups, links, bytes: it sizes the tables) and, when the job has
 * a chain, one for the chain tables: a pinned D2H of the group table, the link table and the staging arena
 * (group keys and link values, gathered contiguously on the device), the operator calls, and an H2D of the
 * merged values and their offsets.  A job without a chain does no copy and never calls the operator.
 * sdb_compactor_run_ssts_merge sizes its value buffer as declared val_bytes - link_bytes + merged_bytes (a
 * merged value may be longer than all of its inputs).  sdb_compactor_sst / sdb_compactor_merged read the
 * results as for the other jobs.
 * ------------------------------------------------------------------------------------------- */
typedef int32_t (*sdb_merge_batch_fn)(void *ctx, const uint8_t *key, uint64_t key_len,
                                      const uint8_t *existing /* NULL: none */, uint64_t existing_len,
                                      const uint8_t *const *operands, const uint64_t *operand_len, uint32_t n,
                                      const uint8_t **result, uint64_t *result_len);
typedef struct sdb_merge_op_stats {
    uint64_t groups;                /* chains */
    uint64_t links;                 /* operands plus bases of every chain */
    uint64_t link_bytes;            /* value bytes of the links (D2H) */
    uint64_t merged_bytes;          /* value bytes of the chains' merged values (H2D) */
    uint64_t operator_calls;
} sdb_merge_op_stats;
sdb_status sdb_compactor_run_merge(sdb_compactor *c, const sdb_run *runs, uint32_t nruns,
                                   const sdb_retention *retention, sdb_merge_batch_fn op, void *ctx,
                                   const sdb_sst_params *params, uint64_t max_sst_size, void *stream,
                                   uint32_t *num_ssts);
sdb_status sdb_compactor_run_ssts_merge(sdb_compactor *c, const sdb_compaction_input *inputs, uint32_t ninputs,
                                        const uint32_t *run_start, uint32_t nruns, uint16_t input_sst_version,
                                        const sdb_retention *retention, sdb_merge_batch_fn op, void *ctx,
                                        const sdb_sst_params *params, uint64_t max_sst_size, void *stream,
                                        uint32_t *num_ssts);
/* The chains of the last sdb_compactor_run_merge / sdb_compactor_run_ssts_merge job (zeros after any other). */
sdb_status sdb_compactor_merge_stats(const sdb_compactor *c, sdb_merge_op_stats *stats);

/* ---------------------------------------------------------------------------------------------
 * Ranged compaction over SST views: sdb_compactor_run_ssts / _merge as the reference runs every job.
 * run_subcompaction_merge (compactor_executor.rs:779-881) handles a whole job (an unbounded range) and an RFC-0028
 * subcompaction on one path: load_iterators (:327-435) opens every input over job_args.range and its view, so an
 * input SST is read only over calculate_view_range(range) = range intersected with visible_range
 * (db_state.rs:243-251), and only the blocks partitions_covering_range returns for it are fetched.  `job_range`
 * and `proj` are sdb_scan_ranges with device arrays, exactly as the tree reads take them.
 *   R1. view range: V[i] = job_range intersected with visible[i] as BytesRange::intersect does
 *       (comparable_range.rs:224-236): the tighter start and the tighter end (P1).  V[i] is empty exactly when the
 *       start key lies above the end key, or equals it with a side excluded.  A projection of (UNBOUNDED, UNBOUNDED)
 *       means None.  An input whose V is empty contributes nothing: none of its blocks is read and none of its
 *       errors surfaces;
 *   R2. blocks: input i reads partitions_covering_range(index keys of i, V.start, V.end), exactly as sdb_sst_scan
 *       rule 1 (an excluded end that equals a block's index key leaves that block out).  Only these blocks are
 *       bounds- and CRC-checked and parsed: a corrupt block outside them never fails the job; a failing block inside
 *       them fails it with its status, lowest block first, first_error_entry = that block's index among ALL inputs'
 *       blocks (the numbering of sdb_compactor_run_ssts).  One deviation: an input whose keys all lie outside a
 *       non-empty V still has one covering block checked (the partition search needs no key of the SST's); the
 *       reference's sorted-run search would not open that SST;
 *   R3. rows: input i contributes the entries of those blocks whose key V[i] contains (SstView::contains): all
 *       versions of a key, or none.  A run is the concatenation of its inputs' contributions in input order; the
 *       rows dropped between two inputs leave no gap (the contributions are closed up into columns of their own
 *       whenever a row was dropped).  Ordering within a run is the caller's obligation (as P7); the merge's
 *       run-order check still reports a violation as SDB_INVALID_ARGUMENT;
 *   R4. everything after the inputs is unchanged: merge order, the operator walk when op != NULL
 *       (sdb_compactor_run_ssts_merge) or MergeOperatorRequiredIterator when op == NULL, retention, cuts and encode;
 *       more than SDB_MAX_RUNS runs merge in groups first.  sdb_compactor_sst, sdb_compactor_merged and
 *       sdb_compactor_merge_stats read the results as for the other jobs;
 *   R5. identity: with job_range == NULL (or unbounded) and proj == NULL (or all unbounded) the job's outputs,
 *       statuses and summary words are those of sdb_compactor_run_ssts / _merge on the same inputs;
 *   R6. counts: an input whose V is unbounded on both sides must decode to exactly its declared num_entries, as in
 *       sdb_compactor_run_ssts.  For a clipped input the declared counts are upper bounds: more decoded rows in its
 *       covering blocks than num_entries is SDB_INVALID_ARGUMENT (first_error_entry = its first covering block).
 *       The totals of key_bytes / val_bytes are exact when no input is clipped and upper bounds otherwise (the
 *       declared counts of the inputs that have a covering block size the decode and the merge);
 *   R7. malformed ranges.  Found on the device, failing the job with SDB_INVALID_ARGUMENT, blocks_checked 0 and
 *       nothing read through the arrays: a job bound kind above SDB_BOUND_EXCLUDED; a projection start other than
 *       UNBOUNDED / INCLUDED or an end kind above EXCLUDED; offsets that descend.  Found on the host,
 *       SDB_INVALID_ARGUMENT from the call before SDB_DEVICE_ERROR: job_range->n != 1; proj->n != ninputs; a NULL
 *       array inside a non-NULL struct; num_blocks > 0 with NULL data, block_off, index_keys or index_key_off;
 *   R8. synchronisations: exactly two more than sdb_compactor_run_ssts[_merge] on the same inputs, in every job
 *       (the unbounded one included).  The first reads the covering block range of every input (2 words per input
 *       and the ranges' status): it sizes the decode, its workspace and the merge from the covered blocks and the
 *       declared counts of the inputs that have any.  The second reads the gate and each run's first row (4 + nruns
 *       + 1 words): sdb_run.n and the merge's grid are host values.  A job that fails at either returns there.
 *       No allocation in steady state: the handle's buffers grow, and one handle serves ranged and whole jobs of
 *       any sizes in any order.
 * ------------------------------------------------------------------------------------------- */
typedef struct sdb_compaction_view {     /* one input SST as the ranged job reads it */
    sdb_compaction_input sst;            /* data, block_off, num_blocks and the SstStats counts (rule R6) */
    const uint8_t *index_keys;           /* device: BlockMeta.first_key of block k, as sdb_sst_view */
    const uint64_t *index_key_off;       /* device: num_blocks + 1 */
} sdb_compaction_view;
typedef struct sdb_range_job_stats {
    uint64_t inputs_read;                /* inputs with a non-empty block range */
    uint64_t blocks_total;               /* sum of num_blocks */
    uint64_t blocks_checked;             /* blocks CRC-checked and parsed: exactly the covering blocks (R2) */
    uint64_t entries_decoded;            /* rows of those blocks */
    uint64_t entries_in;                 /* rows inside their view range = merged summary num_in */
} sdb_range_job_stats;
sdb_status sdb_compactor_run_ssts_ranged(sdb_compactor *c, const sdb_compaction_view *inputs, uint32_t ninputs,
                                         const uint32_t *run_start, uint32_t nruns, uint16_t input_sst_version,
                                         const sdb_scan_ranges *job_range /* n == 1; or NULL = unbounded */,
                                         const sdb_scan_ranges *proj /* n == ninputs: visible_range per input; or NULL */,
                                         const sdb_retention *retention, sdb_merge_batch_fn op /* NULL: no operator */,
                                         void *ctx, const sdb_sst_params *params, uint64_t max_sst_size, void *stream,
                                         uint32_t *num_ssts);
/* The input side of the last sdb_compactor_run_ssts_ranged job (zeros after any other). */
sdb_status sdb_compactor_range_stats(const sdb_compactor *c, sdb_range_job_stats *stats);

/* ---------------------------------------------------------------------------------------------
 * Compaction filters and resumed jobs: the last two stages load_iterators builds (compactor_executor.rs:327-435),
 * CompactionFilterIterator (compaction_filter.rs, compaction_filter_iterator.rs) and ResumingIterator
 * (compactor_executor.rs:123-199, :333-338).  Order of a job: merge -> operator (or the required check) ->
 * retention -> filter -> resume drain -> writer (cuts, encode).
 *
 * Filter rules (compaction_filter_iterator.rs:19-66), over the rows retention yields, in stream order; one filter
 * instance per job, single-threaded:
 *   F1. Keep: the row passes unchanged.
 *   F2. Drop: the row vanishes; no tombstone is left.
 *   F3. Modify(Tombstone): kind becomes Tombstone, the value is empty, expire_ts is cleared (ts_mask loses
 *       SDB_TS_EXPIRE); create_ts, seq and key are kept.  This tombstone comes after retention, so filter_tombstone
 *       (is_dest_last_run) does not remove it.
 *   F4. Modify(Value(b)) / Modify(Merge(b)): kind becomes Value / Merge and the value becomes b (it may be empty, and
 *       longer than the original).  Key, seq, create_ts and expire_ts are preserved: a tombstone turned into a Value
 *       keeps its "no expire_ts".  A Merge written by a filter in a job without an operator is legal: the
 *       required-operator check sits before retention.
 *   F5. Errors: a filter error aborts the job.  on_compaction_end (`end`) runs once, after the last row of a job that
 *       did not fail; a job with no rows still runs it; an error from it aborts the job too.
 * Resume rules (ResumingIterator::new, :150-171; seek: retention_iterator.rs:279-283, merge_operator.rs:481-484,
 * merge_iterator.rs:18-37, 211-233), with the cursor (K, S) = the last row the interrupted job wrote:
 *   S1. seek(K) goes down to the inputs: only rows with key >= K are read.  Merge, operator and retention act per
 *       key, so the rows produced for keys >= K are exactly those of the unresumed job.  Rows below K contribute
 *       nothing: no summary counts, no filter calls, no errors from blocks that hold only such rows.
 *   S2. The leading rows with key == K && seq >= S are then drained one next() at a time from the filter's output,
 *       so the filter IS called for them.  The drain stops at the first surviving row with another key or with
 *       seq < S: a literal prefix, not a set.
 *   S3. The writer starts afresh at the first surviving row: the cuts count from there.
 * Reading the cursor out of the last output SST (last_written_key_and_seq) stays with the caller: a descending
 * sdb_sst_scan of one row yields it.
 *
 * The filter callback.  One call = rows [first, first + rows->n) of the retained stream, in HOST (pinned) memory, as
 * an sdb_kv_batch whose arrays are already offset to `first` (key_off / val_off stay absolute into key_bytes /
 * val_bytes).  rows->val_bytes == NULL unless want_values; val_off is always valid (lengths).  decision[] arrives
 * preset to KEEP.  For VALUE / MERGE the callback sets new_val[i] / new_len[i]; the library copies the bytes before
 * the next call.  Non-zero return: the job fails.
 *   F6. Identity: with filter == NULL && resume == NULL the outputs, statuses, summary words and host
 *       synchronisations are those of sdb_compactor_run[_merge] / sdb_compactor_run_ssts_ranged.
 *   F7. Keep-all fast path: a filter that keeps every row uploads nothing and launches no apply kernel
 *       (h2d_bytes == 0, applied == 0); the stream and every SST byte are those of the job without a filter.
 *   F8. Batching and `end`: calls are ascending and contiguous, batch_rows rows each (the last may be shorter; a
 *       stream of no rows gets no call); every retained row with key >= K is shown exactly once, the S2 rows
 *       included.  `end` is called once, after the last call, only if no call failed and the job has not failed
 *       earlier.
 *   F9. Failures.  A non-zero return from `filter`: SDB_COMPACTION_FILTER_ERROR, first_error_entry = `first` of that
 *       call, no SST valid, `end` not called.  A non-zero return from `end`: the same status, first_error_entry =
 *       rows_in.  A decision byte above SDB_CF_MERGE, or new_val == NULL with new_len > 0 (VALUE / MERGE):
 *       SDB_INVALID_ARGUMENT (first_error_entry = the row), found on the host before anything is uploaded; `end` is not
 *       called.  A replacement longer than 0xFFFFFFFF bytes (value lengths are u32): SDB_LIMIT_EXCEEDED, found and
 *       reported the same way.  filter->filter == NULL, resume->key == NULL with key_len > 0, or resume->key_len >
 *       0xFFFFFFFF: SDB_INVALID_ARGUMENT from the call.  In the decoded-runs job a cursor does not change what a run
 *       must carry: a run with n > 0 and a NULL key_arena, key_off, val_off, val_len, seq or flags is
 *       SDB_INVALID_ARGUMENT before anything is launched, as without a cursor.
 *   F10. Results: sdb_compactor_merged returns the final stream, after the filter and the drain (its key_off /
 *       val_off need not start at 0: a drained prefix stays in the arenas; its bytes end at key_off[n] / val_off[n]).
 *       summary.num_out / key_bytes / val_bytes / expired_* stay retention's.  sdb_compacted_sst.entry_start / _end
 *       index the final stream.  Every row dropped or drained: *num_ssts == 0 and SDB_OK, like an empty merge.
 * Host synchronisations, on top of the job's own (run: 3; ssts: R8's):
 *   - a filter adds one: the pinned D2H of the stream's columns (kind, seq, create_ts, expire_ts, ts_mask, key_off,
 *     val_off) and key bytes, and of the value bytes only when want_values; d2h_bytes counts exactly what was copied.
 *     The host then knows the final row count and bytes exactly, so the apply step and the cuts add none;
 *   - the ssts job sizes its merged stream from declared counts and learns n with its cut list; with a filter or a
 *     cursor it reads the merged summary first and cuts an unpadded stream: one more;
 *   - a cursor in the decoded-runs job adds one: the lower bound of K in every run (nruns words), so sdb_run.n and
 *     the merge's grid stay host values.  In the ssts job Included(K) is a third operand of R1's intersection: every
 *     V[i].start is tightened by it (such an input counts as clipped for R6), and it adds none;
 *   - S2 is computed on the host when a filter gathered the columns; without a filter a one-workgroup kernel and an
 *     8-byte readback compute it: one more (none when the stream is empty).
 * No allocation in steady state: the handle's buffers grow, and one handle serves filtered, resumed and plain jobs
 * in any order.
 * ------------------------------------------------------------------------------------------- */
enum { SDB_CF_KEEP = 0, SDB_CF_DROP = 1, SDB_CF_TOMBSTONE = 2, SDB_CF_VALUE = 3, SDB_CF_MERGE = 4 };
typedef int32_t (*sdb_compaction_filter_fn)(void *ctx, const sdb_kv_batch *rows, uint64_t first,
                                            uint8_t *decision, const uint8_t **new_val, uint64_t *new_len);
typedef int32_t (*sdb_compaction_end_fn)(void *ctx);          /* on_compaction_end; may be NULL */
typedef struct sdb_compaction_filter {
    sdb_compaction_filter_fn filter; sdb_compaction_end_fn end; void *ctx;
    uint64_t batch_rows;      /* rows per call; 0 = the whole stream in one call */
    uint32_t want_values;     /* 0: value bytes are not copied to the host */
    uint32_t pad;
} sdb_compaction_filter;
typedef struct sdb_resume_cursor { const uint8_t *key; uint64_t key_len; uint64_t seq; } sdb_resume_cursor; /* host */
typedef struct sdb_filter_stats {
    uint64_t rows_in;                  /* rows shown to the filter */
    uint64_t kept, dropped, tombstoned, new_values, new_merges;   /* by the filter's decisions */
    uint64_t calls, d2h_bytes, h2d_bytes;
    uint64_t applied;                  /* 1 iff the apply kernels ran */
    uint64_t resume_drained;           /* rows removed by S2 */
} sdb_filter_stats;
sdb_status sdb_compactor_run_filtered(sdb_compactor *c, const sdb_run *runs, uint32_t nruns,
                                      const sdb_retention *retention, sdb_merge_batch_fn op /* NULL: no operator */,
                                      void *op_ctx, const sdb_compaction_filter *filter /* or NULL */,
                                      const sdb_resume_cursor *resume /* or NULL */, const sdb_sst_params *params,
                                      uint64_t max_sst_size, void *stream, uint32_t *num_ssts);
sdb_status sdb_compactor_run_ssts_filtered(sdb_compactor *c, const sdb_compaction_view *inputs, uint32_t ninputs,
                                           const uint32_t *run_start, uint32_t nruns, uint16_t input_sst_version,
                                           const sdb_scan_ranges *job_range, const sdb_scan_ranges *proj,
                                           const sdb_retention *retention, sdb_merge_batch_fn op, void *ctx,
                                           const sdb_compaction_filter *filter /* or NULL */,
                                           const sdb_resume_cursor *resume /* or NULL */, const sdb_sst_params *params,
                                           uint64_t max_sst_size, void *stream, uint32_t *num_ssts);
/* The filter and resume stages of the last job (zeros after a job without either). */
sdb_status sdb_compactor_filter_stats(const sdb_compactor *c, sdb_filter_stats *stats);

/* ---------------------------------------------------------------------------------------------
 * WAL replay / device memtable: decoded rows in WAL (arrival) order -> the replayed memtables as sorted
 * runs, ready for the flush (sdb_compactor_run with one run).  Replaces WalReplayIterator::next
 * (wal_replay.rs:111-184) feeding KVTable::put (mem_table.rs:524-557), one skiplist insert per row.
 * Input: `nbatches` WAL batches in order, a batch being the rows of one WalRows (wal/slatedb/iterator.rs:
 * 376-423) in insertion order; the rows of all batches are concatenated in one sdb_run (what
 * sdb_decode_blocks* produces from WAL SST blocks), batch b = rows [batch_start[b], batch_start[b + 1]).
 * A batch may be empty.
 *   W1  a row with seq <= min_seq (when has_min_seq) is skipped (wal_replay.rs:146) and touches nothing.
 *   W2  the smallest seq of a non-empty batch must exceed the largest seq of every earlier batch
 *       (iterator.rs:394-419), over all rows, before W1: else status SDB_INVALID_ARGUMENT with
 *       first_error_entry = the first offending batch, and nothing is emitted.
 *   W3  a table's rows are ordered key ascending (<[u8] as Ord>), then seq descending (mem_table.rs:38-44).
 *   W4  of two kept rows with equal (key, seq) the later arrival replaces the earlier (compare_insert with
 *       an always-true predicate, mem_table.rs:540-547); by W2 both lie in one batch.
 *   W5  per batch, after W1 and W4: sdb_wal_batch_facts.
 *   W6  the host walks the facts: batches are applied in order, and a non-empty table whose
 *       estimate_encoded_size_compacted(entry_num, entries_size_in_bytes) >= max_memtable_bytes closes after
 *       the batch (wal_replay.rs:157-165); a table that had a batch applied is returned even when empty.
 *       The estimate is host configuration (format/sst.rs:1041-1160), so this step stays on the host:
 *       slatedb_amd/replay.py split_tables.
 *   W7  table metadata (entry_num, entries_size_in_bytes, first_seq, last_seq, last_tick) are sums / minima /
 *       maxima of the facts of the table's batches.
 * sdb_wal_replay_sort: W1, W2, the order of W3 as a permutation in the workspace, W4, W5 and the summary.
 * sdb_wal_replay_emit: given the W6 split (table t = batches [table_batch_start[t], table_batch_start[t + 1]),
 * ntables <= nbatches), the tables as one output stream: table t = rows [table_row_start[t],
 * table_row_start[t + 1]), viewed as an sdb_kv_batch like a compactor's cut SST views the merged stream
 * (key_off / val_off are offsets into the one arena; values are copied, so every table's are contiguous).
 * Both calls are asynchronous on `stream`, allocate nothing, can be captured into a HIP graph, and reuse
 * the workspace without a host reset.  Capacities: cap_entries >= n, key_cap >= the input's key bytes and
 * val_cap >= its value bytes always suffice; a short one gives SDB_LIMIT_EXCEEDED in the summary (with the
 * sizes needed) and nothing else is written.  batch_start must run monotonically from 0 to n and
 * table_batch_start from 0 to nbatches: checked on the device, a violation gives SDB_INVALID_ARGUMENT in
 * the summary (first_error_entry = the index of the offending element) and nothing is read through it.
 * n == 0 or nbatches == 0: SDB_OK with zeroed facts and summary (with n == 0 and batches, batch_start is still
 * checked: every element 0).  n < 2^31.
 * A live memtable collected in arrival order is the same pair of calls with nbatches = 1, has_min_seq = 0.
 * Out of scope: WAL object listing and fetch, touched_segments, the sequence tracker, and errors the WAL
 * iterator holds back (terminal_result): the caller stops feeding batches at the error.
 * ------------------------------------------------------------------------------------------- */
typedef struct sdb_wal_batch_facts {     /* W5; all zero for a batch no row of which passed W1 */
    uint64_t rows;                       /* rows that survive W1 and W4 */
    uint64_t bytes;                      /* sum of RowEntry::estimated_size (types.rs:48-60) over the survivors */
    uint64_t replaced;                   /* rows W4 removed */
    uint64_t min_seq, max_seq;           /* over every row that passed W1, replaced rows included (put updates
                                            them before the insert, mem_table.rs:531-537); valid iff rows > 0 */
    int64_t max_create_ts;               /* over the same rows that carry one; valid iff any_create_ts */
    uint32_t any_create_ts;
    uint32_t pad;
} sdb_wal_batch_facts;
typedef struct sdb_wal_replay_summary {
    uint64_t rows_in;                    /* n */
    uint64_t rows_skipped;               /* W1 */
    uint64_t rows_replaced;              /* W4 */
    uint64_t rows_out;                   /* survivors = rows of all tables */
    uint64_t key_bytes, val_bytes;       /* of the survivors (a tombstone's value bytes are 0) */
    int32_t status;                      /* SDB_OK | SDB_INVALID_ARGUMENT | SDB_LIMIT_EXCEEDED (emit) */
    uint32_t pad;
    uint64_t first_error_entry;          /* the batch (W2, batch_start) or table_batch_start element; else ~0 */
} sdb_wal_replay_summary;
typedef struct sdb_wal_tables_out {      /* the columns of sdb_merged_out + the tables' row ranges */
    uint8_t *key_bytes;
    uint64_t key_cap;
    uint64_t *key_off;                   /* cap_entries + 1 */
    uint8_t *val_bytes;
    uint64_t val_cap;
    uint64_t *val_off;                   /* cap_entries + 1 */
    uint8_t *kind;                       /* from the RowFlags: tombstone, merge operand, else value */
    uint64_t *seq;
    int64_t *create_ts;
    int64_t *expire_ts;
    uint8_t *ts_mask;
    uint64_t cap_entries;
    uint64_t *table_row_start;           /* device, ntables + 1 */
    sdb_wal_replay_summary *summary;     /* device-writable */
} sdb_wal_tables_out;
uint64_t sdb_wal_replay_workspace_bytes(uint64_t n, uint64_t nbatches);
sdb_status sdb_wal_replay_sort(const sdb_run *rows, const uint64_t *batch_start /* device, nbatches + 1 */,
                               uint64_t nbatches, uint64_t min_seq, int32_t has_min_seq,
                               sdb_wal_batch_facts *facts /* device, nbatches */,
                               sdb_wal_replay_summary *summary /* device */,
                               void *workspace, uint64_t workspace_bytes, void *stream);
sdb_status sdb_wal_replay_emit(const sdb_run *rows, const uint64_t *batch_start, uint64_t nbatches,
                               const uint64_t *table_batch_start /* device, ntables + 1, batch indices */,
                               uint64_t ntables, const sdb_wal_tables_out *out,
                               void *workspace /* as _sort left it */, uint64_t workspace_bytes, void *stream);
/* Rows one tile-sort workgroup orders in LDS (the tests sit on its boundaries). */
uint32_t sdb_diag_replay_tile(void);

/* ---------------------------------------------------------------------------------------------
 * Batched Db::get over device memtables and the tree (device): Reader::get_key_value_with_options
 * (reader.rs:133-182, 203-260) from the active memtable down.  The reference's get is one flat, lazy chain
 * (GetIterator::new, db_iter.rs:55-68, 102-124): the write batch, the active memtable, the immutable memtables
 * front first, the tree; max_seq is applied per leaf (apply_filters, db_iter.rs:215).  sdb_lsm_get_mem is
 * sdb_lsm_get_projected (itself the superset of the plain, _merge and _filtered gets) with memtables, sorted
 * runs in the sdb_run layout such as sdb_wal_replay_emit leaves them, searched ahead of run 0.
 *   M1. layers: a key's chain is tables 0 .. num_tables - 1 in order, then the tree chain of sdb_lsm_get rule 1
 *       (P2 under projection).  Filters and projections concern SSTs only;
 *   M2. one table: its rows are ordered key ascending, then seq descending (W3 of the replay,
 *       mem_table.rs:38-44).  It yields the entries with key == query and seq <= max_seq[q], in table order
 *       (KVTable::range(key..=key) under FilterIterator::new_with_max_seq).  The first of them is the lower
 *       bound of (query, max_seq) in that order, if the row there has the query's key.  A version above the
 *       bound is not seen, and an above-bound tombstone hides nothing.  Rows of other keys never match, also
 *       when one key is a proper prefix of its neighbour.  NULL create_ts / expire_ts mean none anywhere, as
 *       in sdb_run;
 *   M3. decision without a chain: the first layer that yields an entry decides; state and status follow
 *       sdb_lsm_get rule 3 (a merge operand: SDB_GET_MERGE_OPERAND / SDB_MERGE_OPERATOR_MISSING with its own
 *       columns).  When a table decides, mout->table and mout->row name the entry, out->sst = 0xFFFFFFFF,
 *       out->block = 0, val_off / val_len are the row's (tables[t].val_base[val_off .. + val_len); 0, 0 for a
 *       tombstone and for an empty value, as everywhere), seq, flags and the timestamps are the row's, and
 *       ssts_read = ssts_filtered = 0.  When the tree decides or nothing does, mout->table = 0xFFFFFFFF,
 *       mout->row = 0 and every sdb_get_out column is what sdb_lsm_get_projected writes.  Expiry is not
 *       filtered, as before;
 *   M4. with a chain: rules 3'/4' of sdb_lsm_get_merge run across the layers.  The walk goes on inside a table
 *       while rows are operands of the key, then into the next table, then into the tree.  A value ends the
 *       chain as its base; a tombstone ends it with no base, is no link, and its timestamps are not folded
 *       (db_iter.rs:108-114).  Links come newest first; a link lies either in a table (mchain->table / row;
 *       chain->sst = 0xFFFFFFFF, chain->block = 0, the other link columns the row's) or in an SST (chain->sst /
 *       block, mchain->table = 0xFFFFFFFF, mchain->row = 0).  The per-query columns are the newest link's with
 *       the MergeTracker aggregates over all links of all layers.  A link whose seq exceeds the newest link's
 *       fails the query with SDB_INVALID_SEQUENCE_ORDER, found per table as it is per run.  The cap_links
 *       protocol is unchanged, and covers the mchain columns;
 *   M5. laziness: a query that ends in the tables (without a chain: a table yields an entry; with a chain: a
 *       value or tombstone in a table ends it) consults no SST: it marks no block and probes no filter, no SST
 *       error surfaces for it, and ssts_read / ssts_filtered stay 0.  blocks_checked counts only blocks marked
 *       for the other queries; a batch decided entirely in the tables reports 0.  For the other queries
 *       everything is as in the projected call;
 *   M6. no tables: mem == NULL or num_tables == 0 gives exactly sdb_lsm_get_projected, every column, summary
 *       word and chain column; mout->table is all 0xFFFFFFFF and mout->row all 0 (the links' likewise);
 *   M7. no tree: num_ssts == 0, num_runs == 0 or total_blocks == 0 with tables present still searches the
 *       tables (a store that has only replayed its WAL has no SST); nothing is read through the tree's arrays.
 *       nkeys == 0 is SDB_OK with zeroed summaries;
 *   M8. arguments checked on the host: NULL lsm, out or mout, exactly one of chain and mchain, NULL
 *       mem->tables with num_tables > 0, a NULL array that nkeys > 0 (or cap_links > 0) needs, and a short
 *       workspace return SDB_INVALID_ARGUMENT from the call, besides what sdb_lsm_get_projected checks;
 *       nkeys * (num_runs + num_tables) over 2^40: SDB_LIMIT_EXCEEDED; after those, SDB_DEVICE_ERROR when no
 *       device is present;
 *   M9. arguments checked on the device: a table with n > 0 and a NULL key_arena, key_off, val_off, val_len,
 *       seq or flags, or with n >= 2^31, fails EVERY query with SDB_INVALID_ARGUMENT, and nothing is read
 *       through the tables.  The rows' order and the offsets' monotonicity are the caller's obligation, as
 *       sdb_compactor_run trusts its runs: a violation can lose entries but the search never leaves rows
 *       [0, n) of a table;
 *   M10. conventions: no allocation, no synchronisation, launches only on `stream`, capturable into a HIP graph
 *       as a linear sequence, the workspace reusable without a host-side reset.
 * sdb_lsm_get_mem_workspace_bytes(0, ...) equals sdb_lsm_get_projected_workspace_bytes(...).
 * Out of scope: the write batch (its rows all carry seq u64::MAX and are exempt from max_seq; it is one
 * transaction's private state and stays on the host, consulted first); the concurrent skiplist (a table here is a
 * finished sorted run); segments.  Scans over memtables: sdb_lsm_scan_mem below.
 * ------------------------------------------------------------------------------------------- */
typedef struct sdb_mem_view {
    const sdb_run *tables;   /* DEVICE array of num_tables sorted runs in search order: the active memtable,
                                then the immutable memtables front first (reader.rs:142-146) */
    uint32_t num_tables;     /* host value */
    uint32_t pad;
} sdb_mem_view;
typedef struct sdb_mem_get_out {     /* device arrays, one element per query */
    uint32_t *table;                 /* memtable that decided the get (0xFFFFFFFF: none, see out->sst) */
    uint64_t *row;                   /* row of the deciding entry in tables[table] (else 0) */
} sdb_mem_get_out;
typedef struct sdb_mem_chain_out {   /* device arrays, one element per link, cap = chain->cap_links */
    uint32_t *table;                 /* 0xFFFFFFFF: the link lies in chain->sst / chain->block */
    uint64_t *row;
} sdb_mem_chain_out;
uint64_t sdb_lsm_get_mem_workspace_bytes(uint32_t num_tables, uint64_t total_blocks, uint32_t num_ssts,
                                         uint32_t num_runs, uint64_t nkeys, int32_t merge /* 1: a chain is passed */);
sdb_status sdb_lsm_get_mem(const sdb_mem_view *mem /* or NULL */, const sdb_lsm_view *lsm,
                           const sdb_scan_ranges *proj /* n == num_ssts; or NULL */,
                           const sdb_filter_policy *policies /* device, num_ssts; or NULL */,
                           const uint8_t *key_bytes, const uint64_t *key_off, uint64_t nkeys,
                           const int32_t *probe_len /* device, nkeys; or NULL */,
                           const uint64_t *max_seq /* device, nkeys; NULL = no bound */, const sdb_get_out *out,
                           const sdb_mem_get_out *mout, const sdb_chain_out *chain /* or NULL */,
                           const sdb_mem_chain_out *mchain /* iff chain */, void *workspace, uint64_t workspace_bytes,
                           void *stream);

/* ---------------------------------------------------------------------------------------------
 * Batched Db::scan over device memtables and the tree (device): Reader::scan_with_options (reader.rs:275-320)
 * from the active memtable down.  ScanIterator merges the memtable iterators among themselves and the result
 * with the tree's iterators (db_iter.rs:145-163); max_seq is applied per leaf, before any deduplication
 * (db_iter.rs:205-217).  sdb_lsm_scan_mem is sdb_lsm_scan_projected (itself the superset of the plain, _merge and
 * _filtered scans) with the memtables of sdb_lsm_get_mem merged ahead of the tree; it is the scan counterpart of
 * that call and shares sdb_mem_view and sdb_mem_chain_out with it.  Everything not named here is as in
 * sdb_lsm_scan_projected.
 *   S1. sources: a range's sources are tables 0 .. num_tables - 1 in order, then the SSTs of `lsm` in their search
 *       order.  The order of the sources only breaks ties; within one source, rows with equal key and seq keep
 *       their physical order.  Filters, the prefixes' probes and projections concern SSTs only;
 *   S2. one table: its rows are ordered key ascending, then seq descending (M2).  The rows whose key range r
 *       contains are one contiguous stretch [g0, g1), found as two lower bounds over key_off / key_arena.  An
 *       excluded start steps over every version of the bound key, an included end keeps every version of it.  A
 *       key that is a proper prefix of its neighbour is a different key.  A range that is empty as a set, or has a
 *       bound kind above 2, reads nothing from any table.  A table with n == 0 takes part in nothing;
 *   S3. rows: rule 3 of sdb_lsm_scan over the union of the tables' stretches and the SST candidates.  Versions
 *       above max_seq[r] are dropped first, then the newest version per key wins; for an equal (key, seq) the
 *       earlier source wins, so a table wins before any SST.  A winning tombstone yields nothing, an above-bound
 *       tombstone hides nothing.  For a row that a table won: out->sst = 0xFFFFFFFF, val_off / val_len are the
 *       row's (tables[t].val_base[val_off .. + val_len); 0, 0 for an empty value), seq, flags and the timestamps
 *       are the row's (NULL create_ts / expire_ts mean none), and mout->table / row name the row.  For a row that
 *       an SST won every sdb_lsm_scan_out column is what the projected call writes, mout->table = 0xFFFFFFFF and
 *       mout->row = 0;
 *   S4. merge operands: without a chain a winning operand fails its range with SDB_MERGE_OPERATOR_MISSING, in a
 *       table as in an SST.  With a chain, rule 4 of sdb_lsm_scan_merge runs over the merged order of all sources:
 *       a chain runs through the tables and into the tree.  A link lies either in a table (chain->sst =
 *       0xFFFFFFFF, chain->block = 0, mchain->table / row, the other link columns the row's) or in an SST
 *       (mchain->table = 0xFFFFFFFF, mchain->row = 0), as in M4.  The MergeTracker aggregates fold over all links
 *       of all layers (and a tombstone base's timestamps, as in sdb_lsm_scan_merge).  The cap_links protocol is
 *       unchanged and covers the mchain columns;
 *   S5. nothing is lazy: every SST that takes part in a range is read and checked as rule 2 says, point ranges
 *       included.  A table that holds a range's newest versions shields the range from no block error: THIS
 *       DIFFERS FROM M5, where a get decided in the tables consults no SST.  blocks_checked, range_ssts and
 *       range_filtered are exactly the projected call's.  A failing range contributes no row from any source;
 *   S6. capacity: num_candidates / candidate_key_bytes count the tables' stretches too: g1 - g0 rows and
 *       key_off[g1] - key_off[g0] bytes per (range, table), before max_seq.  A range failed by a block, version or
 *       argument error stages none.  Both SDB_LIMIT_EXCEEDED cases are unchanged; when no column byte is written
 *       that includes the mout entry columns.  range_tables[r], the number of tables with a non-empty stretch for
 *       range r, is valid whenever range_ssts is;
 *   S7. no tables: mem == NULL or num_tables == 0 gives exactly sdb_lsm_scan_projected: every column, counter,
 *       summary word and chain column.  For the rows written mout->table is all 0xFFFFFFFF and mout->row all 0,
 *       and the links' likewise; range_tables is all 0.  sdb_lsm_scan_mem_workspace_bytes(0, ...) equals
 *       sdb_lsm_scan_projected_workspace_bytes(...);
 *   S8. no tree: num_ssts == 0, num_runs == 0 or total_blocks == 0 with tables present still scans the tables.
 *       Nothing is read through the tree's arrays, the tree's kernels are not launched, and blocks_checked is 0.
 *       n == 0 is SDB_OK with zeroed summaries;
 *   S9. arguments checked on the host: NULL lsm, out or mout, exactly one of chain and mchain, NULL mem->tables
 *       with num_tables > 0, a NULL array that a non-empty input needs, and a short workspace return
 *       SDB_INVALID_ARGUMENT from the call, besides what sdb_lsm_scan_projected checks; n * (num_ssts +
 *       num_tables) over 2^40: SDB_LIMIT_EXCEEDED; after all host checks, SDB_DEVICE_ERROR when no device is
 *       present.  On the device, as M9: a table with n > 0 and a NULL key_arena, key_off, val_off, val_len, seq or
 *       flags, or with n >= 2^31, fails EVERY range with SDB_INVALID_ARGUMENT and blocks_checked 0, and nothing is
 *       read through the tables.  The rows' order and the offsets' monotonicity are the caller's obligation: a
 *       violation may lose rows but the scan never leaves rows [0, n) of a table, or a pair's staging slots;
 *   S10. conventions: no allocation, no synchronisation, launches only on `stream`, capturable into a HIP graph as
 *       a linear sequence, the workspace reusable without a host-side reset.
 * Out of scope: the write batch (it stays on the host, merged on top); the live skiplist (a table here is a
 * finished sorted run); segments; and the lazy GetIterator the reference substitutes for a point range k..=k (a
 * point range is scanned like any other: callers who need a get's laziness call sdb_lsm_get_mem).
 * ------------------------------------------------------------------------------------------- */
typedef struct sdb_mem_scan_out {    /* device arrays */
    uint32_t *table;                 /* cap_entries: memtable that holds the row (0xFFFFFFFF: see out->sst) */
    uint64_t *row;                   /* cap_entries: its row in tables[table] (else 0) */
    uint32_t *range_tables;          /* n: tables that hold at least one key of range r (before max_seq) */
} sdb_mem_scan_out;
uint64_t sdb_lsm_scan_mem_workspace_bytes(uint32_t num_tables, uint64_t total_blocks, uint32_t num_ssts,
                                          uint32_t num_runs, uint64_t nranges, uint64_t cand_entries,
                                          uint64_t cand_key_bytes, int32_t merge /* 1: a chain is passed */);
sdb_status sdb_lsm_scan_mem(const sdb_mem_view *mem /* or NULL */, const sdb_lsm_view *lsm,
                            const sdb_scan_ranges *proj /* n == num_ssts; or NULL */,
                            const sdb_filter_policy *policies /* device, num_ssts; or NULL */,
                            const sdb_scan_ranges *ranges, const sdb_scan_prefixes *prefixes /* or NULL */,
                            const uint64_t *max_seq /* device, n; NULL = no bound */, int32_t descending,
                            uint64_t cand_entries, uint64_t cand_key_bytes, const sdb_lsm_scan_out *out,
                            const sdb_mem_scan_out *mout, const sdb_chain_out *chain /* or NULL */,
                            const sdb_mem_chain_out *mchain /* iff chain */, const sdb_scan_filter_out *fout,
                            void *workspace, uint64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Batched Db::scan_prefix_by_recency over device memtables and the tree (device): Db::scan_prefix_by_recency /
 * scan_prefix_by_recency_with_options (db.rs:1140-1323) -> Reader::scan_prefix_by_recency_with_options
 * (reader.rs:322-428) -> DbRecencyIterator (db_iter.rs:376-442), read up to a row limit.  This is NOT a merge: the
 * sources are drained one after another, newest source first, nothing is deduplicated across them, tombstones and
 * merge operands come back as raw rows, the key order restarts at every source boundary, and the caller is expected to
 * stop early.  sdb_lsm_scan_recency takes what sdb_lsm_scan_mem takes, minus the chain and plus `limit`; the caller
 * passes the prefix's range (BytesRange::from_prefix, reader.rs:345) in `ranges` and the prefix in `prefixes`, as for
 * sdb_lsm_scan_filtered.  Everything not named here is as in sdb_lsm_scan_mem (S1-S10) and the calls it is the superset
 * of.
 *   R1. sources and walk order (reader.rs:374-424): tables 0 .. num_tables - 1, then the runs of `lsm`, newest first.
 *       A sorted run is ONE source (SortedRunIterator, reader.rs:414-422), and an L0 SST is a run of one
 *       (reader.rs:395-406).  Ascending, a run's SSTs are walked in `ssts` order.  Descending, a run's SSTs are walked
 *       last to first, while the runs themselves stay newest first.  The reference's SortedRunIterator always pops
 *       from the front, and segment_iterator.rs:44-45 states that descending over sorted runs is broken there: this
 *       call implements the intended order.  A table without a row of the range, and a run none of whose SSTs takes
 *       part in the range (rule 1 of sdb_lsm_scan, after the filters), hold nothing to open: they are no sources of
 *       the range;
 *   R2. rows of a source: the pair's candidates exactly as sdb_lsm_scan_mem defines them: participation, the filter
 *       (F1-F3), the view range, the block clip, a table's stretch (S2).  Rows with seq > max_seq[r] are dropped per
 *       source (apply_filters, db_iter.rs:354-374).  Nothing else is dropped: every visible version of every key is
 *       a row.  A tombstone is a row with val_off = val_len = 0.  A merge operand is a row, never an error
 *       (db_iter.rs:404-407): SDB_MERGE_OPERATOR_MISSING cannot come out of this call;
 *   R3. order inside a source: ascending, the physical order (key ascending, seq descending).  Descending, the keys
 *       descend and the versions of one key stay newest first, as sdb_sst_scan rule 3 (sst_iter.rs:567-651).  A
 *       key's versions may straddle two SSTs of a run: each SST is ordered on its own and nothing is joined across
 *       them;
 *   R4. output: range r's rows are the concatenation over the walk order, at [range_entry_start[r],
 *       range_entry_start[r + 1]).  The columns are those of S3 for "a row that a table won" / "a row that an SST
 *       won": out->sst / mout->table, row, the flags as stored, the timestamps.  key_off and key_arena as in every
 *       scan;
 *   R5. limit and laziness (DbRecencyIterator::next_entry initialises a source only when the walk reaches it,
 *       db_iter.rs:413-440).  With L = limit[r] > 0 the range returns the first L rows of R4.  The walk opens
 *       source j iff the sources before it yielded fewer than L rows; a source that yields no visible row is passed
 *       and counts as read; the stop source is the one in which the L-th row lies.  Only an opened source can fail
 *       the range: a block error, an invalid version, a NULL array.  An opened source has every block of its covering
 *       ranges checked, wherever in it the L-th row lies: every participating SST of an opened run counts.  The
 *       status is that of the first failing source in walk order: inside it the first failing SST in walk order, then
 *       the lowest block.  A failing range returns no row, as sdb_lsm_scan rule 5, and its range_visible is 0.  A
 *       filtered-out SST is never opened and counts in range_filtered, not in range_sources_read.  As sdb_lsm_get
 *       rule 4, the call may check blocks of sources the walk never reaches: those results never surface, and
 *       blocks_checked counts what was checked.  limit == NULL or L == 0 drains every source: then any failing
 *       participant fails the range.  range_sources_read[r] counts the sources the walk opened, the stop source or
 *       the failing source included; range_visible[r] counts the rows at or below max_seq[r] in them;
 *   R6. capacity: every pair without an error stages its candidates, reached or not; a pair with an error stages
 *       none.  The two SDB_LIMIT_EXCEEDED cases and "no column byte is written" are as in S6; num_entries counts the
 *       rows after `limit`.  When the candidates do not fit, no row was counted and the walk cannot be told: then
 *       range_status is that of L == 0 (the first failing participant in walk order) and range_sources_read and
 *       range_visible are all 0;
 *   R7. arguments, malformed trees and tables, no tables, no tree, conventions: as S7-S10 (with no table the rows'
 *       mout columns are 0xFFFFFFFF / 0 and range_tables is 0; with no tree only the tables are walked).
 *       Additionally a NULL rout, or a NULL array in it for n > 0, is SDB_INVALID_ARGUMENT.  The call is capturable
 *       into a HIP graph as a linear sequence and the workspace is reusable without a host-side reset.
 * Out of scope: the write batch; segments (RecencyScanPrefixSpansMultipleSegments, reader.rs:360-368, is the host's
 * check before the call); laziness finer than a source.
 * ------------------------------------------------------------------------------------------- */
typedef struct sdb_recency_out {        /* device */
    uint32_t *range_sources_read;       /* n: sources the walk opened for range r, the stop source included (R5) */
    uint64_t *range_visible;            /* n: rows at or below max_seq[r] in those sources (>= rows returned) */
} sdb_recency_out;
uint64_t sdb_lsm_scan_recency_workspace_bytes(uint32_t num_tables, uint64_t total_blocks, uint32_t num_ssts,
                                              uint32_t num_runs, uint64_t nranges, uint64_t cand_entries,
                                              uint64_t cand_key_bytes);
sdb_status sdb_lsm_scan_recency(const sdb_mem_view *mem /* or NULL */, const sdb_lsm_view *lsm,
                                const sdb_scan_ranges *proj /* n == num_ssts; or NULL */,
                                const sdb_filter_policy *policies /* device, num_ssts; or NULL */,
                                const sdb_scan_ranges *ranges, const sdb_scan_prefixes *prefixes /* or NULL */,
                                const uint64_t *max_seq /* device, n; NULL = no bound */,
                                const uint64_t *limit /* device, n; NULL or 0 = drain every source */,
                                int32_t descending, uint64_t cand_entries, uint64_t cand_key_bytes,
                                const sdb_lsm_scan_out *out, const sdb_mem_scan_out *mout,
                                const sdb_scan_filter_out *fout, const sdb_recency_out *rout,
                                void *workspace, uint64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * SST footer (host): everything after the data section, so data ++ footer is the whole SST object
 * EncodedSsTableBuilder::build / EncodedWalSsTableBuilder::build hand to write_sst.
 * Replaces EncodedSsTableFooterBuilder::build (format/sst.rs:383-487) plus the index the builders
 * accumulate per block (sst_builder.rs:228-237, 307-313; wal/slatedb/sst_builder.rs:129-205),
 * SstStats::encode (sst_stats.rs:52-86) and SsTableInfo::encode (format/sst.rs:195-199).
 * Layout: [filter block + crc]? [index + crc] [stats + crc]? [SsTableInfo + crc] [u64 BE meta
 * offset] [u16 BE version]; flatbuffer bytes identical to the `flatbuffers` 25.12.19 crate.
 * ------------------------------------------------------------------------------------------- */
typedef struct sdb_footer_in {
    uint16_t sst_version;             /* trailing u16 (SST_FORMAT_VERSION: 1 or 2) */
    uint8_t sst_type;                 /* SDB_SST_COMPACTED | SDB_SST_WAL */
    uint8_t has_filter;               /* write the composite "_bf" filter block */
    uint32_t num_probes;              /* Filter::encode header (filter.rs:177-180) */
    uint64_t data_len;                /* blocks_size: bytes of the data section before the footer */
    uint64_t num_blocks;
    const uint64_t *block_off;        /* num_blocks: BlockMeta.offset */
    const uint8_t *first_key_bytes;   /* BlockMeta.first_key of block k = */
    const uint64_t *first_key_off;    /*   first_key_bytes[first_key_off[k] .. first_key_off[k+1]) */
    const uint8_t *first_entry;       /* SsTableInfo.first_entry; NULL = None */
    uint64_t first_entry_len;
    const uint8_t *last_entry;        /* SsTableInfo.last_entry; NULL = None (WAL) */
    uint64_t last_entry_len;
    const sdb_sst_summary *stats;     /* SstStats totals; NULL = no stats block (WAL) */
    const uint16_t *block_stats;      /* 3 per block (puts, deletes, merges) */
    const uint8_t *bloom;             /* bitmap (has_filter) */
    uint64_t bloom_len;
    const char *filter_name;          /* FilterPolicy::name: NULL = "_bf"; a prefix / no-whole-key policy
                                         is "_bf:p=<extractor>[:wh=0]" (filter_policy.rs:237-250) */
    uint32_t compression;             /* SsTableInfo.compression_format (SDB_CODEC_*): the filter, index and
                                         stats blocks go through compress_and_transform with that codec: zlib
                                         level 6, hash-chain LZ4 / Snappy, zstd with predefined FSE sequences,
                                         each kept only when shorter than the literal-only stream (host code,
                                         sdb_host_codec.cpp; the data blocks: sdb_compress_blocks) */
    uint32_t pad;
} sdb_footer_in;
/* Writes the footer into out[0..cap) and its length into *len.  out == NULL: size query only.
 * cap too small: SDB_LIMIT_EXCEEDED (with *len set). */
sdb_status sdb_sst_footer(const sdb_footer_in *in, uint8_t *out, uint64_t cap, uint64_t *len);
/* Upper bound on the footer length (arithmetic only), to size `out` for a single sdb_sst_footer call. */
uint64_t sdb_sst_footer_bound(const sdb_footer_in *in);

/* ---------------------------------------------------------------------------------------------
 * Host entry points: device arena + pinned staging per handle (E2E path: H2D -> kernels -> D2H)
 * ------------------------------------------------------------------------------------------- */
typedef struct sdb_encoder sdb_encoder;

/* Host-memory view of one encoded SST (arrays owned by the encoder, valid until the next call). */
typedef struct sdb_sst_host_result {
    sdb_sst_summary summary;
    const uint8_t *data;
    const uint64_t *block_off;
    const uint32_t *block_first_entry;
    const uint32_t *index_key_len;
    const uint16_t *block_stats;
    const uint8_t *bloom;
    double h2d_ms, kernel_ms, d2h_ms;   /* hipEvent timings of the last call */
} sdb_sst_host_result;

sdb_encoder *sdb_encoder_create(int device, const sdb_sst_params *params);
void sdb_encoder_destroy(sdb_encoder *enc);
/* Encode a host batch; returns the first error (host-side or device-side). */
sdb_status sdb_encoder_encode_host(sdb_encoder *enc, const sdb_kv_batch *host_batch,
                                   sdb_sst_host_result *result);
/* Encode `count` host batches (the SSTs of one L0 flush or of a compaction's output, config.rs:
 * 1081, 1383-1390) with their transfers overlapped: SST i+1's marshal and H2D and SST i-1's D2H run
 * while SST i's kernels do (two slots of pinned staging, separate H2D / kernel / D2H streams).
 * results[i] views host memory owned by the encoder, valid until the next call; returns the first
 * SST status that is not SDB_OK (every SST is still attempted); the *_ms timings are 0. */
sdb_status sdb_encoder_encode_host_many(sdb_encoder *enc, uint32_t count, const sdb_kv_batch *host_batches,
                                        sdb_sst_host_result *results);

/* Mirror of EncodedSsTableBuilder's per-entry surface (sst_builder.rs:224-276,370-417). */
typedef struct sdb_sst_builder sdb_sst_builder;
sdb_sst_builder *sdb_sst_builder_new(int device, const sdb_sst_params *params);
void sdb_sst_builder_free(sdb_sst_builder *b);
/* add(entry): kind per SDB_KIND_*, timestamps present iff the has_* flags are non-zero. */
sdb_status sdb_sst_builder_add(sdb_sst_builder *b, const uint8_t *key, uint64_t key_len,
                               uint8_t kind, const uint8_t *val, uint64_t val_len, uint64_t seq,
                               int32_t has_create_ts, int64_t create_ts, int32_t has_expire_ts,
                               int64_t expire_ts);
/* build(): encode everything added so far on the GPU. */
sdb_status sdb_sst_builder_build(sdb_sst_builder *b, sdb_sst_host_result *result);

/* Host decode of encoded blocks (H2D, decode kernels, D2H).  Arrays owned by the handle. */
typedef struct sdb_decoder sdb_decoder;
typedef struct sdb_decode_host_result {
    sdb_decode_summary summary;
    const uint64_t *block_entry_start;
    const uint8_t *key_arena;
    const uint64_t *key_off;
    const uint64_t *val_off;
    const uint32_t *val_len;
    const uint64_t *seq;
    const uint8_t *flags;
    const int64_t *create_ts;
    const int64_t *expire_ts;
    const uint32_t *bad_block;
} sdb_decode_host_result;
sdb_decoder *sdb_decoder_create(int device);
void sdb_decoder_destroy(sdb_decoder *dec);
sdb_status sdb_decoder_decode_host(sdb_decoder *dec, const uint8_t *blocks,
                                   const uint64_t *block_off, uint64_t nblocks,
                                   uint16_t sst_version, sdb_decode_host_result *result);

/* ---------------------------------------------------------------------------------------------
 * Diagnostics (bench / profiling only)
 * ------------------------------------------------------------------------------------------- */
/* Stage timing of sdb_encode_sst: when enabled, hipEvents are recorded around each kernel stage
 * (bloom, k_facts, k_seg, k_anchor, k_blocks, k_emit, k_emit_big, bloom_fill).  sdb_diag_stage_times synchronises the
 * recorded events, writes the summed milliseconds per stage into ms[0..max_stages), the number of
 * encodes measured into *launches, clears the record, and returns the number of stages. */
void sdb_diag_enable_stage_timing(int on);
int sdb_diag_stage_times(double *ms, int max_stages, uint64_t *launches);
/* The block CRC32 (crc32fast::hash, the checksum compress_and_transform appends, format/sst.rs:541-552)
 * of n device ranges data[off[i], off[i+1]), 4 <= length <= 4096, one wave per range: method 0 the
 * slicing-by-8 wave CRC, 1 the matrix-core (MFMA) wave CRC the kernels use.  Results in out[0, n). */
sdb_status sdb_diag_crc32_blocks(const uint8_t *data, const uint64_t *off, uint64_t n, uint32_t *out, int method,
                                 void *stream);
/* One v_mfma_i32_32x32x32_i8 with lane-supplied operands (a, b: 64 lanes x 4 dwords; d: 64 x 16
 * dwords, lane-major): pins the operand / result lane maps the MFMA CRC relies on. */
sdb_status sdb_diag_mfma_i8(const int32_t *a, const int32_t *b, int32_t *d, void *stream);
/* A hand-written STREAM copy (16 bytes per lane, grid-stride) of `bytes` (a multiple of 16, 16-byte aligned):
 * bench.py's attainable-HBM ceiling beside the 8 TB/s spec. */
sdb_status sdb_diag_copy(void *dst, const void *src, uint64_t bytes, void *stream);
/* Bandwidth probes over `bytes` (a multiple of 4096, 16-byte aligned), wg_per_cu x CUs workgroups of 256
 * threads: mode 0 sdb_diag_copy, 1 the same copy with plain loads / stores, 2 a copy by 4 KiB per wave
 * and step, 3 read only, 4 write only. */
sdb_status sdb_diag_bw(void *dst, const void *src, uint64_t bytes, int mode, int wg_per_cu, void *stream);

/* Device query: number of visible HIP devices (0 on a machine without a GPU). */
int sdb_device_count(void);
/* Human-readable name of a status code. */
const char *sdb_status_name(int status);

#ifdef __cplusplus
}
#endif
#endif /* SLATEDB_AMD_H */
