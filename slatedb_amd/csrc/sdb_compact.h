// sdb_compact.h — kernel arguments of the compaction output side (sdb_compact.hip) and of the ranged job's input
// side (sdb_compact_range.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slatedb_amd.h"
#include "sdb_encode.h"

namespace sdb {

constexpr uint32_t kMaxRuns = SDB_MAX_RUNS;
#ifndef SDB_MERGE_TILE
#define SDB_MERGE_TILE 1024
#endif
#ifndef SDB_MERGE_THREADS
#define SDB_MERGE_THREADS 512
#endif
constexpr uint32_t kMergeTile = SDB_MERGE_TILE;  // merged positions per tile: one k_mg_emit workgroup, one row of the tile sums
constexpr uint32_t kMergeThreads = SDB_MERGE_THREADS;

struct RunDesc {  // sdb_run + the run's first global entry index
    uint64_t n, base;
    const uint8_t *key_arena;
    const uint64_t *key_off;
    const uint8_t *val_base;
    const uint64_t *val_off;
    const uint32_t *val_len;
    const uint64_t *seq;
    const uint8_t *flags;
    const int64_t *create_ts;
    const int64_t *expire_ts;
};

// ---- operand chains of a compaction with a merge operator (k_mg_chain, k_mg_chain_scan, k_mg_chain_emit) ----
// What a merged position is in the stream MergeOperatorIterator yields (merge_operator.rs:324-485; the rules
// are restated in include/slatedb_amd.h, "Compaction with a merge operator").
constexpr uint8_t kUnitAbsorbed = 0;  // a link (or the base) of a chain that starts at an earlier position
constexpr uint8_t kUnitPass = 1;      // a unit of its own
constexpr uint8_t kUnitChain = 2;     // the first link of a chain without a base: kind Merge
constexpr uint8_t kUnitChainBase = 3; // the first link of a chain with a base: kind Value
constexpr uint8_t kBaseNone = 0, kBaseValue = 1, kBaseTombstone = 2;
struct ChainGroup {  // one chain; read by the host
    uint64_t head;       // merged position of its first link: its links are positions [head, head + nlinks)
    uint64_t link0;      // its first entry of the link table
    uint64_t nlinks;     // operands plus the base
    uint64_t seq;        // the first link's
    int64_t create_ts, expire_ts;  // max / min over the links that carry one (ts_mask: SDB_TS_*)
    uint64_t key_off;    // its key in the staging arena
    uint32_t key_len;
    uint8_t base, ts_mask;
    uint16_t pad;
};
struct ChainLink {  // newest first within a group; the base (if any) is the group's last link
    uint64_t off;    // its value in the staging arena
    uint64_t pos;    // merged position
    uint32_t len, pad;
};
struct ChainSummary {
    uint64_t groups, links, link_bytes, key_bytes;
};
struct ChainArgs {  // all NULL in a job without a merge operator
    uint8_t *unit;        // per merged position: kUnit*
    uint64_t *uinfo;      // per chain head: its link count (k_mg_chain), then its group (k_mg_chain_emit)
    uint64_t *ubytes;     // per chain head: the value bytes of its links
    uint64_t *tile_sum;   // per tile of head positions: groups, links, link bytes, key bytes (exclusive after the scan)
    ChainSummary *summary;
    ChainGroup *group;    // the tables: sized from the summary
    ChainLink *link;
    uint8_t *arena;       // group keys [0, key_bytes), then link values
    const uint64_t *moff; // uploaded: group g's merged value = mval[moff[g], moff[g + 1])
    const uint8_t *mval;
};
// Sizes (w == NULL) or binds the per-position chain state of a merge of `total` entries.
inline uint64_t chain_bind(ChainArgs &c, uint64_t total, uint8_t *w) {
    const uint64_t ntiles = (total + kMergeTile - 1) / kMergeTile;
    Carver k{w, 0};
    k.take(c.unit, total + 1);
    k.take(c.uinfo, total + 1);
    k.take(c.ubytes, total + 1);
    k.take(c.tile_sum, 4 * (ntiles + 1));
    k.take(c.summary, 1);
    return k.off;
}
// Sizes or binds the chain tables a summary asks for.
inline uint64_t chain_tables_bind(ChainArgs &c, const ChainSummary &s, uint8_t *w) {
    Carver k{w, 0};
    k.take(c.group, s.groups);
    k.take(c.link, s.links);
    k.take(c.arena, s.key_bytes + s.link_bytes);
    return k.off;
}

struct MergeArgs {
    uint32_t nruns, ntiles;
    uint32_t raw, pad;           // raw: no retention, no merge-operand check (every entry kept as it is)
    uint64_t total;
    sdb_retention ret;
    sdb_merged_out out;
    // workspace
    uint64_t *pfx;               // per global entry: key bytes [L0, L0 + 8), big-endian, zero padded
    uint32_t *lcp0;              // L0: the prefix every key of the (sorted) runs shares
    uint64_t *perm;              // merged position -> global entry
    uint8_t *dec;                // merged position: 0 drop, 1 keep, 2 keep as a tombstone
    uint64_t *tile_sum;          // per tile: kept entries, key bytes, value bytes (exclusive offsets after k_mg_scan)
    uint64_t *bound;             // per 256 entries (k_mg_rank workgroup) and side: the first / last entry's count in each run
    unsigned long long *err;     // run order violations: min (global entry << 8 | code)
    unsigned long long *err_merge;  // merge operands (MergeOperatorRequiredIterator): min merged position << 8 | code
    unsigned long long *metric;  // expired values, expired merges
    const unsigned long long *gate;  // NULL, or (entry << 8 | status) of a failed input (~0: none): no merge
    ChainArgs ch;
    RunDesc r[kMaxRuns];
};
static_assert(sizeof(MergeArgs) < 4000, "MergeArgs is passed as kernel arguments");

// Sizes (w == NULL) or binds the workspace of a merge of a.total entries.
inline uint64_t merge_bind(MergeArgs &a, uint8_t *w) {
    const uint64_t ntiles = (a.total + kMergeTile - 1) / kMergeTile;
    Carver c{w, 0};
    c.take(a.pfx, a.total + 1);
    c.take(a.perm, a.total + 1);
    c.take(a.dec, a.total + 1);
    c.take(a.tile_sum, 3 * (ntiles + 1));
    c.take(a.bound, 2 * (uint64_t)kMaxRuns * ((a.total + 255) / 256 + 1));  // k_mg_bounds: 2 x runs per 256 entries
    c.take(a.err, 1);
    c.take(a.err_merge, 1);
    c.take(a.metric, 2);
    c.take(a.lcp0, 2);
    return c.off;
}

sdb_status build_merge_args(const sdb_run *runs, uint32_t nruns, const sdb_retention *ret, const sdb_merged_out *out,
                            void *workspace, uint64_t workspace_bytes, MergeArgs *a, bool raw = false);
// A merged stream as an sdb_run (the per-entry value lengths and RowFlags the runs carry): val_len[i],
// flags[i] for i < n (device, written on st).
hipError_t launch_merged_as_run(const sdb_merged_out &out, uint64_t n, uint32_t *val_len, uint8_t *flags, hipStream_t st);
// A merge in three steps, all on `st`.  Retention and the emit run over the units of a merge operator when
// a.ch is bound (a.ch.unit != NULL; a.ch.moff / mval uploaded), else over the entries.
//   launch_merge_order        perm (the merged order), the run-order check
//   launch_merge_retention    dec, the tile offsets and the summary (+ the emit when `emit`)
//   launch_merge_emit         the emit alone, after launch_merge_retention(a, false) sized the output with
//                             unbounded capacities (the caller then points a.out at buffers of the reported sizes)
//   launch_merge              order + retention
hipError_t launch_merge_order(const MergeArgs &a, hipStream_t st);
hipError_t launch_merge_retention(const MergeArgs &a, bool emit, hipStream_t st);
hipError_t launch_merge_emit(const MergeArgs &a, hipStream_t st);
hipError_t launch_merge(const MergeArgs &a, bool emit, hipStream_t st);
// The operator step between order and retention, around the host's fold (a.ch bound by chain_bind):
//   launch_merge_chains       order, the unit code of every position, the chain summary
//   launch_chain_tables       group table, link table and staging arena (a.ch bound by chain_tables_bind)
hipError_t launch_merge_chains(const MergeArgs &a, hipStream_t st);
hipError_t launch_chain_tables(const MergeArgs &a, hipStream_t st);

// SST cuts over the chain tables of a prep-only encode set of one slot (launch_encode_prep).  n_real
// (device, or NULL = the slot's n): the stream's true length when the slot covers a padded stream; the
// walk stops there (a block before it is the same in both streams) and cuts past it are not recorded.
hipError_t launch_cuts(const SstSet &P, uint64_t max_sst_size, uint64_t *cut, uint64_t cap, uint64_t *num,
                       hipStream_t st, const uint64_t *n_real = nullptr);

// ---- sdb_compactor_run_ssts (decode inside the job) ----
struct CxInputs {  // kernel arguments: the input SSTs' blocks, in input order (tables in device memory)
    uint32_t n, nruns;
    uint64_t base;                     // the decoder's arena: block k = base + start[k] (mod 2^64)
    uint64_t nblocks;                  // blocks of every input
    const uint8_t *const *data;        // n: each input's data section
    const uint64_t *const *block_off;  // n: each input's BlockMeta offsets
    const uint64_t *first_block;       // n + 1: prefix of num_blocks
    const uint64_t *run_block;         // nruns + 1: first block of each run, then the total
    const uint64_t *run_entry;         // nruns + 1: declared first entry of each run, then the total
    uint64_t key_bytes;                // declared total key bytes
};
// block k of the job -> arena offsets [start, end)
hipError_t launch_cx_blocks(const CxInputs &in, uint64_t *start, uint64_t *end, hipStream_t st);
// the decode's summary and run boundaries against the declared counts -> *gate (~0: the merge may run)
hipError_t launch_cx_gate(const CxInputs &in, const sdb_decode_summary *dsum, const unsigned long long *dec_err,
                          const uint64_t *block_entry_start, unsigned long long *gate, hipStream_t st);
// sdb_sst_cuts over a padded stream whose true length is *n_real (device)
sdb_status sst_cuts_padded(const sdb_kv_batch *batch, const sdb_sst_params *params, uint64_t max_sst_size,
                           uint64_t *cut_start, uint64_t cut_cap, uint64_t *num_ssts, void *workspace,
                           uint64_t workspace_bytes, hipStream_t stream, const uint64_t *n_real);
// merged positions [summary.num_out + 1, cap]: empty entries (offsets = the totals), so a prep over the
// padded stream reads defined bytes
hipError_t launch_merge_pad(const sdb_merged_out &out, uint64_t cap, hipStream_t st);

// ---- sdb_compactor_run_ssts_ranged (sdb_compact_range.hip): the job range and the inputs' visible ranges ----
struct RxInputs {  // kernel arguments: per-input tables in device memory
    uint32_t n, nruns;
    uint32_t has_job, has_proj;            // job / proj were passed (else: unbounded)
    sdb_scan_ranges job, proj;             // job.n == 1, proj.n == n
    uint32_t has_resume, resume_len;       // a resume cursor's key K: Included(K) is a third start bound of every V[i] (S1)
    const uint8_t *resume_key;             // uploaded with the tables
    // uploaded by the host
    const uint8_t *const *index_keys;      // n
    const uint64_t *const *index_key_off;  // n
    const uint64_t *const *block_off;      // n: each input's BlockMeta offsets
    const uint64_t *num_blocks;            // n
    const uint64_t *gblock;                // n + 1: prefix of num_blocks (the job's block numbering)
    const uint64_t *num_entries;           // n: declared
    const uint32_t *run_start;             // nruns + 1: first input of each run
    // written by k_rx_cover
    uint64_t *cover;                       // 2 n + 1: covering blocks [start, end) of each input (end <= start:
                                           // none), then the status of the ranges (SDB_OK | SDB_INVALID_ARGUMENT)
    uint8_t *clipped;                      // n: V[i] has a bound
    const uint64_t **cov_off;              // n: block_off[i] + cover start: the covered blocks' offsets
    uint64_t *cov_first;                   // n + 1: prefix of the covered block counts (the decode's numbering)
    // written by k_rx_clip / k_rx_gate
    uint64_t *lo, *hi;                     // n: the rows V[i] contains, in the decoded columns
    uint64_t *out_first, *out_key;         // n + 1: prefix of hi - lo and of their key bytes
    uint64_t *result;                      // kRxResult words, then run_entry (nruns + 1: each run's first row)
};
// result words (read back with run_entry in the job's second synchronisation)
enum { kRxGate = 0, kRxDecoded = 1, kRxIn = 2, kRxKeyBytes = 3, kRxResult = 4 };
// V[i] = job ∩ visible[i], its covering blocks, and their compaction into the decode's block list (a.cov_*)
hipError_t launch_rx_cover(const RxInputs &a, hipStream_t st);
// after the decode of the covered blocks: the rows V[i] contains, the counts against the declared ones (R6), the
// per-run row ranges and the job's result words; decl_*: the declared totals of every input (exact when no input
// is clipped)
hipError_t launch_rx_clip_gate(const RxInputs &a, const sdb_decoded_out &dec, const unsigned long long *dec_err,
                               uint64_t decl_entries, uint64_t decl_key_bytes, hipStream_t st);
// the contributed rows of every input, closed up: columns and keys of `dec` into `out` (`rows` = out_first[n])
hipError_t launch_rx_compact(const RxInputs &a, const sdb_decoded_out &dec, const sdb_decoded_out &out, uint64_t rows,
                             hipStream_t st);

// ---- the compaction filter and the resume cursor (sdb_compact_filter.hip), between the merge emit and the cuts ----
// The host has run the filter over the retained stream `in` (n rows) and uploaded one decision byte per row
// (SDB_CF_*; a row the resume drain removes arrives as SDB_CF_DROP), the offsets of the m replacement values in row
// order and their bytes.  k_cf_size / k_cf_scan / k_cf_emit write the surviving rows, rules F3 / F4 applied, into
// `out`: tiles of kMergeTile rows, one workgroup per tile.
struct CfArgs {
    uint64_t n, ntiles;
    sdb_kv_batch in;           // the retained stream (device)
    const uint8_t *decision;   // n
    const uint64_t *mod_off;   // m + 1: replacement j (of the j-th row whose decision is VALUE or MERGE) = arena[mod_off[j], mod_off[j + 1])
    const uint8_t *arena;
    uint64_t *tile_sum;        // per tile: kept rows, key bytes, modified rows, value bytes of the unmodified kept rows
                               // (exclusive offsets after k_cf_scan); then the four totals
    sdb_merged_out out;        // the final stream: key_off / val_off start at 0 (summary unused)
};
// Sizes (w == NULL) or binds everything the apply step holds on the device: the upload (n decisions, m replacements
// of arena_bytes bytes), the tile sums, and the final stream of n_out rows, key_out key bytes and val_out value bytes
// (each arena with the 16 bytes of slack the merge emit's arenas have).
inline uint64_t cf_bind(CfArgs &a, uint64_t n, uint64_t m, uint64_t arena_bytes, uint64_t n_out, uint64_t key_out,
                        uint64_t val_out, uint8_t *w) {
    a.n = n;
    a.ntiles = (n + kMergeTile - 1) / kMergeTile;
    Carver c{w, 0};
    c.take(a.decision, n);
    c.take(a.mod_off, m + 1);
    c.take(a.arena, arena_bytes + 16);
    c.take(a.tile_sum, 4 * (a.ntiles + 1));
    sdb_merged_out &o = a.out;
    o = sdb_merged_out{};
    o.cap_entries = n_out;
    o.key_cap = key_out;
    o.val_cap = val_out;
    c.take(o.key_off, n_out + 1);
    c.take(o.val_off, n_out + 1);
    c.take(o.kind, n_out + 1);
    c.take(o.seq, n_out + 1);
    c.take(o.create_ts, n_out + 1);
    c.take(o.expire_ts, n_out + 1);
    c.take(o.ts_mask, n_out + 1);
    c.take(o.key_bytes, key_out + 16);
    c.take(o.val_bytes, val_out + 16);
    return c.off;
}
hipError_t launch_cf_apply(const CfArgs &a, hipStream_t st);
// S1 over decoded runs: lb[r] = the first row of run r whose key is >= key (device arrays; one thread per run)
struct CfSeekRun {
    const uint8_t *key_arena;
    const uint64_t *key_off;
    uint64_t n;
};
hipError_t launch_cf_seek(const CfSeekRun *runs, uint32_t nruns, const uint8_t *key, uint32_t key_len, uint64_t *lb,
                          hipStream_t st);
// S2 without a filter: *drained = the first row of the stream m at which key == K && seq >= S fails (one workgroup)
hipError_t launch_cf_drain(const sdb_kv_batch &m, const uint8_t *key, uint32_t key_len, uint64_t seq, uint64_t *drained,
                           hipStream_t st);

// out[2i], out[2i+1] = key_off[cut[i]], val_off[cut[i]] for i <= ns
hipError_t launch_cut_offsets(const uint64_t *cut, const uint64_t *num, const uint64_t *key_off, const uint64_t *val_off,
                              uint64_t *out, hipStream_t st);

}  // namespace sdb
