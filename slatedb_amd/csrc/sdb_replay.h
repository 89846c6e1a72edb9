// sdb_replay.h — kernel arguments and workspace of the WAL replay (sdb_replay.hip; include/slatedb_amd.h,
// "WAL replay / device memtable").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slatedb_amd.h"
#include "sdb_workspace.h"

namespace sdb {

constexpr uint32_t kReplayTile = 1024;  // rows one workgroup sorts in LDS; outputs of one merge workgroup
constexpr uint32_t kReplayThreads = kReplayTile / 2;  // one compare-exchange per thread and bitonic step
constexpr uint32_t kReplayBlock = 256;             // rows / sorted positions / output rows of the other workgroups
constexpr uint32_t kReplayBuckets = 64;            // tables one partition pass separates
constexpr uint32_t kReplaySkip = 0x80000000u;      // permutation entry: a row W1 skipped (they sort behind the kept)
static_assert((kReplayTile & (kReplayTile - 1)) == 0, "the bitonic network wants a power of two");
static_assert(kReplayThreads >= 128, "k_rp_merge finds its two splits on lanes of two waves");

struct ReplayBatchAcc {  // per batch, by atomics; every word has identity 0
    unsigned long long all_min_inv, all_max;    // ~min / max seq over all rows (W2)
    unsigned long long min_inv, max, cts, any;  // ~min / max seq, max create_ts (sign bit flipped), any create_ts: rows past W1
    unsigned long long rows, bytes, replaced, key_bytes, val_bytes;  // W5 after W4
};
enum { kRpStatus = 0, kRpRowsOut, kRpKeyBytes, kRpValBytes, kRpKept, kRpReplaced, kRpEmitStatus, kRpWords };

struct ReplayArgs {
    uint64_t n, nbatches, ntables;
    uint64_t min_seq;
    uint32_t has_min_seq, ntiles, npass, nblocks;  // npass: merge passes; nblocks: workgroups of kReplayBlock rows
    sdb_run r;
    const uint64_t *batch_start;
    const uint64_t *table_batch_start;
    sdb_wal_batch_facts *facts;
    sdb_wal_replay_summary *summary;
    sdb_wal_tables_out out;
    // workspace
    uint64_t *pfx;            // per row: key bytes [L0, L0 + 8), big-endian, zero padded
    uint32_t *perm[2];        // sorted position -> row (| kReplaySkip); the merge passes alternate
    uint32_t *sorted;         // the one of perm[] the last pass wrote
    uint32_t *row_batch;      // per row
    uint8_t *state;           // per row: 0 skipped (W1), 1 kept, 2 replaced (W4)
    ReplayBatchAcc *acc;      // per batch
    uint64_t *batch_pre;      // nbatches + 1: survivors of the earlier batches
    unsigned long long *err;  // ~0, or batch << 8 | status (batch_start, W2)
    uint32_t *lcp0;           // L0: the prefix every key shares
    uint64_t *word;           // kRp*: what _emit needs of _sort's result
    uint32_t *batch_table;    // per batch (emit)
    uint64_t *table_pre;      // ntables + 1: survivors of the earlier tables = table_row_start
    uint32_t *count;          // nblocks x kReplayBuckets: per workgroup and table of the pass, then exclusive over workgroups
    uint32_t *dst;            // output row -> input row
    uint64_t *tile_sum;       // per kReplayBlock output rows: key bytes, value bytes (exclusive after the scan)
};

// Sizes (w == NULL) or binds the workspace of both calls for n rows in nbatches batches.
inline uint64_t replay_bind(ReplayArgs &a, uint8_t *w) {
    const uint64_t nblocks = (a.n + kReplayBlock - 1) / kReplayBlock;
    Carver c{w, 0};
    c.take(a.pfx, a.n + 1);
    c.take(a.perm[0], a.n + 1);
    c.take(a.perm[1], a.n + 1);
    c.take(a.row_batch, a.n + 1);
    c.take(a.state, a.n + 1);
    c.take(a.acc, a.nbatches + 1);
    c.take(a.batch_pre, a.nbatches + 1);
    c.take(a.err, 1);
    c.take(a.lcp0, 1);
    c.take(a.word, kRpWords);
    c.take(a.batch_table, a.nbatches + 1);
    c.take(a.table_pre, a.nbatches + 1);
    c.take(a.count, (nblocks + 1) * kReplayBuckets);
    c.take(a.dst, a.n + 1);
    c.take(a.tile_sum, 2 * (nblocks + 1));
    return c.off;
}

hipError_t launch_replay_sort(const ReplayArgs &a, hipStream_t st);
hipError_t launch_replay_emit(const ReplayArgs &a, hipStream_t st);

}  // namespace sdb
