// sdb_get.hip — batched Db::get over a device-resident tree of encoded SSTs for gfx950.
//
// Replaces the on-disk part of Reader::get_key_value_with_options (reader.rs:203-260): the flat, lazy chain
// of GetIterator::from_lsm_tree (db_iter.rs:79-90, 102-124), many keys per call:
//   chain       every L0 SST newest first, then per sorted run the SSTs covering the key
//               (build_l0_point_iters / build_sr_point_iters, segment_iterator.rs:312-353;
//               tables_covering_point_key, db_state.rs:540-596, 662-665)
//   per SST     bloom filter (sst_iter.rs:201-227), partitions_covering_range([key, key]), every block of
//               it CRC-checked (format/sst.rs:1029-1038), versions above max_seq dropped before the walk
//               sees them (FilterIterator::new_with_max_seq, filter_iterator.rs:22-48, db_iter.rs:354-372)
//   decision    the first entry the first non-empty leaf yields: value / tombstone / merge operand
//               (MergeOperatorRequiredIterator, merge_operator.rs:213-223)
//
// The unit of work is a (query, run) pair: a run contributes at most a few adjacent SSTs to a chain, and what
// a run yields for a key (nothing / an entry / an error) does not depend on the runs before it.  Only the
// last step, picking the first run in order that yields something, is per query.  Per pair the workspace
// keeps one state byte and a 20-byte record, so it is O(blocks + SSTs + keys x runs) however the chains look.
//   k_get_validate  one workgroup: run_start / block_base / the views are consistent (else every query
//                   fails with SDB_INVALID_ARGUMENT and nothing is dereferenced through them); per-SST
//                   status (version, NULL arrays); resets the summary accumulators
//   k_get_locate    thread per (query, run): the run's covering SSTs, per SST the filter, the block range
//                   and the marks at block_base[sst] + block — for the whole chain (eager: which SST
//                   decides is not known before the blocks are checked).  A thread per pair, not per
//                   query: the work is dependent loads (binary searches, filter probes), and 64 Ki queries
//                   alone leave a CU four waves to hide them behind
//   k_check         wave per marked block: bounds + CRC, the pass the lookups and scans run (sdb_lookup.hip)
//   k_get_rows      thread per checked block: every row parsed, by the walker sdb_sst_scan's k_sc_block uses
//                   (for_each_row of sdb_read.h)
//   k_get_walk      thread per (query, run) that has an unfiltered covering SST: block statuses, the seek,
//                   the versions above max_seq skipped -> the pair's record (entry position or error)
//   k_get_resolve   thread per query: the first run in order whose record holds an entry or an error decides;
//                   records behind it are never looked at, so their block errors never surface; one row
//                   re-parsed for the columns; wave reduction + one atomic per counter and workgroup
//   k_get_final     the summary
// sdb_lsm_get_merge (launch_get with a chain) shares everything up to k_get_rows and replaces the tail: a pair's
// walk goes on past the first entry while the entries are merge operands, into a 72-byte record of its own.
//   k_gm_walk       thread per (query, run) with an unfiltered covering SST: the count walk -> the pair's MergeRec
//   k_get_resolve   its <true> instantiation: the runs in order up to the first that ended the chain or failed; the
//                   sequence order, the aggregates, the per-query columns, each run's link offset, the query's
//                   link count
//   scan            the link counts -> chain_start
//   k_gm_final      both summaries, do the links fit
//   k_gm_emit       thread per pair the chain takes: the walk again, its links written at chain_start[q] + off
// sdb_lsm_get_mem (a GetCall with layers) puts device memtables, sorted runs in the sdb_run layout, in front of run 0: a
// (query, table) pair is one more pair, whose record comes from a binary search over the table's columns.
//   k_mem_reset     the queries' decided bytes cleared, and the blocks' marks and statuses in place of two memsets
//   k_mem_validate  one workgroup: every table has its columns and fewer than 2^31 rows (else the call is malformed)
//   k_mem_probe     thread per (query, table): the lower bound of (key, max_seq) in key ascending / seq descending
//                   order -> the pair's RunRec (hit + row) or, with a chain, the count walk's MergeRec; a query that
//                   the tables end sets its decided byte
//   k_get_locate    its <P, V, true> instantiation skips the pairs of decided queries before it probes or marks
//   k_get_resolve   its <MERGE, true> instantiation takes the tables' records ahead of run 0; a deciding table row's
//                   columns come from the table's columns
//   k_mem_links     after k_gm_final: every link starts as a tree link (table 0xFFFFFFFF, row 0)
//   k_mem_emit      thread per (query, table) the chain takes: its links written at chain_start[q] + off
// The calls without tables launch none of these and the instantiations they always launched.
// One launcher (launch_get), one workspace layout (get_bind: the plain get's arrays are a prefix of the merging
// get's) and one resolve body serve both; what differs between them is chosen at compile time.
// sdb_lsm_get_filtered passes the SSTs' filter policies: the filter step of k_get_locate and of the walk asks
// Filter::might_match for Point(key) under the SST's policy (sdb_filter.h) where sdb_lsm_get, the plain policy, probes the
// full key.  What a key probes depends on the policy alone: k_get_validate finds whether the policies agree, and then
// a pair's thread hashes once for all its SSTs, as before; else once per SST that has a filter.
// sdb_lsm_get_projected passes a visible range per SST (SsTableView.visible_range, db_state.rs:61-78): an SST is in a
// key's chain iff its effective range, [first_key, last_key] intersected with the visible range, holds the key, and a
// run is searched by its effective start keys (get_run<V>).  Inside an SST of the chain every version of the key is
// visible, so only the chain changes; k_get_validate also checks the projections.
// Host side: one descriptor (GetCall, sdb_reads.h) from the C entry point to the launches.  launch_get -> launch_get_search
// (memsets, GetArgs, get_bind) -> launch_get_bound<M> -> launch_get_kernels<P, V, M>, where the instantiations are
// chosen once.  The special cases, each with the rule of include/slatedb_amd.h it implements:
//   nothing to search   no query, or neither a tree nor a table: every query NOT_FOUND (sst 0xFFFFFFFF) and no link, by
//                       memsets alone; no kernel
//   no_tree             the tree has no SST, no run or no block.  The get counts a tree without runs as none with or
//                       without tables (its pairs are per run; the scan's predicate differs).  With tables (M7) only they
//                       are searched and nothing is read through the tree's arrays: the tree counts, pol and proj are
//                       cleared, and launch_get_kernels launches none of the tree's kernels
//   marks and statuses  without tables two memsets; with tables k_mem_reset, which also clears the decided bytes
//   no table (M6)       sdb_lsm_get_mem with mem NULL, no table or no query is the projected call, then k_mem_reset over
//                       mout alone and, with a chain, k_mem_links (launch_mem_links): nothing names a table
#include <algorithm>

#include "sdb_decode.h"
#include "sdb_mem.h"
#include "sdb_range.h"

namespace sdb {

// no covering SST / its one covering SST filtered / search the run / search its one covering SST, whose block
// range the record already holds
enum { kRunNone = 0, kRunFiltered = 1, kRunOpen = 2, kRunOpen1 = 3 };
// k_get_locate -> k_get_walk (kRunOpen1): sst, block = range start, at = range end.
// k_get_walk -> k_get_resolve: st != 0: the run fails the query; hit: the entry at `at` (V2: byte offset, V1:
// index) of block `block` of `sst`; nread / nfilt: the run's SSTs consulted / filtered up to there (a run's
// covering SSTs are those whose range holds one key: a handful; the counts saturate at 65535).
struct RunRec {
    uint32_t sst, block, at;
    uint16_t nread, nfilt;
    uint8_t st, hit, pad[2];
};
// sdb_lsm_get_merge, k_gm_walk -> k_gm_resolve -> k_gm_emit: what the run contributes to the key's operand chain,
// its visible versions up to and including the first that is no operand.  hit: the first of them, of any kind, at
// `at` of block `block` of `sst`; nlinks: the operands and the value among them; end: how the run ended the chain;
// seq0 / maxseq: the first link's seq and the highest; has / cts / ets: MergeTracker over the links (the flag bits
// of the timestamps seen, the maximum create_ts, the minimum expire_ts).  The resolve adds off, the links of the
// runs before this one, and use, for the runs the query's chain takes.
enum { kEndOpen = 0, kEndValue = 1, kEndTombstone = 2 };
struct MergeRec {
    uint64_t seq0, maxseq, off;
    int64_t cts, ets;
    uint32_t sst, block, at, nlinks;
    uint16_t nread, nfilt;
    uint8_t st, hit, end, has, use, pad[3];
};
enum { kMaccMaxChain = 0, kMaccGo, kMaccWords };
struct GetArgs {
    sdb_lsm_view t;
    const uint8_t *key_bytes;
    const uint64_t *key_off;
    uint64_t nkeys;
    const uint64_t *max_seq;
    sdb_get_out out;
    uint8_t *mark;             // per tree block: 1 = some chain reads it (cleared by k_check)
    int32_t *bstat;            // per tree block: -1 = not read, else its sdb_status
    int32_t *sstat;            // per SST: 0, SDB_INVALID_VERSION or SDB_INVALID_ARGUMENT
    uint8_t *rstate;           // per pair, at run * nkeys + query: kRun*
    RunRec *rec;               // per pair: see RunRec
    unsigned long long *acc;   // kAcc* accumulators
    uint32_t *bad;             // 1 = the tree is malformed
    // sdb_lsm_get_filtered only (else nullptr: every SST has the plain whole-key policy)
    const sdb_filter_policy *pol;  // per SST
    const int32_t *probe_len;  // per query: prefix_len(Point(key)) for SDB_PREFIX_LENGTHS SSTs
    uint32_t *uni;             // 1 = the policies agree: a key's probe is the same for every SST
    // sdb_lsm_get_merge only
    sdb_chain_out chain;
    MergeRec *mrec;            // per pair: see MergeRec
    uint64_t *qn, *qscan;      // per query: its links; the second output of their scan (the first is chain_start)
    uint64_t *tx, *ty;         // scan tiles
    unsigned long long *macc;  // kMacc* words
    // sdb_lsm_get_projected only
    sdb_scan_ranges proj;      // per SST: SsTableView.visible_range, (UNBOUNDED, UNBOUNDED) = None
    // sdb_lsm_get_mem only
    const sdb_run *tabs;       // the memtables in search order
    uint32_t ntab;
    sdb_mem_get_out mout;
    sdb_mem_chain_out mchain;
    RunRec *trec;              // per (table, query) pair, at table * nkeys + query: sst = the table, at = the row
    MergeRec *tmrec;           // the same with a chain
    uint8_t *decided;          // per query: 1 = the tables end its chain, no SST is consulted (M5)
};
enum { kAccFound = 0, kAccDeleted, kAccNotFound, kAccMerge, kAccFailed, kAccBlocks, kAccFirstBad, kAccWords };

// V: the call has projections (sdb_lsm_get_projected).  As P below: the kernels that read them exist once without the
// step, so the calls without projections launch what they always launched.
template <bool V>
__global__ __launch_bounds__(256) void k_get_validate(GetArgs a) {
    int bad = lsm_validate(a.t, a.sstat);
    const int uni = policies_validate(a.pol, a.t.num_ssts, a.sstat);
    if (V) {  // P5: a malformed projection makes the call malformed
        int pb = 0;
        for (uint32_t i = threadIdx.x; i < a.t.num_ssts; i += blockDim.x)
            if (bad_projection(a.proj, i)) pb = 1;
        bad |= __syncthreads_or(pb);
    }
    if (threadIdx.x == 0) {
        *a.bad = bad ? 1u : 0u;
        *a.uni = uni ? 1u : 0u;
        for (int i = 0; i < kAccWords; i++) a.acc[i] = i == kAccFirstBad ? ~0ull : 0ull;
    }
}

SDB_DEV Key key_of(const GetArgs &a, uint64_t q) { return Key{a.key_bytes + a.key_off[q], (uint32_t)(a.key_off[q + 1] - a.key_off[q])}; }
// sign(SsTableInfo.first_entry / last_entry of SST i cmp key)
SDB_DEV int cmp_first(const GetArgs &a, uint32_t i, const Key &k) {
    const uint64_t o = a.t.first_key_off[i];
    return cmp_bytes(a.t.first_key_bytes + o, (uint32_t)(a.t.first_key_off[i + 1] - o), k.t, k.nt, 0).c;
}
SDB_DEV int cmp_last(const GetArgs &a, uint32_t i, const Key &k) {
    const uint64_t o = a.t.last_key_off[i];
    return cmp_bytes(a.t.last_key_bytes + o, (uint32_t)(a.t.last_key_off[i + 1] - o), k.t, k.nt, 0).c;
}

// Under projection (P1-P2 of sdb_lsm_get_projected): the effective start key of SST i, max(first_key, visible start)
// (compacted_effective_start_key, db_state.rs:198-204), is <= k; and the effective range E[i] = [first_key, last_key]
// intersected with the visible range (effective_range, :116-141) holds k.
SDB_DEV bool eff_start_le(const GetArgs &a, uint32_t i, const Key &k) {
    if (cmp_first(a, i, k) > 0) return false;
    const Bound s = range_start(a.proj, i);
    return !s.kind || cmp_bytes(k.t, k.nt, s.t, s.n, 0).c >= 0;
}
SDB_DEV bool eff_holds(const GetArgs &a, uint32_t i, const Key &k) {
    if (cmp_first(a, i, k) > 0 || cmp_last(a, i, k) < 0) return false;
    const Bound s = range_start(a.proj, i), e = range_end(a.proj, i);
    if (s.kind && precedes(s, cmp_bytes(k.t, k.nt, s.t, s.n, 0).c)) return false;
    return !(e.kind && exceeds(e, cmp_bytes(k.t, k.nt, e.t, e.n, 0).c));
}

// The covering SSTs [first, last] of run r for key k, in run order: the last SST whose first key is <= k if
// its range holds k, and the SSTs right before it while their range still reaches k
// (point_table_idx_covering_key, db_state.rs:578-596).  false: none.  The chain of k is these, over the runs
// in order.  V: over the effective start keys and the effective ranges.
template <bool V>
SDB_DEV bool get_run(const GetArgs &a, uint32_t r, const Key &k, uint32_t &first, uint32_t &last) {
    const uint32_t rs = a.t.run_start[r], re = a.t.run_start[r + 1];
    uint32_t lo = rs, hi = re;  // partition_point(first_key <= k)
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (V ? eff_start_le(a, mid, k) : cmp_first(a, mid, k) <= 0) lo = mid + 1;
        else hi = mid;
    }
    if (lo == rs) return false;
    last = lo - 1;
    if (V ? !eff_holds(a, last, k) : cmp_last(a, last, k) < 0) return false;
    first = last;
    while (first > rs && (V ? eff_holds(a, first - 1, k) : cmp_last(a, first - 1, k) >= 0)) first--;
    return true;
}

// What one SST of the chain means to a key: ruled out by the filter, unusable (st), or the block range
// partitions_covering_range([k, k]) over its index keys.
struct Step {
    bool filtered;
    int st;
    uint32_t start, end;
};
// What Point(k) of query q probes in the filter of SST i (filter_probe of sdb_filter.h); it depends on the SST only
// through its policy.
SDB_DEV Probe get_probe(const GetArgs &a, uint64_t q, const Key &k, uint32_t i) {
    return filter_probe(policy_spec(a.pol, i, a.probe_len), false, k.t, k.nt, q);
}
// P: the call has filter policies (sdb_lsm_get_filtered); the kernels of the filter step exist once without them, where
// the probe is the full key's hash as sdb_lsm_get always computed it, and once with them, so the plain calls keep
// their registers and occupancy.  pr: the probe of the last SST with a filter, have: there was one; when the policies
// agree (uni) it is every SST's, so a pair's thread hashes once.
template <bool P>
struct PairProbe {
    bool uni, have;
    Probe pr;
    SDB_DEV PairProbe(const GetArgs &a, const Key &k)
        : uni(P ? *a.uni != 0 : true), have(!P), pr(P ? Probe{-1, 0} : Probe{(int64_t)k.nt, siphash13(k.t, k.nt)}) {}
};
template <bool P>
SDB_DEV Step get_step(const GetArgs &a, const sdb_sst_view &v, uint32_t i, uint64_t q, const Key &k, PairProbe<P> &pp) {
    Step s{false, 0, 0, 0};
    if (v.bloom) {
        if (P && (!pp.have || !pp.uni)) pp.pr = get_probe(a, q, k, i);
        pp.have = true;
        if (!filter_might_match(v.bloom, v.bloom_len, v.num_probes, pp.pr.len, pp.pr.h)) {
            s.filtered = true;
            return s;
        }
    }
    if (!(s.st = a.sstat[i])) point_block_range(v, k.t, k.nt, s.start, s.end);
    return s;
}

// M: the call has memtables (sdb_lsm_get_mem): the pairs of a query that the tables decided stay kRunNone.
template <bool P, bool V, bool M = false>
__global__ __launch_bounds__(256) void k_get_locate(GetArgs a) {
    if (*a.bad) return;
    const uint32_t R = a.t.num_runs;
    const uint64_t total = a.nkeys * R;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t q = t % a.nkeys;  // pair t = run * nkeys + query: a wave holds neighbouring queries of one run
        const uint32_t r = (uint32_t)(t / a.nkeys);
        if (M && a.decided[q]) {
            a.rstate[t] = kRunNone;
            continue;
        }
        const Key k = key_of(a, q);
        uint32_t first, last;
        uint8_t rs = kRunNone;
        if (get_run<V>(a, r, k, first, last)) {
            PairProbe<P> pp(a, k);  // filter_hash (filter.rs:196-204): one hash for every SST's filter
            rs = last > first ? kRunOpen : kRunFiltered;  // several covering SSTs: the resolve counts them itself
            for (uint32_t i = first; i <= last; i++) {
                const sdb_sst_view v = a.t.ssts[i];
                const Step s = get_step<P>(a, v, i, q, k, pp);
                if (s.filtered) continue;
                rs = kRunOpen;
                if (s.st) continue;
                const uint64_t base = a.t.block_base[i];
                for (uint32_t b = s.start; b < s.end; b++) a.mark[base + b] = 1;
                if (last == first) {
                    rs = kRunOpen1;
                    a.rec[t] = RunRec{i, s.start, s.end, 0, 0, 0, 0, {0, 0}};
                }
            }
        }
        a.rstate[t] = rs;
    }
}

// Every row of a checked block parsed (flags, varints, lengths), as sdb_sst_scan reports them.
__global__ __launch_bounds__(64) void k_get_rows(GetArgs a) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int st = -1;
    if (k < a.t.total_blocks && !*a.bad) st = a.bstat[k];
    if (st == 0) {
        const uint32_t i = sst_of_block(a.t, k);
        const sdb_sst_view v = a.t.ssts[i];
        Blk b;
        st = blk_open(v, k - a.t.block_base[i], b);
        if (!st) st = for_each_row(v.sst_version, b, [](uint32_t, uint32_t, const Row &) {});
        a.bstat[k] = st;
    }
    const unsigned long long read = __ballot(st != -1);
    if (threadIdx.x == 0 && read) atomicAdd(&a.acc[kAccBlocks], (unsigned long long)__popcll(read));
}

struct Hit {
    bool ok;
    uint32_t block, at;
};

// Every entry of blocks [start, end) of one SST with key == k and seq <= bound, in physical order:
// visit(block, its Blk, position, row) -> false: stop (done).
template <typename F>
SDB_DEV int get_versions(const sdb_sst_view &v, const Step &s, const Key &k, uint64_t bound, bool &done, F &&visit) {
    const bool v2 = v.sst_version == 2;
    for (uint32_t blk = s.start; blk < s.end; blk++) {
        Blk b;
        if (int st = blk_open(v, blk, b)) return st;
        if (b.count == 0) continue;
        Pos P;
        if (blk != s.start) {  // the first block is seeked; later blocks are entered at their first entry
            if (int st = first_entry(v2, b, k.t, k.nt, P)) return st;
        } else if (int st = v2 ? v2_seek_asc(b, k.t, k.nt, P) : v1_seek(b, k.t, k.nt, false, P)) {
            return st;
        }
        while (P.ok) {  // entries from P on while they hold the key
            if (P.key.c > 0) return 0;  // past the key: this SST has no further version
            Row r;
            if (int st = v2 ? v2_row(b, P.at, r) : v1_row(b, P.at, r)) return st;
            if (P.key.c == 0 && r.seq <= bound && !visit(blk, b, P.at, r)) {
                done = true;
                return 0;
            }
            if (int st = next_entry(v2, b, r, k.t, k.nt, P)) return st;
        }
    }
    return 0;
}

// The walk of pair t: the visible versions of query t % nkeys in the covering SSTs of run t / nkeys, in chain order,
// every block of an SST's range checked before its rows are used: visit(sst, block, its Blk, position, row) ->
// false: stop.  -> the status that ends the walk; nread / nfilt: the SSTs consulted / filtered up to there.
template <bool P, bool V, typename F>
SDB_DEV int walk_pair(const GetArgs &a, uint64_t t, uint8_t rs, uint32_t &nread, uint32_t &nfilt, F &&visit) {
    const uint64_t q = t % a.nkeys;
    const Key k = key_of(a, q);
    const uint64_t bound = a.max_seq ? a.max_seq[q] : ~0ull;
    int st = 0;
    bool done = false;
    auto search = [&](uint32_t i, const sdb_sst_view &v, const Step &s) {  // false: the walk is over
        if (s.end <= s.start) return true;
        nread++;
        const uint64_t base = a.t.block_base[i];
        for (uint32_t b = s.start; b < s.end && !st; b++) st = a.bstat[base + b];  // the lowest failing block
        if (st < 0) st = SDB_INVALID_ARGUMENT;  // unreachable: locate marked this range
        if (!st)
            st = get_versions(v, s, k, bound, done,
                              [&](uint32_t blk, const Blk &b, uint32_t at, const Row &r) { return visit(i, blk, b, at, r); });
        return !st && !done;
    };
    if (rs == kRunOpen1) {
        const RunRec in = a.rec[t];
        const sdb_sst_view v = a.t.ssts[in.sst];
        search(in.sst, v, Step{false, 0, in.block, in.at});
    } else {
        uint32_t first = 0, last = 0;
        bool go = get_run<V>(a, (uint32_t)(t / a.nkeys), k, first, last);
        PairProbe<P> pp(a, k);
        for (uint32_t i = first; go && i <= last; i++) {
            const sdb_sst_view v = a.t.ssts[i];
            const Step s = get_step<P>(a, v, i, q, k, pp);
            if (s.filtered) nfilt++;
            else if ((st = s.st)) go = false;
            else go = search(i, v, s);
        }
    }
    return st;
}

template <bool P, bool V>
__global__ __launch_bounds__(64) void k_get_walk(GetArgs a) {
    if (*a.bad) return;
    const uint64_t total = a.nkeys * a.t.num_runs;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t rs = a.rstate[t];
        if (rs != kRunOpen && rs != kRunOpen1) continue;
        uint32_t sst = 0xFFFFFFFFu, nread = 0, nfilt = 0;
        Hit H;
        H.ok = false;
        const int st = walk_pair<P, V>(a, t, rs, nread, nfilt, [&](uint32_t i, uint32_t blk, const Blk &, uint32_t at, const Row &) {
            H.ok = true;  // the first visible version decides
            H.block = blk;
            H.at = at;
            sst = i;
            return false;
        });
        RunRec out{sst, H.ok ? H.block : 0, H.ok ? H.at : 0, (uint16_t)(nread > 0xFFFF ? 0xFFFF : nread),
                   (uint16_t)(nfilt > 0xFFFF ? 0xFFFF : nfilt), (uint8_t)st, (uint8_t)(H.ok && !st), {0, 0}};
        a.rec[t] = out;
    }
}

// The summary's counters of a wave of one-lane workgroups' queries (every lane calls it): ballots and one atomic per
// counter, the lowest failing query by atomicMin on query << 8 | status.
SDB_DEV void get_count(const GetArgs &a, uint64_t q, bool live, uint32_t state, bool failed, int st) {
    const unsigned long long nf = __ballot(live && state == SDB_GET_FOUND), nd = __ballot(live && state == SDB_GET_DELETED),
                             nm = __ballot(live && state == SDB_GET_MERGE_OPERAND), nx = __ballot(failed),
                             nn = __ballot(live && state == SDB_GET_NOT_FOUND && !failed);
    if (threadIdx.x == 0) {
        if (nf) atomicAdd(&a.acc[kAccFound], (unsigned long long)__popcll(nf));
        if (nd) atomicAdd(&a.acc[kAccDeleted], (unsigned long long)__popcll(nd));
        if (nm) atomicAdd(&a.acc[kAccMerge], (unsigned long long)__popcll(nm));
        if (nn) atomicAdd(&a.acc[kAccNotFound], (unsigned long long)__popcll(nn));
        if (nx) atomicAdd(&a.acc[kAccFailed], (unsigned long long)__popcll(nx));
    }
    if (failed) atomicMin(&a.acc[kAccFirstBad], (unsigned long long)(q << 8 | (uint64_t)st));
}

// The records of the pairs as the walk left them: k_get_walk's (MERGE false) or k_gm_walk's.
template <bool MERGE>
SDB_DEV auto pair_recs(const GetArgs &a) {
    if constexpr (MERGE) return a.mrec;
    else return a.rec;
}

// MERGE false, sdb_lsm_get: the first run in order whose record holds an entry or an error decides; an operand there
// is reported (SDB_MERGE_OPERATOR_MISSING) with its own columns and does not count as failed.  MERGE true,
// sdb_lsm_get_merge: the runs in order until one ends the chain or fails; the columns are the first entry's with the
// links' aggregates, and every run the chain takes learns where its links go (off, use).  A compile-time choice: the
// plain resolve keeps the registers of a kernel that knows nothing of chains.
// The records of the (query, table) pairs as k_mem_probe left them.
template <bool MERGE>
SDB_DEV auto table_recs(const GetArgs &a) {
    if constexpr (MERGE) return a.tmrec;
    else return a.trec;
}

// M: the call has memtables (sdb_lsm_get_mem): their records come first, in table order.
template <bool MERGE, bool M = false>
__global__ __launch_bounds__(64) void k_get_resolve(GetArgs a) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = q < a.nkeys;
    int st = 0;
    uint32_t state = SDB_GET_NOT_FOUND;
    if (live) {
        uint32_t sst = 0xFFFFFFFFu, nread = 0, nfilt = 0;
        Hit H;
        H.ok = false;
        Row r{};
        uint64_t vbase = 0, links = 0, newest = 0;
        int64_t cts = 0, ets = 0;
        uint8_t has = 0, end = kEndOpen;
        bool intab = false;  // M: the first entry lies in table `sst`, at row H.at
        if (*a.bad) {
            st = SDB_INVALID_ARGUMENT;
        } else {
            auto take = [&](auto &x, bool table) {  // the next pair of the query's chain that has a record
                nread += x.nread;
                nfilt += x.nfilt;
                if (x.hit && !H.ok) {  // (a record with an error holds no hit unless it is a chain's)
                    H.ok = true;
                    H.block = x.block;
                    H.at = x.at;
                    sst = x.sst;
                    intab = table;
                }
                if constexpr (MERGE) {
                    if (x.nlinks) {
                        if (!links) newest = x.seq0;
                        if (x.maxseq > newest) {  // MergeTracker::update (merge_operator.rs:293-299)
                            st = SDB_INVALID_SEQUENCE_ORDER;
                            return;
                        }
                        if (x.has & SDB_FLAG_HAS_CREATE_TS) cts = (has & SDB_FLAG_HAS_CREATE_TS) && cts > x.cts ? cts : x.cts;
                        if (x.has & SDB_FLAG_HAS_EXPIRE_TS) ets = (has & SDB_FLAG_HAS_EXPIRE_TS) && ets < x.ets ? ets : x.ets;
                        has |= x.has;
                        x.off = links;
                        x.use = 1;
                        links += x.nlinks;
                    }
                    end = x.end;
                }
                st = x.st;
            };
            if constexpr (M)
                for (uint32_t j = 0; j < a.ntab && !st && (MERGE ? !end : !H.ok); j++) take(table_recs<MERGE>(a)[j * a.nkeys + q], true);
            const uint32_t R = a.t.num_runs;
            for (uint32_t j = 0; j < R && !st && (MERGE ? !end : !H.ok); j++) {
                const uint8_t rs = a.rstate[j * a.nkeys + q];
                if (rs == kRunFiltered) nfilt++;
                if (rs != kRunOpen && rs != kRunOpen1) continue;
                take(pair_recs<MERGE>(a)[j * a.nkeys + q], false);
            }
            if (M && intab) {
                if (H.ok && !st) r = tab_row(a.tabs[sst], H.at, vbase);  // the first entry's columns are the table's
            } else if (H.ok && !st) {  // the first entry again, for its columns
                const sdb_sst_view v = a.t.ssts[sst];
                Blk b;
                if (!(st = blk_open(v, H.block, b))) st = v.sst_version == 2 ? v2_row(b, H.at, r) : v1_row(b, H.at, r);
                vbase = b.base;
            }
        }
        if (st) {
            H.ok = false;
            links = 0;
        }
        intab = intab && H.ok;
        if (H.ok) {
            const bool operand = (r.flags & SDB_FLAG_MERGE_OPERAND) != 0;
            if (r.flags & SDB_FLAG_TOMBSTONE) {
                state = SDB_GET_DELETED;
            } else if (MERGE) {  // the entry MergeOperatorIterator returns (merge_operator.rs:437-447)
                state = operand ? SDB_GET_MERGE_OPERAND : SDB_GET_FOUND;
                r.flags = (uint8_t)(has | (operand && end != kEndValue ? SDB_FLAG_MERGE_OPERAND : 0));
                r.cts = cts;
                r.ets = ets;
            } else if (operand) {
                state = SDB_GET_MERGE_OPERAND;
                st = SDB_MERGE_OPERATOR_MISSING;
            } else {
                state = SDB_GET_FOUND;
            }
        } else {  // no entry: zero columns
            sst = 0xFFFFFFFFu;
            r = Row{};
        }
        a.out.state[q] = (uint8_t)state;
        a.out.status[q] = st;
        a.out.sst[q] = M && intab ? 0xFFFFFFFFu : sst;
        a.out.block[q] = H.ok ? H.block : 0;
        put_row(a.out, q, vbase, r);
        if constexpr (M) {
            a.mout.table[q] = intab ? sst : 0xFFFFFFFFu;
            a.mout.row[q] = intab ? H.at : 0;
        }
        a.out.ssts_read[q] = nread;
        a.out.ssts_filtered[q] = nfilt;
        if constexpr (MERGE) {
            a.qn[q] = links;
            if (links) atomicMax(&a.macc[kMaccMaxChain], (unsigned long long)links);
        }
    }
    const bool failed = live && st != 0 && (MERGE || state == SDB_GET_NOT_FOUND);
    get_count(a, q, live, state, failed, st);
}

SDB_DEV void get_summary(const GetArgs &a) {
    sdb_get_summary s{};
    s.num_found = a.acc[kAccFound];
    s.num_deleted = a.acc[kAccDeleted];
    s.num_not_found = a.acc[kAccNotFound];
    s.num_merge = a.acc[kAccMerge];
    s.num_failed = a.acc[kAccFailed];
    s.blocks_checked = a.acc[kAccBlocks];
    s.status = a.acc[kAccFirstBad] == ~0ull ? 0 : (int32_t)(a.acc[kAccFirstBad] & 0xFF);
    *a.out.summary = s;
}
__global__ void k_get_final(GetArgs a) {
    if (threadIdx.x == 0) get_summary(a);
}

// =================================================================================================
// sdb_lsm_get_merge: the same chain of SSTs, walked past the first entry while the entries are merge operands
// (MergeOperatorIterator::merge_with_older_entries over GetIterator, merge_operator.rs:369-448, db_iter.rs:102-124).
// Its own kernels: the count walk before the resolve (k_get_resolve<true> above), the final and the emit after it.
// =================================================================================================

// The count walk's step: the next visible version r of the key, in chain order, into the pair's record -> false: it
// ended the chain.
SDB_DEV bool chain_count(MergeRec &m, const Row &r) {
    if (r.flags & SDB_FLAG_TOMBSTONE) {  // ends the chain and is no link (GetIterator returns None, db_iter.rs:108-114)
        m.end = kEndTombstone;
        return false;
    }
    if (!m.nlinks) m.seq0 = r.seq;
    if (m.nlinks != 0xFFFFFFFFu) m.nlinks++;
    if (r.seq > m.maxseq) m.maxseq = r.seq;
    if (r.flags & SDB_FLAG_HAS_CREATE_TS) {  // MergeTracker::update (merge_operator.rs:289-292)
        m.cts = (m.has & SDB_FLAG_HAS_CREATE_TS) && m.cts > r.cts ? m.cts : r.cts;
        m.has |= SDB_FLAG_HAS_CREATE_TS;
    }
    if (r.flags & SDB_FLAG_HAS_EXPIRE_TS) {
        m.ets = (m.has & SDB_FLAG_HAS_EXPIRE_TS) && m.ets < r.ets ? m.ets : r.ets;
        m.has |= SDB_FLAG_HAS_EXPIRE_TS;
    }
    if (!(r.flags & SDB_FLAG_MERGE_OPERAND)) {  // the base value: the last link
        m.end = kEndValue;
        return false;
    }
    return true;
}

template <bool P, bool V>
__global__ __launch_bounds__(64) void k_gm_walk(GetArgs a) {
    if (blockIdx.x == 0 && threadIdx.x == 0) a.macc[kMaccMaxChain] = a.macc[kMaccGo] = 0;
    if (*a.bad) return;
    const uint64_t total = a.nkeys * a.t.num_runs;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t rs = a.rstate[t];
        if (rs != kRunOpen && rs != kRunOpen1) continue;
        MergeRec m{};
        uint32_t nread = 0, nfilt = 0;
        const int st = walk_pair<P, V>(a, t, rs, nread, nfilt, [&](uint32_t i, uint32_t blk, const Blk &, uint32_t at, const Row &r) {
            if (!m.hit) {
                m.hit = 1;
                m.sst = i;
                m.block = blk;
                m.at = at;
            }
            return chain_count(m, r);
        });
        m.st = (uint8_t)st;
        m.nread = (uint16_t)(nread > 0xFFFF ? 0xFFFF : nread);
        m.nfilt = (uint16_t)(nfilt > 0xFFFF ? 0xFFFF : nfilt);
        a.mrec[t] = m;
    }
}

__global__ void k_gm_final(GetArgs a) {
    if (threadIdx.x != 0) return;
    get_summary(a);
    sdb_chain_summary s{};
    s.num_links = a.chain.chain_start[a.nkeys];
    s.max_chain_len = a.macc[kMaccMaxChain];
    const bool fits = s.num_links <= a.chain.cap_links;
    s.status = fits ? SDB_OK : SDB_LIMIT_EXCEEDED;
    *a.chain.summary = s;
    a.macc[kMaccGo] = fits;
}

template <bool P, bool V>
__global__ __launch_bounds__(64) void k_gm_emit(GetArgs a) {
    if (*a.bad || !a.macc[kMaccGo]) return;
    const uint64_t total = a.nkeys * a.t.num_runs;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint8_t rs = a.rstate[t];
        if (rs != kRunOpen && rs != kRunOpen1) continue;
        const uint64_t q = t % a.nkeys;
        const uint32_t n = a.mrec[t].nlinks;
        if (!a.mrec[t].use || !n || a.out.status[q]) continue;
        const uint64_t at0 = a.chain.chain_start[q] + a.mrec[t].off;
        uint32_t x = 0, nread = 0, nfilt = 0;
        walk_pair<P, V>(a, t, rs, nread, nfilt, [&](uint32_t i, uint32_t blk, const Blk &b, uint32_t, const Row &r) {
            if (r.flags & SDB_FLAG_TOMBSTONE) return false;
            const uint64_t d = at0 + x;
            if (x >= n || d >= a.chain.cap_links) return false;  // never out of the pair's slots
            a.chain.sst[d] = i;
            a.chain.block[d] = blk;
            put_row(a.chain, d, b.base, r);
            x++;
            return (r.flags & SDB_FLAG_MERGE_OPERAND) != 0 && x < n;
        });
    }
}

// =================================================================================================
// sdb_lsm_get_mem: device memtables in front of the tree (Reader::get_key_value_with_options, reader.rs:133-182: the
// active memtable, then the immutable ones front first, then the tree).  A table is a sorted run: key ascending, seq
// descending (mem_table.rs:38-44), so what it yields for (key, max_seq) starts at one lower bound.
// =================================================================================================

__global__ __launch_bounds__(256) void k_mem_validate(GetArgs a) {  // after k_get_validate: it may only add to *bad
    int bad = 0;
    for (uint32_t j = threadIdx.x; j < a.ntab; j += blockDim.x) bad |= tab_malformed(a.tabs[j]);
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) {
        if (bad) *a.bad = 1u;
        if (a.macc) a.macc[kMaccMaxChain] = a.macc[kMaccGo] = 0;  // k_gm_walk's reset, for a call without a tree
    }
}

// Per query: no table has decided it yet, and it names no table (k_get_resolve<., true> writes the latter again; the
// call without tables leaves it so).  Per tree block (mark != nullptr): not marked, not read, what launch_get's two
// memsets do.  A kernel: under HIP graph replay the memset nodes in front of a captured call's kernels were seen
// not to take effect (stale decided bytes, blocks_checked growing from replay to replay); kernels order like kernels.
__global__ __launch_bounds__(256) void k_mem_reset(uint8_t *decided, sdb_mem_get_out mout, uint64_t n, uint8_t *mark,
                                                   int32_t *bstat, uint64_t tb) {
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t q = t0; q < n; q += step) {
        if (decided) decided[q] = 0;
        mout.table[q] = 0xFFFFFFFFu;
        mout.row[q] = 0;
    }
    for (uint64_t k = t0; mark && k < tb; k += step) {
        mark[k] = 0;
        bstat[k] = -1;
    }
}

// The rows from `from` on with key == k and seq <= bound, in table order (KVTable::range(key..=key) under
// FilterIterator::new_with_max_seq): visit(row, value base, the row) -> false: stop.
template <typename F>
SDB_DEV void tab_versions(const sdb_run &T, const Key &k, uint64_t bound, uint64_t from, F &&visit) {
    for (uint64_t i = from; i < T.n; i++) {
        if (tab_cmp(T, i, k) != 0) return;
        if (T.seq[i] > bound) continue;
        uint64_t vbase;
        const Row r = tab_row(T, i, vbase);
        if (!visit(i, vbase, r)) return;
    }
}

template <bool MERGE>
__global__ __launch_bounds__(256) void k_mem_probe(GetArgs a) {
    if (*a.bad) return;
    const uint64_t total = a.nkeys * a.ntab;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t q = t % a.nkeys;  // pair t = table * nkeys + query: a wave holds neighbouring queries of one table
        const uint32_t j = (uint32_t)(t / a.nkeys);
        const sdb_run T = a.tabs[j];
        const Key k = key_of(a, q);
        const uint64_t bound = a.max_seq ? a.max_seq[q] : ~0ull;
        const uint64_t from = T.n ? tab_seek(T, k, bound) : 0;
        if constexpr (MERGE) {
            MergeRec m{};
            tab_versions(T, k, bound, from, [&](uint64_t i, uint64_t, const Row &r) {
                if (!m.hit) {
                    m.hit = 1;
                    m.sst = j;
                    m.at = (uint32_t)i;
                }
                return chain_count(m, r);
            });
            a.tmrec[t] = m;
            if (m.end != kEndOpen) a.decided[q] = 1;
        } else {
            RunRec out{j, 0, 0, 0, 0, 0, 0, {0, 0}};
            tab_versions(T, k, bound, from, [&](uint64_t i, uint64_t, const Row &) {
                out.at = (uint32_t)i;  // the first visible version decides
                out.hit = 1;
                return false;
            });
            a.trec[t] = out;
            if (out.hit) a.decided[q] = 1;
        }
    }
}

// Every link of a chain that fits starts as a tree link; k_mem_emit then names the tables' links.
__global__ __launch_bounds__(256) void k_mem_links(sdb_chain_out chain, sdb_mem_chain_out mchain) {
    const sdb_chain_summary s = *chain.summary;
    if (s.status != SDB_OK) return;
    const uint64_t n = s.num_links < chain.cap_links ? s.num_links : chain.cap_links;
    for (uint64_t d = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; d < n; d += (uint64_t)gridDim.x * blockDim.x) {
        mchain.table[d] = 0xFFFFFFFFu;
        mchain.row[d] = 0;
    }
}

static hipError_t launch_mem_links(const sdb_chain_out &chain, const sdb_mem_chain_out &mchain, hipStream_t st) {
    const uint32_t g = (uint32_t)std::min<uint64_t>((chain.cap_links + 255) / 256, 1024);
    if (g) hipLaunchKernelGGL(k_mem_links, dim3(g), dim3(256), 0, st, chain, mchain);
    return hipGetLastError();
}

__global__ __launch_bounds__(64) void k_mem_emit(GetArgs a) {
    if (*a.bad || !a.macc[kMaccGo]) return;
    const uint64_t total = a.nkeys * a.ntab;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t q = t % a.nkeys;
        const uint32_t j = (uint32_t)(t / a.nkeys), n = a.tmrec[t].nlinks;
        if (!a.tmrec[t].use || !n || a.out.status[q]) continue;
        const uint64_t at0 = a.chain.chain_start[q] + a.tmrec[t].off;
        uint32_t x = 0;
        tab_versions(a.tabs[j], key_of(a, q), a.max_seq ? a.max_seq[q] : ~0ull, a.tmrec[t].at, [&](uint64_t i, uint64_t vbase, const Row &r) {
            if (r.flags & SDB_FLAG_TOMBSTONE) return false;
            const uint64_t d = at0 + x;
            if (x >= n || d >= a.chain.cap_links) return false;  // never out of the pair's slots
            a.chain.sst[d] = 0xFFFFFFFFu;
            a.chain.block[d] = 0;
            put_row(a.chain, d, vbase, r);
            a.mchain.table[d] = j;
            a.mchain.row[d] = i;
            x++;
            return (r.flags & SDB_FLAG_MERGE_OPERAND) != 0 && x < n;
        });
    }
}

// The workspace arrays of a get of a.nkeys keys over the tree a.t, bound into a from w; -> their size.  merge: those
// of the plain get, then the merging get's own; a.ntab > 0: then those of the (query, table) pairs.
static uint64_t get_bind(GetArgs &a, uint8_t *w, bool merge) {
    const uint64_t tb = a.t.total_blocks, n = a.nkeys, pairs = n * a.t.num_runs;
    Carver c{w, 0};
    c.take(a.mark, tb + 1);
    c.take(a.bstat, tb + 1);
    c.take(a.sstat, (uint64_t)a.t.num_ssts + 1);
    c.take(a.rstate, pairs + 1);
    c.take(a.rec, pairs + 1);
    c.take(a.acc, kAccWords + 1);  // the accumulators, then bad and uni
    if (w) a.bad = (uint32_t *)(a.acc + kAccWords);
    if (w) a.uni = a.bad + 1;
    if (merge) {
        c.take(a.mrec, pairs + 1);
        c.take(a.qn, n + 1);
        c.take(a.qscan, n + 2);
        c.take(a.tx, (n + 1023) / 1024 + 2);
        c.take(a.ty, (n + 1023) / 1024 + 2);
        c.take(a.macc, kMaccWords);
    }
    if (a.ntab) {
        c.take(a.decided, n + 1);
        if (merge) c.take(a.tmrec, n * a.ntab + 1);
        else c.take(a.trec, n * a.ntab + 1);
    }
    return c.off;
}

uint64_t get_workspace_bytes(const ReadShape &s) {
    GetArgs a{};
    a.t.total_blocks = s.total_blocks;
    a.t.num_ssts = s.num_ssts;
    a.t.num_runs = s.num_runs;
    a.nkeys = s.n;
    a.ntab = s.num_tables;
    return get_bind(a, nullptr, s.merge);
}

// The kernels of a bound get in stream order.  P: the call has filter policies, V: it has projections, each chosen
// once for the kernels that hold the step; merge: a.chain is given.  M: the call has memtables: their pairs are
// probed first, and a tree without SSTs, runs or blocks (a.t.num_runs == 0 then) launches none of its kernels.
template <bool P, bool V, bool M = false>
static hipError_t launch_get_kernels(const GetArgs &a, bool merge, hipStream_t st) {
    const uint64_t tb = a.t.total_blocks, n = a.nkeys, pairs = n * a.t.num_runs;
    const bool tree = !M || pairs != 0;
    // the kernels stride past these caps; the per-block parse and the per-pair walks are latency-bound threads: one
    // wave per workgroup spreads them over the CUs
    const dim3 lg((uint32_t)std::min<uint64_t>((pairs + 255) / 256, 1u << 20));
    const dim3 wg((uint32_t)std::min<uint64_t>((pairs + 63) / 64, 1u << 22)), qg((uint32_t)((n + 63) / 64));
    hipError_t e;
    const uint64_t tpairs = n * a.ntab;
    const dim3 tg((uint32_t)std::min<uint64_t>((tpairs + 255) / 256, 1u << 20));
    hipLaunchKernelGGL(k_get_validate<V>, dim3(1), dim3(256), 0, st, a);
    if constexpr (M) {
        hipLaunchKernelGGL(k_mem_validate, dim3(1), dim3(256), 0, st, a);
        if (merge) hipLaunchKernelGGL(k_mem_probe<true>, tg, dim3(256), 0, st, a);
        else hipLaunchKernelGGL(k_mem_probe<false>, tg, dim3(256), 0, st, a);
    }
    if (tree) {
        hipLaunchKernelGGL((k_get_locate<P, V, M>), lg, dim3(256), 0, st, a);
        if ((e = launch_check(CheckArgs{{}, a.t, a.bad, tb, a.mark, a.bstat}, st)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_get_rows, dim3((uint32_t)((tb + 63) / 64)), dim3(64), 0, st, a);
    }
    if (!merge) {
        if (tree) hipLaunchKernelGGL((k_get_walk<P, V>), wg, dim3(64), 0, st, a);
        hipLaunchKernelGGL((k_get_resolve<false, M>), qg, dim3(64), 0, st, a);
        hipLaunchKernelGGL(k_get_final, dim3(1), dim3(64), 0, st, a);
    } else {
        if (tree) hipLaunchKernelGGL((k_gm_walk<P, V>), wg, dim3(64), 0, st, a);
        hipLaunchKernelGGL((k_get_resolve<true, M>), qg, dim3(64), 0, st, a);
        if ((e = launch_excl_scan2(a.qn, a.qn, n, a.tx, a.ty, a.chain.chain_start, a.qscan, st)) != hipSuccess) return e;
        hipLaunchKernelGGL(k_gm_final, dim3(1), dim3(64), 0, st, a);
        if (tree) hipLaunchKernelGGL((k_gm_emit<P, V>), wg, dim3(64), 0, st, a);
        if constexpr (M) {
            if ((e = launch_mem_links(a.chain, a.mchain, st)) != hipSuccess) return e;
            hipLaunchKernelGGL(k_mem_emit, dim3((uint32_t)std::min<uint64_t>((tpairs + 63) / 64, 1u << 22)), dim3(64), 0, st, a);
        }
    }
    return hipGetLastError();
}

template <bool M>
static hipError_t launch_get_bound(const GetArgs &a, bool filters, bool projected, bool merge, hipStream_t st) {
    if (projected) return filters ? launch_get_kernels<true, true, M>(a, merge, st) : launch_get_kernels<false, true, M>(a, merge, st);
    return filters ? launch_get_kernels<true, false, M>(a, merge, st) : launch_get_kernels<false, false, M>(a, merge, st);
}

// k_mem_reset over a's queries and, with marks, a's tree blocks.
static hipError_t launch_mem_reset(const GetArgs &a, bool marks, hipStream_t st) {
    const uint64_t n = a.nkeys, tb = a.t.total_blocks;
    const uint32_t g = (uint32_t)std::min<uint64_t>((std::max(n, marks ? tb : 0) + 255) / 256, 1024);
    if (g) hipLaunchKernelGGL(k_mem_reset, dim3(g), dim3(256), 0, st, a.decided, a.mout, n, marks ? a.mark : nullptr, a.bstat, tb);
    return hipGetLastError();
}

// The search of one get call (the special cases: the file comment).  tabs: c.mem holds a table and there is a query
// (with c.mout, and c.mchain iff c.chain).
static hipError_t launch_get_search(const GetCall &c, bool tabs, uint8_t *w, hipStream_t st) {
    const sdb_lsm_view &t = *c.lsm;
    const sdb_get_out &out = *c.out;
    const sdb_chain_out *chain = c.chain;
    const uint64_t tb = t.total_blocks, n = c.nkeys;
    const bool no_tree = t.num_ssts == 0 || t.num_runs == 0 || tb == 0;
    const bool none = n == 0 || (no_tree && !tabs);  // nothing to search
    hipError_t e;
    if (none && chain) {  // no links
        if ((e = hipMemsetAsync(chain->summary, 0, sizeof(sdb_chain_summary), st)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(chain->chain_start, 0, 8 * (n + 1), st)) != hipSuccess) return e;
    }
    if ((e = hipMemsetAsync(out.summary, 0, sizeof(sdb_get_summary), st)) != hipSuccess) return e;
    if (none) {  // every query NOT_FOUND: sst 0xFFFFFFFF, the other columns zero
        const struct {
            void *p;
            int fill;
            uint64_t width;
        } cols[] = {{out.state, 0, 1},     {out.status, 0, 4},    {out.sst, 0xFF, 4},    {out.block, 0, 4},
                    {out.val_off, 0, 8},   {out.val_len, 0, 4},   {out.seq, 0, 8},       {out.flags, 0, 1},
                    {out.create_ts, 0, 8}, {out.expire_ts, 0, 8}, {out.ssts_read, 0, 4}, {out.ssts_filtered, 0, 4}};
        for (const auto &col : cols)
            if (n && (e = hipMemsetAsync(col.p, col.fill, col.width * n, st)) != hipSuccess) return e;
        return hipSuccess;
    }
    GetArgs a{};
    a.t = t;
    a.key_bytes = c.key_bytes;
    a.key_off = c.key_off;
    a.nkeys = n;
    a.max_seq = c.max_seq;
    a.out = out;
    a.pol = c.pol;
    a.probe_len = c.probe_len;
    if (chain) a.chain = *chain;
    if (tabs) {
        a.tabs = c.mem->tables;
        a.ntab = c.mem->num_tables;
        a.mout = *c.mout;
        if (chain) a.mchain = *c.mchain;
    }
    const bool merge = chain != nullptr;
    get_bind(a, w, merge);
    const sdb_scan_ranges *proj = c.proj;
    if (no_tree) {  // (M7) only the tables are searched, and nothing is read through the tree's arrays
        a.t.num_ssts = a.t.num_runs = 0;
        a.t.total_blocks = 0;
        a.pol = nullptr;
        proj = nullptr;
    } else if (!tabs) {
        if ((e = hipMemsetAsync(a.mark, 0, tb, st)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(a.bstat, 0xFF, 4 * tb, st)) != hipSuccess) return e;
    }
    if (proj) a.proj = *proj;
    const bool filters = c.pol || c.probe_len;
    if (!tabs) return launch_get_bound<false>(a, filters, proj != nullptr, merge, st);
    if ((e = launch_mem_reset(a, !no_tree, st)) != hipSuccess) return e;
    return launch_get_bound<true>(a, filters, proj != nullptr, merge, st);
}

hipError_t launch_get(const GetCall &c, uint8_t *w, hipStream_t st) {
    const bool tabs = c.mem && c.mem->num_tables && c.nkeys;
    hipError_t e = launch_get_search(c, tabs, w, st);
    if (e != hipSuccess || tabs || !c.layers) return e;
    // (M6) sdb_lsm_get_mem without a table: the projected call, and no query or link names a table
    GetArgs r{};
    r.nkeys = c.nkeys;
    r.mout = *c.mout;
    if ((e = launch_mem_reset(r, false, st)) != hipSuccess) return e;
    return c.chain ? launch_mem_links(*c.chain, *c.mchain, st) : hipSuccess;
}

}  // namespace sdb
