// sdb_lsm_scan.hip — batched Db::scan over a device-resident tree of encoded SSTs for gfx950.
//
// Replaces the on-disk part of Reader::scan_with_options (reader.rs:275-320) -> DbIterator::new
// (db_iter.rs:189-257), drained, many ranges per call:
//   SSTs        every SST whose [first_key, last_key] meets the range (the reference opens every L0 SST and, per
//               sorted run, tables_covering_range: segment_iterator.rs:355-414, db_state.rs:600-660)
//   per SST     partitions_covering_range(index, start, end), every block of it CRC-checked and parsed
//               (partitioned_keyspace.rs:87-110, format/sst.rs:1029-1038); the entries the range contains
//   filter      versions above max_seq dropped before the merge (FilterIterator::new_with_max_seq,
//               db_iter.rs:205-217)
//   merge       key ascending, seq descending, the newest version per key (MergeIterator with dedup,
//               merge_iterator.rs:55-69, 180-209); a tombstone yields nothing (db_iter.rs:280-303), a merge
//               operand fails the range (MergeOperatorRequiredIterator, merge_operator.rs:213-223)
//
// The unit of work is a (range, SST) pair, p = range * num_ssts + sst, so a range's pairs and its staged
// candidates are contiguous.  What depends only on a block is computed once per tree block; a pair's candidates
// are the rows between two ranks in its SST, found by clipping one block at each end.  The bounds, the block
// range, the clip of a block and the restored key are those of sdb_range.h, shared with sdb_scan.hip.
//   k_ls_validate  one workgroup: lsm_validate of sdb_read.h (shared with sdb_lsm_get); resets the control words
//   k_ls_ranges    thread per range: range offsets that descend make the call malformed
//   k_ls_locate    thread per pair: participation, the block range (covering_blocks), the marks at
//                  block_base[sst] + block
//   k_check        wave per marked tree block: bounds + CRC (sdb_lookup.hip, shared)
//   k_ls_block     thread per tree block: every row parsed (for_each_row) -> status, entries, restored-key bytes
//   scans          entries / key bytes / failed / read over the tree blocks
//   k_ls_edge      thread per pair: the lowest failing block (lowest_failure), else the ranks [g0, g1) of its
//                  candidates (clip_block)
//   k_ls_rstat     thread per range: status (lowest SST, then lowest block), range_ssts; a failing range stages
//                  nothing
//   scans          candidates / key bytes / work items over the pairs; k_ls_gate: do the candidates fit (and the winner flags zeroed)
//   k_ls_stage     thread per (pair, block) item: keys restored (restore_key) into the staging arena, seq, flags and
//                  the row's position, contiguous per pair in physical order (an SST holds key ascending, seq
//                  descending)
//   k_ls_rank      thread per candidate: merged rank in its range = own index + one binary search per other
//                  participating SST (the k_mg_rank pattern); the candidate's index goes to that rank, and with it
//                  the winner flag: visible, and in no SST the last candidate before it is a visible version of
//                  its key; an operand winner flags its range
//   scan           winners / their key bytes over the merged positions
//   k_ls_count     thread per range: rule 4, the totals -> scans -> range_entry_start
//   k_ls_final     summary, capacity check
//   k_ls_emit      thread per winner: key and columns (the row parsed once more) at its place
// sdb_lsm_scan_merge (merge != 0; MergeOperatorIterator over the same merge, merge_operator.rs:369-448) runs the same
// sequence with an operand winner a row instead of a failure, and between k_ls_rank and the winner scan
//   k_ls_links     thread per merged position: a winner's links, the contiguous stretch down to its key's first
//                  non-operand, each position of it given its winner; a scan of the link counts
// k_ls_final adds the chain summary (candidates, then rows, then links); then
//   k_ls_fold      thread per merged position of a chain: the row parsed, folded into its winner's aggregates
//                  (atomics), written as a link
// and k_ls_emit takes a winner's chain_start, aggregates and flags from there.
// sdb_lsm_scan_filtered (filter != 0; Db::scan_prefix: SstIteratorOptions.prefix, reader.rs:284-293, evaluated by every
// per-SST iterator before it opens the SST, sst_iter.rs:848-862) runs either sequence with the filters consulted:
//   k_ls_validate  also: do the SSTs' policies agree; a prefix_kind that does not exist makes its SST unusable
//   k_ls_ranges    also: prefix offsets that descend; when the policies agree, what the range's query probes
//                  (filter_probe of sdb_filter.h) and its SipHash, once for every SST
//   k_ls_locate    ahead of the marking: Filter::might_match of the pair (the range's probe, else the pair's own) ->
//                  the pair's `filt` byte; a ruled-out SST takes no part, so nothing of it is marked, checked or staged
//                  and none of its errors shows; neighbouring ranges of one SST share a wave, so a wave's probes hit
//                  one bitmap
//   k_ls_rstat     also: range_filtered, and their sum for k_ls_final
// sdb_lsm_scan_projected (a filtered scan with proj: SsTableView.visible_range per SST, db_state.rs:61-78) runs that
// sequence with a pair's range replaced by its view range V = range r intersected with visible[i]
// (calculate_view_range, db_state.rs:243-251; ls_view):
//   k_ls_validate  also: a projection with a start kind other than unbounded / included, an end kind above excluded or
//                  offsets that descend makes the call malformed
//   k_ls_locate    participation, the block range and the marks from V; a pair whose V is a point while its range is
//                  not asks Point(k) and hashes for itself (point_key is judged on the view range, sst_iter.rs:82-87)
//   k_ls_edge      the candidates are the rows V contains
// Everything behind k_ls_edge sees fewer pairs and candidates and knows nothing of projections.
// sdb_lsm_scan_mem (MEM; ScanIterator: the memtables merged among themselves, then with the tree, db_iter.rs:145-163)
// makes the second index of a pair a source: p = range * (T + num_ssts) + j, j < T a table, j - T an SST.  A table
// is a sorted run (sdb_mem.h), so its candidates are the rows between two lower bounds and need no block:
//   k_ls_mreset    the blocks' marks and statuses, in place of the two memsets (see k_mem_reset of sdb_get.hip)
//   k_ls_tvalidate one workgroup, after k_ls_validate: tab_malformed of every table; a malformed table makes the call malformed
//   k_ls_tprobe    thread per (range, table) pair, neighbouring ranges of one table in a wave: [g0, g1), the counts
//                  and the key-byte rank of g0 into the slots k_ls_edge fills for an SST pair
//   k_ls_rstat     also: range_tables; a failing range zeroes its table pairs' counts too
//   k_ls_trows     thread per candidate of a table pair: key offset and length, seq, flags, the row, and the key
//                  copied into the pair's span of the staging arena (neighbouring threads, neighbouring keys)
//   k_ls_fold / k_ls_emit  a candidate of a table takes its columns from the table's (tab_row) and opens no block;
//                  they name the table and the row in mchain / mout
// k_ls_rank, k_ls_links, the scans and k_ls_count work on staged candidates and see sources where they saw SSTs: the
// stride is nsrc, and j < i still means "the earlier source".  Without tables nsrc == num_ssts and the seven other
// entry points launch the instantiations without the table step (k_ls_mfill then names no table for what they wrote).
// sdb_lsm_scan_recency (Db::scan_prefix_by_recency: DbRecencyIterator drains its sources one after another and opens one
// only when the walk reaches it, db_iter.rs:376-442; rules R1-R7 of include/slatedb_amd.h) runs sdb_lsm_scan_mem's
// sequence through staging, with k_ls_rstat<MEM, true> leaving the range's status open, and then no merge:
//   k_lr_vis       thread per candidate: visible (seq <= max_seq), and first of its key group in its pair
//   scan           both flags -> vpos (a pair's visible rows are a difference of two entries), gpos (group ids)
//   k_lr_groups    descending only, thread per candidate: where every key group starts
//   k_lr_plan      thread per range: the walk over the sources (tables, then runs; a run's SSTs last to first when
//                  descending) against limit[r]: the status of the first opened failing source, the sources read, the
//                  visible rows, and per pair its output base and take
//   k_lr_place     thread per candidate: its rank inside its pair from vpos (descending: groups reversed, versions
//                  newest first) -> morder / wn / wkb at the range's start + the pair's base + the rank: no key of
//                  another source is compared
// and then the winner scan, k_ls_count, k_ls_final and k_ls_emit<true> as they are, with rule 4 off (rop stays 0),
// tombstones flagged as rows and the rows written in the order of their positions (desc = 0 for these launches).
// Host side: one descriptor (ScanCall, sdb_reads.h) from the C entry point to the launches.  launch_lsm_scan ->
// launch_ls_search (memsets, LsArgs, the bind) -> launch_ls_bound -> launch_ls_front<FILTER, PROJ, MEM, REC> (through
// staging) and one of the two tails, launch_ls_merged<MEM> or launch_lr_placed, which share launch_ls_rows.  The
// instantiations are chosen once: the five of (plain or merging), filtered, projected, tables, tables and projected,
// and the recency scan's two (with and without projections).
// The special cases, each with the rule of include/slatedb_amd.h it implements:
//   nothing to search   no range, or neither a tree nor a table: every range is empty, by memsets alone; no kernel
//   no_tree             the tree has no SST or no block; a tree without runs counts as none only with tables (a scan's
//                       pairs are per SST, and the calls without tables never looked at num_runs; the get's predicate
//                       differs).  With tables (S8) only they are scanned and nothing is read through the tree's
//                       arrays: the tree counts, pol and proj are cleared, and launch_ls_kernels launches none of the
//                       tree's kernels
//   marks and statuses  without tables two memsets; with tables k_ls_mreset
//   no table (S7)       sdb_lsm_scan_mem with mem NULL, no table or no range is the projected call, then k_ls_mfill: no
//                       row, link or range names a table
//   recency             always the tables' path (over no table when it has none); a tree without runs is none (R1
//                       walks runs); with neither table nor tree the memsets, the recency outputs included
//   filter              a property of the entry point (ScanCall::filter), not of fout: it sizes the workspace, selects
//                       k_ls_locate<true, ...> and has range_filtered / num_filtered written
#include <algorithm>
#include <climits>

#include "sdb_range.h"
#include "sdb_decode.h"
#include "sdb_mem.h"

namespace sdb {

struct LsArgs {
    sdb_lsm_view t;
    sdb_scan_ranges r;
    const uint64_t *max_seq;
    sdb_lsm_scan_out out;
    uint32_t desc, pad;
    uint64_t cand_entries, cand_key_bytes, pairs;
    // per tree block
    uint8_t *mark;                  // 1 = some range reads it (cleared by k_check)
    int32_t *bstat;                 // -1 = not read, else the block's sdb_status
    uint64_t *cnt, *kb, *bbad, *rd; // entries, restored-key bytes, failed, read
    uint64_t *pc, *pk, *pb, *pr;    // their exclusive scans (total_blocks + 1)
    int32_t *sstat;                 // per SST: 0, SDB_INVALID_VERSION or SDB_INVALID_ARGUMENT
    // per pair
    uint8_t *part;                  // the SST takes part in the range
    uint32_t *bs, *be;              // its block range in the SST
    int32_t *pst;                   // the pair's status: the SST's, else its lowest failing block's
    uint32_t *fb;                   // the block of the first candidate
    uint64_t *g0, *g1, *k0;         // tree-wide row ranks [g0, g1) of the candidates; key-byte rank of g0
    uint64_t *pn, *pkb, *pit;       // candidates, their key bytes, work items (blocks with candidates)
    uint64_t *cs, *cks, *pis;       // exclusive scans (pairs + 1)
    // per range
    uint32_t *rop;                  // 1 = an operand won a key of the range
    uint64_t *rn, *rkb, *rks;       // entries, key bytes; the key-byte scan (n + 1)
    // per candidate
    uint8_t *ckeys;                 // restored keys (cand_key_bytes)
    uint64_t *ckoff, *cseq;
    uint32_t *cklen, *cblk, *cat;   // key length; block in the SST; V2: byte offset, V1: index of the row
    uint8_t *cflags;
    uint64_t *morder;               // candidate at merged position m
    uint64_t *wn, *wkb, *wpos, *wkpos;  // winner flag / key bytes per merged position and their scans
    uint64_t *tx, *ty;              // scan tiles
    unsigned long long *ctl;        // kCtl* words
    // sdb_lsm_scan_merge only
    uint32_t merge, pad2;           // 1 = operands win and carry their chains
    sdb_chain_out chain;
    uint64_t *wl, *wlpos, *wldum;   // links per merged position (a winner's chain); their scan; its second output
    uint64_t *lwin;                 // per merged position: the winner whose chain it belongs to (~0: none)
    long long *wcts, *wets;         // per winner: MergeTracker's maximum create_ts / minimum expire_ts
    uint32_t *whas;                 // per winner: the timestamp flag bits seen | kBase
    // sdb_lsm_scan_filtered only
    uint32_t filter, pad3;          // 1 = the SSTs' filters are consulted
    const sdb_filter_policy *pol;   // per SST, or nullptr: the plain whole-key policy
    sdb_scan_prefixes px;           // all nullptr: no range has a prefix
    sdb_scan_filter_out fout;
    uint8_t *filt;                  // per pair: 1 = the SST's filter ruled it out for the range
    int64_t *qlen;                  // per range, when the policies agree: what its query probes in every SST:
    uint64_t *qh;                   //   the length (< 0: nothing) and the filter hash
    // sdb_lsm_scan_projected only
    sdb_scan_ranges proj;           // per SST: SsTableView.visible_range, (UNBOUNDED, UNBOUNDED) = None
    // sources: a pair is p = range * nsrc + source; without tables nsrc == t.num_ssts and spairs == pairs
    uint32_t ntab, nsrc;            // tables; sources per range = ntab + t.num_ssts
    uint64_t spairs;                // (range, SST) pairs
    // sdb_lsm_scan_mem only
    const sdb_run *tabs;            // device: the tables, sources 0 .. ntab - 1
    sdb_mem_scan_out mout;
    sdb_mem_chain_out mchain;
    // sdb_lsm_scan_recency only
    const uint64_t *limit;          // per range, or nullptr: every source is drained
    sdb_recency_out rout;
    uint64_t *vis, *head;           // per candidate: visible; first of its key group in its pair
    uint64_t *vpos, *gpos;          // their exclusive scans (cand_entries + 1)
    uint64_t *gstart;               // descending: per key group its first candidate; one past the last group: the total
    uint64_t *pbase, *ptake;        // per pair: where its rows start in the range's output, and how many it gives
};
enum { kBase = 0x100 };  // a value or a tombstone ended the chain
enum { kCtlFirstBad = 0, kCtlFailed, kCtlBad, kCtlGo1, kCtlGo2, kCtlGo3, kCtlMaxChain, kCtlFiltered, kCtlUniform, kCtlWords = 16 };

// PROJ: the call has projections (sdb_lsm_scan_projected).  As FILTER below: the kernels that read them exist once
// without the step, so the six calls without projections launch what they always launched.
template <bool PROJ>
__global__ __launch_bounds__(256) void k_ls_validate(LsArgs a) {
    int bad = lsm_validate(a.t, a.sstat);
    const int uni = policies_validate(a.pol, a.t.num_ssts, a.sstat);
    if (PROJ) {  // P5: a malformed projection makes the call malformed
        int pb = 0;
        for (uint32_t i = threadIdx.x; i < a.t.num_ssts; i += blockDim.x)
            if (bad_projection(a.proj, i)) pb = 1;
        bad |= __syncthreads_or(pb);
    }
    if (threadIdx.x == 0) {
        for (int i = 0; i < kCtlWords; i++) a.ctl[i] = i == kCtlFirstBad ? ~0ull : 0ull;
        a.ctl[kCtlBad] = bad ? 1ull : 0ull;
        a.ctl[kCtlUniform] = uni ? 1ull : 0ull;
    }
}

// What range r asks the filters (F1 of sdb_lsm_scan_filtered): a point range Point(key), else Prefix(p) where it has a
// prefix; false: nothing.
struct Query {
    const uint8_t *t;
    uint32_t n;
    bool prefix;
};
SDB_DEV bool ls_query(const LsArgs &a, uint64_t r, const Bound &s, const Bound &e, Query &q) {
    if (s.kind == SDB_BOUND_INCLUDED && e.kind == SDB_BOUND_INCLUDED && s.n == e.n && cmp_bytes(s.t, s.n, e.t, e.n, 0).c == 0) {
        q = Query{s.t, s.n, false};  // SstView::point_key
        return true;
    }
    if (!a.px.has_prefix || !a.px.has_prefix[r]) return false;
    const uint64_t o = a.px.prefix_off[r];
    q = Query{a.px.prefix_bytes + o, (uint32_t)(a.px.prefix_off[r + 1] - o), true};
    return true;
}
// What that query probes in the filter of SST i; it depends on the SST only through its policy.
SDB_DEV Probe ls_probe(const LsArgs &a, uint64_t r, const Query &q, uint32_t i) {
    return filter_probe(policy_spec(a.pol, i, a.px.probe_len), q.prefix, q.t, q.n, r);
}

__global__ __launch_bounds__(256) void k_ls_ranges(LsArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.r.n) return;
    bool bad = a.r.start_off[r + 1] < a.r.start_off[r] || a.r.end_off[r + 1] < a.r.end_off[r];
    if (a.filter && a.px.prefix_off && a.px.prefix_off[r + 1] < a.px.prefix_off[r]) bad = true;
    if (bad) atomicOr(&a.ctl[kCtlBad], 1ull);
    if (bad || !a.filter || !a.ctl[kCtlUniform]) return;
    // the policies agree: what the range probes, and its SipHash, once for every SST
    const Bound s = range_start(a.r, r), e = range_end(a.r, r);
    Probe pr{-1, 0};
    Query q;
    if (!bad_kind(s, e) && ls_query(a, r, s, e, q)) pr = ls_probe(a, r, q, 0);
    a.qlen[r] = pr.len;
    a.qh[r] = pr.h;
}

// Thread t of the per-pair kernels: neighbouring ranges of one SST share a wave.  MEM: the call has memtables
// (sdb_lsm_scan_mem): a range's table pairs stand before its SST pairs.
template <bool MEM>
SDB_DEV void ls_pair(const LsArgs &a, uint64_t t, uint64_t &r, uint32_t &i, uint64_t &p) {
    r = t % a.r.n;
    i = (uint32_t)(t / a.r.n);
    p = MEM ? r * a.nsrc + a.ntab + i : r * a.t.num_ssts + i;
}

// The view range of pair (r, SST i) (P3 of sdb_lsm_scan_projected; calculate_view_range, db_state.rs:243-251): range r
// with the SST's projection intersected into s / e.  The pair takes part only while it is not empty as a set.
SDB_DEV void ls_view(const LsArgs &a, uint32_t i, Bound &s, Bound &e) {
    s = tighter_start(s, range_start(a.proj, i));
    e = tighter_end(e, range_end(a.proj, i));
}

// FILTER: the call consults the filters (sdb_lsm_scan_filtered); the kernel exists once without the step, so the plain
// scans keep their registers and occupancy.
template <bool FILTER, bool PROJ, bool MEM = false>
__global__ __launch_bounds__(256) void k_ls_locate(LsArgs a) {
    if (a.ctl[kCtlBad]) return;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < a.spairs; t += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t r, p;
        uint32_t i;
        ls_pair<MEM>(a, t, r, i, p);
        Bound s = range_start(a.r, r), e = range_end(a.r, r);
        const sdb_sst_view v = a.t.ssts[i];
        const bool okind = !bad_kind(s, e);
        bool own = false;  // P4: the view range is a point and the range is not: the pair asks Point(k) on its own
        if (PROJ && okind) {
            const bool rpoint = is_point(s, e);
            ls_view(a, i, s, e);
            own = !rpoint && is_point(s, e);
        }
        bool part = okind && v.num_blocks > 0 && !empty_as_set(s, e);
        if (part && s.kind) {  // the SST's last key precedes the range
            const uint64_t o = a.t.last_key_off[i];
            part = !precedes(s, cmp_bytes(a.t.last_key_bytes + o, (uint32_t)(a.t.last_key_off[i + 1] - o), s.t, s.n, 0).c);
        }
        if (part && e.kind) {  // its first key exceeds it
            const uint64_t o = a.t.first_key_off[i];
            part = !exceeds(e, cmp_bytes(a.t.first_key_bytes + o, (uint32_t)(a.t.first_key_off[i + 1] - o), e.t, e.n, 0).c);
        }
        if (FILTER) {  // the filter first (FilterIterator::init): a ruled-out SST takes no part, whatever its state
            uint8_t filt = 0;
            if (part && v.bloom) {
                Probe pr{-1, 0};
                Query q;
                if (PROJ && own) pr = filter_probe(policy_spec(a.pol, i, nullptr), false, s.t, s.n, r);  // (probe_len is the range's)
                else if (a.ctl[kCtlUniform]) pr = Probe{a.qlen[r], a.qh[r]};
                else if (ls_query(a, r, s, e, q)) pr = ls_probe(a, r, q, i);
                filt = !filter_might_match(v.bloom, v.bloom_len, v.num_probes, pr.len, pr.h);
                if (filt) part = false;
            }
            a.filt[p] = filt;
        }
        BlockRange g{0, 0};
        if (part && !a.sstat[i]) {
            g = covering_blocks(v, s, e);
            if (g.end < g.start) g.end = g.start;
            const uint64_t base = a.t.block_base[i];
            for (uint64_t b = g.start; b < g.end; b++) a.mark[base + b] = 1;
        }
        a.part[p] = part;
        a.bs[p] = (uint32_t)g.start;
        a.be[p] = (uint32_t)g.end;
    }
}

__global__ __launch_bounds__(64) void k_ls_block(LsArgs a) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.t.total_blocks) return;
    int st = a.ctl[kCtlBad] ? -1 : a.bstat[k];
    uint64_t cnt = 0, kb = 0;
    if (st == 0) {
        const uint32_t i = sst_of_block(a.t, k);
        const sdb_sst_view v = a.t.ssts[i];
        Blk b;
        st = blk_open(v, k - a.t.block_base[i], b);
        if (!st) {
            st = for_each_row(v.sst_version, b, [&](uint32_t x, uint32_t, const Row &r) {
                cnt = x + 1;
                kb += r.sh + r.un;
            });
            // descending: the first error in that order (a V2 block without restarts is walked ascending here too)
            if (st > 0 && a.desc && !(v.sst_version == 2 && b.count == 0))
                if (const int ds = desc_status(v.sst_version, b)) st = ds;
        }
    }
    if (st != 0) cnt = kb = 0;
    a.bstat[k] = st;
    a.cnt[k] = cnt;
    a.kb[k] = kb;
    a.bbad[k] = st > 0;
    a.rd[k] = st != -1;
}

// clip_block of checked block k of v.
SDB_DEV Clip ls_clip(const sdb_sst_view &v, uint64_t k, const Bound &s, const Bound &e) {
    Blk b;
    if (blk_open(v, k, b)) return Clip{0, 0, 0, 0};
    return clip_block(v.sst_version, b, s, e);
}

template <bool PROJ, bool MEM = false>
__global__ __launch_bounds__(64) void k_ls_edge(LsArgs a) {
    const bool bad = a.ctl[kCtlBad] != 0;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < a.spairs; t += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t r, p;
        uint32_t i;
        ls_pair<MEM>(a, t, r, i, p);
        int st = 0;
        uint32_t fb = 0;
        uint64_t g0 = 0, g1 = 0, k0 = 0, k1 = 0, items = 0;
        const bool part = !bad && a.part[p];
        if (part && !(st = a.sstat[i]) && a.be[p] > a.bs[p]) {
            const uint64_t base = a.t.block_base[i], bs = a.bs[p], be = a.be[p];
            if (!(st = lowest_failure(a.pb, a.bstat, base, bs, be))) {
                // The rows of [bs, be) that the range contains lie between two ranks.  Interior blocks hold only keys
                // of the range, except where a bound's key fills whole blocks (a long run of versions under an
                // excluded bound): the walks move inwards past blocks that keep nothing.
                const sdb_sst_view v = a.t.ssts[i];
                Bound s = range_start(a.r, r), e = range_end(a.r, r);
                const Bound open{nullptr, 0, 0};
                if (PROJ) ls_view(a, i, s, e);  // the candidates are the entries the view range contains
                g0 = a.pc[base + be];
                k0 = a.pk[base + be];
                fb = (uint32_t)be;
                if (!s.kind) {
                    g0 = a.pc[base + bs];
                    k0 = a.pk[base + bs];
                    fb = (uint32_t)bs;
                }
                for (uint64_t k = bs; s.kind && k < be; k++) {
                    const Clip c = ls_clip(v, k, s, open);
                    if (c.lo < a.cnt[base + k]) {
                        g0 = a.pc[base + k] + c.lo;
                        k0 = a.pk[base + k] + c.kb_before;
                        fb = (uint32_t)k;
                        break;
                    }
                }
                g1 = a.pc[e.kind ? base + bs : base + be];
                k1 = a.pk[e.kind ? base + bs : base + be];
                for (uint64_t k = be; e.kind && k-- > bs;) {
                    const Clip c = ls_clip(v, k, open, e);
                    if (c.hi > 0) {
                        g1 = a.pc[base + k] + c.hi;
                        k1 = a.pk[base + k] + c.kb;
                        break;
                    }
                }
                if (g1 <= g0 || k1 < k0) {
                    g1 = g0;
                    k1 = k0;
                } else {  // the blocks fb .. the block of row g1 - 1
                    uint64_t x = fb, y = be - 1;
                    while (x < y) {
                        const uint64_t m = x + (y - x) / 2;
                        if (a.pc[base + m + 1] >= g1) y = m;
                        else x = m + 1;
                    }
                    items = x - fb + 1;
                }
            }
        }
        a.part[p] = part;
        a.pst[p] = st;
        a.fb[p] = fb;
        a.g0[p] = g0;
        a.g1[p] = g1;
        a.k0[p] = k0;
        a.pn[p] = st ? 0 : g1 - g0;
        a.pkb[p] = st ? 0 : k1 - k0;
        a.pit[p] = st ? 0 : items;
    }
}

// REC: sdb_lsm_scan_recency: a failing pair fails its range only where the walk opens it (R5), which k_lr_plan decides
// once the visible rows are counted; here only a malformed call or range has a status, and the failing pairs (whose
// counts k_ls_edge left 0) are the only ones that stage nothing.
template <bool MEM, bool REC = false>
__global__ __launch_bounds__(64) void k_ls_rstat(LsArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.r.n) return;
    const uint32_t S = a.t.num_ssts, T = MEM ? a.ntab : 0, NS = S + T;
    const uint64_t p0 = r * NS + T;  // the range's first SST pair
    int st = 0;
    uint32_t ns = 0, nf = 0, nt = 0;
    if (a.ctl[kCtlBad]) {
        st = SDB_INVALID_ARGUMENT;
    } else if (bad_kind(range_start(a.r, r), range_end(a.r, r))) {
        st = SDB_INVALID_ARGUMENT;
    } else {
        for (uint32_t i = 0; i < S; i++) {
            if (a.filter && a.filt[p0 + i]) nf++;
            if (!a.part[p0 + i]) continue;
            ns++;
            if (!REC && !st) st = a.pst[p0 + i];
        }
        for (uint32_t j = 0; j < T; j++) nt += a.part[r * NS + j];  // (k_ls_tprobe: the table holds a key of the range)
    }
    if (st)
        for (uint32_t j = 0; j < NS; j++) a.pn[r * NS + j] = a.pkb[r * NS + j] = a.pit[r * NS + j] = 0;
    a.out.range_status[r] = st;
    a.out.range_ssts[r] = ns;
    if (MEM) a.mout.range_tables[r] = nt;
    a.rop[r] = 0;
    if (a.filter) {
        a.fout.range_filtered[r] = nf;
        if (nf) atomicAdd(&a.ctl[kCtlFiltered], (unsigned long long)nf);
    }
}

// Do the candidates fit; and the winner flags of every merged position zeroed (k_ls_rank sets the winners').
__global__ __launch_bounds__(256) void k_ls_gate(LsArgs a) {
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t0 == 0) a.ctl[kCtlGo1] = a.cs[a.pairs] <= a.cand_entries && a.cks[a.pairs] <= a.cand_key_bytes;
    for (uint64_t m = t0; m < a.cand_entries; m += (uint64_t)gridDim.x * blockDim.x) {
        a.wn[m] = a.wkb[m] = 0;
        if (a.merge) {  // k_ls_links / k_ls_fold fill these
            a.lwin[m] = ~0ull;
            a.wcts[m] = LLONG_MIN;
            a.wets[m] = LLONG_MAX;
            a.whas[m] = 0;
        }
    }
}

template <bool MEM>
__global__ __launch_bounds__(64) void k_ls_stage(LsArgs a) {
    if (!a.ctl[kCtlGo1]) return;
    const uint32_t S = MEM ? a.nsrc : a.t.num_ssts;
    const uint64_t total = a.pis[a.pairs];
    for (uint64_t it = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; it < total; it += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = last_le(a.pis, a.pairs, 1, it);
        const uint32_t i = (uint32_t)(p % S) - (MEM ? a.ntab : 0);  // (only SST pairs have items)
        const sdb_sst_view v = a.t.ssts[i];
        const uint64_t kl = a.fb[p] + (it - a.pis[p]), K = a.t.block_base[i] + kl;  // the block: in the SST, in the tree
        if (kl >= v.num_blocks) continue;
        const uint64_t g0 = a.g0[p], g1 = a.g1[p], c0 = a.pc[K], n = a.cnt[K];
        const uint64_t lo = g0 > c0 ? g0 - c0 : 0, hi = g1 - c0 < n ? g1 - c0 : n;
        if (g1 <= c0 || hi <= lo) continue;
        const uint64_t cbase = a.cs[p], cend = a.cs[p + 1], kbase = a.cks[p], kend = a.cks[p + 1];
        Blk b;
        if (blk_open(v, kl, b)) continue;
        const bool v2 = v.sst_version == 2;
        uint64_t kb = 0;              // key bytes of the rows before the current one
        const uint8_t *prev = nullptr;  // the previous staged key (V2 chains from it)
        for_each_row(v.sst_version, b, [&](uint32_t x, uint32_t pos, const Row &r) {
            const uint32_t L = r.sh + r.un;
            const uint64_t kbx = kb;
            kb += L;
            if (x < lo || x >= hi) return;
            const uint64_t c = cbase + (c0 + x - g0), ko = kbase + (a.pk[K] + kbx - a.k0[p]);
            if (c >= cend || ko > kend || L > kend - ko) return;  // never out of the pair's slots
            uint8_t *dst = a.ckeys + ko;
            restore_key(v2, b, x, r, prev, dst);
            prev = dst;
            a.ckoff[c] = ko;
            a.cklen[c] = L;
            a.cblk[c] = (uint32_t)kl;
            a.cat[c] = v2 ? pos : x;
            a.cseq[c] = r.seq;
            a.cflags[c] = r.flags;
        });
    }
}

SDB_DEV int ls_key_cmp(const LsArgs &a, uint64_t x, const uint8_t *t, uint32_t nt) {
    return cmp_bytes(a.ckeys + a.ckoff[x], a.cklen[x], t, nt, 0).c;
}

// Candidate q is a visible version of the key t.
SDB_DEV bool ls_hides(const LsArgs &a, uint64_t q, uint64_t bound, const uint8_t *t, uint32_t nt) {
    return a.cseq[q] <= bound && a.cklen[q] == nt && ls_key_cmp(a, q, t, nt) == 0;
}

__global__ __launch_bounds__(64) void k_ls_rank(LsArgs a) {
    if (!a.ctl[kCtlGo1]) return;
    const uint32_t S = a.nsrc;  // sources: the tables, then the SSTs
    const uint64_t total = a.cs[a.pairs];
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = last_le(a.cs, a.pairs, 1, c), r = p / S;
        const uint32_t i = (uint32_t)(p % S);
        const uint8_t *t = a.ckeys + a.ckoff[c];
        const uint32_t nt = a.cklen[c];
        const uint64_t seq = a.cseq[c], bound = a.max_seq ? a.max_seq[r] : ~0ull;
        uint64_t rank = c - a.cs[p];
        // c loses if it is not visible, or a visible version of its key comes before it.  In every SST the versions
        // of a key stand newest first, so those above the bound come first: if any visible one comes before c, the last
        // candidate of that SST before c is one.
        bool lose = seq > bound || (rank > 0 && ls_hides(a, c - 1, bound, t, nt));
        for (uint32_t j = 0; j < S; j++) {  // the candidates of SST j that come before c
            if (j == i) continue;
            uint64_t lo = a.cs[r * S + j], hi = a.cs[r * S + j + 1];
            const uint64_t first = lo;
            while (lo < hi) {
                const uint64_t m = lo + (hi - lo) / 2;
                const int k = ls_key_cmp(a, m, t, nt);
                const uint64_t sm = a.cseq[m];
                if (k < 0 || (k == 0 && (sm > seq || (sm == seq && j < i)))) lo = m + 1;
                else hi = m;
            }
            rank += lo - first;
            if (!lose && lo > first) lose = ls_hides(a, lo - 1, bound, t, nt);
        }
        const uint64_t rs = a.cs[r * S], re = a.cs[(r + 1) * S];
        if (rank >= re - rs) continue;  // rows that are not sorted: never out of the range's slots
        const uint8_t f = a.cflags[c];
        a.morder[rs + rank] = c;
        if (!lose && (f & SDB_FLAG_MERGE_OPERAND) && !a.merge) a.rop[r] = 1;
        if (!lose && !(f & SDB_FLAG_TOMBSTONE) && (a.merge || !(f & SDB_FLAG_MERGE_OPERAND))) {  // k_ls_gate zeroed the flags
            a.wn[rs + rank] = 1;
            a.wkb[rs + rank] = nt;
        }
    }
}

// Candidate morder[mm] of range [rs, re) continues the chain of the winner at merged position m, whose key is t:
// -> its index, or ~0 (a position the rank left unwritten, or another key).
SDB_DEV uint64_t ls_chain_cand(const LsArgs &a, uint64_t rs, uint64_t re, uint64_t m, uint64_t mm, const uint8_t *t, uint32_t nt) {
    const uint64_t c = a.morder[mm];
    if (c < rs || c >= re) return ~0ull;
    if (mm > m && !(a.cklen[c] == nt && ls_key_cmp(a, c, t, nt) == 0)) return ~0ull;
    return c;
}

// sdb_lsm_scan_merge: the links of every winner: the contiguous stretch of the merged order from the winner to its
// key's first non-operand, the tombstone excluded (merge_with_older_entries, merge_operator.rs:388-411).  The
// versions behind a winner are visible: they are older than it.
__global__ __launch_bounds__(64) void k_ls_links(LsArgs a) {
    const uint32_t S = a.nsrc;
    const bool go = a.ctl[kCtlGo1] != 0;
    const uint64_t total = go ? a.cs[a.pairs] : 0;
    for (uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; m < a.cand_entries; m += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t n = 0;
        if (m < total && a.wn[m]) {
            const uint64_t r = last_le(a.cs, a.r.n, S, m), rs = a.cs[r * S], re = a.cs[(r + 1) * S], c0 = a.morder[m];
            if (c0 >= rs && c0 < re) {
                const uint8_t *t = a.ckeys + a.ckoff[c0];
                const uint32_t nt = a.cklen[c0];
                for (uint64_t mm = m; mm < re; mm++) {
                    const uint64_t c = ls_chain_cand(a, rs, re, m, mm, t, nt);
                    if (c == ~0ull) break;
                    a.lwin[mm] = m;  // the links, and the tombstone behind them: k_ls_fold folds its timestamps
                    if (a.cflags[c] & SDB_FLAG_TOMBSTONE) break;
                    n++;
                    if (!(a.cflags[c] & SDB_FLAG_MERGE_OPERAND)) break;
                }
            }
            if (n) atomicMax(&a.ctl[kCtlMaxChain], (unsigned long long)n);
        }
        a.wl[m] = n;
    }
}

// Where the links of the winner at merged position m of range r start: a range's rows descend with `desc`, a row's
// links do not.
SDB_DEV uint64_t ls_chain_start(const LsArgs &a, uint64_t r, uint64_t m) {
    const uint32_t S = a.nsrc;
    const uint64_t rs = a.cs[r * S], re = a.cs[(r + 1) * S];
    const uint64_t before = a.wlpos[m] - a.wlpos[rs], all = a.wlpos[re] - a.wlpos[rs];
    return a.wlpos[rs] + (a.desc ? all - before - a.wl[m] : before);
}

__global__ __launch_bounds__(64) void k_ls_count(LsArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.r.n) return;
    const uint32_t S = a.nsrc;
    int st = a.out.range_status[r];
    uint64_t n = 0, kb = 0;
    if (a.ctl[kCtlGo1]) {
        if (!st && a.rop[r]) st = SDB_MERGE_OPERATOR_MISSING;
        if (!st) {
            const uint64_t rs = a.cs[r * S], re = a.cs[(r + 1) * S];
            n = a.wpos[re] - a.wpos[rs];
            kb = a.wkpos[re] - a.wkpos[rs];
        }
        a.out.range_status[r] = st;
    }
    a.rn[r] = n;
    a.rkb[r] = kb;
    if (st) {
        atomicAdd(&a.ctl[kCtlFailed], 1ull);
        atomicMin(&a.ctl[kCtlFirstBad], (unsigned long long)(r << 8 | (uint64_t)st));
    }
}

__global__ void k_ls_final(LsArgs a) {
    if (threadIdx.x != 0) return;
    const uint64_t n = a.r.n;
    sdb_lsm_scan_summary s{};
    s.num_entries = a.out.range_entry_start[n];
    s.key_bytes = a.rks[n];
    s.num_candidates = a.cs[a.pairs];
    s.candidate_key_bytes = a.cks[a.pairs];
    s.num_failed_ranges = a.ctl[kCtlFailed];
    s.blocks_checked = a.t.total_blocks ? a.pr[a.t.total_blocks] : 0;  // (S8: tables and no tree)
    s.status = a.ctl[kCtlFirstBad] == ~0ull ? 0 : (int32_t)(a.ctl[kCtlFirstBad] & 0xFF);
    const bool fits = a.ctl[kCtlGo1] && s.num_entries <= a.out.cap_entries && s.key_bytes <= a.out.key_arena_cap;
    if (!fits) s.status = SDB_LIMIT_EXCEEDED;
    else a.out.key_off[s.num_entries] = s.key_bytes;
    *a.out.summary = s;
    if (a.filter) *a.fout.num_filtered = a.ctl[kCtlFiltered];
    a.ctl[kCtlGo2] = fits;
    if (a.merge) {  // candidates, then rows, then links
        sdb_chain_summary cs{};
        cs.num_links = a.ctl[kCtlGo1] ? a.wlpos[a.cand_entries] : 0;
        cs.max_chain_len = a.ctl[kCtlMaxChain];
        const bool lfits = fits && cs.num_links <= a.chain.cap_links;
        cs.status = lfits ? SDB_OK : SDB_LIMIT_EXCEEDED;
        if (fits) a.chain.chain_start[s.num_entries] = cs.num_links;
        *a.chain.summary = cs;
        a.ctl[kCtlGo3] = lfits;
    }
}

// sdb_lsm_scan_merge, thread per merged position that k_ls_links gave to a winner w: the row parsed, its timestamps
// folded into w's aggregates (MergeTracker, merge_operator.rs:289-292; a tombstone base too, :421-425), and, unless it
// is that tombstone, written as link (position - w) of w's chain where the links fit.
template <bool MEM>
__global__ __launch_bounds__(64) void k_ls_fold(LsArgs a) {
    if (!a.ctl[kCtlGo2]) return;
    const uint32_t S = a.nsrc, T = MEM ? a.ntab : 0;
    const bool put = a.ctl[kCtlGo3] != 0;
    const uint64_t total = a.cs[a.pairs];
    for (uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; m < total; m += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t w = a.lwin[m];
        if (w == ~0ull) continue;
        const uint64_t c = a.morder[m];
        const uint32_t j = (uint32_t)(last_le(a.cs, a.pairs, 1, c) % S);
        const bool tab = MEM && j < T;  // the link lies in a table: its columns are the table's, no block is opened
        uint64_t base;
        Row lr;
        if (tab) {
            lr = tab_row(a.tabs[j], a.cat[c], base);
        } else {
            const sdb_sst_view v = a.t.ssts[j - T];
            Blk b;
            if (blk_open(v, a.cblk[c], b)) continue;
            if (v.sst_version == 2 ? v2_row(b, a.cat[c], lr) : v1_row(b, a.cat[c], lr)) continue;
            base = b.base;
        }
        if (lr.flags & SDB_FLAG_HAS_CREATE_TS) atomicMax(&a.wcts[w], (long long)lr.cts);
        if (lr.flags & SDB_FLAG_HAS_EXPIRE_TS) atomicMin(&a.wets[w], (long long)lr.ets);
        const uint32_t has = (lr.flags & (SDB_FLAG_HAS_CREATE_TS | SDB_FLAG_HAS_EXPIRE_TS)) |
                             ((lr.flags & SDB_FLAG_MERGE_OPERAND) ? 0u : (uint32_t)kBase);
        if (has) atomicOr(&a.whas[w], has);
        if ((lr.flags & SDB_FLAG_TOMBSTONE) || !put) continue;
        const uint64_t x = m - w, d = ls_chain_start(a, last_le(a.cs, a.r.n, S, w), w) + x;
        if (x >= a.wl[w] || d >= a.chain.cap_links) continue;  // never out of the winner's slots
        a.chain.sst[d] = tab ? 0xFFFFFFFFu : j - T;
        a.chain.block[d] = tab ? 0 : a.cblk[c];
        put_row(a.chain, d, base, lr);
        if (MEM) {
            a.mchain.table[d] = tab ? j : 0xFFFFFFFFu;
            a.mchain.row[d] = tab ? a.cat[c] : 0;
        }
    }
}

template <bool MEM>
__global__ __launch_bounds__(64) void k_ls_emit(LsArgs a) {
    if (!a.ctl[kCtlGo2]) return;
    const uint32_t S = a.nsrc, T = MEM ? a.ntab : 0;
    const uint64_t total = a.cs[a.pairs];
    for (uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; m < total; m += (uint64_t)gridDim.x * blockDim.x) {
        if (!a.wn[m]) continue;
        const uint64_t r = last_le(a.cs, a.r.n, S, m);
        if (a.out.range_status[r]) continue;
        const uint64_t rs = a.cs[r * S], c = a.morder[m];
        const uint64_t E0 = a.out.range_entry_start[r], N = a.rn[r], K0 = a.rks[r], KB = a.rkb[r];
        const uint64_t x = a.wpos[m] - a.wpos[rs], kx = a.wkpos[m] - a.wkpos[rs];
        const uint32_t L = a.cklen[c];
        if (x >= N || kx > KB || L > KB - kx) continue;
        const uint64_t di = a.desc ? N - 1 - x : x, dk = a.desc ? KB - kx - L : kx;
        const uint32_t j = (uint32_t)(last_le(a.cs, a.pairs, 1, c) % S);
        const bool tab = MEM && j < T;  // a table won the row (S3)
        uint64_t base;
        Row row;
        if (tab) {
            row = tab_row(a.tabs[j], a.cat[c], base);
        } else {
            const sdb_sst_view v = a.t.ssts[j - T];
            Blk b;
            if (blk_open(v, a.cblk[c], b)) continue;
            if (v.sst_version == 2 ? v2_row(b, a.cat[c], row) : v1_row(b, a.cat[c], row)) continue;
            base = b.base;
        }
        copy_bytes(a.out.key_arena + K0 + dk, a.ckeys + a.ckoff[c], L);
        a.out.key_off[E0 + di] = K0 + dk;
        a.out.sst[E0 + di] = tab ? 0xFFFFFFFFu : j - T;
        if (MEM) {
            a.mout.table[E0 + di] = tab ? j : 0xFFFFFFFFu;
            a.mout.row[E0 + di] = tab ? a.cat[c] : 0;
        }
        if (a.merge) {  // the entry MergeOperatorIterator returns (merge_operator.rs:437-447): k_ls_fold's aggregates
            a.chain.chain_start[E0 + di] = ls_chain_start(a, r, m);
            const uint32_t has = a.whas[m];
            row.flags = (uint8_t)((has & 0xFF) | ((has & kBase) ? 0 : SDB_FLAG_MERGE_OPERAND));
            row.cts = a.wcts[m];
            row.ets = a.wets[m];
        }
        put_row(a.out, E0 + di, base, row);
    }
}

// =================================================================================================
// sdb_lsm_scan_mem: the table sources
// =================================================================================================

// Per tree block: not marked, not read: launch_lsm_scan's two memsets as a kernel (under HIP graph replay memset nodes
// ahead of a captured call's kernels were seen not to take effect: k_mem_reset of sdb_get.hip).
__global__ __launch_bounds__(256) void k_ls_mreset(uint8_t *mark, int32_t *bstat, uint64_t tb) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < tb; k += (uint64_t)gridDim.x * blockDim.x) {
        mark[k] = 0;
        bstat[k] = -1;
    }
}

__global__ __launch_bounds__(256) void k_ls_tvalidate(LsArgs a) {  // after k_ls_validate: it may only add to kCtlBad
    int bad = 0;
    for (uint32_t j = threadIdx.x; j < a.ntab; j += blockDim.x) bad |= tab_malformed(a.tabs[j]);
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0 && bad) a.ctl[kCtlBad] = 1ull;
}

// The first row of T whose key is >= k, or > k with `after`: a lower bound in the table's order, where every
// version of a key stands together.
SDB_DEV uint64_t tab_bound(const sdb_run &T, const Key &k, bool after) {
    uint64_t lo = 0, hi = T.n;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        const int c = tab_cmp(T, mid, k);
        if (c < 0 || (after && c == 0)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// S2, thread per (range, table) pair, t = table * n + range so that a wave holds neighbouring ranges of one table:
// the stretch [g0, g1) of the rows whose key the range contains, into the slots k_ls_edge fills for an SST pair.
// `part` here: the table holds a key of the range (range_tables).
__global__ __launch_bounds__(256) void k_ls_tprobe(LsArgs a) {
    const bool bad = a.ctl[kCtlBad] != 0;
    const uint64_t total = a.r.n * a.ntab;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = t % a.r.n;
        const uint32_t j = (uint32_t)(t / a.r.n);
        const uint64_t p = r * a.nsrc + j;
        uint64_t g0 = 0, g1 = 0, k0 = 0, kb = 0;
        if (!bad) {  // (a malformed call reads nothing through the tables)
            const sdb_run T = a.tabs[j];
            const Bound s = range_start(a.r, r), e = range_end(a.r, r);
            if (T.n && !bad_kind(s, e) && !empty_as_set(s, e)) {
                g0 = s.kind ? tab_bound(T, Key{s.t, s.n}, s.kind == SDB_BOUND_EXCLUDED) : 0;
                g1 = e.kind ? tab_bound(T, Key{e.t, e.n}, e.kind == SDB_BOUND_INCLUDED) : T.n;
                if (g1 < g0) g1 = g0;  // rows that are not sorted
                k0 = T.key_off[g0];
                const uint64_t k1 = T.key_off[g1];
                if (k1 < k0) g1 = g0;  // offsets that descend
                else kb = k1 - k0;
            }
        }
        a.part[p] = g1 > g0;
        a.bs[p] = a.be[p] = a.fb[p] = 0;
        a.pst[p] = 0;
        a.g0[p] = g0;
        a.g1[p] = g1;
        a.k0[p] = k0;
        a.pn[p] = g1 - g0;
        a.pkb[p] = g1 > g0 ? kb : 0;
        a.pit[p] = 0;  // no block items: k_ls_trows stages a table pair
    }
}

// Thread per staged candidate; one of a table pair gets its words from the table's columns, read along the rows: its
// length, seq, flags and the row (cat), and its key, copied to its place in the pair's span of the staging arena.  A
// pair's key bytes are one span key_arena[k0, k0 + bytes) of its table and neighbouring threads copy neighbouring keys,
// so the copy is coalesced as it stands: a separate span copy of 16 bytes a lane was measured and was not faster
// (DESIGN.md, round 15).
__global__ __launch_bounds__(256) void k_ls_trows(LsArgs a) {
    if (!a.ctl[kCtlGo1]) return;
    const uint64_t total = a.cs[a.pairs];
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = last_le(a.cs, a.pairs, 1, c);
        const uint32_t j = (uint32_t)(p % a.nsrc);
        if (j >= a.ntab) continue;  // an SST's: k_ls_stage
        const uint64_t i = a.g0[p] + (c - a.cs[p]), span = a.cks[p + 1] - a.cks[p];
        if (i >= a.g1[p]) continue;
        const sdb_run T = a.tabs[j];
        const uint64_t o0 = T.key_off[i], o1 = T.key_off[i + 1];
        uint64_t o = o0 - a.k0[p], L = o1 - o0;
        if (o0 < a.k0[p] || o1 < o0 || o > span || L > span - o) o = L = 0;  // offsets that descend: never out of the pair's slots
        copy_bytes(a.ckeys + a.cks[p] + o, T.key_arena + o0, (uint32_t)L);
        a.ckoff[c] = a.cks[p] + o;
        a.cklen[c] = (uint32_t)L;
        a.cblk[c] = 0;
        a.cat[c] = (uint32_t)i;
        a.cseq[c] = T.seq[i];
        a.cflags[c] = T.flags[i];
    }
}

// Nothing a call without tables wrote lies in a table (S7): the rows' and the links' table columns, where the row
// and the link columns were written, and range_tables.
__global__ __launch_bounds__(256) void k_ls_mfill(sdb_lsm_scan_out out, sdb_mem_scan_out mout, uint64_t n, sdb_chain_summary *csum,
                                                  uint64_t cap_links, sdb_mem_chain_out mchain) {
    const uint64_t t0 = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = t0; r < n; r += step) mout.range_tables[r] = 0;
    const sdb_lsm_scan_summary s = *out.summary;
    const uint64_t ne = s.status == SDB_LIMIT_EXCEEDED ? 0 : (s.num_entries < out.cap_entries ? s.num_entries : out.cap_entries);
    for (uint64_t x = t0; x < ne; x += step) {
        mout.table[x] = 0xFFFFFFFFu;
        mout.row[x] = 0;
    }
    if (!csum) return;
    const sdb_chain_summary c = *csum;
    const uint64_t nl = c.status != SDB_OK ? 0 : (c.num_links < cap_links ? c.num_links : cap_links);
    for (uint64_t d = t0; d < nl; d += step) {
        mchain.table[d] = 0xFFFFFFFFu;
        mchain.row[d] = 0;
    }
}

// =================================================================================================
// sdb_lsm_scan_recency: the sources drained one after another instead of merged
// =================================================================================================

// Thread per staged candidate (R2, R3): is it visible (seq <= max_seq of its range), and does it open a key group
// of its pair: the pair's first candidate, or its key differs from the candidate's before it.  Neighbouring threads
// read neighbouring staged keys; the lengths are compared first.  Past the candidates, and when they did not fit,
// both flags are 0.
__global__ __launch_bounds__(256) void k_lr_vis(LsArgs a) {
    const uint32_t S = a.nsrc;
    const uint64_t total = a.ctl[kCtlGo1] ? a.cs[a.pairs] : 0;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.cand_entries; c += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t vis = 0, head = 0;
        if (c < total) {
            const uint64_t p = last_le(a.cs, a.pairs, 1, c);
            vis = a.cseq[c] <= (a.max_seq ? a.max_seq[p / S] : ~0ull);
            const uint32_t n = a.cklen[c];
            head = c == a.cs[p] || a.cklen[c - 1] != n || ls_key_cmp(a, c - 1, a.ckeys + a.ckoff[c], n) != 0;
        }
        a.vis[c] = vis;
        a.head[c] = head;
    }
}

// Descending only, thread per candidate: a group's head writes where the group starts, so that group g is
// [gstart[g], gstart[g + 1]); the group of candidate c is gpos[c + 1] - 1.
__global__ __launch_bounds__(256) void k_lr_groups(LsArgs a) {
    if (!a.ctl[kCtlGo1]) return;
    const uint64_t total = a.cs[a.pairs];
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c <= total && c <= a.cand_entries; c += (uint64_t)gridDim.x * blockDim.x)
        if (c == total || a.head[c]) a.gstart[a.gpos[c]] = c;
}

// Pair (r, source j)'s visible rows (k_lr_vis counted them; 0 for a pair that staged nothing).
SDB_DEV uint64_t lr_visible(const LsArgs &a, uint64_t p) { return a.vpos[a.cs[p + 1]] - a.vpos[a.cs[p]]; }

// Thread per range: the walk of R1 / R5.  The sources are the tables, then the runs, newest first; a run's SSTs are
// walked in `ssts` order, descending last to first.  A source is opened while the sources before it gave fewer than
// limit[r] rows; the first opened source with a failing SST fails the range (first failing SST in walk order; its pst is
// its lowest failing block's).  Per pair: where its rows start in the range's output and how many it gives.  When
// the candidates did not fit nothing was counted: the status is then that of limit 0 (every participant is
// opened), and nothing counts as read.
__global__ __launch_bounds__(64) void k_lr_plan(LsArgs a) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.r.n) return;
    const uint32_t S = a.t.num_ssts, T = a.ntab, NS = a.nsrc;
    const bool go = a.ctl[kCtlGo1] != 0;
    const uint64_t L = go && a.limit ? a.limit[r] : 0, p0 = r * NS;
    int st = a.out.range_status[r];  // k_ls_rstat: a malformed call or range
    uint64_t got = 0, seen = 0;
    uint32_t nread = 0;
    bool stop = st != 0;
    for (uint32_t j = 0; j < NS; j++) a.pbase[p0 + j] = a.ptake[p0 + j] = 0;
    for (uint32_t j = 0; j < T && !stop; j++) {  // a table cannot fail; one without a row of the range is no source
        if (!a.part[p0 + j]) continue;
        const uint64_t v = go ? lr_visible(a, p0 + j) : 0, take = L && v > L - got ? L - got : v;
        a.pbase[p0 + j] = got;
        a.ptake[p0 + j] = take;
        got += take;
        seen += v;
        nread++;
        stop = L && got >= L;
    }
    for (uint32_t q = 0; q < a.t.num_runs && !stop; q++) {
        const uint32_t i0 = a.t.run_start[q], i1 = a.t.run_start[q + 1];
        bool any = false;
        for (uint32_t k = i0; k < i1 && k < S; k++) {
            const uint32_t i = a.desc ? i1 - 1 - (k - i0) : k;
            const uint64_t p = p0 + T + i;
            if (i >= S || !a.part[p]) continue;  // (a filtered-out SST takes no part: never opened)
            any = true;
            if (!st) st = a.pst[p];
            const uint64_t v = go ? lr_visible(a, p) : 0, take = L && v > L - got ? L - got : v;
            a.pbase[p] = got;
            a.ptake[p] = take;
            got += take;
            seen += v;
        }
        nread += any;
        stop = st != 0 || (L && got >= L);
    }
    if (st) {  // a failing range returns no row
        for (uint32_t j = 0; j < NS; j++) a.ptake[p0 + j] = 0;
        seen = 0;
    }
    a.out.range_status[r] = st;
    a.rout.range_sources_read[r] = go ? nread : 0;
    a.rout.range_visible[r] = seen;
}

// Thread per candidate (R3, R4): its rank among its pair's visible rows.  Ascending that is the physical order;
// descending the key groups are reversed and a group's versions stay newest first.  A visible candidate whose rank is
// below its pair's take goes to its place in the range's output: its index into morder and the keep flag and key bytes
// into wn / wkb (k_ls_gate zeroed them), the arrays k_ls_rank fills for the merging scans.  No key of another source
// is looked at.
__global__ __launch_bounds__(256) void k_lr_place(LsArgs a) {
    if (!a.ctl[kCtlGo1]) return;
    const uint32_t S = a.nsrc;
    const uint64_t total = a.cs[a.pairs];
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total && c < a.cand_entries; c += (uint64_t)gridDim.x * blockDim.x) {
        if (!a.vis[c]) continue;
        const uint64_t p = last_le(a.cs, a.pairs, 1, c), r = p / S, ps = a.cs[p];
        uint64_t rank = a.vpos[c] - a.vpos[ps];
        if (a.desc) {
            const uint64_t g = a.gpos[c + 1] - 1, gs = a.gstart[g], ge = a.gstart[g + 1];
            if (gs > c || ge <= c || ge > a.cs[p + 1]) continue;  // (never: the groups tile the pair)
            rank = (lr_visible(a, p) - (a.vpos[ge] - a.vpos[ps])) + (a.vpos[c] - a.vpos[gs]);
        }
        if (rank >= a.ptake[p]) continue;
        const uint64_t m = a.cs[r * S] + a.pbase[p] + rank;
        if (m >= a.cs[(r + 1) * S]) continue;  // never out of the range's slots
        a.morder[m] = c;
        a.wn[m] = 1;
        a.wkb[m] = a.cklen[c];
    }
}

// The workspace arrays of a scan of a.r.n ranges over the tree a.t with room for a.cand_entries candidates of
// a.cand_key_bytes key bytes, bound into a from w; -> their size.
static uint64_t lsm_scan_bind(LsArgs &a, uint8_t *w) {
    a.nsrc = a.t.num_ssts + a.ntab;  // (range, source) pairs: the tables' stand before the SSTs'
    a.spairs = a.r.n * a.t.num_ssts;
    const uint64_t tb = a.t.total_blocks, n = a.r.n, P = n * a.nsrc, ce = a.cand_entries;
    uint64_t big = tb > n ? tb : n;
    if (P > big) big = P;
    if (ce > big) big = ce;
    const uint64_t nt = (big + 1023) / 1024 + 2;  // scan tiles
    a.pairs = P;
    Carver c{w, 0};
    c.take(a.mark, tb + 1);
    c.take(a.bstat, tb + 1);
    c.take(a.cnt, tb + 1);
    c.take(a.kb, tb + 1);
    c.take(a.bbad, tb + 1);
    c.take(a.rd, tb + 1);
    c.take(a.pc, tb + 2);
    c.take(a.pk, tb + 2);
    c.take(a.pb, tb + 2);
    c.take(a.pr, tb + 2);
    c.take(a.sstat, (uint64_t)a.t.num_ssts + 1);
    c.take(a.part, P + 1);
    c.take(a.bs, P + 1);
    c.take(a.be, P + 1);
    c.take(a.pst, P + 1);
    c.take(a.fb, P + 1);
    c.take(a.g0, P + 1);
    c.take(a.g1, P + 1);
    c.take(a.k0, P + 1);
    c.take(a.pn, P + 1);
    c.take(a.pkb, P + 1);
    c.take(a.pit, P + 1);
    c.take(a.cs, P + 2);
    c.take(a.cks, P + 2);
    c.take(a.pis, P + 2);
    c.take(a.rop, n + 1);
    c.take(a.rn, n + 1);
    c.take(a.rkb, n + 1);
    c.take(a.rks, n + 2);
    c.take(a.ckeys, a.cand_key_bytes + 1);
    c.take(a.ckoff, ce + 1);
    c.take(a.cseq, ce + 1);
    c.take(a.cklen, ce + 1);
    c.take(a.cblk, ce + 1);
    c.take(a.cat, ce + 1);
    c.take(a.cflags, ce + 1);
    c.take(a.morder, ce + 1);
    c.take(a.wn, ce + 1);
    c.take(a.wkb, ce + 1);
    c.take(a.wpos, ce + 2);
    c.take(a.wkpos, ce + 2);
    c.take(a.tx, nt);
    c.take(a.ty, nt);
    c.take(a.ctl, kCtlWords);
    return c.off;
}

// The workspace arrays of a merging scan: those of the scan, then its own.
static uint64_t lsm_scan_merge_bind(LsArgs &a, uint8_t *w) {
    Carver c{w, lsm_scan_bind(a, w)};
    c.take(a.wl, a.cand_entries + 1);
    c.take(a.wlpos, a.cand_entries + 2);
    c.take(a.wldum, a.cand_entries + 2);
    c.take(a.lwin, a.cand_entries + 1);
    c.take(a.wcts, a.cand_entries + 1);
    c.take(a.wets, a.cand_entries + 1);
    c.take(a.whas, a.cand_entries + 1);
    return c.off;
}

// The workspace arrays of a filtered scan: those of the scan or the merging scan, then its own.
static uint64_t lsm_scan_filter_bind(LsArgs &a, uint8_t *w, bool merge) {
    Carver c{w, merge ? lsm_scan_merge_bind(a, w) : lsm_scan_bind(a, w)};
    c.take(a.filt, a.pairs + 1);
    c.take(a.qlen, a.r.n + 1);
    c.take(a.qh, a.r.n + 1);
    return c.off;
}

// The workspace arrays of the recency scan: those of the filtered scan, then its own.
static uint64_t lsm_scan_recency_bind(LsArgs &a, uint8_t *w) {
    Carver c{w, lsm_scan_filter_bind(a, w, false)};
    c.take(a.vis, a.cand_entries + 1);
    c.take(a.head, a.cand_entries + 1);
    c.take(a.vpos, a.cand_entries + 2);
    c.take(a.gpos, a.cand_entries + 2);
    c.take(a.gstart, a.cand_entries + 2);
    c.take(a.pbase, a.pairs + 1);
    c.take(a.ptake, a.pairs + 1);
    return c.off;
}

// The layout of the entry point: the plain scan's arrays, then the merging scan's, then the filtered scan's, then
// the recency scan's.
static uint64_t lsm_scan_bind_for(LsArgs &a, uint8_t *w, bool merge, bool filter, bool recency) {
    if (recency) return lsm_scan_recency_bind(a, w);
    if (filter) return lsm_scan_filter_bind(a, w, merge);
    return merge ? lsm_scan_merge_bind(a, w) : lsm_scan_bind(a, w);
}

uint64_t lsm_scan_workspace_bytes(const ReadShape &s) {
    LsArgs a{};
    a.t.total_blocks = s.total_blocks;
    a.t.num_ssts = s.num_ssts;
    a.ntab = s.num_tables;  // the pairs count the tables; no array of their own
    a.r.n = s.n;
    a.cand_entries = s.cand_entries;
    a.cand_key_bytes = s.cand_key_bytes;
    return lsm_scan_bind_for(a, nullptr, s.merge, s.filter, s.recency);
}

// The kernels of a bound scan in stream order, through staging.  FILTER: the filters are consulted, PROJ: the call has
// projections, MEM: it has tables (and then always FILTER), REC: the recency scan (and then always MEM), each chosen
// once for the kernels that hold the step.  tree: false only with tables over a tree without SSTs or blocks (S8): none
// of the tree's kernels is launched.
template <bool FILTER, bool PROJ, bool MEM, bool REC = false>
static hipError_t launch_ls_front(const LsArgs &a, bool tree, hipStream_t st) {
    const uint64_t tb = a.t.total_blocks, n = a.r.n, P = a.pairs, SP = a.spairs, ce = a.cand_entries;
    const uint32_t rw = (uint32_t)((n + 63) / 64);
    hipError_t e;
    if constexpr (MEM) {  // the marks and statuses: by a kernel with tables (k_ls_mreset), else by two memsets
        if (tree) hipLaunchKernelGGL(k_ls_mreset, dim3(scan_grid(tb, 256)), dim3(256), 0, st, a.mark, a.bstat, tb);
    } else {
        if ((e = hipMemsetAsync(a.mark, 0, tb, st)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(a.bstat, 0xFF, 4 * tb, st)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_ls_validate<PROJ>, dim3(1), dim3(256), 0, st, a);
    if constexpr (MEM) hipLaunchKernelGGL(k_ls_tvalidate, dim3(1), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_ls_ranges, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, a);
    if constexpr (MEM) hipLaunchKernelGGL(k_ls_tprobe, dim3(scan_grid(n * a.ntab, 256)), dim3(256), 0, st, a);
    if (tree) {
        hipLaunchKernelGGL((k_ls_locate<FILTER, PROJ, MEM>), dim3(scan_grid(SP, 256)), dim3(256), 0, st, a);
        if ((e = launch_check(CheckArgs{{}, a.t, (const uint32_t *)(a.ctl + kCtlBad), tb, a.mark, a.bstat}, st)) != hipSuccess) return e;
        // the per-block, per-pair and per-item walks are latency-bound threads: one wave per workgroup spreads them over the CUs
        hipLaunchKernelGGL(k_ls_block, dim3((uint32_t)((tb + 63) / 64)), dim3(64), 0, st, a);
        if ((e = launch_excl_scan2(a.cnt, a.kb, tb, a.tx, a.ty, a.pc, a.pk, st)) != hipSuccess) return e;
        if ((e = launch_excl_scan2(a.bbad, a.rd, tb, a.tx, a.ty, a.pb, a.pr, st)) != hipSuccess) return e;
        hipLaunchKernelGGL((k_ls_edge<PROJ, MEM>), dim3(scan_grid(SP, 64)), dim3(64), 0, st, a);
    }
    hipLaunchKernelGGL((k_ls_rstat<MEM, REC>), dim3(rw), dim3(64), 0, st, a);
    if ((e = launch_excl_scan2(a.pit, a.pit, P, a.tx, a.ty, a.pis, a.cs, st)) != hipSuccess) return e;
    if ((e = launch_excl_scan2(a.pn, a.pkb, P, a.tx, a.ty, a.cs, a.cks, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ls_gate, dim3(scan_grid(ce, 256)), dim3(256), 0, st, a);
    if (tree) hipLaunchKernelGGL(k_ls_stage<MEM>, dim3(scan_grid(ce + P, 64)), dim3(64), 0, st, a);
    if constexpr (MEM) hipLaunchKernelGGL(k_ls_trows, dim3(scan_grid(ce, 256)), dim3(256), 0, st, a);
    return hipSuccess;
}

// What both tails end with: the winner scan over the positions morder / wn / wkb name, the ranges' totals, the
// summary and the rows.
template <bool MEM>
static hipError_t launch_ls_rows(const LsArgs &a, hipStream_t st) {
    const uint64_t n = a.r.n, ce = a.cand_entries;
    const uint32_t rw = (uint32_t)((n + 63) / 64);
    hipError_t e;
    if ((e = launch_excl_scan2(a.wn, a.wkb, ce, a.tx, a.ty, a.wpos, a.wkpos, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ls_count, dim3(rw), dim3(64), 0, st, a);
    if ((e = launch_excl_scan2(a.rn, a.rkb, n, a.tx, a.ty, a.out.range_entry_start, a.rks, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ls_final, dim3(1), dim3(64), 0, st, a);
    if (a.merge) hipLaunchKernelGGL(k_ls_fold<MEM>, dim3(scan_grid(ce, 64)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_ls_emit<MEM>, dim3(scan_grid(ce, 64)), dim3(64), 0, st, a);
    return hipGetLastError();
}

// After staging, the merging scans: the merged rank and the winners (a.merge: and their chains), then the rows.
template <bool MEM>
static hipError_t launch_ls_merged(const LsArgs &a, hipStream_t st) {
    const uint64_t ce = a.cand_entries;
    hipError_t e;
    hipLaunchKernelGGL(k_ls_rank, dim3(scan_grid(ce, 64)), dim3(64), 0, st, a);
    if (a.merge) {
        hipLaunchKernelGGL(k_ls_links, dim3(scan_grid(ce, 64)), dim3(64), 0, st, a);
        if ((e = launch_excl_scan2(a.wl, a.wl, ce, a.tx, a.ty, a.wlpos, a.wldum, st)) != hipSuccess) return e;
    }
    return launch_ls_rows<MEM>(a, st);
}

// After staging, the recency scan: the flags and their scans, the walk, the placement, then the rows.  The placement
// has put every row where it belongs, descending too, so the rows are written in the order of their positions.
static hipError_t launch_lr_placed(const LsArgs &a, hipStream_t st) {
    const uint64_t ce = a.cand_entries;
    hipError_t e;
    hipLaunchKernelGGL(k_lr_vis, dim3(scan_grid(ce, 256)), dim3(256), 0, st, a);
    if ((e = launch_excl_scan2(a.vis, a.head, ce, a.tx, a.ty, a.vpos, a.gpos, st)) != hipSuccess) return e;
    if (a.desc) hipLaunchKernelGGL(k_lr_groups, dim3(scan_grid(ce + 1, 256)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_lr_plan, dim3((uint32_t)((a.r.n + 63) / 64)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(k_lr_place, dim3(scan_grid(ce, 256)), dim3(256), 0, st, a);
    LsArgs rows = a;
    rows.desc = 0;
    return launch_ls_rows<true>(rows, st);
}

template <bool FILTER, bool PROJ, bool MEM>
static hipError_t launch_ls_kernels(const LsArgs &a, bool tree, hipStream_t st) {
    const hipError_t e = launch_ls_front<FILTER, PROJ, MEM>(a, tree, st);
    return e != hipSuccess ? e : launch_ls_merged<MEM>(a, st);
}

template <bool PROJ>
static hipError_t launch_lr_kernels(const LsArgs &a, bool tree, hipStream_t st) {
    const hipError_t e = launch_ls_front<true, PROJ, true, true>(a, tree, st);
    return e != hipSuccess ? e : launch_lr_placed(a, st);
}

// The instantiations there are: tables come with the filters, and projections too; the recency scan always has the
// tables' step (over none when it has no table).
static hipError_t launch_ls_bound(const LsArgs &a, bool projected, bool tabs, bool tree, bool recency, hipStream_t st) {
    if (recency) return projected ? launch_lr_kernels<true>(a, tree, st) : launch_lr_kernels<false>(a, tree, st);
    if (tabs) return projected ? launch_ls_kernels<true, true, true>(a, tree, st) : launch_ls_kernels<true, false, true>(a, tree, st);
    if (projected) return launch_ls_kernels<true, true, false>(a, tree, st);
    return a.filter ? launch_ls_kernels<true, false, false>(a, tree, st) : launch_ls_kernels<false, false, false>(a, tree, st);
}

// The scan of one call (the special cases: the file comment).  tabs: c.mem holds a table and there is a range (with
// c.mout, and c.mchain iff c.chain).
static hipError_t launch_ls_search(const ScanCall &c, bool tabs, uint8_t *w, hipStream_t st) {
    const sdb_lsm_view &t = *c.lsm;
    const sdb_lsm_scan_out &out = *c.out;
    const sdb_chain_out *chain = c.chain;
    const sdb_scan_filter_out *fout = c.filter ? c.fout : nullptr;
    const uint64_t n = c.ranges->n;
    const bool no_tree = t.num_ssts == 0 || t.total_blocks == 0 || ((tabs || c.recency) && t.num_runs == 0);
    hipError_t e;
    if (n == 0 || (no_tree && !tabs)) {  // every range is empty
        if (chain) {
            if ((e = hipMemsetAsync(chain->summary, 0, sizeof(sdb_chain_summary), st)) != hipSuccess) return e;
            if ((e = hipMemsetAsync(chain->chain_start, 0, 8, st)) != hipSuccess) return e;
        }
        if ((e = hipMemsetAsync(out.summary, 0, sizeof(sdb_lsm_scan_summary), st)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(out.range_entry_start, 0, 8 * (n + 1), st)) != hipSuccess) return e;
        if (n && (e = hipMemsetAsync(out.range_status, 0, 4 * n, st)) != hipSuccess) return e;
        if (n && (e = hipMemsetAsync(out.range_ssts, 0, 4 * n, st)) != hipSuccess) return e;
        if (fout && n && (e = hipMemsetAsync(fout->range_filtered, 0, 4 * n, st)) != hipSuccess) return e;
        if (fout && fout->num_filtered && (e = hipMemsetAsync(fout->num_filtered, 0, 8, st)) != hipSuccess) return e;
        if (c.recency && n) {
            if ((e = hipMemsetAsync(c.rout->range_sources_read, 0, 4 * n, st)) != hipSuccess) return e;
            if ((e = hipMemsetAsync(c.rout->range_visible, 0, 8 * n, st)) != hipSuccess) return e;
        }
        return hipMemsetAsync(out.key_off, 0, 8, st);
    }
    LsArgs a{};
    a.t = t;
    a.r = *c.ranges;
    a.max_seq = c.max_seq;
    a.out = out;
    a.desc = c.desc;
    a.cand_entries = c.cand_entries;
    a.cand_key_bytes = c.cand_key_bytes;
    if (chain) {
        a.merge = 1;
        a.chain = *chain;
    }
    const bool tree = !(tabs && no_tree);
    if (tabs) {
        a.tabs = c.mem ? c.mem->tables : nullptr;  // (the recency scan takes this path without a table too)
        a.ntab = c.mem ? c.mem->num_tables : 0;
        a.mout = *c.mout;
        if (chain) a.mchain = *c.mchain;
        if (!tree) {  // (S8) only the tables are scanned, and nothing is read through the tree's arrays
            a.t.num_ssts = a.t.num_runs = 0;
            a.t.total_blocks = 0;
        }
    }
    const bool projected = fout && tree && c.proj;
    if (fout) {
        a.filter = 1;
        a.pol = tree ? c.pol : nullptr;
        if (c.prefixes) a.px = *c.prefixes;
        a.fout = *fout;
        if (projected) a.proj = *c.proj;
    }
    if (c.recency) {
        a.limit = c.limit;
        a.rout = *c.rout;
    }
    lsm_scan_bind_for(a, w, chain != nullptr, fout != nullptr, c.recency);
    return launch_ls_bound(a, projected, tabs, tree, c.recency, st);
}

hipError_t launch_lsm_scan(const ScanCall &c, uint8_t *w, hipStream_t st) {
    const sdb_lsm_view &t = *c.lsm;
    bool tabs = c.mem && c.mem->num_tables && c.ranges->n;
    // the recency scan walks sources: the tables' path whenever it has a table or a tree (with runs: R1) to walk
    if (c.recency && c.ranges->n && t.num_ssts && t.total_blocks && t.num_runs) tabs = true;
    hipError_t e = launch_ls_search(c, tabs, w, st);
    if (e != hipSuccess || tabs || !c.layers) return e;
    // (S7) sdb_lsm_scan_mem without a table: the projected call, and no row, link or range names a table
    const sdb_chain_out *chain = c.chain;
    uint64_t most = std::max(c.ranges->n, c.out->cap_entries);
    if (chain) most = std::max(most, chain->cap_links);
    if (most)
        hipLaunchKernelGGL(k_ls_mfill, dim3(scan_grid(most, 256)), dim3(256), 0, st, *c.out, *c.mout, c.ranges->n,
                           chain ? chain->summary : nullptr, chain ? chain->cap_links : 0,
                           chain ? *c.mchain : sdb_mem_chain_out{nullptr, nullptr});
    return hipGetLastError();
}

}  // namespace sdb
