// sdb_compactor.cpp — host orchestration of one compaction job on the device (sdb_compactor_*):
// CompactionExecutor::run_subcompaction_merge (compactor_executor.rs:327-390 load_iterators, 818-871
// the output side).  A job is a Job descriptor (the handle and the arguments every entry point takes) passed through
// stages, each of which exists once; [S] marks a host synchronisation:
//   begin_job        the handle's last results reset, the common arguments checked                        every job
//   check_run_shape  the inputs' SST version, the run count, run_start                                    ssts, ranged
//   TableUpload      the per-input and per-run tables: pinned, one copy to the device, tab_ev recorded    ssts, ranged
//                    on every return behind the copy
//   decode_inputs    the block list of the inputs (launch_cx_blocks) and its fail-fast decode             ssts, ranged
//   merge_front      group_runs beyond SDB_MAX_RUNS runs [S per group], the merge workspace and           every job
//                    arguments, the gate, the merged order; with an operator chain_step instead of the
//                    order: the chains [S], their tables when there is a chain [S], the host's fold, the
//                    upload (up_ev); a.ch, bound by it, selects the unit forms of retention and emit
//   cut_step         the cut walk over a stream (padded or not), the cuts' byte offsets, their readback,  every job
//                    with the merged summary in front when asked for [S]
//   encode_outputs   sdb_encode_ssts over the cut ranges, one launch sequence per 8 SSTs, summaries [S]   every job
// The three job functions are those stages plus what is their own:
//   run_job (sdb_compactor_run, _run_merge): merge_front, then retention sized with unbounded capacities [S: the
//       sizes] and the emit into buffers of those sizes; cut_step over the stream as it is, encode_outputs.  3 [S].
//   run_ssts_job (sdb_compactor_run_ssts, _run_ssts_merge): check_run_shape, TableUpload, decode_inputs, its gate
//       (launch_cx_gate: the decode against the declared counts, read by the merge on the device), merge_encode.  2 [S].
//   run_ranged_job (sdb_compactor_run_ssts_ranged): check_run_shape, TableUpload, the covering blocks of every
//       input's view range (k_rx_cover) [S: they size the decode], decode_inputs, the rows inside the ranges and the
//       gate (k_rx_clip, k_rx_gate) [S: the per-run row ranges size the merge], the rows closed up when a range
//       dropped any (k_rx_compact), merge_encode.  4 [S].
//   merge_encode (both jobs over encoded inputs): merge_front, retention + emit into buffers of the declared sizes,
//       the stream padded to the declared count, cut_step over the padded stream with the summary, encode_outputs.
// An operator adds chain_step's two [S] to any of them (the second only when there is a chain).
// A compaction filter and a resume cursor (sdb_compactor_run_filtered, _run_ssts_filtered) are Job fields of the same
// pipeline:
//   seek_runs        S1 of run_job: every run from the lower bound of the cursor's key on [S]; in run_ranged_job the
//                    key is a third start bound of every view range (k_rx_cover) and costs none
//   filtered_tail    replaces what follows the emit: filter_step (the stream gathered to pinned memory [S], the
//                    callbacks, the upload and the apply kernels unless every row is kept; without a filter the
//                    drain count from the device [S]), then cut_step over the final, unpadded stream and
//                    encode_outputs.  merge_encode reads the merged summary first [S] to learn the stream's length.
// The outputs stay in the handle's device memory.  The handle's buffers (DevBuf, PinBuf) and every layout inside them
// come from sdb_host.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/slatedb_amd.h"
#include "sdb_compact.h"
#include "sdb_decode.h"
#include "sdb_host.h"

using namespace sdb;

struct GroupBufs {  // a group of runs merged ahead of the job (runs beyond SDB_MAX_RUNS)
    DevBuf cols, keys, vals, asrun;
};

// A device buffer of the merge-operator step.  With canaries on (sdb_diag_compactor_canaries) every ensure()
// allocates exactly the bytes asked for between two guard bands and fills all of it with 0xA5, so a test sees
// a write outside the sized regions, or a kernel that relies on zeroed memory.
struct GuardBuf {
    static constexpr uint64_t kGuard = 512;
    DevBuf buf;
    uint64_t bytes = 0;
    bool guarded = false;
    bool ensure(uint64_t n, bool guard) {
        if (!guard) {
            guarded = false;
            return buf.ensure(n);
        }
        buf.release();
        guarded = false;
        if (!buf.ensure(n + 2 * kGuard) || hipMemset(buf.p, 0xA5, buf.cap) != hipSuccess ||
            hipDeviceSynchronize() != hipSuccess)
            return false;
        bytes = n;
        guarded = true;
        return true;
    }
    uint8_t *base() const { return buf.at<uint8_t>(guarded ? kGuard : 0); }
    // guard bytes that changed (the slack behind the sized bytes counts as guard), or -1
    int64_t damaged() const {
        if (!guarded) return 0;
        std::vector<uint8_t> h(buf.cap);
        if (hipMemcpy(h.data(), buf.p, buf.cap, hipMemcpyDeviceToHost) != hipSuccess) return -1;
        int64_t bad = 0;
        for (uint64_t i = 0; i < buf.cap; i++)
            if ((i < kGuard || i >= kGuard + bytes) && h[i] != 0xA5) bad++;
        return bad;
    }
};

// Orders the reuse of a host buffer behind the stream work that still reads it: the job that queued the work
// records the event, the next job waits for it before it rewrites the buffer.
struct StreamEvent {
    hipEvent_t ev = nullptr;
    bool live = false;
    bool wait() {  // (creates the event once)
        if (live && hipEventSynchronize(ev) != hipSuccess) return false;
        live = false;
        if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
        return ev != nullptr;
    }
    void record(hipStream_t s) { live = hipEventRecord(ev, s) == hipSuccess; }
    ~StreamEvent() {
        if (ev) (void)hipEventSynchronize(ev);
        if (ev) (void)hipEventDestroy(ev);
    }
};

struct sdb_compactor {
    int device = 0;
    DevBuf merge_ws, cols, keys, vals, cut_ws, cuts, sst_meta, sst_data, sst_bloom, enc_ws, dec, dec_ws, cx_tab;
    std::vector<GroupBufs> groups;
    PinBuf pin, pin_tab;
    // the filter and resume stages: the stream gathered for the filter (pinned, with the decisions), the replacement
    // values (pinned), the uploaded decisions and the final stream (device, cf_bind); the cursor's key and the runs'
    // lower bounds (seek_ws and its pinned mirror)
    PinBuf pin_cf, pin_cf_up, pin_seek;
    DevBuf cf_ws, seek_ws;
    sdb_filter_stats fstats{};
    std::vector<const uint8_t *> cf_nv;  // one filter call's replacement pointers and lengths
    std::vector<uint64_t> cf_nl;
    std::vector<sdb_run> seeked;         // a resumed job's runs from their lower bounds on
    // the merge-operator step: per-position chain state, the chain tables + staging arena (device and pinned
    // mirror), the merged values (pinned, then device)
    GuardBuf chain_ws, chain_tab, chain_up;
    PinBuf pin_chain, pin_up;
    StreamEvent up_ev;  // the upload of pin_up: the next job waits for it before it rewrites pin_up
    bool canaries = false;
    sdb_merge_op_stats mstats{};
    // the ranged job: what its cover, clip and gate kernels write (rx_ws), and the contributed rows closed up
    // into columns of their own when a range dropped any (rx_cols)
    GuardBuf rx_ws, rx_cols;
    sdb_range_job_stats rstats{};
    // recorded on the job's stream when a run_ssts job returns (every path): the next job waits for it
    // before it rewrites pin_tab / cx_tab, which that job's upload and kernels may still be reading
    StreamEvent tab_ev;
    StreamEvent cf_ev;  // the upload out of pin_cf / pin_cf_up: the next job waits for it before it rewrites them
    sdb_kv_batch merged{};
    sdb_merge_summary msum{};
    std::vector<sdb_compacted_sst> ssts;
    // the members free themselves after this, last declared first: the two events wait for the last job's
    // uploads before the pinned tables they read (declared above them) go
    ~sdb_compactor() { (void)hipSetDevice(device); }
};

namespace {

// One job: the handle and the arguments every entry point takes, as every stage takes them.
struct Job {
    sdb_compactor *c;
    const sdb_retention *ret;
    sdb_merge_batch_fn op;  // NULL: a job without a merge operator
    void *ctx;
    const sdb_sst_params *params;
    uint64_t max_sst_size;
    void *stream;  // as the public calls take it
    uint32_t *num_ssts;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const sdb_compaction_filter *filter = nullptr;  // NULL: a job without a compaction filter
    const sdb_resume_cursor *resume = nullptr;      // NULL: a job that starts at its first row
};

// An sdb_run of n entries over columns, from their entry e0 on (the arenas are not offset: *_off index them).
sdb_run run_over(uint64_t e0, uint64_t n, const uint8_t *key_arena, const uint64_t *key_off, const uint8_t *val_base,
                 const uint64_t *val_off, const uint32_t *val_len, const uint64_t *seq, const uint8_t *flags,
                 const int64_t *create_ts, const int64_t *expire_ts) {
    return sdb_run{n, key_arena, key_off + e0, val_base, val_off + e0, val_len + e0, seq + e0, flags + e0, create_ts + e0,
                   expire_ts + e0};
}

// Sizes (base == NULL) or binds the merged-stream columns of `total` entries.
uint64_t merged_bind(sdb_merged_out &o, uint64_t total, uint8_t *base) {
    Carver c{base, 0};
    c.take(o.key_off, total + 1);
    c.take(o.val_off, total + 1);
    c.take(o.kind, total + 1);
    c.take(o.seq, total + 1);
    c.take(o.create_ts, total + 1);
    c.take(o.expire_ts, total + 1);
    c.take(o.ts_mask, total + 1);
    c.take(o.summary, 1);
    return c.off;
}
// merged-stream columns for `total` entries in `cols`: the sdb_merged_out (byte arenas unset)
sdb_status merged_columns_in(DevBuf &cols, uint64_t total, sdb_merged_out *out) {
    *out = sdb_merged_out{};
    out->key_cap = ~0ull;
    out->val_cap = ~0ull;
    out->cap_entries = total;
    if (!cols.ensure(merged_bind(*out, total, nullptr))) return SDB_DEVICE_ERROR;
    merged_bind(*out, total, cols.at<uint8_t>(0));
    return SDB_OK;
}

// The cut list of a stream of n entries: the cut count, n + 2 cuts, n + 2 (key, value) byte offset pairs.
struct CutLayout {
    uint64_t num, cut, off;
};
CutLayout cut_layout(Carver &c, uint64_t n) { return {c.bytes(8), c.bytes(8 * (n + 2)), c.bytes(16 * (n + 2))}; }

// A job with more runs than one merge takes (SDB_MAX_RUNS): groups of SDB_MAX_RUNS consecutive runs are
// merged first without retention (every entry kept as it is, in the group's MergeIterator order: key asc,
// seq desc, run), and the group streams become the job's runs.  Groups are consecutive runs, so equal keys
// with equal seqs keep their run order and the job's merged stream is the one a single merge of every run
// would give (merge_iterator.rs:55-69).  One host synchronisation per group (its byte sizes).  A run out
// of order fails the job like the single merge: c->msum = the group merge's summary, first_error_entry
// rebased to the job's entry numbering.  gate: the decode gate of sdb_compactor_run_ssts (or NULL).
sdb_status group_runs(const Job &j, const sdb_run *runs, uint32_t nruns, const unsigned long long *gate,
                      std::vector<sdb_run> &grouped) {
    sdb_compactor *c = j.c;
    hipStream_t s = j.s;
    const uint32_t ng = (nruns + kMaxRuns - 1) / kMaxRuns;
    if (ng > kMaxRuns) return SDB_LIMIT_EXCEEDED;
    uint64_t job_total = 0;
    for (uint32_t r = 0; r < nruns; r++) job_total += runs[r].n;
    if (c->groups.size() < ng) c->groups.resize(ng);
    grouped.clear();
    uint64_t base = 0;
    const sdb_retention none{};
    for (uint32_t g = 0; g < ng; g++) {
        const uint32_t r0 = g * kMaxRuns, r1 = std::min(nruns, r0 + kMaxRuns);
        GroupBufs &B = c->groups[g];
        uint64_t total = 0;
        for (uint32_t r = r0; r < r1; r++) total += runs[r].n;
        sdb_merged_out out{};
        sdb_status st = merged_columns_in(B.cols, total, &out);
        if (st) return st;
        if (!c->merge_ws.ensure(sdb_merge_runs_workspace_bytes(runs + r0, r1 - r0))) return SDB_DEVICE_ERROR;
        MergeArgs a;
        st = build_merge_args(runs + r0, r1 - r0, &none, &out, c->merge_ws.p, c->merge_ws.cap, &a, true);
        if (st) return st;
        a.gate = gate;
        sdb_merge_summary sm{};
        if (launch_merge(a, false, s) != hipSuccess ||
            hipMemcpyAsync(&sm, out.summary, sizeof(sm), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return SDB_DEVICE_ERROR;
        if (sm.status) {
            c->msum = sm;
            c->msum.num_in = job_total;
            // the group's entry numbering starts at `base` in the job's (a gate error can only come from
            // group 0, whose base is 0)
            if (sm.status == SDB_INVALID_ARGUMENT && sm.first_error_entry != ~0ull) c->msum.first_error_entry += base;
            return (sdb_status)sm.status;
        }
        Carver rc{nullptr, 0};  // what a run has and a merged stream lacks: value lengths, then row flags
        const uint64_t o_vlen = rc.bytes(4 * (total + 1)), o_flags = rc.bytes(total + 1);
        if (!B.keys.ensure(sm.key_bytes + 16) || !B.vals.ensure(sm.val_bytes + 16) || !B.asrun.ensure(rc.off))
            return SDB_DEVICE_ERROR;
        a.out.key_bytes = B.keys.at<uint8_t>(0);
        a.out.key_cap = sm.key_bytes;
        a.out.val_bytes = B.vals.at<uint8_t>(0);
        a.out.val_cap = sm.val_bytes;
        uint32_t *vlen = B.asrun.at<uint32_t>(o_vlen);
        uint8_t *flags = B.asrun.at<uint8_t>(o_flags);
        if (launch_merge_emit(a, s) != hipSuccess || launch_merged_as_run(a.out, total, vlen, flags, s) != hipSuccess)
            return SDB_DEVICE_ERROR;
        grouped.push_back(run_over(0, total, a.out.key_bytes, a.out.key_off, a.out.val_bytes, a.out.val_off, vlen, a.out.seq,
                                   flags, a.out.create_ts, a.out.expire_ts));
        base += total;
    }
    return SDB_OK;
}

// One chain through the operator as MergeOperatorIterator::merge_with_older_entries does it
// (merge_operator.rs:341-447; slatedb_amd/merge.py fold): the operands, newest first, in batches of
// MERGE_BATCH_SIZE, each batch reversed to oldest first and merged with no existing value; the batch results,
// reversed to oldest first, merged once with the base.  Appends the merged value to `out`.
constexpr uint32_t kMergeBatch = 100;  // merge_operator.rs:194
bool fold_chain(sdb_merge_batch_fn op, void *ctx, const uint8_t *key, uint64_t key_len,
                const std::vector<const uint8_t *> &vals, const std::vector<uint64_t> &lens, const uint8_t *base,
                uint64_t base_len, std::vector<uint8_t> &out, uint64_t *calls) {
    std::vector<std::vector<uint8_t>> results;
    std::vector<const uint8_t *> bp;
    std::vector<uint64_t> bl;
    const uint64_t m = vals.size();
    for (uint64_t i = 0; i < m; i += kMergeBatch) {
        const uint64_t e = std::min<uint64_t>(m, i + kMergeBatch);
        bp.clear();
        bl.clear();
        for (uint64_t j = e; j-- > i;) {
            bp.push_back(vals[j]);
            bl.push_back(lens[j]);
        }
        const uint8_t *r = nullptr;
        uint64_t rl = 0;
        ++*calls;
        if (op(ctx, key, key_len, nullptr, 0, bp.data(), bl.data(), (uint32_t)bp.size(), &r, &rl) != 0 || (rl && !r))
            return false;
        results.emplace_back(r, r + rl);  // copied at once: *result lives until the next call
    }
    bp.clear();
    bl.clear();
    for (uint64_t j = results.size(); j-- > 0;) {
        bp.push_back(results[j].data());
        bl.push_back(results[j].size());
    }
    const uint8_t *r = nullptr;
    uint64_t rl = 0;
    ++*calls;
    if (op(ctx, key, key_len, base, base ? base_len : 0, bp.data(), bl.data(), (uint32_t)bp.size(), &r, &rl) != 0 ||
        (rl && !r))
        return false;
    out.insert(out.end(), r, r + rl);
    return true;
}

// The merge-operator step of a job, between the merged order and retention: a's merged order and unit codes
// (one synchronisation: the chain summary), then, when there is a chain, the chain tables and the staging
// arena to pinned memory (one synchronisation), the fold of every chain through `op`, and the merged values
// and their offsets back to the device (a.ch.moff / mval; asynchronous, from pin_up).  Leaves the job's chain
// counts in c->mstats.  An operator failure: SDB_MERGE_OPERATOR_ERROR, with c->msum filled.
sdb_status chain_step(const Job &j, MergeArgs &a) {
    sdb_compactor *c = j.c;
    hipStream_t s = j.s;
    if (!c->chain_ws.ensure(chain_bind(a.ch, a.total, nullptr), c->canaries)) return SDB_DEVICE_ERROR;
    chain_bind(a.ch, a.total, c->chain_ws.base());
    ChainSummary cs{};
    if (launch_merge_chains(a, s) != hipSuccess ||
        hipMemcpyAsync(&cs, a.ch.summary, sizeof(cs), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SDB_DEVICE_ERROR;
    sdb_merge_op_stats &ms = c->mstats;
    ms.groups = cs.groups;
    ms.links = cs.links;
    ms.link_bytes = cs.link_bytes;
    if (!cs.groups) return SDB_OK;  // no chain: no copy, no operator call

    const uint64_t tab_bytes = chain_tables_bind(a.ch, cs, nullptr);
    if (!c->chain_tab.ensure(tab_bytes, c->canaries) || !c->pin_chain.ensure(tab_bytes)) return SDB_DEVICE_ERROR;
    chain_tables_bind(a.ch, cs, c->chain_tab.base());
    if (launch_chain_tables(a, s) != hipSuccess ||
        hipMemcpyAsync(c->pin_chain.p, c->chain_tab.base(), tab_bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SDB_DEVICE_ERROR;
    ChainArgs h{};  // the tables' host mirror
    chain_tables_bind(h, cs, c->pin_chain.at<uint8_t>(0));

    std::vector<uint8_t> merged;
    std::vector<uint64_t> moff(cs.groups + 1);
    std::vector<const uint8_t *> vals;
    std::vector<uint64_t> lens;
    merged.reserve(cs.link_bytes);
    for (uint64_t g = 0; g < cs.groups; g++) {
        const ChainGroup &G = h.group[g];
        const uint64_t nops = G.nlinks - (G.base != kBaseNone ? 1 : 0);
        vals.clear();
        lens.clear();
        for (uint64_t j = 0; j < nops; j++) {
            const ChainLink &L = h.link[G.link0 + j];
            vals.push_back(h.arena + L.off);
            lens.push_back(L.len);
        }
        const uint8_t *base = nullptr;
        uint64_t base_len = 0;
        if (G.base == kBaseValue) {  // (a tombstone base has no value: None)
            const ChainLink &L = h.link[G.link0 + nops];
            base = h.arena + L.off;
            base_len = L.len;
        }
        moff[g] = merged.size();
        if (!fold_chain(j.op, j.ctx, h.arena + G.key_off, G.key_len, vals, lens, base, base_len, merged, &ms.operator_calls)) {
            c->msum = sdb_merge_summary{};
            c->msum.num_in = a.total;
            c->msum.status = SDB_MERGE_OPERATOR_ERROR;
            c->msum.first_error_entry = G.head;
            return SDB_MERGE_OPERATOR_ERROR;
        }
        if (merged.size() - moff[g] > 0xFFFFFFFFull) return SDB_LIMIT_EXCEEDED;  // value lengths are u32
    }
    moff[cs.groups] = merged.size();
    ms.merged_bytes = merged.size();

    // the upload: offsets, then bytes (+ 16: the emit's 16-byte chunk loads stay inside)
    Carver uc{nullptr, 0};
    const uint64_t u_off = uc.bytes(8 * (cs.groups + 1)), u_val = uc.bytes(merged.size() + 16);
    if (!c->up_ev.wait() || !c->chain_up.ensure(uc.off, c->canaries) || !c->pin_up.ensure(uc.off)) return SDB_DEVICE_ERROR;
    memcpy(c->pin_up.at<uint8_t>(u_off), moff.data(), 8 * (cs.groups + 1));
    if (!merged.empty()) memcpy(c->pin_up.at<uint8_t>(u_val), merged.data(), merged.size());
    memset(c->pin_up.at<uint8_t>(u_val) + merged.size(), 0, 16);
    uint8_t *up = c->chain_up.base();
    if (hipMemcpyAsync(up + u_off, c->pin_up.at<uint8_t>(u_off), 8 * (cs.groups + 1), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(up + u_val, c->pin_up.at<uint8_t>(u_val), merged.size() + 16, hipMemcpyHostToDevice, s) != hipSuccess)
        return SDB_DEVICE_ERROR;
    c->up_ev.record(s);
    a.ch.moff = reinterpret_cast<const uint64_t *>(up + u_off);
    a.ch.mval = up + u_val;
    return SDB_OK;
}

sdb_kv_batch batch_of(const sdb_merged_out &o, uint64_t n) {
    sdb_kv_batch m{};
    m.n = n;
    m.key_bytes = o.key_bytes;
    m.key_off = o.key_off;
    m.val_bytes = o.val_bytes;
    m.val_off = o.val_off;
    m.kind = o.kind;
    m.seq = o.seq;
    m.create_ts = o.create_ts;
    m.expire_ts = o.expire_ts;
    m.ts_mask = o.ts_mask;
    m.prefix_len = nullptr;
    return m;
}

// F9 on the host: what a filter and a cursor must carry (either may be NULL).
bool filter_args_ok(const sdb_compaction_filter *f, const sdb_resume_cursor *r) {
    return !(f && !f->filter) && !(r && ((!r->key && r->key_len) || r->key_len > 0xFFFFFFFFull));
}

// The prologue of every job: the handle's results of the last job reset, the arguments every job takes checked.
sdb_status begin_job(const Job &j) {
    sdb_compactor *c = j.c;
    if (!c || !j.params || !j.num_ssts) return SDB_INVALID_ARGUMENT;
    *j.num_ssts = 0;
    c->ssts.clear();
    c->merged = sdb_kv_batch{};
    c->msum = sdb_merge_summary{};
    c->mstats = sdb_merge_op_stats{};
    c->rstats = sdb_range_job_stats{};
    c->fstats = sdb_filter_stats{};
    if (!filter_args_ok(j.filter, j.resume)) return SDB_INVALID_ARGUMENT;  // F9
    if (j.params->sst_type != SDB_SST_COMPACTED || !j.ret) return SDB_INVALID_ARGUMENT;  // compactions write compacted SSTs
    return SDB_OK;
}

// The front of every merge: `runs` grouped when one merge does not take them all (group_runs), the merge workspace
// and arguments over `out` (a copies the runs), the decode gate (or NULL), and the merged order; with an operator the
// chains, the fold and the upload behind it (chain_step), which bind a.ch, so the retention and emit launches that
// follow run over the units.
sdb_status merge_front(const Job &j, const sdb_run *runs, uint32_t nruns, const unsigned long long *gate,
                       const sdb_merged_out &out, MergeArgs &a) {
    sdb_compactor *c = j.c;
    sdb_status st;
    std::vector<sdb_run> grouped;
    if (nruns > kMaxRuns) {
        if ((st = group_runs(j, runs, nruns, gate, grouped))) return st;
        runs = grouped.data();
        nruns = (uint32_t)grouped.size();
    }
    if (!c->merge_ws.ensure(sdb_merge_runs_workspace_bytes(runs, nruns))) return SDB_DEVICE_ERROR;
    if ((st = build_merge_args(runs, nruns, j.ret, &out, c->merge_ws.p, c->merge_ws.cap, &a))) return st;
    a.gate = gate;
    if (j.op) return chain_step(j, a);
    return launch_merge_order(a, j.s) == hipSuccess ? SDB_OK : SDB_DEVICE_ERROR;
}

// The readback of a job's cuts through c->pin, around the job's synchronisation.  Every SST but the last holds
// more than max_sst_size bytes of blocks, and a block costs at most its keys, values and 64 bytes per row, so g
// bounds the count for a stream of n entries and `bytes` key and value bytes; a larger one takes a second copy.
struct CutRead {
    uint64_t g;
    const uint64_t *d_cut, *d_off;
    const sdb_merge_summary *sum;     // pinned: the merged summary (NULL: not asked for)
    const uint64_t *num, *cut, *off;  // pinned: the count, g + 1 cuts, their offsets
};
// The cut step of every job, over the stream m of m.n entries whose true length is *n_real on the device (NULL: m.n,
// a stream that is not padded) and whose keys and values are at most `bytes` bytes: the cut list in c->cuts (the cut
// walk, then the byte offsets of every cut, which size the SSTs), its readback into c->pin as r describes it, with
// the merged summary d_sum in front (unless NULL), and the job's synchronisation.  Nothing is walked when m.n == 0.
sdb_status cut_step(const Job &j, const sdb_kv_batch &m, const uint64_t *n_real, uint64_t bytes,
                    const sdb_merge_summary *d_sum, CutRead &r) {
    sdb_compactor *c = j.c;
    const uint64_t n = m.n;
    Carver dc{nullptr, 0};
    const CutLayout dl = cut_layout(dc, n);
    if (!c->cut_ws.ensure(sdb_sst_cuts_workspace_bytes(n, j.params)) || !c->cuts.ensure(dc.off)) return SDB_DEVICE_ERROR;
    uint64_t *d_num = c->cuts.at<uint64_t>(dl.num), *d_cut = c->cuts.at<uint64_t>(dl.cut), *d_off = c->cuts.at<uint64_t>(dl.off);
    if (n) {
        const sdb_status st = sst_cuts_padded(&m, j.params, j.max_sst_size, d_cut, n + 1, d_num, c->cut_ws.p, c->cut_ws.cap,
                                              j.s, n_real);
        if (st) return st;
        if (launch_cut_offsets(d_cut, d_num, m.key_off, m.val_off, d_off, j.s) != hipSuccess) return SDB_DEVICE_ERROR;
    }
    const uint64_t g = j.max_sst_size ? std::min<uint64_t>(n, 2 + (bytes + 64 * n) / j.max_sst_size) : n;
    Carver hc{nullptr, 0};
    const uint64_t h_sum = hc.bytes(sizeof(sdb_merge_summary));
    const CutLayout hl = cut_layout(hc, g);
    if (!c->pin.ensure(hc.off)) return SDB_DEVICE_ERROR;
    sdb_merge_summary *hsum = c->pin.at<sdb_merge_summary>(h_sum);
    uint64_t *hnum = c->pin.at<uint64_t>(hl.num), *hcut = c->pin.at<uint64_t>(hl.cut), *hoff = c->pin.at<uint64_t>(hl.off);
    *hnum = 0;
    r = CutRead{g, d_cut, d_off, d_sum ? hsum : nullptr, hnum, hcut, hoff};
    const bool queued =
        (!d_sum || hipMemcpyAsync(hsum, d_sum, sizeof(sdb_merge_summary), hipMemcpyDeviceToHost, j.s) == hipSuccess) &&
        (!n || (hipMemcpyAsync(hnum, d_num, 8, hipMemcpyDeviceToHost, j.s) == hipSuccess &&
                hipMemcpyAsync(hcut, d_cut, 8 * (g + 1), hipMemcpyDeviceToHost, j.s) == hipSuccess &&
                hipMemcpyAsync(hoff, d_off, 16 * (g + 1), hipMemcpyDeviceToHost, j.s) == hipSuccess));
    return queued && hipStreamSynchronize(j.s) == hipSuccess ? SDB_OK : SDB_DEVICE_ERROR;
}
// After the synchronisation: the SST count of a merged stream of n > 0 entries, its cuts and their offsets (taken
// out of c->pin, which encode_outputs reuses).
sdb_status cut_read_end(const CutRead &r, uint64_t n, uint64_t *num, std::vector<uint64_t> &cut, std::vector<uint64_t> &off) {
    const uint64_t ns = *r.num;
    if (ns == 0 || ns > n) return SDB_DEVICE_ERROR;
    cut.resize(ns + 1);
    off.resize(2 * (ns + 1));
    if (ns > r.g) {
        if (hipMemcpy(cut.data(), r.d_cut, 8 * (ns + 1), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(off.data(), r.d_off, 16 * (ns + 1), hipMemcpyDeviceToHost) != hipSuccess)
            return SDB_DEVICE_ERROR;
    } else {
        memcpy(cut.data(), r.cut, 8 * (ns + 1));
        memcpy(off.data(), r.off, 16 * (ns + 1));
    }
    *num = ns;
    return SDB_OK;
}

// The last step of every job, after the synchronisation of cut_step: encode every output SST (sets of up to 8
// per launch sequence) over the cut ranges of c->merged (n > 0 entries), then read the summaries back (one
// synchronisation)
sdb_status encode_outputs(const Job &j, const CutRead &rd, uint64_t n) {
    sdb_compactor *c = j.c;
    const sdb_sst_params *params = j.params;
    hipStream_t s = j.s;
    const sdb_kv_batch &m = c->merged;
    uint64_t ns = 0;
    std::vector<uint64_t> cut, off;
    sdb_status st = cut_read_end(rd, n, &ns, cut, off);
    if (st) return st;
    std::vector<sdb_kv_batch> batches(ns);
    std::vector<sdb_sst_out> outs(ns);
    for (uint64_t i = 0; i < ns; i++) {
        const uint64_t b = cut[i], e = cut[i + 1], ni = e - b;
        sdb_kv_batch &x = batches[i];
        x = m;
        x.n = ni;
        x.key_off = m.key_off + b;
        x.val_off = m.val_off + b;
        x.kind = m.kind + b;
        x.seq = m.seq + b;
        x.create_ts = m.create_ts + b;
        x.expire_ts = m.expire_ts + b;
        x.ts_mask = m.ts_mask + b;
        st = sdb_encode_bounds(ni, off[2 * (i + 1)] - off[2 * i], off[2 * (i + 1) + 1] - off[2 * i + 1], params,
                               &outs[i].data_cap, &outs[i].block_cap, &outs[i].bloom_cap);
        if (st) return st;
    }
    // data sections, filters and per-block arrays each in a buffer of their own; the summaries packed at the
    // front of sst_meta, so one copy reads them back.  Sized with NULL bases, then bound.
    uint64_t data_total = 0, bloom_total = 0, meta_total = 0;
    auto bind = [&](uint8_t *data, uint8_t *bloom, uint8_t *meta) {
        Carver cd{data, 0}, cb{bloom, 0}, cm{meta, 0};
        sdb_sst_summary *sums = nullptr;
        cm.take(sums, ns);
        for (uint64_t i = 0; i < ns; i++) {
            cd.take(outs[i].data, outs[i].data_cap);
            cb.take(outs[i].bloom, outs[i].bloom_cap);
            bind_sst_out(cm, outs[i], false);
            outs[i].summary = sums ? sums + i : nullptr;
        }
        data_total = cd.off, bloom_total = cb.off, meta_total = cm.off;
    };
    bind(nullptr, nullptr, nullptr);
    if (!c->sst_data.ensure(data_total) || !c->sst_bloom.ensure(bloom_total) || !c->sst_meta.ensure(meta_total))
        return SDB_DEVICE_ERROR;
    bind(c->sst_data.at<uint8_t>(0), c->sst_bloom.at<uint8_t>(0), c->sst_meta.at<uint8_t>(0));
    const uint64_t ews = sdb_encode_ssts_workspace_bytes((uint32_t)ns, batches.data(), params);
    if (!c->enc_ws.ensure(ews)) return SDB_DEVICE_ERROR;
    st = sdb_encode_ssts((uint32_t)ns, batches.data(), params, outs.data(), c->enc_ws.p, c->enc_ws.cap, j.stream);
    if (st) return st;
    if (!c->pin.ensure(ns * sizeof(sdb_sst_summary))) return SDB_DEVICE_ERROR;
    sdb_sst_summary *sums = static_cast<sdb_sst_summary *>(c->pin.p);
    if (hipMemcpyAsync(sums, c->sst_meta.p, ns * sizeof(sdb_sst_summary), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SDB_DEVICE_ERROR;
    c->ssts.resize(ns);
    sdb_status first = SDB_OK;
    for (uint64_t i = 0; i < ns; i++) {
        sdb_compacted_sst &v = c->ssts[i];
        v.entry_start = cut[i];
        v.entry_end = cut[i + 1];
        v.data = outs[i].data;
        v.block_off = outs[i].block_off;
        v.block_first_entry = outs[i].block_first_entry;
        v.index_key_len = outs[i].index_key_len;
        v.block_stats = outs[i].block_stats;
        v.bloom = outs[i].bloom;
        v.summary = sums[i];
        if (!first && sums[i].status) first = (sdb_status)sums[i].status;
    }
    *j.num_ssts = (uint32_t)ns;
    return first;
}

// ---- the compaction filter and the resume cursor (rules F1-F10, S1-S3 of the header) ----

// S1 of the decoded-runs job: `runs` from each run's first row with key >= K on (a device lower bound per run, read
// back: one synchronisation), so sdb_run.n and the bases stay host values.
sdb_status seek_runs(const Job &j, const sdb_run *runs, uint32_t nruns, std::vector<sdb_run> &out) {
    sdb_compactor *c = j.c;
    const sdb_resume_cursor &rc = *j.resume;
    // what build_merge_args asks of a run, before k_cf_seek reads its keys
    for (uint32_t r = 0; r < nruns; r++) {
        const sdb_run &R = runs[r];
        if (R.n && (!R.key_arena || !R.key_off || !R.val_off || !R.val_len || !R.seq || !R.flags)) return SDB_INVALID_ARGUMENT;
    }
    out.assign(runs, runs + nruns);
    if (!nruns) return SDB_OK;
    CfSeekRun *h_runs = nullptr, *d_runs = nullptr;
    uint8_t *h_key = nullptr, *d_key = nullptr;
    uint64_t *h_lb = nullptr, *d_lb = nullptr;
    auto bind = [&](uint8_t *base, CfSeekRun *&r, uint8_t *&k, uint64_t *&lb) {
        Carver k_{base, 0};
        k_.take(r, nruns);
        k_.take(k, rc.key_len + 1);
        k_.take(lb, nruns);
        return k_.off;
    };
    const uint64_t bytes = bind(nullptr, h_runs, h_key, h_lb);
    if (!c->pin_seek.ensure(bytes) || !c->seek_ws.ensure(bytes)) return SDB_DEVICE_ERROR;
    bind(c->pin_seek.at<uint8_t>(0), h_runs, h_key, h_lb);
    bind(c->seek_ws.at<uint8_t>(0), d_runs, d_key, d_lb);
    for (uint32_t r = 0; r < nruns; r++) h_runs[r] = CfSeekRun{runs[r].key_arena, runs[r].key_off, runs[r].n};
    if (rc.key_len) memcpy(h_key, rc.key, rc.key_len);
    const uint64_t up = (uint64_t)(reinterpret_cast<uint8_t *>(h_lb) - reinterpret_cast<uint8_t *>(h_runs));
    if (hipMemcpyAsync(d_runs, h_runs, up, hipMemcpyHostToDevice, j.s) != hipSuccess ||
        launch_cf_seek(d_runs, nruns, d_key, (uint32_t)rc.key_len, d_lb, j.s) != hipSuccess ||
        hipMemcpyAsync(h_lb, d_lb, 8 * (uint64_t)nruns, hipMemcpyDeviceToHost, j.s) != hipSuccess ||
        hipStreamSynchronize(j.s) != hipSuccess)
        return SDB_DEVICE_ERROR;
    for (uint32_t r = 0; r < nruns; r++) {
        const uint64_t lb = std::min(h_lb[r], runs[r].n);
        sdb_run &x = out[r];
        x.n -= lb;
        x.key_off += lb;
        x.val_off += lb;
        x.val_len += lb;
        x.seq += lb;
        x.flags += lb;
        if (x.create_ts) x.create_ts += lb;
        if (x.expire_ts) x.expire_ts += lb;
    }
    return SDB_OK;
}

// The stream m from its row d on (the arenas are not offset: *_off index them).
void skip_rows(sdb_kv_batch &m, uint64_t d) {
    m.n -= d;
    m.key_off += d;
    m.val_off += d;
    m.kind += d;
    m.seq += d;
    m.create_ts += d;
    m.expire_ts += d;
    m.ts_mask += d;
}

// The retained stream as the filter reads it, in pinned memory: the columns, the key bytes, the value bytes (vb == 0:
// not gathered), and the decisions the callbacks write.
struct CfHost {
    uint8_t *kind, *ts_mask, *decision, *keys, *vals;
    uint64_t *seq, *key_off, *val_off;
    int64_t *create_ts, *expire_ts;
    uint64_t *mod_off;  // n + 1: the offsets of the replacements packed so far (in c->pin_cf_up)
};
uint64_t cf_host_bind(CfHost &h, uint64_t n, uint64_t kb, uint64_t vb, uint8_t *base) {
    Carver k{base, 0};
    k.take(h.key_off, n + 1);
    k.take(h.val_off, n + 1);
    k.take(h.seq, n);
    k.take(h.create_ts, n);
    k.take(h.expire_ts, n);
    k.take(h.kind, n);
    k.take(h.ts_mask, n);
    k.take(h.decision, n);
    k.take(h.mod_off, n + 1);
    k.take(h.keys, kb);
    k.take(h.vals, vb);
    return k.off;
}

// b grown to `need` bytes with its first `used` bytes kept (at least doubling: amortised over a job's replacements).
bool grow_keep(PinBuf &b, uint64_t used, uint64_t need) {
    if (b.p && need <= b.cap) return true;
    PinBuf nb;
    if (!nb.ensure(std::max(need, 2 * b.cap))) return false;
    if (used) memcpy(nb.p, b.p, used);
    b = std::move(nb);
    return true;
}

sdb_status filter_failed(sdb_compactor *c, sdb_status st, uint64_t at) {
    c->msum.status = st;
    c->msum.first_error_entry = at;
    return st;
}

// The filter and the drain over the retained stream m (its rows start at 0; kb / vb: its key and value bytes): m
// becomes the final stream, *bytes its key and value bytes.  With a filter: the gather [S], the callbacks, and, unless
// every row is kept (F7), the upload and the apply kernels into c->cf_ws.  A cursor without a filter: the drain
// count from the device [S].
sdb_status filter_step(const Job &j, sdb_kv_batch &m, uint64_t kb, uint64_t vb, uint64_t *bytes) {
    sdb_compactor *c = j.c;
    hipStream_t s = j.s;
    sdb_filter_stats &fs = c->fstats;
    const sdb_compaction_filter *f = j.filter;
    const sdb_resume_cursor *rc = j.resume;
    const uint64_t n = m.n;
    *bytes = kb + vb;
    if (!f) {  // S2 alone: the first row at which key == K && seq >= S fails
        if (!rc || !n) return SDB_OK;
        Carver k{nullptr, 0};
        const uint64_t o_key = k.bytes(rc->key_len + 1), o_d = k.bytes(8);
        if (!c->pin_seek.ensure(k.off) || !c->seek_ws.ensure(k.off)) return SDB_DEVICE_ERROR;
        if (rc->key_len) memcpy(c->pin_seek.at<uint8_t>(o_key), rc->key, rc->key_len);
        uint64_t *h_d = c->pin_seek.at<uint64_t>(o_d);
        if (hipMemcpyAsync(c->seek_ws.at<uint8_t>(o_key), c->pin_seek.at<uint8_t>(o_key), rc->key_len + 1, hipMemcpyHostToDevice, s) != hipSuccess ||
            launch_cf_drain(m, c->seek_ws.at<uint8_t>(o_key), (uint32_t)rc->key_len, rc->seq, c->seek_ws.at<uint64_t>(o_d), s) != hipSuccess ||
            hipMemcpyAsync(h_d, c->seek_ws.at<uint64_t>(o_d), 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return SDB_DEVICE_ERROR;
        fs.resume_drained = std::min(*h_d, n);
        skip_rows(m, fs.resume_drained);
        return SDB_OK;
    }

    // 1. the stream to the host: columns and key bytes, value bytes only when the filter wants them
    const uint64_t hv = f->want_values ? vb : 0;
    CfHost h{};
    if (!c->cf_ev.wait() || !c->pin_cf.ensure(cf_host_bind(h, n, kb, hv, nullptr))) return SDB_DEVICE_ERROR;
    cf_host_bind(h, n, kb, hv, c->pin_cf.at<uint8_t>(0));
    if (n) {
        auto back = [&](void *dst, const void *src, uint64_t b) {
            fs.d2h_bytes += b;
            return !b || hipMemcpyAsync(dst, src, b, hipMemcpyDeviceToHost, s) == hipSuccess;
        };
        if (!back(h.key_off, m.key_off, 8 * (n + 1)) || !back(h.val_off, m.val_off, 8 * (n + 1)) || !back(h.seq, m.seq, 8 * n) ||
            !back(h.create_ts, m.create_ts, 8 * n) || !back(h.expire_ts, m.expire_ts, 8 * n) || !back(h.kind, m.kind, n) ||
            !back(h.ts_mask, m.ts_mask, n) || !back(h.keys, m.key_bytes, kb) || !back(h.vals, m.val_bytes, hv) ||
            hipStreamSynchronize(s) != hipSuccess)
            return SDB_DEVICE_ERROR;
        memset(h.decision, SDB_CF_KEEP, n);
    }

    // 2. the callbacks (F8), the checks of what they returned (F9), the replacements packed in row order, the drain
    //    (S2) over the surviving rows as they come, and the final stream's exact sizes
    //    The replacements go straight into the pinned arena c->pin_cf_up, their offsets into h.mod_off.
    std::vector<const uint8_t *> &nv = c->cf_nv;  // (the handle's: no allocation in steady state)
    std::vector<uint64_t> &nl = c->cf_nl;
    uint64_t nm = 0, arena_bytes = 0;
    h.mod_off[0] = 0;
    bool draining = rc != nullptr, all_keep = true;
    uint64_t n_out = 0, kb_out = 0, vb_out = 0;
    const uint64_t step = f->batch_rows ? f->batch_rows : n;
    for (uint64_t first = 0; first < n; first += step) {
        const uint64_t cnt = std::min(step, n - first);
        sdb_kv_batch rows{};
        rows.n = cnt;
        rows.key_bytes = h.keys;
        rows.key_off = h.key_off + first;
        rows.val_bytes = f->want_values ? h.vals : nullptr;
        rows.val_off = h.val_off + first;
        rows.kind = h.kind + first;
        rows.seq = h.seq + first;
        rows.create_ts = h.create_ts + first;
        rows.expire_ts = h.expire_ts + first;
        rows.ts_mask = h.ts_mask + first;
        nv.assign(cnt, nullptr);
        nl.assign(cnt, 0);
        fs.calls++;
        fs.rows_in += cnt;
        if (f->filter(f->ctx, &rows, first, h.decision + first, nv.data(), nl.data()) != 0)
            return filter_failed(c, SDB_COMPACTION_FILTER_ERROR, first);
        for (uint64_t q = 0; q < cnt; q++) {
            const uint64_t i = first + q;
            const uint8_t d = h.decision[i];
            const bool mod = d == SDB_CF_VALUE || d == SDB_CF_MERGE;
            if (d > SDB_CF_MERGE || (mod && !nv[q] && nl[q])) return filter_failed(c, SDB_INVALID_ARGUMENT, i);
            if (mod && nl[q] > 0xFFFFFFFFull) return filter_failed(c, SDB_LIMIT_EXCEEDED, i);  // value lengths are u32
            (d == SDB_CF_KEEP ? fs.kept : d == SDB_CF_DROP ? fs.dropped : d == SDB_CF_TOMBSTONE ? fs.tombstoned
             : d == SDB_CF_VALUE ? fs.new_values : fs.new_merges)++;
            if (d != SDB_CF_KEEP) all_keep = false;
            if (d == SDB_CF_DROP) continue;
            const uint64_t kl = h.key_off[i + 1] - h.key_off[i];
            if (draining) {
                if (kl == rc->key_len && (!kl || !memcmp(h.keys + h.key_off[i], rc->key, kl)) && h.seq[i] >= rc->seq) {
                    fs.resume_drained++;
                    h.decision[i] = SDB_CF_DROP;  // (as the apply kernels take it; its replacement is not packed)
                    continue;
                }
                draining = false;
            }
            n_out++;
            kb_out += kl;
            if (mod) {
                if (!grow_keep(c->pin_cf_up, arena_bytes, arena_bytes + nl[q])) return SDB_DEVICE_ERROR;
                if (nl[q]) memcpy(c->pin_cf_up.at<uint8_t>(arena_bytes), nv[q], nl[q]);
                arena_bytes += nl[q];
                h.mod_off[++nm] = arena_bytes;
                vb_out += nl[q];
            } else if (d == SDB_CF_KEEP) {
                vb_out += h.val_off[i + 1] - h.val_off[i];
            }
        }
    }
    if (f->end && f->end(f->ctx) != 0) return filter_failed(c, SDB_COMPACTION_FILTER_ERROR, fs.rows_in);
    if (all_keep) {  // F7: the stream as it is, from the first row the drain left
        skip_rows(m, fs.resume_drained);
        return SDB_OK;
    }
    *bytes = kb_out + vb_out;
    if (!n_out) {
        m = sdb_kv_batch{};
        return SDB_OK;
    }

    // 3. the upload: the decisions, the replacements' offsets, their bytes
    CfArgs a{};
    if (!c->cf_ws.ensure(cf_bind(a, n, nm, arena_bytes, n_out, kb_out, vb_out, nullptr))) return SDB_DEVICE_ERROR;
    cf_bind(a, n, nm, arena_bytes, n_out, kb_out, vb_out, c->cf_ws.at<uint8_t>(0));
    a.in = m;
    auto up = [&](const void *dst, const void *src, uint64_t b) {
        fs.h2d_bytes += b;
        return !b || hipMemcpyAsync(const_cast<void *>(dst), src, b, hipMemcpyHostToDevice, s) == hipSuccess;
    };
    const bool sent = up(a.decision, h.decision, n) && up(a.mod_off, h.mod_off, 8 * (nm + 1)) &&
                      up(a.arena, c->pin_cf_up.p, arena_bytes);
    c->cf_ev.record(s);
    // 4. the apply kernels: the final stream in c->cf_ws
    if (!sent || launch_cf_apply(a, s) != hipSuccess) return SDB_DEVICE_ERROR;
    fs.applied = 1;
    m = batch_of(a.out, n_out);
    return SDB_OK;
}

// What follows the emit in a job with a filter or a cursor: filter_step over the retained stream m of exactly m.n
// rows, then (S3) the cuts over the final stream as it is and the output SSTs.
sdb_status filtered_tail(const Job &j, sdb_kv_batch m, uint64_t kb, uint64_t vb) {
    sdb_compactor *c = j.c;
    uint64_t bytes = 0;
    sdb_status st = filter_step(j, m, kb, vb, &bytes);
    if (st) return st;
    c->merged = m;
    if (!m.n) return hipStreamSynchronize(j.s) == hipSuccess ? SDB_OK : SDB_DEVICE_ERROR;
    CutRead rd;
    st = cut_step(j, m, nullptr, bytes, nullptr, rd);
    if (st) return st;
    return encode_outputs(j, rd, m.n);
}

}  // namespace

extern "C" {

sdb_compactor *sdb_compactor_create(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return nullptr;
    sdb_compactor *c = new sdb_compactor();
    c->device = device;
    return c;
}

void sdb_compactor_destroy(sdb_compactor *c) { delete c; }

}  // extern "C"

namespace {

// sdb_compactor_run (j.op == NULL) / sdb_compactor_run_merge
sdb_status run_job(const Job &j, const sdb_run *runs, uint32_t nruns) {
    sdb_status st = begin_job(j);
    if (st) return st;
    if (nruns && !runs) return SDB_INVALID_ARGUMENT;  // before group_runs reads runs[]
    sdb_compactor *c = j.c;
    if (hipSetDevice(c->device) != hipSuccess) return SDB_DEVICE_ERROR;
    hipStream_t s = j.s;
    std::vector<sdb_run> &seeked = c->seeked;  // (the handle's: no allocation in steady state)
    if (j.resume) {  // S1: every run from its first row with key >= K on (one synchronisation)
        if ((st = seek_runs(j, runs, nruns, seeked))) return st;
        runs = seeked.data();
    }
    uint64_t total = 0;
    for (uint32_t r = 0; r < nruns; r++) total += runs[r].n;

    // merge + retention, sized with unbounded byte capacities (synchronisation 1: the sizes), then emitted
    sdb_merged_out out{};
    st = merged_columns_in(c->cols, total, &out);
    if (st) return st;
    MergeArgs a;
    st = merge_front(j, runs, nruns, nullptr, out, a);
    if (st) return st;
    if (launch_merge_retention(a, false, s) != hipSuccess ||
        hipMemcpyAsync(&c->msum, out.summary, sizeof(sdb_merge_summary), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SDB_DEVICE_ERROR;
    if (c->msum.status) return (sdb_status)c->msum.status;
    if (!c->keys.ensure(c->msum.key_bytes + 16) || !c->vals.ensure(c->msum.val_bytes + 16)) return SDB_DEVICE_ERROR;
    a.out.key_bytes = c->keys.at<uint8_t>(0);
    a.out.key_cap = c->msum.key_bytes;
    a.out.val_bytes = c->vals.at<uint8_t>(0);
    a.out.val_cap = c->msum.val_bytes;
    if (launch_merge_emit(a, s) != hipSuccess) return SDB_DEVICE_ERROR;
    const uint64_t n = c->msum.num_out;
    if (j.filter || j.resume) return filtered_tail(j, batch_of(a.out, n), c->msum.key_bytes, c->msum.val_bytes);
    sdb_kv_batch &m = c->merged;
    m = batch_of(a.out, n);
    if (!n) return hipStreamSynchronize(s) == hipSuccess ? SDB_OK : SDB_DEVICE_ERROR;

    // the cuts of the stream as it is (synchronisation 2), the output SSTs (synchronisation 3)
    CutRead rd;
    st = cut_step(j, m, nullptr, c->msum.key_bytes + c->msum.val_bytes, nullptr, rd);
    if (st) return st;
    return encode_outputs(j, rd, n);
}

// The decode of a job's input blocks: its block list, the decoded columns and the gate word, in c->dec.
struct DecodeBufs {
    uint64_t *bstart, *bend;
    unsigned long long *gate;
    sdb_decoded_out out;
    const unsigned long long *err;  // the decode's error word, in c->dec_ws (set by decode_inputs)
};
// Takes the columns of E decoded entries and K key bytes: what a run over them reads (runs_over).
void take_columns(Carver &k, sdb_decoded_out &o, uint64_t K, uint64_t E) {
    o.key_arena_cap = K;
    o.cap_entries = E;
    k.take(o.key_arena, K + 64);
    k.take(o.key_off, E + 1);
    k.take(o.val_off, E + 1);
    k.take(o.val_len, E + 1);
    k.take(o.seq, E + 1);
    k.take(o.flags, E + 1);
    k.take(o.create_ts, E + 1);
    k.take(o.expire_ts, E + 1);
}
// Sizes (base == NULL) or binds them for B blocks of at most E entries and K key bytes.
uint64_t decode_bufs_bind(DecodeBufs &b, uint64_t B, uint64_t K, uint64_t E, uint8_t *base) {
    sdb_decoded_out &dout = b.out;
    dout = sdb_decoded_out{};
    dout.bad_cap = 16;
    Carver k{base, 0};
    k.take(b.bstart, B + 1);
    k.take(b.bend, B + 1);
    k.take(dout.block_entry_start, B + 2);
    take_columns(k, dout, K, E);
    k.take(dout.bad_block, dout.bad_cap);
    k.take(dout.summary, 1);
    k.take(b.gate, 1);
    return k.off;
}

// The decode step of the jobs over encoded inputs: the blocks `in` lists (launch_cx_blocks), decoded into one columnar
// output of at most E entries and K key bytes in c->dec (run r = its entries [run_entry[r], run_entry[r + 1])).
// Fail-fast (a failing block fails the job anyway, as load_iterators' reads would): checksums in the emit pass.  The
// job's gate kernel follows.
sdb_status decode_inputs(const Job &j, const CxInputs &in, uint64_t K, uint64_t E, uint16_t version, DecodeBufs &db) {
    sdb_compactor *c = j.c;
    const uint64_t B = in.nblocks;
    if (!c->dec.ensure(decode_bufs_bind(db, B, K, E, nullptr)) || !c->dec_ws.ensure(sdb_decode_workspace_bytes(B)))
        return SDB_DEVICE_ERROR;
    decode_bufs_bind(db, B, K, E, c->dec.at<uint8_t>(0));
    db.err = decode_err_word(c->dec_ws.p, B);
    if (launch_cx_blocks(in, db.bstart, db.bend, j.s) != hipSuccess) return SDB_DEVICE_ERROR;
    return sdb_decode_blocks_ex(reinterpret_cast<const uint8_t *>(in.base), db.bstart, db.bend, B, version,
                                SDB_DECODE_FAIL_FAST, &db.out, c->dec_ws.p, c->dec_ws.cap, j.stream);
}

// The runs of a job over decoded columns: run r = entries [run_entry[r], run_entry[r + 1]), values in `arena`.
std::vector<sdb_run> runs_over(const sdb_decoded_out &dout, const uint8_t *arena, const uint64_t *run_entry, uint32_t nruns) {
    std::vector<sdb_run> runs(nruns);
    for (uint32_t r = 0; r < nruns; r++)
        runs[r] = run_over(run_entry[r], run_entry[r + 1] - run_entry[r], dout.key_arena, dout.key_off, arena, dout.val_off,
                           dout.val_len, dout.seq, dout.flags, dout.create_ts, dout.expire_ts);
    return runs;
}

// What follows the decode in the jobs over encoded inputs: `runs` of E entries, K key bytes and at most V value
// bytes; gate: the decode's gate word on the device (NULL: the host has already read it).
sdb_status merge_encode(const Job &j, const std::vector<sdb_run> &runs, uint64_t E, uint64_t K, uint64_t V,
                        const unsigned long long *gate) {
    sdb_compactor *c = j.c;
    hipStream_t s = j.s;
    const bool op = j.op != nullptr;
    // merge + retention + emit into buffers of the declared sizes (retention only drops entries and values), gated
    // on the decode; the stream padded to E entries for the cut walk
    sdb_merged_out out{};
    sdb_status st = merged_columns_in(c->cols, E, &out);
    if (st) return st;
    if (!c->keys.ensure(K + 16) || (!op && !c->vals.ensure(V + 16))) return SDB_DEVICE_ERROR;
    out.key_bytes = c->keys.at<uint8_t>(0);
    out.key_cap = K;
    out.val_bytes = op ? nullptr : c->vals.at<uint8_t>(0);  // (with an operator: sized after the fold)
    out.val_cap = V;
    MergeArgs a;
    st = merge_front(j, runs.data(), (uint32_t)runs.size(), gate, out, a);
    if (st) return st;
    if (op) {
        // a merged value can be longer than all of its inputs: the links' bytes leave, the merged bytes come
        V = (V > c->mstats.link_bytes ? V - c->mstats.link_bytes : 0) + c->mstats.merged_bytes;
        if (!c->vals.ensure(V + 16)) return SDB_DEVICE_ERROR;
        a.out.val_bytes = out.val_bytes = c->vals.at<uint8_t>(0);
        a.out.val_cap = out.val_cap = V;
    }
    if (launch_merge_retention(a, true, s) != hipSuccess) return SDB_DEVICE_ERROR;
    if (j.filter || j.resume) {
        // the filter and the drain need the stream's exact length: the merged summary first (one synchronisation
        // more than the plain job), then the cuts over an unpadded stream
        if (hipMemcpyAsync(&c->msum, out.summary, sizeof(sdb_merge_summary), hipMemcpyDeviceToHost, s) != hipSuccess ||
            hipStreamSynchronize(s) != hipSuccess)
            return SDB_DEVICE_ERROR;
        if (c->msum.status) return (sdb_status)c->msum.status;
        return filtered_tail(j, batch_of(out, c->msum.num_out), c->msum.key_bytes, c->msum.val_bytes);
    }
    if (launch_merge_pad(out, E, s) != hipSuccess) return SDB_DEVICE_ERROR;
    // cuts over the padded stream, ending at the merged count; the merged summary rides along (one synchronisation)
    CutRead rd;
    st = cut_step(j, batch_of(out, E), &out.summary->num_out, K + V, out.summary, rd);
    if (st) return st;
    c->msum = *rd.sum;
    if (c->msum.status) return (sdb_status)c->msum.status;
    const uint64_t n = c->msum.num_out;
    c->merged = batch_of(out, n);
    if (!n) return SDB_OK;
    return encode_outputs(j, rd, n);  // (one synchronisation)
}

// What the jobs over encoded inputs check of their run shape, in this order: the inputs' SST version, the run count
// (*nruns = ninputs without run_start: every input a run of its own) against the two merge levels, run_start.
sdb_status check_run_shape(uint16_t input_sst_version, const uint32_t *run_start, uint32_t *nruns, uint32_t ninputs) {
    if (input_sst_version != 1 && input_sst_version != 2) return SDB_INVALID_VERSION;
    if (!run_start) *nruns = ninputs;
    if ((uint64_t)*nruns > (uint64_t)kMaxRuns * kMaxRuns) return SDB_LIMIT_EXCEEDED;
    if (run_start) {
        if (run_start[0] != 0 || run_start[*nruns] != ninputs) return SDB_INVALID_ARGUMENT;
        for (uint32_t r = 0; r < *nruns; r++)
            if (run_start[r + 1] < run_start[r]) return SDB_INVALID_ARGUMENT;
    }
    return SDB_OK;
}

// The per-input and per-run tables a job over encoded inputs hands its kernels (any number of inputs).  The job lists
// them once, in `tables(t)`, as t.take(host, dev, count): begin() runs the list to size them and again to bind every
// table's host pointer (in c->pin_tab, which the job then fills) and device pointer (the same offset of c->cx_tab,
// which the kernels read); send() uploads them in one copy.
struct TableUpload {
    sdb_compactor *c;
    hipStream_t s;
    Carver h{nullptr, 0}, d{nullptr, 0};
    bool sent = false;
    template <typename T>
    void take(T *&host, const T *&dev, uint64_t count) {
        h.take(host, count);
        d.take(dev, count);
    }
    template <typename F>
    bool begin(F tables) {
        tables(*this);
        // the previous job's upload and kernels may still read pin_tab / cx_tab (a job that failed early returns
        // without a synchronisation, and the caller may alternate streams)
        if (!c->tab_ev.wait() || !c->pin_tab.ensure(h.off) || !c->cx_tab.ensure(h.off)) return false;
        h = Carver{c->pin_tab.at<uint8_t>(0), 0};
        d = Carver{c->cx_tab.at<uint8_t>(0), 0};
        tables(*this);
        return true;
    }
    bool send() { return sent = hipMemcpyAsync(c->cx_tab.p, c->pin_tab.p, h.off, hipMemcpyHostToDevice, s) == hipSuccess; }
    // on every return of the job behind send(): everything the job enqueued precedes the event
    ~TableUpload() {
        if (sent) c->tab_ev.record(s);
    }
};

// sdb_compactor_run_ssts (j.op == NULL) / sdb_compactor_run_ssts_merge
sdb_status run_ssts_job(const Job &j, const sdb_compaction_input *inputs, uint32_t ninputs, const uint32_t *run_start,
                        uint32_t nruns, uint16_t input_sst_version) {
    sdb_status st = begin_job(j);
    if (st) return st;
    if (ninputs && !inputs) return SDB_INVALID_ARGUMENT;
    if ((st = check_run_shape(input_sst_version, run_start, &nruns, ninputs))) return st;
    sdb_compactor *c = j.c;
    if (hipSetDevice(c->device) != hipSuccess) return SDB_DEVICE_ERROR;

    // the inputs' blocks, in input order, as offsets from the lowest data address
    CxInputs in{};
    in.n = ninputs;
    in.nruns = nruns;
    const uint8_t **h_data;
    const uint64_t **h_boff;
    uint64_t *h_first, *h_rblk, *h_rent;
    TableUpload tab{c, j.s};
    if (!tab.begin([&](TableUpload &t) {
            t.take(h_data, in.data, ninputs);
            t.take(h_boff, in.block_off, ninputs);
            t.take(h_first, in.first_block, (uint64_t)ninputs + 1);
            t.take(h_rblk, in.run_block, (uint64_t)nruns + 1);
            t.take(h_rent, in.run_entry, (uint64_t)nruns + 1);
        }))
        return SDB_DEVICE_ERROR;
    uint64_t E = 0, K = 0, V = 0, B = 0;
    uintptr_t base = ~(uintptr_t)0;
    for (uint32_t i = 0; i < ninputs; i++) {
        const sdb_compaction_input &x = inputs[i];
        if (x.num_blocks && (!x.data || !x.block_off)) return SDB_INVALID_ARGUMENT;
        if (x.num_blocks && (uintptr_t)x.data < base) base = (uintptr_t)x.data;
        h_data[i] = x.data;
        h_boff[i] = x.block_off;
        h_first[i] = B;
        B += x.num_blocks;
        E += x.num_entries;
        K += x.key_bytes;
        V += x.val_bytes;
    }
    h_first[ninputs] = B;
    if (base == ~(uintptr_t)0) base = 0;
    in.base = base;
    in.nblocks = B;
    std::vector<uint64_t> run_entry(nruns + 1);
    {
        uint64_t e = 0;
        for (uint32_t r = 0; r < nruns; r++) {
            const uint32_t i0 = run_start ? run_start[r] : r, i1 = run_start ? run_start[r + 1] : r + 1;
            h_rblk[r] = h_first[i0];
            h_rent[r] = run_entry[r] = e;
            for (uint32_t i = i0; i < i1; i++) e += inputs[i].num_entries;
        }
        h_rblk[nruns] = B;
        h_rent[nruns] = run_entry[nruns] = e;
    }
    in.key_bytes = K;
    if (E >= (1ull << 31)) return SDB_LIMIT_EXCEEDED;
    if (!tab.send()) return SDB_DEVICE_ERROR;

    // decode every input block, gate the merge on the decode and the declared counts, merge and encode (the job's two
    // synchronisations are merge_encode's)
    DecodeBufs db;
    if ((st = decode_inputs(j, in, K, E, input_sst_version, db))) return st;
    if (launch_cx_gate(in, db.out.summary, db.err, db.out.block_entry_start, db.gate, j.s) != hipSuccess)
        return SDB_DEVICE_ERROR;
    const std::vector<sdb_run> runs = runs_over(db.out, reinterpret_cast<const uint8_t *>(base), run_entry.data(), nruns);
    return merge_encode(j, runs, E, K, V, db.gate);
}

bool ranges_null(const sdb_scan_ranges *g) {  // a NULL array inside a non-NULL struct
    return !g->start_bytes || !g->start_off || !g->start_kind || !g->end_bytes || !g->end_off || !g->end_kind;
}

// Sizes (base == NULL) or binds the columns of `rows` contributed rows and K key bytes.
uint64_t range_cols_bind(sdb_decoded_out &o, uint64_t rows, uint64_t K, uint8_t *base) {
    o = sdb_decoded_out{};
    Carver k{base, 0};
    take_columns(k, o, K, rows);
    return k.off;
}

// sdb_compactor_run_ssts_ranged.  The host arguments were checked by the entry point (R7).
sdb_status run_ranged_job(const Job &j, const sdb_compaction_view *inputs, uint32_t ninputs, const uint32_t *run_start,
                          uint32_t nruns, uint16_t input_sst_version, const sdb_scan_ranges *job,
                          const sdb_scan_ranges *proj) {
    sdb_status st = begin_job(j);
    if (st) return st;
    if ((st = check_run_shape(input_sst_version, run_start, &nruns, ninputs))) return st;
    sdb_compactor *c = j.c;
    if (hipSetDevice(c->device) != hipSuccess) return SDB_DEVICE_ERROR;
    hipStream_t s = j.s;
    const uint64_t n = ninputs;

    // the per-input and per-run tables the host knows
    RxInputs a{};
    a.n = ninputs;
    a.nruns = nruns;
    if (job) a.has_job = 1, a.job = *job;
    if (proj) a.has_proj = 1, a.proj = *proj;
    if (j.resume) a.has_resume = 1, a.resume_len = (uint32_t)j.resume->key_len;  // S1: a third start bound of every V[i]
    uint8_t *h_rkey;
    const uint8_t **h_data, **h_ikeys;
    const uint8_t *const *d_data;  // (read by the decode: CxInputs below)
    const uint64_t **h_ikoff, **h_boff;
    uint64_t *h_nblk, *h_gblk, *h_nent;
    uint32_t *h_rstart;
    TableUpload tab{c, s};
    if (!tab.begin([&](TableUpload &t) {
            t.take(h_data, d_data, n);
            t.take(h_ikeys, a.index_keys, n);
            t.take(h_ikoff, a.index_key_off, n);
            t.take(h_boff, a.block_off, n);
            t.take(h_nblk, a.num_blocks, n);
            t.take(h_gblk, a.gblock, n + 1);
            t.take(h_nent, a.num_entries, n);
            t.take(h_rstart, a.run_start, (uint64_t)nruns + 1);
            t.take(h_rkey, a.resume_key, (uint64_t)a.resume_len + 1);
        }))
        return SDB_DEVICE_ERROR;
    if (a.resume_len) memcpy(h_rkey, j.resume->key, a.resume_len);
    uint64_t B_all = 0, E_all = 0, K_all = 0;
    uintptr_t base = ~(uintptr_t)0;
    for (uint32_t i = 0; i < ninputs; i++) {
        const sdb_compaction_input &x = inputs[i].sst;
        if (x.num_blocks && (uintptr_t)x.data < base) base = (uintptr_t)x.data;
        h_data[i] = x.data;
        h_ikeys[i] = inputs[i].index_keys;
        h_ikoff[i] = inputs[i].index_key_off;
        h_boff[i] = x.block_off;
        h_nblk[i] = x.num_blocks;
        h_gblk[i] = B_all;
        h_nent[i] = x.num_entries;
        B_all += x.num_blocks;
        E_all += x.num_entries;
        K_all += x.key_bytes;
    }
    h_gblk[ninputs] = B_all;
    if (base == ~(uintptr_t)0) base = 0;
    for (uint32_t r = 0; r <= nruns; r++) h_rstart[r] = run_start ? run_start[r] : r;
    if (!tab.send()) return SDB_DEVICE_ERROR;
    // what the kernels write
    const uint64_t nres = kRxResult + (uint64_t)nruns + 1;
    auto bind_rx = [&](uint8_t *w) {
        Carver k{w, 0};
        k.take(a.cover, 2 * n + 1);
        k.take(a.cov_off, n);
        k.take(a.cov_first, n + 1);
        k.take(a.lo, n);
        k.take(a.hi, n);
        k.take(a.out_first, n + 1);
        k.take(a.out_key, n + 1);
        k.take(a.result, nres);
        k.take(a.clipped, n);
        return k.off;
    };
    if (!c->rx_ws.ensure(bind_rx(nullptr), c->canaries)) return SDB_DEVICE_ERROR;
    bind_rx(c->rx_ws.base());

    // 1. the view ranges and their covering blocks; synchronisation 1: the host sizes the decode from them
    if (!c->pin.ensure(8 * std::max(2 * n + 1, nres))) return SDB_DEVICE_ERROR;
    uint64_t *h_words = c->pin.at<uint64_t>(0);
    if (launch_rx_cover(a, s) != hipSuccess ||
        hipMemcpyAsync(h_words, a.cover, 8 * (2 * n + 1), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SDB_DEVICE_ERROR;
    sdb_range_job_stats &rs = c->rstats;
    rs.blocks_total = B_all;
    if (h_words[2 * n]) {  // R7: a malformed range
        c->msum.status = (int32_t)h_words[2 * n];
        c->msum.first_error_entry = ~0ull;
        return (sdb_status)c->msum.status;
    }
    uint64_t B = 0, E = 0, K = 0, V = 0;  // the covered blocks, and the declared counts of the inputs that have any
    for (uint32_t i = 0; i < ninputs; i++) {
        const uint64_t nb = h_words[2 * i + 1] - h_words[2 * i];
        if (!nb) continue;
        const sdb_compaction_input &x = inputs[i].sst;
        rs.inputs_read++;
        B += nb;
        E += x.num_entries;
        K += x.key_bytes;
        V += x.val_bytes;
    }
    rs.blocks_checked = B;
    if (E >= (1ull << 31)) return SDB_LIMIT_EXCEEDED;

    // 2. decode the covered blocks, clip their rows to the view ranges, gate; synchronisation 2: the row ranges
    CxInputs in{};
    in.n = ninputs;
    in.nruns = nruns;
    in.base = base;
    in.nblocks = B;
    in.data = d_data;
    in.block_off = a.cov_off;
    in.first_block = a.cov_first;
    DecodeBufs db;
    if ((st = decode_inputs(j, in, K, E, input_sst_version, db))) return st;
    if (launch_rx_clip_gate(a, db.out, db.err, E_all, K_all, s) != hipSuccess ||
        hipMemcpyAsync(h_words, a.result, 8 * nres, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
        return SDB_DEVICE_ERROR;
    const uint64_t gate = h_words[kRxGate], rows = h_words[kRxIn], key_bytes = h_words[kRxKeyBytes];
    rs.entries_decoded = h_words[kRxDecoded];
    rs.entries_in = rows;
    if (gate != ~0ull) {  // a failing covered block, or counts that disagree (R6): nothing is merged
        c->msum.num_in = E;
        c->msum.status = (int32_t)(gate & 0xFF);
        c->msum.first_error_entry = gate >> 8;
        return (sdb_status)c->msum.status;
    }
    const std::vector<uint64_t> run_entry(h_words + kRxResult, h_words + nres);  // (c->pin is reused below)
    const sdb_decoded_out *src = &db.out;
    sdb_decoded_out closed;
    if (rows != rs.entries_decoded) {  // a range dropped rows: the runs must not have gaps
        if (!c->rx_cols.ensure(range_cols_bind(closed, rows, key_bytes, nullptr), c->canaries)) return SDB_DEVICE_ERROR;
        range_cols_bind(closed, rows, key_bytes, c->rx_cols.base());
        if (launch_rx_compact(a, db.out, closed, rows, s) != hipSuccess) return SDB_DEVICE_ERROR;
        src = &closed;
    }
    const std::vector<sdb_run> runs = runs_over(*src, reinterpret_cast<const uint8_t *>(base), run_entry.data(), nruns);
    return merge_encode(j, runs, rows, key_bytes, V, nullptr);
}

}  // namespace

extern "C" {

sdb_status sdb_compactor_run(sdb_compactor *c, const sdb_run *runs, uint32_t nruns, const sdb_retention *ret,
                             const sdb_sst_params *params, uint64_t max_sst_size, void *stream, uint32_t *num_ssts) {
    return run_job(Job{c, ret, nullptr, nullptr, params, max_sst_size, stream, num_ssts}, runs, nruns);
}

sdb_status sdb_compactor_run_merge(sdb_compactor *c, const sdb_run *runs, uint32_t nruns, const sdb_retention *ret,
                                   sdb_merge_batch_fn op, void *ctx, const sdb_sst_params *params,
                                   uint64_t max_sst_size, void *stream, uint32_t *num_ssts) {
    if (!op) return SDB_INVALID_ARGUMENT;
    return run_job(Job{c, ret, op, ctx, params, max_sst_size, stream, num_ssts}, runs, nruns);
}

sdb_status sdb_compactor_run_ssts(sdb_compactor *c, const sdb_compaction_input *inputs, uint32_t ninputs,
                                  const uint32_t *run_start, uint32_t nruns, uint16_t input_sst_version,
                                  const sdb_retention *ret, const sdb_sst_params *params, uint64_t max_sst_size,
                                  void *stream, uint32_t *num_ssts) {
    return run_ssts_job(Job{c, ret, nullptr, nullptr, params, max_sst_size, stream, num_ssts}, inputs, ninputs, run_start,
                        nruns, input_sst_version);
}

sdb_status sdb_compactor_run_ssts_merge(sdb_compactor *c, const sdb_compaction_input *inputs, uint32_t ninputs,
                                        const uint32_t *run_start, uint32_t nruns, uint16_t input_sst_version,
                                        const sdb_retention *ret, sdb_merge_batch_fn op, void *ctx,
                                        const sdb_sst_params *params, uint64_t max_sst_size, void *stream,
                                        uint32_t *num_ssts) {
    if (!op) return SDB_INVALID_ARGUMENT;
    return run_ssts_job(Job{c, ret, op, ctx, params, max_sst_size, stream, num_ssts}, inputs, ninputs, run_start, nruns,
                        input_sst_version);
}

sdb_status sdb_compactor_run_filtered(sdb_compactor *c, const sdb_run *runs, uint32_t nruns, const sdb_retention *ret,
                                      sdb_merge_batch_fn op, void *op_ctx, const sdb_compaction_filter *filter,
                                      const sdb_resume_cursor *resume, const sdb_sst_params *params,
                                      uint64_t max_sst_size, void *stream, uint32_t *num_ssts) {
    Job j{c, ret, op, op_ctx, params, max_sst_size, stream, num_ssts};
    j.filter = filter;
    j.resume = resume;
    return run_job(j, runs, nruns);
}

sdb_status sdb_compactor_run_ssts_filtered(sdb_compactor *c, const sdb_compaction_view *inputs, uint32_t ninputs,
                                           const uint32_t *run_start, uint32_t nruns, uint16_t input_sst_version,
                                           const sdb_scan_ranges *job_range, const sdb_scan_ranges *proj,
                                           const sdb_retention *ret, sdb_merge_batch_fn op, void *ctx,
                                           const sdb_compaction_filter *filter, const sdb_resume_cursor *resume,
                                           const sdb_sst_params *params, uint64_t max_sst_size, void *stream,
                                           uint32_t *num_ssts) {
    // R7 and F9 on the host, before anything needs a device
    if (!ret || !params || !num_ssts || (ninputs && !inputs) || !filter_args_ok(filter, resume)) return SDB_INVALID_ARGUMENT;
    if (job_range && (job_range->n != 1 || ranges_null(job_range))) return SDB_INVALID_ARGUMENT;
    if (proj && (proj->n != ninputs || ranges_null(proj))) return SDB_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < ninputs; i++) {
        const sdb_compaction_view &x = inputs[i];
        if (x.sst.num_blocks && (!x.sst.data || !x.sst.block_off || !x.index_keys || !x.index_key_off))
            return SDB_INVALID_ARGUMENT;
    }
    if (!c) {  // (no handle exists without a device)
        int n = 0;
        return hipGetDeviceCount(&n) != hipSuccess || n == 0 ? SDB_DEVICE_ERROR : SDB_INVALID_ARGUMENT;
    }
    Job j{c, ret, op, ctx, params, max_sst_size, stream, num_ssts};
    j.filter = filter;
    j.resume = resume;
    return run_ranged_job(j, inputs, ninputs, run_start, nruns, input_sst_version, job_range, proj);
}

sdb_status sdb_compactor_run_ssts_ranged(sdb_compactor *c, const sdb_compaction_view *inputs, uint32_t ninputs,
                                         const uint32_t *run_start, uint32_t nruns, uint16_t input_sst_version,
                                         const sdb_scan_ranges *job_range, const sdb_scan_ranges *proj,
                                         const sdb_retention *ret, sdb_merge_batch_fn op, void *ctx,
                                         const sdb_sst_params *params, uint64_t max_sst_size, void *stream,
                                         uint32_t *num_ssts) {
    return sdb_compactor_run_ssts_filtered(c, inputs, ninputs, run_start, nruns, input_sst_version, job_range, proj, ret, op,
                                           ctx, nullptr, nullptr, params, max_sst_size, stream, num_ssts);
}

sdb_status sdb_compactor_filter_stats(const sdb_compactor *c, sdb_filter_stats *stats) {
    if (!c || !stats) return SDB_INVALID_ARGUMENT;
    *stats = c->fstats;
    return SDB_OK;
}

sdb_status sdb_compactor_range_stats(const sdb_compactor *c, sdb_range_job_stats *stats) {
    if (!c || !stats) return SDB_INVALID_ARGUMENT;
    *stats = c->rstats;
    return SDB_OK;
}

sdb_status sdb_compactor_merge_stats(const sdb_compactor *c, sdb_merge_op_stats *stats) {
    if (!c || !stats) return SDB_INVALID_ARGUMENT;
    *stats = c->mstats;
    return SDB_OK;
}

// Diagnostics (not in the header): guard bands around the buffers of the merge-operator step and of the ranged
// job's input side (GuardBuf), and
// the guard bytes the last job changed (synchronises the device; -1: the check could not run).
void sdb_diag_compactor_canaries(sdb_compactor *c, int on) {
    if (c) c->canaries = on != 0;
}
int64_t sdb_diag_compactor_canary_damage(sdb_compactor *c) {
    if (!c || hipSetDevice(c->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -1;
    int64_t sum = 0;
    for (const GuardBuf *b : {&c->chain_ws, &c->chain_tab, &c->chain_up, &c->rx_ws, &c->rx_cols}) {
        const int64_t x = b->damaged();
        if (x < 0) return -1;
        sum += x;
    }
    return sum;
}

sdb_status sdb_compactor_sst(const sdb_compactor *c, uint32_t i, sdb_compacted_sst *out) {
    if (!c || !out || i >= c->ssts.size()) return SDB_INVALID_ARGUMENT;
    *out = c->ssts[i];
    return SDB_OK;
}

sdb_status sdb_compactor_merged(const sdb_compactor *c, sdb_kv_batch *batch, sdb_merge_summary *summary) {
    if (!c) return SDB_INVALID_ARGUMENT;
    if (batch) *batch = c->merged;
    if (summary) *summary = c->msum;
    return SDB_OK;
}

}  // extern "C"
