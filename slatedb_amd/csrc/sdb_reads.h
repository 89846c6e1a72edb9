// sdb_reads.h — the host entry points of the read path: per family (sdb_lookup.hip, sdb_scan.hip, sdb_get.hip,
// sdb_lsm_scan.hip) the workspace sizer and the launcher, declared once for the file that defines them and for
// sdb_api.cpp, which calls them after the argument checks.  The sizes are without the 256 bytes the public
// sdb_*_workspace_bytes functions add for the round-up of the caller's pointer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slatedb_amd.h"

namespace sdb {

uint64_t lookup_workspace_bytes(uint64_t num_blocks, uint64_t nkeys);
hipError_t launch_lookup(const sdb_sst_view &v, const uint8_t *key_bytes, const uint64_t *key_off, uint64_t nkeys,
                         uint32_t desc, const sdb_lookup_out &out, uint8_t *w, hipStream_t st);

uint64_t scan_workspace_bytes(uint64_t num_blocks, uint64_t nranges);
hipError_t launch_scan(const sdb_sst_view &v, const sdb_scan_ranges &r, uint32_t desc, const sdb_scan_out &out, uint8_t *w,
                       hipStream_t st);

// ---- the tree reads: sdb_lsm_get* (sdb_get.hip) and sdb_lsm_scan* (sdb_lsm_scan.hip) ----
// One call descriptor per family: exactly what its widest entry point (sdb_lsm_*_mem) receives, in that order.  A
// lesser entry point leaves what it lacks NULL, and a NULL selects nothing by itself but what its comment says; what
// the NULLs cannot say is a flag.  sdb_api.cpp fills and checks a descriptor, the launcher reads it.

// What a tree-read workspace is sized by.
struct ReadShape {
    uint32_t num_tables;                   // sdb_lsm_*_mem: the memtables; 0 sizes exactly the call without them
    uint64_t total_blocks;
    uint32_t num_ssts, num_runs;           // (a scan's workspace does not depend on the runs)
    uint64_t n;                            // keys or ranges
    uint64_t cand_entries, cand_key_bytes; // scans: the staging room
    bool merge;                            // the call has a chain
    bool filter;                           // scans: the entry point consults the filters (ScanCall::filter)
    bool recency;                          // scans: sdb_lsm_scan_recency (ScanCall::recency; then filter, no merge)
};

struct GetCall {
    const sdb_mem_view *mem;          // the memtables searched ahead of the tree; NULL or num_tables == 0: none
    const sdb_lsm_view *lsm;
    const sdb_scan_ranges *proj;      // sdb_lsm_get_projected: a visible range per SST; NULL: no SST is projected
    const sdb_filter_policy *pol;     // sdb_lsm_get_filtered: a policy per SST; NULL: the plain whole-key policy
    const uint8_t *key_bytes;
    const uint64_t *key_off;
    uint64_t nkeys;
    const int32_t *probe_len;         // sdb_lsm_get_filtered: per query, for SDB_PREFIX_LENGTHS SSTs; may be NULL
    const uint64_t *max_seq;          // may be NULL: no bound
    const sdb_get_out *out;
    const sdb_mem_get_out *mout;      // iff layers
    const sdb_chain_out *chain;       // the merging get; NULL: the plain one
    const sdb_mem_chain_out *mchain;  // iff layers and chain
    bool merge;                       // operand chains are merged: chain must be there (sdb_lsm_*_merge always, the wider
                                      // entry points iff they got a chain)
    bool layers;                      // the entry point is sdb_lsm_get_mem: mout (and mchain) are filled even when
                                      // mem holds no table (M6)
};
uint64_t get_workspace_bytes(const ReadShape &s);
hipError_t launch_get(const GetCall &c, uint8_t *w, hipStream_t st);

struct ScanCall {
    const sdb_mem_view *mem;          // the memtables merged ahead of the tree; NULL or num_tables == 0: none
    const sdb_lsm_view *lsm;
    const sdb_scan_ranges *proj;      // sdb_lsm_scan_projected: a visible range per SST; NULL: no SST is projected
    const sdb_filter_policy *pol;     // with filter: a policy per SST; NULL: the plain whole-key policy
    const sdb_scan_ranges *ranges;
    const sdb_scan_prefixes *prefixes;  // with filter: NULL: no range has a prefix
    const uint64_t *max_seq;          // may be NULL: no bound
    uint32_t desc;                    // 1: descending
    uint64_t cand_entries, cand_key_bytes;
    const sdb_lsm_scan_out *out;
    const sdb_mem_scan_out *mout;     // iff layers
    const sdb_chain_out *chain;       // the merging scan; NULL: the plain one
    const sdb_mem_chain_out *mchain;  // iff layers and chain
    const sdb_scan_filter_out *fout;  // iff filter
    bool merge;                       // operand chains are merged: chain must be there (sdb_lsm_*_merge always, the wider
                                      // entry points iff they got a chain)
    bool filter;                      // the entry point is sdb_lsm_scan_filtered or wider: the filters are consulted
                                      // and fout is written
    bool layers;                      // the entry point is sdb_lsm_scan_mem: mout (and mchain) are filled even when
                                      // mem holds no table (S7)
    bool recency;                     // the entry point is sdb_lsm_scan_recency (then filter and layers, no chain): the
                                      // sources are drained one after another instead of merged
    const uint64_t *limit;            // iff recency; may be NULL: every source is drained
    const sdb_recency_out *rout;      // iff recency
};
uint64_t lsm_scan_workspace_bytes(const ReadShape &s);
hipError_t launch_lsm_scan(const ScanCall &c, uint8_t *w, hipStream_t st);

}  // namespace sdb
