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

// chain != NULL: the merging get (sdb_lsm_get_merge); pol / probe_len: sdb_lsm_get_filtered's, else NULL; proj:
// sdb_lsm_get_projected's, else NULL
uint64_t get_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs, uint64_t nkeys, bool merge);
hipError_t launch_get(const sdb_lsm_view &t, const sdb_filter_policy *pol, const uint8_t *key_bytes, const uint64_t *key_off,
                      uint64_t nkeys, const int32_t *probe_len, const uint64_t *max_seq, const sdb_get_out &out,
                      const sdb_chain_out *chain, const sdb_scan_ranges *proj, uint8_t *w, hipStream_t st);

// sdb_lsm_get_mem: launch_get with the memtables `mem` (NULL or num_tables == 0: none) searched ahead of the tree;
// mchain iff chain.  num_tables == 0 sizes exactly get_workspace_bytes.
uint64_t get_mem_workspace_bytes(uint32_t num_tables, uint64_t total_blocks, uint32_t num_ssts, uint32_t num_runs,
                                 uint64_t nkeys, bool merge);
hipError_t launch_get_mem(const sdb_mem_view *mem, const sdb_lsm_view &t, const sdb_filter_policy *pol, const uint8_t *key_bytes,
                          const uint64_t *key_off, uint64_t nkeys, const int32_t *probe_len, const uint64_t *max_seq,
                          const sdb_get_out &out, const sdb_mem_get_out &mout, const sdb_chain_out *chain,
                          const sdb_mem_chain_out *mchain, const sdb_scan_ranges *proj, uint8_t *w, hipStream_t st);

// chain != NULL: the merging scan; fout != NULL: the filtered one, with pol and px; proj != NULL (with fout): the
// projected one
uint64_t lsm_scan_workspace_bytes(uint64_t total_blocks, uint32_t num_ssts, uint64_t nranges, uint64_t cand_entries,
                                  uint64_t cand_key_bytes, bool merge, bool filter);
hipError_t launch_lsm_scan(const sdb_lsm_view &t, const sdb_scan_ranges &r, const uint64_t *max_seq, uint32_t desc,
                           uint64_t cand_entries, uint64_t cand_key_bytes, const sdb_lsm_scan_out &out,
                           const sdb_chain_out *chain, const sdb_filter_policy *pol, const sdb_scan_prefixes *px,
                           const sdb_scan_filter_out *fout, const sdb_scan_ranges *proj, uint8_t *w, hipStream_t st);

// sdb_lsm_scan_mem: the projected launch_lsm_scan with the memtables `mem` (NULL or num_tables == 0: none) merged
// ahead of the tree; mchain iff chain.  num_tables == 0 sizes exactly lsm_scan_workspace_bytes(..., filter = true).
uint64_t lsm_scan_mem_workspace_bytes(uint32_t num_tables, uint64_t total_blocks, uint32_t num_ssts, uint64_t nranges,
                                      uint64_t cand_entries, uint64_t cand_key_bytes, bool merge);
hipError_t launch_lsm_scan_mem(const sdb_mem_view *mem, const sdb_lsm_view &t, const sdb_scan_ranges &r,
                               const uint64_t *max_seq, uint32_t desc, uint64_t cand_entries, uint64_t cand_key_bytes,
                               const sdb_lsm_scan_out &out, const sdb_mem_scan_out &mout, const sdb_chain_out *chain,
                               const sdb_mem_chain_out *mchain, const sdb_filter_policy *pol, const sdb_scan_prefixes *px,
                               const sdb_scan_filter_out &fout, const sdb_scan_ranges *proj, uint8_t *w, hipStream_t st);

}  // namespace sdb
