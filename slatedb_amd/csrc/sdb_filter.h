// sdb_filter.h — Filter::might_match (filter.rs:150-175) on the device: what a FilterQuery probes in an SST's "_bf"
// filter under that SST's policy, and the probe itself.  Shared by k_bloom_match (sdb_bloom.hip), the tree gets
// (sdb_get.hip) and the tree scans (sdb_lsm_scan.hip); the builders of sdb_bloom.hip extract with the same pf_len.
#pragma once
#include <stdint.h>

#include "../../include/slatedb_amd.h"
#include "sdb_bloom.h"

namespace sdb {

struct PrefixSpec {
    uint32_t kind, arg, whole, pad;
    const int32_t *lens;  // SDB_PREFIX_LENGTHS: the extractor's answer per key (build) or per query (match)
};

// PrefixExtractor::prefix_len of key i = k[0, kl): -1 = None.
SDB_DEV int64_t pf_len(const PrefixSpec &ps, const uint8_t *k, uint32_t kl, uint64_t i) {
    if (ps.kind == SDB_PREFIX_FIXED) return kl >= ps.arg ? (int64_t)ps.arg : -1;
    if (ps.kind == SDB_PREFIX_DELIM) {
        for (uint32_t x = 0; x < kl; x++)
            if (k[x] == (uint8_t)ps.arg) return (int64_t)x + 1;
        return -1;
    }
    if (ps.kind == SDB_PREFIX_LENGTHS) return ps.lens ? (int64_t)ps.lens[i] : -1;
    return -1;
}

// How many bytes of target i = t[0, n) the query probes (filter.rs:150-175): a Point under whole-key filtering
// the full key, anything else the extracted prefix; -1 = None, nothing to probe, the filter answers "might match".
// A length the extractor gives beyond the target counts as None, so no probe reads past it.
SDB_DEV int64_t filter_probe_len(const PrefixSpec &ps, bool is_prefix, const uint8_t *t, uint32_t n, uint64_t i) {
    if (ps.kind > SDB_PREFIX_LENGTHS) return -1;  // no such extractor: the tree reads fail the SST instead
    if (!is_prefix && ps.whole) return n;
    if (ps.kind == SDB_PREFIX_NONE) return -1;
    const int64_t len = pf_len(ps, t, n, i);
    return len > (int64_t)n ? -1 : len;
}

// What a query probes: len < 0: nothing, else the filter hash h (filter_hash, filter.rs:196-204) of the target's
// first len bytes.
struct Probe {
    int64_t len;
    uint64_t h;
};
SDB_DEV Probe filter_probe(const PrefixSpec &ps, bool is_prefix, const uint8_t *t, uint32_t n, uint64_t i) {
    const int64_t len = filter_probe_len(ps, is_prefix, t, n, i);
    return Probe{len, len >= 0 ? siphash13(t, (uint64_t)len) : 0};
}

// might_contain (filter.rs:124-136) for the filter hash h; an empty bitmap answers false.
SDB_DEV bool bloom_might_contain(const uint8_t *bloom, uint64_t bloom_len, uint32_t num_probes, uint64_t h) {
    const uint32_t m = (uint32_t)(bloom_len * 8);
    if (!m) return false;
    uint32_t hh = (uint32_t)h % m, d = (uint32_t)(h >> 32) % m;
    for (uint32_t i = 0; i < num_probes; i++) {
        d = (uint32_t)(((uint64_t)d + i) % m);
        if (!((bloom[hh >> 3] >> (hh & 7)) & 1)) return false;
        hh = (uint32_t)(((uint64_t)hh + d) % m);
    }
    return true;
}

// Filter::might_match once the probe length is known: None answers true, else might_contain of the hash h of the
// probe bytes (filter_hash, filter.rs:196-204).
SDB_DEV bool filter_might_match(const uint8_t *bloom, uint64_t bloom_len, uint32_t num_probes, int64_t len, uint64_t h) {
    return len < 0 || bloom_might_contain(bloom, bloom_len, num_probes, h);
}

// The policy of SST i of a tree read: policies == NULL is the plain whole-key policy.
SDB_DEV PrefixSpec policy_spec(const sdb_filter_policy *pol, uint32_t i, const int32_t *lens) {
    if (!pol) return PrefixSpec{SDB_PREFIX_NONE, 0, 1, 0, lens};
    const sdb_filter_policy p = pol[i];
    return PrefixSpec{p.prefix_kind, p.prefix_arg, p.no_whole_key ? 0u : 1u, 0, lens};
}

// One workgroup (every thread calls it): the policies of a tree's SSTs agree, so a query's probe bytes and their
// hash are the same for every SST.  A prefix_kind above SDB_PREFIX_LENGTHS makes SST i unusable: sstat[i] becomes
// SDB_INVALID_ARGUMENT, and filter_probe_len gives it no probe, so its filter rules nothing out before that shows.
SDB_DEV int policies_validate(const sdb_filter_policy *pol, uint32_t ns, int32_t *sstat) {
    int differ = 0;
    if (pol) {
        const sdb_filter_policy p0 = pol[0];
        for (uint32_t i = threadIdx.x; i < ns; i += blockDim.x) {
            const sdb_filter_policy p = pol[i];
            if (p.prefix_kind != p0.prefix_kind || p.prefix_arg != p0.prefix_arg || !p.no_whole_key != !p0.no_whole_key) differ = 1;
            if (p.prefix_kind > SDB_PREFIX_LENGTHS) sstat[i] = SDB_INVALID_ARGUMENT;
        }
    }
    return !__syncthreads_or(differ);
}

}  // namespace sdb
