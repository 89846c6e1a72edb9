// sdb_host.h — what the host-buffer handles (sdb_host.cpp, sdb_compactor.cpp) share: the growing device and
// pinned buffers, and the layout of one SST's outputs inside them.  Handle buffers follow the workspace rule
// (sdb_workspace.h): a Carver takes their arrays in order, with a NULL base for the offsets and the size.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slatedb_amd.h"
#include "sdb_workspace.h"

namespace sdb {

inline hipError_t dev_alloc(void **p, uint64_t bytes) { return hipMalloc(p, bytes); }
inline void dev_free(void *p) { (void)hipFree(p); }
inline hipError_t pin_alloc(void **p, uint64_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
inline void pin_free(void *p) { (void)hipHostFree(p); }

// A buffer that only grows, owned by a handle: move-only, freed with its owner.  After ensure(bytes) returned
// true, p != NULL (0 bytes too) and cap >= bytes; growing drops the contents.
template <hipError_t (*Alloc)(void **, uint64_t), void (*Free)(void *)>
struct GrowBuf {
    void *p = nullptr;
    uint64_t cap = 0;
    GrowBuf() = default;
    GrowBuf(const GrowBuf &) = delete;
    GrowBuf &operator=(const GrowBuf &) = delete;
    GrowBuf(GrowBuf &&o) noexcept { *this = static_cast<GrowBuf &&>(o); }
    GrowBuf &operator=(GrowBuf &&o) noexcept {
        if (this != &o) {
            release();
            p = o.p;
            cap = o.cap;
            o.p = nullptr;
            o.cap = 0;
        }
        return *this;
    }
    ~GrowBuf() { release(); }
    bool ensure(uint64_t bytes) {
        if (p && bytes <= cap) return true;
        release();
        const uint64_t want = bytes + bytes / 4 + 256;
        if (Alloc(&p, want) != hipSuccess) {
            p = nullptr;
            return false;
        }
        cap = want;
        return true;
    }
    void release() {
        if (p) Free(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T>
    T *at(uint64_t off) const {
        return reinterpret_cast<T *>(static_cast<uint8_t *>(p) + off);
    }
};
struct DevBuf : GrowBuf<dev_alloc, dev_free> {};  // device memory
struct PinBuf : GrowBuf<pin_alloc, pin_free> {};  // pinned host staging (async copies)

// Byte offsets of one SST's output arrays in a buffer (and in its host mirror).
struct SstLayout {
    uint64_t block_off, block_first, index_key_len, block_stats;  // o.block_cap + 1 elements each
    uint64_t data, bloom, summary;                                // whole SSTs only
};

// Takes o's per-block arrays (and, `whole`, its data, bloom and summary around them) from c, by the capacities o
// holds, and binds them: NULL with a NULL base, which leaves the offsets and, in c.off, the size.
inline SstLayout bind_sst_out(Carver &c, sdb_sst_out &o, bool whole) {
    const uint64_t nb = o.block_cap + 1;
    SstLayout l{};
    auto take = [&](uint64_t &at, auto *&p, uint64_t count) {
        at = c.off;
        c.take(p, count);
    };
    if (whole) take(l.data, o.data, o.data_cap);
    take(l.block_off, o.block_off, nb);
    take(l.block_first, o.block_first_entry, nb);
    take(l.index_key_len, o.index_key_len, nb);
    take(l.block_stats, o.block_stats, 3 * nb);
    if (whole) {
        take(l.bloom, o.bloom, o.bloom_cap);
        take(l.summary, o.summary, 1);
    }
    return l;
}

// The used parts of a whole SST at dev (nothing of a failed one) to the same offsets at host, on s.
inline void copy_sst_back(uint8_t *host, const uint8_t *dev, const SstLayout &l, const sdb_sst_summary &sm,
                          hipStream_t s) {
    if (sm.status != SDB_OK) return;
    const uint64_t nb = sm.num_blocks;
    auto back = [&](uint64_t at, uint64_t bytes) { hipMemcpyAsync(host + at, dev + at, bytes, hipMemcpyDeviceToHost, s); };
    back(l.data, sm.data_len);
    back(l.block_off, 8 * (nb + 1));
    back(l.block_first, 4 * (nb + 1));
    back(l.index_key_len, 4 * nb);
    back(l.block_stats, 6 * nb);
    if (sm.bloom_len) back(l.bloom, sm.bloom_len);
}

// r = the SST at host (copy_sst_back's destination), no timings.
inline void fill_result(sdb_sst_host_result &r, const uint8_t *host, const SstLayout &l, const sdb_sst_summary &sm) {
    r.summary = sm;
    r.data = host + l.data;
    r.block_off = (const uint64_t *)(host + l.block_off);
    r.block_first_entry = (const uint32_t *)(host + l.block_first);
    r.index_key_len = (const uint32_t *)(host + l.index_key_len);
    r.block_stats = (const uint16_t *)(host + l.block_stats);
    r.bloom = host + l.bloom;
    r.h2d_ms = r.kernel_ms = r.d2h_ms = 0;
}

}  // namespace sdb
