// sdb_workspace.h — how every launch sizes and binds its device workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdb {

// 256-byte-aligned arrays taken in order from base.  One function that takes a launch's arrays both sizes its
// workspace (base == nullptr: nothing is bound, `off` ends as the size) and binds it, so the two cannot disagree.
struct Carver {
    uint8_t *base;
    uint64_t off;
    __host__ __device__ uint64_t bytes(uint64_t n) {  // the offset of the next n bytes
        const uint64_t at = off;
        off += (n + 255) & ~255ull;
        return at;
    }
    template <typename T>
    __host__ __device__ void take(T *&p, uint64_t count) {
        p = base ? (T *)(base + off) : nullptr;
        bytes(sizeof(T) * count);
    }
};

// The caller's workspace pointer rounded up to the arrays' alignment (NULL stays NULL).  The + 256 of the public
// sdb_*_workspace_bytes functions pays for it.
inline uint8_t *ws_align(void *workspace) { return (uint8_t *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255); }

}  // namespace sdb
