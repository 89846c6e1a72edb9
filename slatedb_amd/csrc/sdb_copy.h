// sdb_copy.h — wave-cooperative copies of many short byte ranges (keys and values) at any alignment: the
// chunk copies k_mg_emit, k_mg_chain_emit (sdb_compact.hip) and k_rp_gather (sdb_replay.hip) move their bytes with.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdb_device.h"

namespace sdb {
namespace {

// Unaligned vector / scalar accesses for byte ranges at any alignment (unaligned global access is
// enabled on gfx9).
typedef uint32_t u32x4_u __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t u32x2_u __attribute__((ext_vector_type(2), aligned(1)));
typedef uint32_t u32_u __attribute__((aligned(1)));

// Key / value copies of the merge emit and of the replay gather: the entries' descriptors sit in LDS and a wave copies 64 of them
// at a time, eight lanes per entry and 16 bytes per lane per step, so a load instruction reads eight
// contiguous 128-byte spans (a thread copying its own entries, one load in flight, ran at 0.7 TB/s).
struct CopyDesc {
    const uint8_t *ks, *vs;
    uint8_t *kd, *vd;
    uint32_t kb, vb;
};
// <= 16 bytes as independent loads (16, or 8 / 4 / 2 / 1 pieces: never past the range), so a lane's
// chunks of several entries are all in flight before the first store waits
struct Chunk {  // (its length is recomputed at the store from the descriptor: fewer live registers)
    uint64_t lo, hi;
};
typedef uint16_t u16_u __attribute__((aligned(1)));
typedef uint64_t u64_u __attribute__((aligned(1)));
SDB_DEV void chunk_load(Chunk &c, const uint8_t *src, uint32_t n) {
    if (n >= 16) {  // one 16-byte access
        const u32x4_u v = *(const u32x4_u *)src;
        c.lo = (uint64_t)v.x | ((uint64_t)v.y << 32);
        c.hi = (uint64_t)v.z | ((uint64_t)v.w << 32);
        return;
    }
    const uint32_t o = n & 8, b4 = n & 4, b2 = n & 2;
    c.lo = o ? *(const u64_u *)src : 0;
    uint64_t t = 0;
    if (b4) t = *(const u32_u *)(src + o);
    if (b2) t |= (uint64_t)*(const u16_u *)(src + o + b4) << (8 * b4);
    if (n & 1) t |= (uint64_t)src[o + b4 + b2] << (8 * (b4 + b2));
    if (o) c.hi = t;
    else c.lo = t;
}
// The unconditional form of a lane chunk (a load under a branch makes the compiler wait for every earlier
// load at the join, so the chunks of eight entries went out one at a time): a range of >= 16 bytes reads
// the 16 bytes at x, or for its tail the 16 ending at its end (shifted down at the store); a lane with no
// chunk, or a range under 16 bytes, reads g_safe16 and (the latter) copies piecewise afterwards.
static __device__ uint4 g_safe16;
SDB_DEV const uint8_t *chunk_src(const uint8_t *src, uint32_t len, uint32_t x) {
    const bool live = x < len && len >= 16;
    return live ? src + (x + 16 <= len ? x : len - 16) : (const uint8_t *)&g_safe16;
}
// global (not flat) accesses: a flat access also counts on lgkmcnt, so every LDS descriptor read after the
// stores waited for all of them
typedef __attribute__((address_space(1))) u32x4_u g_u32x4_u;
typedef __attribute__((address_space(1))) u64_u g_u64_u;
typedef __attribute__((address_space(1))) u32_u g_u32_u;
typedef __attribute__((address_space(1))) u16_u g_u16_u;
typedef __attribute__((address_space(1))) uint8_t g_u8;
SDB_DEV u32x4_u chunk_ld(const uint8_t *p) { return *(const g_u32x4_u *)(uintptr_t)p; }
// (the destination of every copy is global memory)
SDB_DEV void chunk_store(const Chunk &c, uint8_t *dst0, uint32_t n) {
    const uintptr_t dst = (uintptr_t)dst0;
    if (n >= 16) {
        u32x4_u v;
        v.x = (uint32_t)c.lo, v.y = (uint32_t)(c.lo >> 32), v.z = (uint32_t)c.hi, v.w = (uint32_t)(c.hi >> 32);
        *(g_u32x4_u *)dst = v;
        return;
    }
    const uint32_t o = n & 8, b4 = n & 4, b2 = n & 2;
    if (o) *(g_u64_u *)dst = c.lo;
    const uint64_t t = o ? c.hi : c.lo;
    if (b4) *(g_u32_u *)(dst + o) = (uint32_t)t;
    if (b2) *(g_u16_u *)(dst + o + b4) = (uint16_t)(t >> (8 * b4));
    if (n & 1) *(g_u8 *)(dst + o + b4 + b2) = (uint8_t)(t >> (8 * (b4 + b2)));
}
// store bytes [x, min(len, x + 16)) of the range from the chunk_src window w
SDB_DEV void chunk_put(const u32x4_u &w, const uint8_t *src, uint8_t *dst, uint32_t len, uint32_t x) {
    if (x >= len) return;
    const uint32_t n = len - x < 16 ? len - x : 16;
    if (len < 16) {  // a short range: exact pieces (rare for keys and values)
        Chunk c;
        chunk_load(c, src + x, n);
        chunk_store(c, dst + x, n);
        return;
    }
    uint64_t lo = (uint64_t)w.x | ((uint64_t)w.y << 32), hi = (uint64_t)w.z | ((uint64_t)w.w << 32);
    const uint32_t sh = 16 - n;  // bytes of the window before x (a tail window ends at len)
    if (sh >= 8) {
        lo = hi >> (8 * (sh - 8));
        hi = 0;
    } else if (sh) {
        lo = (lo >> (8 * sh)) | (hi << (64 - 8 * sh));
        hi >>= 8 * sh;
    }
    Chunk c;
    c.lo = lo;
    c.hi = hi;
    chunk_store(c, dst + x, n);
}
// lane chunk x of every listed entry's key and value bytes: all sixteen loads, then the stores
SDB_DEV void copy_group_chunks_kv(const CopyDesc *cd, uint32_t l, uint32_t x) {
    u32x4_u ck[8], cv[8];
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) {
        const CopyDesc &c = cd[8 * q + (l >> 3)];
        ck[q] = chunk_ld(chunk_src(c.ks, c.kb, x));
        cv[q] = chunk_ld(chunk_src(c.vs, c.vb, x));
    }
    asm volatile("" ::: "memory");  // re-read the descriptors from LDS rather than hold 8 of them
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) {
        const CopyDesc &c = cd[8 * q + (l >> 3)];
        chunk_put(ck[q], c.ks, c.kd, c.kb, x);
        chunk_put(cv[q], c.vs, c.vd, c.vb, x);
    }
}
// lane chunk x of every listed entry's key (K) or value bytes: all eight loads, then the stores
template <bool K>
SDB_DEV void copy_group_chunks(const CopyDesc *cd, uint32_t l, uint32_t x) {
    u32x4_u ch[8];
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) {
        const CopyDesc &c = cd[8 * q + (l >> 3)];
        ch[q] = chunk_ld(chunk_src(K ? c.ks : c.vs, K ? c.kb : c.vb, x));
    }
    asm volatile("" ::: "memory");
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) {
        const CopyDesc &c = cd[8 * q + (l >> 3)];
        chunk_put(ch[q], K ? c.ks : c.vs, K ? c.kd : c.vd, K ? c.kb : c.vb, x);
    }
}

// One wave's 64 ranges cd[0 .. 64) (lane l), keys and values, for k_rp_gather: lanes 8q' .. 8q' + 7 copy entry
// 8q + q' of these 64; lane l's 16-byte chunks start at 16 (l & 7) and step by 128 (entries over 128 bytes take more
// steps, wave-uniformly).  k_mg_emit runs the same steps in its own loop over the groups of its half tile: that loop's
// constants are what tests/test_merge_cases.py reads from sdb_compact.hip, so it stays spelled out there.
SDB_DEV void copy_wave_rows(const CopyDesc *cd, uint32_t l) {
    const uint32_t mk = wave_max(cd[l].kb), mv = wave_max(cd[l].vb);
    const uint32_t mb = mk < mv ? mk : mv;  // chunk steps every entry's key and value share
    uint32_t x0 = 0;
    for (; x0 < mb; x0 += 128) copy_group_chunks_kv(cd, l, x0 + 16 * (l & 7));
    for (uint32_t xk = x0; xk < mk; xk += 128) copy_group_chunks<true>(cd, l, xk + 16 * (l & 7));
    for (uint32_t xv = x0; xv < mv; xv += 128) copy_group_chunks<false>(cd, l, xv + 16 * (l & 7));
}

}  // namespace
}  // namespace sdb
