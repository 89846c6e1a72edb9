// sdb_decode.h — kernel arguments of the batched block decoder.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slatedb_amd.h"
#include "sdb_workspace.h"

namespace sdb {

struct DecodeArgs {
    const uint8_t *blocks;
    const uint64_t *block_off;  // nblocks+1 (contiguous) or nblocks starts (with block_end)
    const uint64_t *block_end;  // nblocks ends, or NULL: block k ends at block_off[k + 1]
    uint64_t nblocks;
    uint32_t version;
    sdb_decoded_out out;  // device pointers
    // workspace
    uint64_t *cnt, *kbytes;            // per block
    uint8_t *flag;                     // per block: 1 = sequential V2 walk
    uint64_t *rcnt;                    // per block: rows of restart regions 0..3 (16 bits each; ~0: not recorded)
    uint16_t *rowpos;                  // per block: 4 x 32 row positions (region q, row i at q * 32 + i)
    uint64_t *ent_start, *key_start;   // nblocks+1
    uint64_t *tile_x, *tile_y;         // per 1024-block tile (+1)
    unsigned long long *err, *nbad;
    uint32_t *done;                    // k_dec_emit workgroups finished (small batches: the last one finishes)
    uint32_t small;                    // 1: nblocks <= 1024 and one block per wave: k_dec_emit scans the counts itself
    uint32_t descending;               // 1: output in descending iteration order (written mirrored by k_dec_emit)
    uint32_t fail_fast, pad_ff;        // 1: read_blocks semantics (the first failing block fails the call, the
                                       //    columns are unspecified then): the checksums move to the emit pass
    uint32_t *bad_block;
    uint64_t bad_cap;
    uint64_t dn, dkb;                  // descending: entries and key bytes of the whole output (k_dec_emit)
};

// Sizes (w == NULL) or binds the workspace of a decode of a.nblocks blocks.  sdb_decode_workspace_bytes has no
// 256 bytes of its own for the round-up of the caller's pointer: rowpos comes last, and its spare block's 256
// bytes (the kernels index it by block < nblocks) pay for it.
inline uint64_t decode_bind(DecodeArgs &a, uint8_t *w) {
    const uint64_t nb = a.nblocks, nt = (nb + 1023) / 1024 + 1;
    Carver c{w, 0};
    c.take(a.cnt, nb + 1);
    c.take(a.kbytes, nb + 1);
    c.take(a.flag, nb + 1);
    c.take(a.rcnt, nb + 1);
    c.take(a.ent_start, nb + 1);
    c.take(a.key_start, nb + 1);
    c.take(a.tile_x, nt + 1);
    c.take(a.tile_y, nt + 1);
    c.take(a.err, 1);
    c.take(a.nbad, 1);
    c.take(a.done, 2);
    c.take(a.rowpos, 128 * (nb + 1));
    return c.off;
}
// The error word of a decode in the caller's `workspace` (min block << 8 | status, ~0: none).
inline const unsigned long long *decode_err_word(void *workspace, uint64_t nblocks) {
    DecodeArgs a{};
    a.nblocks = nblocks;
    decode_bind(a, ws_align(workspace));
    return a.err;
}

hipError_t launch_decode(DecodeArgs a, hipStream_t st);
hipError_t launch_excl_scan2(const uint64_t *x, const uint64_t *y, uint64_t n, uint64_t *tx, uint64_t *ty,
                             uint64_t *ox, uint64_t *oy, hipStream_t st);

// f3: per-block decompression (sdb_codec.hip)
uint64_t decompress_workspace_bytes(uint64_t nblocks);
hipError_t launch_decompress_plan(uint32_t codec, const uint8_t *blocks, const uint64_t *block_off, uint64_t nblocks,
                                  uint64_t *out_start, uint8_t *w, hipStream_t st);
hipError_t launch_decompress_run(uint32_t codec, const uint8_t *blocks, const uint64_t *block_off, uint64_t nblocks,
                                 uint8_t *out, uint64_t out_cap, const uint64_t *out_start, uint64_t *out_end,
                                 unsigned long long *err, hipStream_t st);
uint64_t decompress_once_workspace_bytes(uint64_t nblocks);
hipError_t launch_decompress_once(uint32_t codec, const uint8_t *blocks, const uint64_t *block_off, uint64_t nblocks,
                                  uint64_t slot_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_start,
                                  uint64_t *out_end, unsigned long long *err, uint8_t *w, hipStream_t st);
// f3: per-block compression, the write side (sdb_codec_enc.hip)
uint64_t compress_workspace_bytes(uint64_t nblocks, uint64_t in_bytes);
hipError_t launch_compress(uint32_t codec, const uint8_t *blocks, const uint64_t *block_off, uint64_t nblocks,
                           uint64_t in_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_off,
                           unsigned long long *err, uint8_t *w, hipStream_t st);

}  // namespace sdb
