// sdb_codec.h — what the block decompressors share (sdb_codec.hip: LZ4 / Snappy and the launchers,
// sdb_codec_ent.hip: zlib / zstd): the kernel arguments, the frame rules of one block and the grid cap.
#pragma once
#include "sdb_crc.h"
#include "sdb_decode.h"
#include "sdb_device.h"

namespace sdb {

// a block's output bound: LZ4 / Snappy headers declaring more get SDB_LIMIT_EXCEEDED, the entropy decoders stop there
constexpr uint64_t kMaxBlockOut = 64ull << 20;

struct DzArgs {
    uint32_t codec;
    const uint8_t *blocks;
    const uint64_t *block_off;  // nblocks + 1
    uint64_t nblocks;
    uint64_t *slot;             // workspace: per block slot bytes (nblocks + 1)
    uint8_t *out;
    uint64_t out_cap;
    const uint64_t *out_start;  // nblocks + 1 (the plan)
    uint64_t *out_end;          // nblocks
    unsigned long long *err;    // min (block << 8 | status), ~0 = none
};
struct EntArgs : DzArgs {
    // zlib decode-once (launch_decompress_once): slot i decodes block list[i] (i < *nlist) instead of block
    // i; the optimistic run lists the blocks whose output overflowed their slot instead of failing them,
    // the wide run those with dynamic-Huffman blocks; out_by_block: a list pass writes to out_start[list[i]]
    const uint32_t *list;
    const unsigned long long *nlist;
    uint32_t *ovf_list;
    unsigned long long *ovf_count;
    uint32_t *dyn_list;
    unsigned long long *dyn_count;
    bool out_by_block;
    uint64_t *wres;  // the wide pass's per-block results for k_zl_verify: 2 words per block
};

// ---- one block's frame: payload ++ CRC32 big-endian of the payload, stored and re-framed alike -----------------
// (SsTableFormat::decode_block, format/sst.rs:980-999).  A block's status is the first of: too short for its
// CRC (or over 4 GiB) -> SDB_CORRUPT_BLOCK; the stored CRC (validate_checksum, format/sst.rs:1029-1038); an
// empty slot (the plan could not size the block: the codec family's status); a slot past out_cap; the decode.

// crc32fast::hash of msg[0, n) (generic pointer: LDS or HBM), every lane; tab: slicing tables in LDS.
SDB_DEV uint32_t frame_crc(const uint8_t *msg, uint64_t n, const uint32_t (*tab)[256]) {
    if (n >= 4) return wave_crc32_lds(msg, (uint32_t)n, tab);
    uint32_t x = 0xFFFFFFFFu;
    for (uint32_t q = 0; q < n; q++) x = tab[0][(x ^ msg[q]) & 0xFF] ^ (x >> 8);
    return x ^ 0xFFFFFFFFu;
}
SDB_DEV uint32_t frame_stored_crc(const uint8_t *in, uint64_t bl) {
    return (uint32_t)in[bl] << 24 | (uint32_t)in[bl + 1] << 16 | (uint32_t)in[bl + 2] << 8 | (uint32_t)in[bl + 3];
}
SDB_DEV bool frame_corrupt(uint64_t s, uint64_t e) { return e < s || e - s < 4 || e - s > 0xFFFFFFFFull; }
// The status before the decode of a block that is not frame_corrupt: in[0, bl) is its payload (LDS or HBM),
// [o, o + slot) its output; no_slot: the status of an empty slot (SDB_DECOMPRESSION_ERROR for the entropy
// codecs; k_dz_run passes SDB_LIMIT_EXCEEDED and looks at the header again only when it comes back).  Every lane.
SDB_DEV int frame_status(const uint8_t *in, uint64_t bl, const uint32_t (*tab)[256], uint64_t o, uint64_t slot,
                         uint64_t out_cap, int no_slot) {
    const uint32_t stored = frame_stored_crc(in, bl);  // (its loads in flight over the CRC's)
    if (frame_crc(in, bl, tab) != stored) return SDB_CHECKSUM_MISMATCH;
    if (slot == 0) return no_slot;
    if (o + slot > out_cap) return SDB_INVALID_ARGUMENT;
    return 0;
}
// The CRC of the decoded bytes p[0, n) appended (p in LDS or HBM; lane 0 stores).  Whole wave.
SDB_DEV void frame_trailer(uint8_t *p, uint64_t n, const uint32_t (*tab)[256]) {
    const uint32_t c = frame_crc(p, n, tab);
    if (lane_id() == 0) {
        p[n] = (uint8_t)(c >> 24);
        p[n + 1] = (uint8_t)(c >> 16);
        p[n + 2] = (uint8_t)(c >> 8);
        p[n + 3] = (uint8_t)c;
    }
}
// Block b's result: ol bytes and their trailer at o, or nothing and status st in the error word.  Whole wave.
SDB_DEV void frame_publish(const DzArgs &a, uint64_t b, uint64_t o, uint64_t ol, int st) {
    if (lane_id() == 0) {
        a.out_end[b] = st ? o : o + ol + 4;
        if (st) atomicMin(a.err, (unsigned long long)((b << 8) | (uint64_t)st));
    }
}

// Workgroups for a launch that wants `want`, at most per_cu for each CU of the current device.
inline uint32_t wgs_capped(uint64_t want, uint32_t per_cu) {
    int dev = 0, cus = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const uint64_t most = (uint64_t)(cus > 0 ? cus : 256) * per_cu;
    return (uint32_t)(want < most ? want : most);
}

// The entropy-coded codecs' passes (sdb_codec_ent.hip), each on the filled arguments.
// a.slot <- the blocks' slot bytes (zlib: of the blocks a.list names, when set; zero past the list)
hipError_t launch_ent_slots(const EntArgs &a, hipStream_t st);
// one decoder per wave (zstd) or five (zlib: identity, or a decode-once list pass)
hipError_t launch_ent_run(const EntArgs &a, hipStream_t st);
// zlib decode-once's first pass over the fixed slots: k_zl_wide, then k_zl_verify
hipError_t launch_zl_wide(const EntArgs &a, hipStream_t st);

}  // namespace sdb
