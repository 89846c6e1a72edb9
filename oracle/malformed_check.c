/* malformed_check -- the oracle over a catalogue of malformed blocks, built with the address and
 * undefined-behaviour sanitizers (make malformed_check).  The catalogue file is written by
 * tests/test_malformed_blocks.py: every case is three blocks, the middle one mutated, in a buffer of exactly the
 * data's length, so a read past the bytes the oracle judges is a sanitizer error.  Each case runs
 * orc_decode_blocks, orc_decode_blocks_desc (statuses checked against the file's; -1: not checked) and
 * orc_sst_lookup in both orders. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sdb_oracle.h"

static void need(FILE *f, void *p, size_t n) {
    if (n && fread(p, 1, n, f) != n) {
        fprintf(stderr, "short catalogue file\n");
        exit(2);
    }
}

static void *exact(FILE *f, size_t n) { /* n bytes in an allocation of n bytes (1 when empty) */
    uint8_t *p = (uint8_t *)malloc(n ? n : 1);
    need(f, p, n);
    return p;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    char magic[4];
    uint32_t ncases;
    need(f, magic, 4);
    need(f, &ncases, 4);
    if (memcmp(magic, "MBC1", 4)) return 2;
    int failed = 0;
    for (uint32_t c = 0; c < ncases; c++) {
        struct { uint32_t version, nblocks; int32_t asc, desc; uint32_t nkeys; uint64_t data_len, ik_len; } __attribute__((packed)) h;
        need(f, &h, sizeof h);
        const uint64_t nb = h.nblocks;
        uint64_t *off = (uint64_t *)exact(f, 8 * (nb + 1)), *iko = (uint64_t *)exact(f, 8 * (nb + 1));
        uint8_t *data = (uint8_t *)exact(f, h.data_len), *ik = (uint8_t *)exact(f, h.ik_len);
        uint64_t *koff = (uint64_t *)calloc(h.nkeys + 1, 8);
        uint8_t *keys = NULL;
        for (uint32_t q = 0; q < h.nkeys; q++) {
            uint32_t n;
            need(f, &n, 4);
            keys = (uint8_t *)realloc(keys, koff[q] + n + 1);
            need(f, keys + koff[q], n);
            koff[q + 1] = koff[q] + n;
        }
        const uint64_t cap = h.data_len / 8 + 64, kcap = h.data_len * 16 + 4096;
        for (int desc = 0; desc < 2; desc++) {
            sdb_decode_summary sm;
            sdb_decoded_out o;
            memset(&o, 0, sizeof o);
            o.block_entry_start = (uint64_t *)calloc(nb + 1, 8);
            o.key_arena = (uint8_t *)malloc(kcap);
            o.key_arena_cap = kcap;
            o.key_off = (uint64_t *)calloc(cap + 1, 8);
            o.val_off = (uint64_t *)calloc(cap, 8);
            o.val_len = (uint32_t *)calloc(cap, 4);
            o.seq = (uint64_t *)calloc(cap, 8);
            o.flags = (uint8_t *)calloc(cap, 1);
            o.create_ts = (int64_t *)calloc(cap, 8);
            o.expire_ts = (int64_t *)calloc(cap, 8);
            o.cap_entries = cap;
            o.bad_block = (uint32_t *)calloc(nb + 1, 4);
            o.bad_cap = nb + 1;
            o.summary = &sm;
            const int st = (int)(desc ? orc_decode_blocks_desc : orc_decode_blocks)(data, off, nb, (uint16_t)h.version, &o);
            const int want = desc ? h.desc : h.asc;
            if (want >= 0 && st != want) {
                fprintf(stderr, "case %u desc %d: status %d, catalogue %d\n", c, desc, st, want);
                failed++;
            }
            free(o.block_entry_start); free(o.key_arena); free(o.key_off); free(o.val_off); free(o.val_len);
            free(o.seq); free(o.flags); free(o.create_ts); free(o.expire_ts); free(o.bad_block);
            if (h.nkeys) {
                sdb_sst_view v;
                memset(&v, 0, sizeof v);
                v.data = data;
                v.block_off = off;
                v.num_blocks = nb;
                v.index_keys = ik;
                v.index_key_off = iko;
                v.sst_version = (uint16_t)h.version;
                sdb_lookup_out l;
                const size_t n = h.nkeys;
                l.state = (uint8_t *)calloc(n, 1);
                l.status = (int32_t *)calloc(n, 4);
                l.block = (uint32_t *)calloc(n, 4);
                l.entry = (uint32_t *)calloc(n, 4);
                l.key_len = (uint32_t *)calloc(n, 4);
                l.val_off = (uint64_t *)calloc(n, 8);
                l.val_len = (uint32_t *)calloc(n, 4);
                l.seq = (uint64_t *)calloc(n, 8);
                l.flags = (uint8_t *)calloc(n, 1);
                l.create_ts = (int64_t *)calloc(n, 8);
                l.expire_ts = (int64_t *)calloc(n, 8);
                orc_sst_lookup(&v, keys, koff, n, desc, &l);
                free(l.state); free(l.status); free(l.block); free(l.entry); free(l.key_len); free(l.val_off);
                free(l.val_len); free(l.seq); free(l.flags); free(l.create_ts); free(l.expire_ts);
            }
        }
        free(off); free(iko); free(data); free(ik); free(koff); free(keys);
    }
    fclose(f);
    if (failed) return 1;
    printf("%u cases ok\n", ncases);
    return 0;
}
