// sdb_host.cpp — the host-buffer handles over the device-pointer ABI (sdb_api.cpp): sdb_encoder (one SST, or
// several with their transfers overlapped), sdb_sst_builder (EncodedSsTableBuilder's per-entry surface,
// slatedb/src/sst_builder.rs:224-417) and sdb_decoder (SsTableFormat::read_blocks, format/sst.rs:938-1038).
// A handle owns a device arena, pinned staging and its streams (sdb_host.h); it reaches the device only
// through the public calls, which check the parameters and the device.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../include/slatedb_amd.h"
#include "sdb_host.h"

using namespace sdb;

// One in-flight SST of the pipelined host path (sdb_encoder_encode_host_many).
struct EncSlot {
    PinBuf h_in;
    DevBuf d_in, d_out, d_ws;
    hipEvent_t h2d_done = nullptr, comp_done = nullptr, d2h_done = nullptr;
    bool used = false;
};

struct sdb_encoder {
    int device = 0;
    sdb_sst_params params{};
    hipStream_t stream = nullptr;  // kernels (and the whole single-SST path)
    hipEvent_t ev[4] = {};
    // device: input, output, workspace
    DevBuf d_in, d_out, d_ws;
    PinBuf h_in, h_out;
    // pipelined path: H2D and D2H on their own streams (the two copy directions overlap each other
    // and the kernels), two slots of staging / device buffers, one pinned output area per SST
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    EncSlot slot[2];
    std::vector<PinBuf> outs;
    PinBuf sums;
};

namespace {

struct InLayout {  // packed input arrays inside one allocation (256-byte aligned pieces)
    uint64_t key_bytes, key_off, val_bytes, val_off, kind, seq, cts, ets, mask, plen, total;
};
// Only the columns the batch has take space (and H2D bytes).
InLayout in_layout(const sdb_kv_batch *hb, uint64_t kb, uint64_t vb) {
    const uint64_t n = hb->n;
    Carver c{nullptr, 0};
    InLayout l{};
    l.key_bytes = c.bytes(kb + 16);
    l.key_off = c.bytes(8 * (n + 1));
    l.val_bytes = c.bytes(vb + 16);
    l.val_off = c.bytes(8 * (n + 1));
    l.kind = c.bytes(hb->kind ? n + 1 : 0);
    l.seq = c.bytes(hb->seq ? 8 * (n + 1) : 0);
    l.cts = c.bytes(hb->create_ts ? 8 * (n + 1) : 0);
    l.ets = c.bytes(hb->expire_ts ? 8 * (n + 1) : 0);
    l.mask = c.bytes(hb->ts_mask ? n + 1 : 0);
    l.plen = c.bytes(hb->prefix_len ? 4 * (n + 1) : 0);
    l.total = c.off;
    return l;
}

// The caller's (pageable) batch into pinned staging, offsets rebased to 0.  Large copies are split
// over a few host threads: one thread's memcpy bandwidth is below the PCIe rate.
void marshal(const sdb_kv_batch *hb, const InLayout &il, uint8_t *hi, uint64_t k0, uint64_t kb, uint64_t v0, uint64_t vb) {
    const uint64_t n = hb->n;
    if (!n) return;
    std::vector<std::pair<uint8_t *, const uint8_t *>> dst_src;
    std::vector<uint64_t> len;
    auto add = [&](uint8_t *d, const void *s, uint64_t l) {
        if (s && l) {
            dst_src.push_back({d, (const uint8_t *)s});
            len.push_back(l);
        }
    };
    add(hi + il.key_bytes, hb->key_bytes + k0, kb);
    add(hi + il.val_bytes, hb->val_bytes ? hb->val_bytes + v0 : nullptr, vb);
    add(hi + il.kind, hb->kind, n);
    add(hi + il.seq, hb->seq, 8 * n);
    add(hi + il.cts, hb->create_ts, 8 * n);
    add(hi + il.ets, hb->expire_ts, 8 * n);
    add(hi + il.mask, hb->ts_mask, n);
    add(hi + il.plen, hb->prefix_len, 4 * n);
    uint64_t total = 0;
    for (uint64_t l : len) total += l;
    const unsigned nt = total >= (16u << 20) ? 8 : 1;
    auto work = [&](unsigned t) {
        // byte range [t * total / nt, (t + 1) * total / nt) of the concatenated copies
        const uint64_t lo = total * t / nt, hi_ = total * (t + 1) / nt;
        uint64_t base = 0;
        for (size_t q = 0; q < len.size(); q++) {
            const uint64_t a = std::max(lo, base), b = std::min(hi_, base + len[q]);
            if (a < b) memcpy(dst_src[q].first + (a - base), dst_src[q].second + (a - base), b - a);
            base += len[q];
        }
        // and entries [t * (n + 1) / nt, ...) of the rebased offsets
        uint64_t *ko = (uint64_t *)(hi + il.key_off), *vo = (uint64_t *)(hi + il.val_off);
        const uint64_t e0 = (n + 1) * t / nt, e1 = (n + 1) * (t + 1) / nt;
        for (uint64_t i = e0; i < e1; i++) {
            ko[i] = hb->key_off[i] - k0;
            vo[i] = hb->val_off[i] - v0;
        }
    };
    if (nt == 1) {
        work(0);
        return;
    }
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; t++) th.emplace_back(work, t);
    work(0);
    for (auto &x : th) x.join();
}

sdb_kv_batch dev_batch(const sdb_kv_batch *hb, const InLayout &il, uint8_t *di) {
    sdb_kv_batch db{};
    db.n = hb->n;
    db.key_bytes = di + il.key_bytes;
    db.key_off = (const uint64_t *)(di + il.key_off);
    db.val_bytes = di + il.val_bytes;
    db.val_off = (const uint64_t *)(di + il.val_off);
    db.kind = hb->kind ? di + il.kind : nullptr;
    db.seq = hb->seq ? (const uint64_t *)(di + il.seq) : nullptr;
    db.create_ts = hb->create_ts ? (const int64_t *)(di + il.cts) : nullptr;
    db.expire_ts = hb->expire_ts ? (const int64_t *)(di + il.ets) : nullptr;
    db.ts_mask = hb->ts_mask ? di + il.mask : nullptr;
    db.prefix_len = hb->prefix_len ? (const int32_t *)(di + il.plen) : nullptr;
    return db;
}

// One host batch's plan: where its key and value bytes start, its input layout, its output capacities (in
// `out`, nothing bound), their layout and the sizes of the buffers.
struct EncPlan {
    uint64_t k0, kb, v0, vb;
    InLayout il;
    sdb_sst_out out;
    SstLayout ol;
    uint64_t out_total, ws_bytes;
};
sdb_status plan_batch(const sdb_kv_batch *hb, const sdb_sst_params *params, EncPlan *p) {
    const uint64_t n = hb->n;
    p->k0 = n ? hb->key_off[0] : 0, p->kb = n ? hb->key_off[n] - p->k0 : 0;
    p->v0 = n ? hb->val_off[0] : 0, p->vb = n ? hb->val_off[n] - p->v0 : 0;
    p->out = sdb_sst_out{};
    if (sdb_encode_bounds(n, p->kb, p->vb, params, &p->out.data_cap, &p->out.block_cap, &p->out.bloom_cap))
        return SDB_INVALID_ARGUMENT;
    if (p->out.data_cap >= (1ull << 32)) return SDB_LIMIT_EXCEEDED;  // u32 per-block/chunk byte counters
    p->il = in_layout(hb, p->kb, p->vb);
    Carver c{nullptr, 0};
    p->ol = bind_sst_out(c, p->out, true);
    p->out_total = c.off;
    p->ws_bytes = sdb_encode_workspace_bytes(n, params);
    return SDB_OK;
}
// p's outputs bound at the device buffer dout
sdb_sst_out bound_out(const EncPlan &p, void *dout) {
    sdb_sst_out o = p.out;
    Carver c{(uint8_t *)dout, 0};
    bind_sst_out(c, o, true);
    return o;
}

}  // namespace

extern "C" {

sdb_encoder *sdb_encoder_create(int device, const sdb_sst_params *params) {
    if (sdb_encode_bounds(0, 0, 0, params, nullptr, nullptr, nullptr) || sdb_device_count() <= 0) return nullptr;
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    sdb_encoder *e = new sdb_encoder();
    e->device = device;
    e->params = *params;
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) {
        delete e;
        return nullptr;
    }
    for (auto &x : e->ev) hipEventCreate(&x);
    if (hipStreamCreateWithFlags(&e->s_h2d, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&e->s_d2h, hipStreamNonBlocking) != hipSuccess) {
        sdb_encoder_destroy(e);
        return nullptr;
    }
    for (EncSlot &sl : e->slot) {
        hipEventCreateWithFlags(&sl.h2d_done, hipEventDisableTiming);
        hipEventCreateWithFlags(&sl.comp_done, hipEventDisableTiming);
        hipEventCreateWithFlags(&sl.d2h_done, hipEventDisableTiming);
    }
    return e;
}

void sdb_encoder_destroy(sdb_encoder *e) {
    if (!e) return;
    hipSetDevice(e->device);
    for (hipStream_t st : {e->stream, e->s_h2d, e->s_d2h})
        if (st) hipStreamSynchronize(st);
    for (auto &x : e->ev) hipEventDestroy(x);
    for (EncSlot &sl : e->slot)
        for (hipEvent_t x : {sl.h2d_done, sl.comp_done, sl.d2h_done})
            if (x) hipEventDestroy(x);
    for (hipStream_t st : {e->stream, e->s_h2d, e->s_d2h})
        if (st) hipStreamDestroy(st);
    delete e;
}

sdb_status sdb_encoder_encode_host(sdb_encoder *e, const sdb_kv_batch *hb, sdb_sst_host_result *r) {
    if (!e || !hb || !r) return SDB_INVALID_ARGUMENT;
    hipSetDevice(e->device);
    EncPlan p;
    sdb_status st = plan_batch(hb, &e->params, &p);
    if (st) return st;
    if (!e->h_in.ensure(p.il.total) || !e->d_in.ensure(p.il.total) || !e->h_out.ensure(p.out_total) ||
        !e->d_out.ensure(p.out_total) || !e->d_ws.ensure(p.ws_bytes))
        return SDB_DEVICE_ERROR;
    uint8_t *hi = e->h_in.at<uint8_t>(0);
    marshal(hb, p.il, hi, p.k0, p.kb, p.v0, p.vb);
    uint8_t *di = e->d_in.at<uint8_t>(0), *dout = e->d_out.at<uint8_t>(0);
    hipEventRecord(e->ev[0], e->stream);
    hipMemcpyAsync(di, hi, p.il.total, hipMemcpyHostToDevice, e->stream);
    hipEventRecord(e->ev[1], e->stream);
    const sdb_kv_batch db = dev_batch(hb, p.il, di);
    const sdb_sst_out o = bound_out(p, dout);
    st = sdb_encode_sst(&db, &e->params, &o, e->d_ws.p, e->d_ws.cap, e->stream);
    if (st) return st;
    hipEventRecord(e->ev[2], e->stream);
    // D2H: summary first (sizes), then only the used parts
    uint8_t *ho = e->h_out.at<uint8_t>(0);
    hipMemcpyAsync(ho + p.ol.summary, o.summary, sizeof(sdb_sst_summary), hipMemcpyDeviceToHost, e->stream);
    if (hipStreamSynchronize(e->stream) != hipSuccess) return SDB_DEVICE_ERROR;
    sdb_sst_summary sm;
    memcpy(&sm, ho + p.ol.summary, sizeof sm);
    copy_sst_back(ho, dout, p.ol, sm, e->stream);
    hipEventRecord(e->ev[3], e->stream);
    if (hipStreamSynchronize(e->stream) != hipSuccess) return SDB_DEVICE_ERROR;
    float t01 = 0, t12 = 0, t23 = 0;
    hipEventElapsedTime(&t01, e->ev[0], e->ev[1]);
    hipEventElapsedTime(&t12, e->ev[1], e->ev[2]);
    hipEventElapsedTime(&t23, e->ev[2], e->ev[3]);
    fill_result(*r, ho, p.ol, sm);
    r->h2d_ms = t01;
    r->kernel_ms = t12;
    r->d2h_ms = t23;
    return (sdb_status)sm.status;
}

// Several host batches, transfers overlapped: while SST i's kernels run, SST i+1 is marshalled
// into the other slot's pinned staging and copied H2D, and SST i-1's outputs come back D2H (three
// streams; the copy engines serve both directions at once).  The host waits only for each SST's
// summary (to size its D2H) and for the last D2H.
sdb_status sdb_encoder_encode_host_many(sdb_encoder *e, uint32_t count, const sdb_kv_batch *hbs,
                                        sdb_sst_host_result *results) {
    if (!e || (count && (!hbs || !results))) return SDB_INVALID_ARGUMENT;
    if (hipSetDevice(e->device) != hipSuccess) return SDB_DEVICE_ERROR;
    if (e->outs.size() < count) e->outs.resize(count);
    if (!e->sums.ensure(sizeof(sdb_sst_summary) * (count + 1))) return SDB_DEVICE_ERROR;
    sdb_sst_summary *sums = e->sums.at<sdb_sst_summary>(0);
    std::vector<EncPlan> jobs(count);
    sdb_status first = SDB_OK;
    auto fail = [&](sdb_status st) {
        for (hipStream_t x : {e->s_h2d, e->stream, e->s_d2h}) hipStreamSynchronize(x);
        return st;
    };
    for (uint32_t i = 0; i <= count; i++) {
        if (i < count) {
            const sdb_kv_batch *hb = &hbs[i];
            EncSlot &sl = e->slot[i & 1];
            EncPlan &jb = jobs[i];
            const sdb_status ps = plan_batch(hb, &e->params, &jb);
            if (ps) return fail(ps);
            // the slot's previous SST (i - 2) must be out of its staging (H2D) before the marshal
            // overwrites it; buffers only grow after every use of the slot has drained
            if (sl.used) hipEventSynchronize(sl.h2d_done);
            const bool grow = sl.h_in.cap < jb.il.total || sl.d_in.cap < jb.il.total || sl.d_out.cap < jb.out_total ||
                              sl.d_ws.cap < jb.ws_bytes;
            if (grow && sl.used) {
                hipEventSynchronize(sl.comp_done);
                hipEventSynchronize(sl.d2h_done);
            }
            if (!sl.h_in.ensure(jb.il.total) || !sl.d_in.ensure(jb.il.total) || !sl.d_out.ensure(jb.out_total) ||
                !sl.d_ws.ensure(jb.ws_bytes))
                return fail(SDB_DEVICE_ERROR);
            marshal(hb, jb.il, sl.h_in.at<uint8_t>(0), jb.k0, jb.kb, jb.v0, jb.vb);
            // H2D once the slot's previous kernels no longer read d_in
            if (sl.used) hipStreamWaitEvent(e->s_h2d, sl.comp_done, 0);
            hipMemcpyAsync(sl.d_in.p, sl.h_in.p, jb.il.total, hipMemcpyHostToDevice, e->s_h2d);
            hipEventRecord(sl.h2d_done, e->s_h2d);
            // kernels once the input is there and the slot's previous outputs are back on the host
            hipStreamWaitEvent(e->stream, sl.h2d_done, 0);
            if (sl.used) hipStreamWaitEvent(e->stream, sl.d2h_done, 0);
            const sdb_kv_batch db = dev_batch(hb, jb.il, sl.d_in.at<uint8_t>(0));
            const sdb_sst_out o = bound_out(jb, sl.d_out.p);
            const sdb_status st = sdb_encode_sst(&db, &e->params, &o, sl.d_ws.p, sl.d_ws.cap, e->stream);
            if (st) return fail(st);
            hipMemcpyAsync(&sums[i], o.summary, sizeof(sdb_sst_summary), hipMemcpyDeviceToHost, e->stream);
            hipEventRecord(sl.comp_done, e->stream);
            sl.used = true;
        }
        if (i >= 1) {  // SST j's outputs: sized by its summary, copied on the D2H stream
            const uint32_t j = i - 1;
            EncSlot &sl = e->slot[j & 1];
            const EncPlan &jb = jobs[j];
            if (hipEventSynchronize(sl.comp_done) != hipSuccess) return fail(SDB_DEVICE_ERROR);
            const sdb_sst_summary sm = sums[j];
            PinBuf &ho = e->outs[j];
            if (!ho.ensure(jb.out_total)) return fail(SDB_DEVICE_ERROR);
            hipStreamWaitEvent(e->s_d2h, sl.comp_done, 0);
            copy_sst_back(ho.at<uint8_t>(0), sl.d_out.at<uint8_t>(0), jb.ol, sm, e->s_d2h);
            hipEventRecord(sl.d2h_done, e->s_d2h);
            fill_result(results[j], ho.at<uint8_t>(0), jb.ol, sm);
            if (!first && sm.status) first = (sdb_status)sm.status;
        }
    }
    if (hipStreamSynchronize(e->s_d2h) != hipSuccess) return SDB_DEVICE_ERROR;
    return first;
}

}  // extern "C"

// -------------------------------------------------------------------------------------------------
// EncodedSsTableBuilder mirror
// -------------------------------------------------------------------------------------------------
struct sdb_sst_builder {
    sdb_encoder *enc = nullptr;
    std::vector<uint8_t> keys, vals, kind, mask;
    std::vector<uint64_t> koff{0}, voff{0}, seq;
    std::vector<int64_t> cts, ets;
};

extern "C" {

sdb_sst_builder *sdb_sst_builder_new(int device, const sdb_sst_params *params) {
    sdb_encoder *e = sdb_encoder_create(device, params);
    if (!e) return nullptr;
    sdb_sst_builder *b = new sdb_sst_builder();
    b->enc = e;
    return b;
}

void sdb_sst_builder_free(sdb_sst_builder *b) {
    if (!b) return;
    sdb_encoder_destroy(b->enc);
    delete b;
}

sdb_status sdb_sst_builder_add(sdb_sst_builder *b, const uint8_t *key, uint64_t key_len, uint8_t kind,
                               const uint8_t *val, uint64_t val_len, uint64_t seq, int32_t has_create_ts,
                               int64_t create_ts, int32_t has_expire_ts, int64_t expire_ts) {
    if (!b || kind > SDB_KIND_TOMBSTONE) return SDB_INVALID_ARGUMENT;
    b->keys.insert(b->keys.end(), key, key + key_len);
    if (kind != SDB_KIND_TOMBSTONE && val_len) b->vals.insert(b->vals.end(), val, val + val_len);
    b->koff.push_back(b->keys.size());
    b->voff.push_back(b->vals.size());
    b->kind.push_back(kind);
    b->seq.push_back(seq);
    b->cts.push_back(create_ts);
    b->ets.push_back(expire_ts);
    b->mask.push_back((uint8_t)((has_create_ts ? SDB_TS_CREATE : 0) | (has_expire_ts ? SDB_TS_EXPIRE : 0)));
    return SDB_OK;
}

sdb_status sdb_sst_builder_build(sdb_sst_builder *b, sdb_sst_host_result *r) {
    if (!b) return SDB_INVALID_ARGUMENT;
    sdb_kv_batch hb{};
    hb.n = b->kind.size();
    static const uint8_t zero16[16] = {0};
    hb.key_bytes = b->keys.empty() ? zero16 : b->keys.data();
    hb.key_off = b->koff.data();
    hb.val_bytes = b->vals.empty() ? zero16 : b->vals.data();
    hb.val_off = b->voff.data();
    hb.kind = b->kind.data();
    hb.seq = b->seq.data();
    hb.create_ts = b->cts.data();
    hb.expire_ts = b->ets.data();
    hb.ts_mask = b->mask.data();
    return sdb_encoder_encode_host(b->enc, &hb, r);
}

}  // extern "C"

// -------------------------------------------------------------------------------------------------
// Host decode
// -------------------------------------------------------------------------------------------------
struct sdb_decoder {
    int device = 0;
    hipStream_t stream = nullptr;
    DevBuf d_in, d_out, d_ws;
    PinBuf h_in, h_out;
};

extern "C" {

sdb_decoder *sdb_decoder_create(int device) {
    if (sdb_device_count() <= 0 || hipSetDevice(device) != hipSuccess) return nullptr;
    sdb_decoder *d = new sdb_decoder();
    d->device = device;
    if (hipStreamCreateWithFlags(&d->stream, hipStreamNonBlocking) != hipSuccess) {
        delete d;
        return nullptr;
    }
    return d;
}

void sdb_decoder_destroy(sdb_decoder *d) {
    if (!d) return;
    hipSetDevice(d->device);
    hipStreamSynchronize(d->stream);
    hipStreamDestroy(d->stream);
    delete d;
}

sdb_status sdb_decoder_decode_host(sdb_decoder *d, const uint8_t *blocks, const uint64_t *block_off,
                                   uint64_t nblocks, uint16_t sst_version, sdb_decode_host_result *r) {
    if (!d || !r || (nblocks && (!blocks || !block_off))) return SDB_INVALID_ARGUMENT;
    hipSetDevice(d->device);
    const uint64_t b0 = nblocks ? block_off[0] : 0;
    const uint64_t total = nblocks ? block_off[nblocks] - b0 : 0;
    // capacities: every row >= 12 bytes; restored keys can exceed encoded bytes (shared prefixes),
    // bounded by rows x (64 KiB V0 keys) — use a generous first guess and retry once if too small.
    uint64_t cap_e = total / 12 + 16;
    uint64_t key_cap = total * 4 + 4096;
    for (int attempt = 0; attempt < 2; attempt++) {
        // the outputs in the device buffer (o) and, at the same offsets, in its host mirror (h)
        sdb_decoded_out o{}, h{};
        o.key_arena_cap = key_cap;
        o.cap_entries = cap_e;
        o.bad_cap = nblocks + 1;
        auto bind = [&](sdb_decoded_out &x, uint8_t *base) {
            Carver c{base, 0};
            c.take(x.block_entry_start, nblocks + 1);
            c.take(x.key_arena, key_cap);
            c.take(x.key_off, cap_e + 1);
            c.take(x.val_off, cap_e);
            c.take(x.val_len, cap_e);
            c.take(x.seq, cap_e);
            c.take(x.flags, cap_e);
            c.take(x.create_ts, cap_e);
            c.take(x.expire_ts, cap_e);
            c.take(x.bad_block, nblocks + 1);
            c.take(x.summary, 1);
            return c.off;
        };
        const uint64_t out_total = bind(o, nullptr);
        Carver ci{nullptr, 0};  // the input: the blocks, then their offsets
        ci.bytes(total + 16);
        const uint64_t o_boff = ci.bytes(8 * (nblocks + 1)), in_total = ci.off;
        uint64_t wsb = sdb_decode_workspace_bytes(nblocks);
        if (!d->h_in.ensure(in_total) || !d->d_in.ensure(in_total) || !d->h_out.ensure(out_total) ||
            !d->d_out.ensure(out_total) || !d->d_ws.ensure(wsb))
            return SDB_DEVICE_ERROR;
        uint8_t *hi = d->h_in.at<uint8_t>(0);
        memcpy(hi, blocks + b0, total);
        uint64_t *bo = (uint64_t *)(hi + o_boff);
        for (uint64_t k = 0; k <= nblocks; k++) bo[k] = block_off[k] - b0;
        uint8_t *di = d->d_in.at<uint8_t>(0);
        hipMemcpyAsync(di, hi, in_total, hipMemcpyHostToDevice, d->stream);
        bind(o, d->d_out.at<uint8_t>(0));
        bind(h, d->h_out.at<uint8_t>(0));
        sdb_status st = sdb_decode_blocks(di, (const uint64_t *)(di + o_boff), nblocks, sst_version, &o, d->d_ws.p,
                                          d->d_ws.cap, d->stream);
        if (st) return st;
        hipMemcpyAsync(d->h_out.p, d->d_out.p, out_total, hipMemcpyDeviceToHost, d->stream);
        if (hipStreamSynchronize(d->stream) != hipSuccess) return SDB_DEVICE_ERROR;
        const sdb_decode_summary sm = *h.summary;
        if (sm.status == SDB_INVALID_ARGUMENT && attempt == 0 &&
            (sm.num_entries > cap_e || sm.key_bytes > key_cap)) {
            cap_e = sm.num_entries + 16;
            key_cap = sm.key_bytes + 4096;
            continue;
        }
        // value references are positions in the caller's `blocks` (block_off[0] was rebased to 0)
        if (b0)
            for (uint64_t i = 0; i < sm.num_entries && i < cap_e; i++)
                if (h.val_len[i]) h.val_off[i] += b0;
        r->summary = sm;
        r->block_entry_start = h.block_entry_start;
        r->key_arena = h.key_arena;
        r->key_off = h.key_off;
        r->val_off = h.val_off;
        r->val_len = h.val_len;
        r->seq = h.seq;
        r->flags = h.flags;
        r->create_ts = h.create_ts;
        r->expire_ts = h.expire_ts;
        r->bad_block = h.bad_block;
        return (sdb_status)sm.status;
    }
    return SDB_INVALID_ARGUMENT;
}

}  // extern "C"
