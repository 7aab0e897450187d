// rs16_api_coders.cpp -- C ABI (include/rs16.h): the rs16_encoder /
// rs16_decoder state machines (EncoderWork / DecoderWork semantics of
// src/rate/{encoder,decoder}_work.rs) with HBM-resident work space.
#include "rs16_api.hpp"

using namespace rs16;

// ---------------------------------------------------------------------------
// Host staging of the Rate-level API.  The reference copies every added shard
// into its work buffer (src/rate/encoder_work.rs:49-69,
// src/rate/decoder_work.rs:62-116) and serves results out of it
// (EncoderResult::recovery / DecoderResult::restored_original).  Here a shard
// added from host memory is copied (host memcpy, no HIP call) into a
// page-locked image of the work buffer; runs of consecutive rows stream to
// HBM in DMA copies of >= STREAM_BYTES while the caller keeps adding, the
// rest goes at encode()/decode(); the results come back in one DMA copy into
// the page-locked image, and the result accessors wait for it.  encode() and
// decode() return once everything is enqueued on the engine stream.
// ---------------------------------------------------------------------------
static constexpr size_t STREAM_BYTES = (size_t)1 << 20;

// Result row `index` of an encoder / decoder in its page-locked h_out.
// on_device: the *_device accessor's answer (nullptr: no such row, which is
// no error); fetch: the coder's D2H of its result rows, once per round.
template <class C, class Fetch>
static const void* result_host(C* c, const void* on_device, size_t index, Fetch fetch, rs16_error* err) {
    if (!on_device) return set_error(err, RS16_OK), nullptr;
    // (the common case -- rows already copied back -- makes no HIP call)
    if (!c->out_on_host || c->dev.out_done.busy) {
        if (c->eng->activate(err) || fetch(c, err)) return nullptr;
        if (hipError_t he = c->dev.out_done.wait()) return hip_fail(err, he), nullptr;
    }
    set_error(err, RS16_OK);
    return (const uint8_t*)c->dev.h_out.p + index * c->S;
}
template <class C, class Fetch>
static int result_copy(C* c, const void* on_device, size_t index, void* dst, size_t len, Fetch fetch,
                       rs16_error* err) {
    if (!on_device) return set_error(err, RS16_OK), 0;
    if (len < c->S) return set_error(err, RS16_INVALID_ARGUMENT), -1;
    const void* src = result_host(c, on_device, index, fetch, err);
    if (!src) return -1;
    memcpy(dst, src, c->S);
    return 1;
}

// ---------------------------------------------------------------------------
// Encoder -- EncoderWork (src/rate/encoder_work.rs) + Rate encoders.
// ---------------------------------------------------------------------------
struct rs16_encoder {
    rs16_engine* eng;  // nullptr once the engine was freed (detached)
    int rate_kind;
    bool high = true;
    // encoded: an EncoderResult is alive (encode ran, result not dropped).
    // The encode works in place, so a second encode before the drop would
    // read recovery rows as originals; the reference's borrow rules rule
    // that out at compile time (src/rate.rs:157-166), here it is an error.
    bool encoded = false;
    size_t k = 0, m = 0, S = 0, work_count = 0, received = 0;
    // Host staging: h_in holds the rows added from host memory (row = the
    // shard's position, as the reference's work buffer); rows [run0,
    // received) are there but not yet copied to `work`.  h_out receives the
    // recovery rows.  in_done: the last H2D out of h_in (h_in may be
    // rewritten once it completed); out_done: the D2H into h_out.
    struct Dev {
        DevBuf work;
        HostBuf h_in, h_out;
        Pending in_done, out_done;
    } dev;
    size_t run0 = 0;
    bool host_round = false;  // a shard of this round came from host memory
    bool out_on_host = false;  // the D2H of this round's recovery rows is issued
};
template void rs16::detach(rs16_encoder*);

static void encoder_new_round(rs16_encoder* enc) {
    enc->received = 0;
    enc->encoded = false;
    enc->run0 = 0;
    enc->host_round = false;
    enc->out_on_host = false;
}

extern "C" int rs16_encoder_reset(rs16_encoder* enc, size_t k, size_t m, size_t S, rs16_error* err) {
    if (!enc->eng) return set_error(err, RS16_INVALID_ARGUMENT);
    bool high;
    if (int rc = resolve_rate(enc->rate_kind, k, m, S, &high, err)) return rc;
    const size_t wc = rs16_encoder_work_count(high, k, m);
    if (int rc = enc->eng->activate(err)) return rc;
    RS16_HIP(enc->dev.work.reserve(wc * S));
    enc->high = high;
    enc->k = k;
    enc->m = m;
    enc->S = S;
    enc->work_count = wc;
    encoder_new_round(enc);
    return set_error(err, RS16_OK);
}

extern "C" rs16_encoder* rs16_encoder_new(rs16_engine* eng, int rate, size_t k, size_t m, size_t S, rs16_error* err) {
    if (!eng) return set_error(err, RS16_INVALID_ARGUMENT), nullptr;
    rs16_encoder* enc = new (std::nothrow) rs16_encoder();
    if (!enc) return set_error(err, RS16_INVALID_ARGUMENT), nullptr;
    enc->eng = eng;
    enc->rate_kind = rate;
    eng->encoders.push_back(enc);
    if (rs16_encoder_reset(enc, k, m, S, err)) {
        rs16_encoder_free(enc);
        return nullptr;
    }
    return enc;
}
extern "C" void rs16_encoder_free(rs16_encoder* enc) { free_attached(enc, &rs16_engine::encoders); }
// Copy the staged host rows [run0, upto) to the device work rows.
static int encoder_stream(rs16_encoder* enc, size_t upto, rs16_error* err) {
    if (upto <= enc->run0) return RS16_OK;
    const size_t S = enc->S;
    RS16_HIP(hipMemcpyAsync((uint8_t*)enc->dev.work.p + enc->run0 * S, (const uint8_t*)enc->dev.h_in.p + enc->run0 * S,
                            (upto - enc->run0) * S, hipMemcpyHostToDevice, enc->eng->stream));
    enc->run0 = upto;
    return RS16_OK;
}
static int encoder_add(rs16_encoder* enc, const void* shard, size_t len, bool device, rs16_error* err) {
    if (!enc->eng) return set_error(err, RS16_INVALID_ARGUMENT);
    if (enc->received == enc->k) return set_error(err, RS16_TOO_MANY_ORIGINAL_SHARDS, enc->k);
    if (len != enc->S) return set_error(err, RS16_DIFFERENT_SHARD_SIZE, enc->S, len);
    const size_t r = enc->received, S = enc->S;
    if (device) {
        if (int rc = enc->eng->activate(err)) return rc;
        if (int rc = encoder_stream(enc, r, err)) return rc;  // (host rows before it)
        RS16_HIP(hipMemcpyAsync((uint8_t*)enc->dev.work.p + r * S, shard, len, hipMemcpyDeviceToDevice, enc->eng->stream));
        enc->run0 = r + 1;
    } else {
        if (r == 0) {
            // the previous round's copies out of h_in must be done
            RS16_HIP(enc->dev.in_done.wait());
            RS16_HIP(enc->dev.h_in.reserve(enc->k * S));
        }
        memcpy((uint8_t*)enc->dev.h_in.p + r * S, shard, len);
        enc->host_round = true;
        if ((r + 1 - enc->run0) * S >= STREAM_BYTES) {
            if (int rc = enc->eng->activate(err)) return rc;
            if (int rc = encoder_stream(enc, r + 1, err)) return rc;
        }
    }
    enc->received = r + 1;
    return set_error(err, RS16_OK);
}
extern "C" int rs16_encoder_add_original_shard(rs16_encoder* enc, const void* shard, size_t len, rs16_error* err) {
    return encoder_add(enc, shard, len, false, err);
}
extern "C" int rs16_encoder_add_original_shard_device(rs16_encoder* enc, const void* d, size_t len, rs16_error* err) {
    return encoder_add(enc, d, len, true, err);
}
// D2H of every recovery row into h_out (once per round).
static int encoder_fetch(rs16_encoder* enc, rs16_error* err) {
    if (enc->out_on_host) return RS16_OK;
    RS16_HIP(enc->dev.h_out.reserve(enc->m * enc->S));
    RS16_HIP(hipMemcpyAsync(enc->dev.h_out.p, enc->dev.work.p, enc->m * enc->S, hipMemcpyDeviceToHost, enc->eng->stream));
    RS16_HIP(enc->dev.out_done.record(enc->eng->stream));
    enc->out_on_host = true;
    return RS16_OK;
}
extern "C" int rs16_encoder_encode(rs16_encoder* enc, rs16_error* err) {
    if (!enc->eng || enc->encoded) return set_error(err, RS16_INVALID_ARGUMENT);
    if (enc->received != enc->k) return set_error(err, RS16_TOO_FEW_ORIGINAL_SHARDS, enc->k, enc->received);
    rs16_engine* e = enc->eng;
    if (int rc = e->activate(err)) return rc;
    if (int rc = e->order(e->stream, err)) return rc;
    if (enc->host_round) {
        if (int rc = encoder_stream(enc, enc->received, err)) return rc;
        RS16_HIP(enc->dev.in_done.record(e->stream));
    }
    uint8_t* w = (uint8_t*)enc->dev.work.p;
    uint8_t* U;
    if (int rc = engine_u(e, enc->high, enc->k, enc->S, &U, err)) return rc;
    if (int rc = encode_dev(e, enc->high, enc->k, enc->m, enc->S, w, w, w, U, e->stream, err)) return rc;
    if (int rc = e->scratch_done(e->stream, err)) return rc;
    // a host round gets its results back in one copy, right behind the passes
    if (enc->host_round)
        if (int rc = encoder_fetch(enc, err)) return rc;
    enc->encoded = true;
    return set_error(err, RS16_OK);
}
extern "C" const void* rs16_encoder_recovery_device(rs16_encoder* enc, size_t index) {
    return enc->eng && enc->encoded && index < enc->m ? (const uint8_t*)enc->dev.work.p + index * enc->S : nullptr;
}
extern "C" const void* rs16_encoder_recovery(rs16_encoder* enc, size_t index, rs16_error* err) {
    return result_host(enc, rs16_encoder_recovery_device(enc, index), index, encoder_fetch, err);
}
extern "C" int rs16_encoder_recovery_copy(rs16_encoder* enc, size_t index, void* dst, size_t len, rs16_error* err) {
    return result_copy(enc, rs16_encoder_recovery_device(enc, index), index, dst, len, encoder_fetch, err);
}
extern "C" void rs16_encoder_result_drop(rs16_encoder* enc) { encoder_new_round(enc); }
extern "C" int rs16_encoder_is_high_rate(const rs16_encoder* enc) { return enc->high; }

// ---------------------------------------------------------------------------
// Decoder -- DecoderWork (src/rate/decoder_work.rs) + Rate decoders.
// ---------------------------------------------------------------------------
struct rs16_decoder {
    rs16_engine* eng;  // nullptr once the engine was freed (detached)
    int rate_kind;
    bool high = true;
    // decoded: a DecoderResult is alive.  The decode restores in place, so
    // adding shards or decoding again before the drop is an error (the
    // reference's borrow rules, src/rate.rs:235-244).
    bool decoded = false;
    size_t k = 0, m = 0, S = 0, work_count = 0;
    size_t orig_base = 0, rec_base = 0, orig_recv = 0, rec_recv = 0;
    std::vector<uint8_t> received;  // by work position
    // Host staging: h_img is a page-locked image of the work layout.  hrow[pos]
    // = 1: row pos was added from host memory and is not yet on the device;
    // [run_lo, run_hi) is the latest stretch of consecutive host rows (it
    // streams to HBM once it reaches STREAM_BYTES).  h_flags: the received
    // flags of the two segments, for the device.
    struct Dev {
        DevBuf work, ubuf, flags;       // work = shards (z), ubuf = second work array (u)
        HostBuf h_img, h_flags, h_out;  // h_out: restored originals, row = original index
        Pending in_done, out_done;
    } dev;
    std::vector<uint8_t> hrow;
    size_t run_lo = 0, run_hi = 0;
    bool host_round = false, dev_round = false, out_on_host = false;
};
template void rs16::detach(rs16_decoder*);

static void decoder_new_round(rs16_decoder* d) {
    d->decoded = false;
    d->orig_recv = d->rec_recv = 0;
    std::fill(d->received.begin(), d->received.end(), 0);
    std::fill(d->hrow.begin(), d->hrow.end(), 0);
    d->run_lo = d->run_hi = 0;
    d->host_round = d->dev_round = d->out_on_host = false;
}

extern "C" int rs16_decoder_reset(rs16_decoder* d, size_t k, size_t m, size_t S, rs16_error* err) {
    if (!d->eng) return set_error(err, RS16_INVALID_ARGUMENT);
    bool high;
    if (int rc = resolve_rate(d->rate_kind, k, m, S, &high, err)) return rc;
    const size_t wc = rs16_decoder_work_count(high, k, m);
    if (int rc = d->eng->activate(err)) return rc;
    RS16_HIP(d->dev.work.reserve(wc * S));
    RS16_HIP(d->dev.ubuf.reserve(wc * S));
    RS16_HIP(d->dev.flags.reserve(GF_ORDER * 2));
    d->high = high;
    d->k = k;
    d->m = m;
    d->S = S;
    d->work_count = wc;
    const DecodeSides ds(high, k, m, {}, {});
    d->orig_base = ds.orig_base;  // rate_high.rs:279-299 / rate_low.rs:279-299
    d->rec_base = ds.rec_base;
    d->received.assign(std::max(d->received.size(), wc), 0);
    d->hrow.assign(std::max(d->hrow.size(), wc), 0);
    decoder_new_round(d);
    return set_error(err, RS16_OK);
}

extern "C" rs16_decoder* rs16_decoder_new(rs16_engine* eng, int rate, size_t k, size_t m, size_t S, rs16_error* err) {
    if (!eng) return set_error(err, RS16_INVALID_ARGUMENT), nullptr;
    rs16_decoder* d = new (std::nothrow) rs16_decoder();
    if (!d) return set_error(err, RS16_INVALID_ARGUMENT), nullptr;
    d->eng = eng;
    d->rate_kind = rate;
    eng->decoders.push_back(d);
    if (rs16_decoder_reset(d, k, m, S, err)) {
        rs16_decoder_free(d);
        return nullptr;
    }
    return d;
}
extern "C" void rs16_decoder_free(rs16_decoder* d) { free_attached(d, &rs16_engine::decoders); }
// Copy host rows [lo, hi) of the image to the device work rows.
static int decoder_stream(rs16_decoder* d, size_t lo, size_t hi, rs16_error* err) {
    const size_t S = d->S;
    RS16_HIP(hipMemcpyAsync((uint8_t*)d->dev.work.p + lo * S, (const uint8_t*)d->dev.h_img.p + lo * S, (hi - lo) * S,
                            hipMemcpyHostToDevice, d->eng->stream));
    std::fill(d->hrow.begin() + lo, d->hrow.begin() + hi, 0);
    return RS16_OK;
}
// Every host row not yet on the device: maximal runs of such rows, or one
// copy of their whole span when they are scattered (rows in between were
// not received, and their device contents are never read -- unless a row
// in between came from device memory: then run by run).
static int decoder_stream_all(rs16_decoder* d, rs16_error* err) {
    const size_t wc = d->work_count;
    std::vector<std::pair<size_t, size_t>> runs;
    for (size_t i = 0; i < wc;) {
        if (!d->hrow[i]) {
            i++;
            continue;
        }
        size_t j = i;
        while (j < wc && d->hrow[j]) j++;
        runs.push_back({i, j});
        i = j;
    }
    if (runs.empty()) return RS16_OK;
    if (runs.size() > 32 && !d->dev_round) return decoder_stream(d, runs.front().first, runs.back().second, err);
    for (auto& r : runs)
        if (int rc = decoder_stream(d, r.first, r.second, err)) return rc;
    return RS16_OK;
}
static int decoder_add(rs16_decoder* d, bool original, size_t index, const void* shard, size_t len, bool device,
                       rs16_error* err) {
    if (!d->eng || d->decoded) return set_error(err, RS16_INVALID_ARGUMENT);
    const size_t count = original ? d->k : d->m;
    const size_t pos = (original ? d->orig_base : d->rec_base) + index;
    if (index >= count)
        return set_error(err, original ? RS16_INVALID_ORIGINAL_SHARD_INDEX : RS16_INVALID_RECOVERY_SHARD_INDEX, count,
                         index);
    if (d->received[pos])
        return set_error(err, original ? RS16_DUPLICATE_ORIGINAL_SHARD_INDEX : RS16_DUPLICATE_RECOVERY_SHARD_INDEX,
                         index);
    if (len != d->S) return set_error(err, RS16_DIFFERENT_SHARD_SIZE, d->S, len);
    const size_t S = d->S;
    if (device) {
        if (int rc = d->eng->activate(err)) return rc;
        RS16_HIP(hipMemcpyAsync((uint8_t*)d->dev.work.p + pos * S, shard, len, hipMemcpyDeviceToDevice, d->eng->stream));
        d->dev_round = true;
    } else {
        if (!d->host_round) {
            // the previous round's copies out of the image must be done
            RS16_HIP(d->dev.in_done.wait());
            RS16_HIP(d->dev.h_img.reserve(d->work_count * S));
            d->host_round = true;
        }
        memcpy((uint8_t*)d->dev.h_img.p + pos * S, shard, len);
        d->hrow[pos] = 1;
        if (pos == d->run_hi && d->run_hi > d->run_lo) d->run_hi++;
        else d->run_lo = pos, d->run_hi = pos + 1;
        if ((d->run_hi - d->run_lo) * S >= STREAM_BYTES) {
            if (int rc = d->eng->activate(err)) return rc;
            if (int rc = decoder_stream(d, d->run_lo, d->run_hi, err)) return rc;
            d->run_lo = d->run_hi;
        }
    }
    (original ? d->orig_recv : d->rec_recv)++;
    d->received[pos] = 1;
    return set_error(err, RS16_OK);
}
extern "C" int rs16_decoder_add_original_shard(rs16_decoder* d, size_t i, const void* s, size_t len, rs16_error* err) {
    return decoder_add(d, true, i, s, len, false, err);
}
extern "C" int rs16_decoder_add_recovery_shard(rs16_decoder* d, size_t i, const void* s, size_t len, rs16_error* err) {
    return decoder_add(d, false, i, s, len, false, err);
}
extern "C" int rs16_decoder_add_original_shard_device(rs16_decoder* d, size_t i, const void* s, size_t len,
                                                      rs16_error* err) {
    return decoder_add(d, true, i, s, len, true, err);
}
extern "C" int rs16_decoder_add_recovery_shard_device(rs16_decoder* d, size_t i, const void* s, size_t len,
                                                      rs16_error* err) {
    return decoder_add(d, false, i, s, len, true, err);
}
// D2H of the lost originals' rows into h_out (one copy of their span;
// received rows inside it come back as scratch, and are never read there).
static int decoder_fetch(rs16_decoder* d, rs16_error* err) {
    if (d->out_on_host) return RS16_OK;
    size_t lo = d->k, hi = 0;
    for (size_t i = 0; i < d->k; i++)
        if (!d->received[d->orig_base + i]) lo = std::min(lo, i), hi = i + 1;
    if (hi > lo) {
        const size_t S = d->S;
        RS16_HIP(d->dev.h_out.reserve(d->k * S));
        RS16_HIP(hipMemcpyAsync((uint8_t*)d->dev.h_out.p + lo * S, (const uint8_t*)d->dev.work.p + (d->orig_base + lo) * S,
                                (hi - lo) * S, hipMemcpyDeviceToHost, d->eng->stream));
        RS16_HIP(d->dev.out_done.record(d->eng->stream));
    }
    d->out_on_host = true;
    return RS16_OK;
}
extern "C" int rs16_decoder_decode(rs16_decoder* d, rs16_error* err) {
    if (!d->eng || d->decoded) return set_error(err, RS16_INVALID_ARGUMENT);
    // (the Rate decoder counts its own received set, as the reference does:
    // there is nothing for rs16_decode_check, which serves rs16_decode_device)
    d->eng->forget_decode();
    // decode_begin (src/rate/decoder_work.rs:120-139)
    if (int rc = check_received(d->k, d->orig_recv, d->rec_recv, err)) return rc;
    if (d->orig_recv == d->k) return d->decoded = true, set_error(err, RS16_OK);  // nothing to do
    rs16_engine* e = d->eng;
    if (int rc = e->activate(err)) return rc;
    if (int rc = e->order(e->stream, err)) return rc;
    if (int rc = decoder_stream_all(d, err)) return rc;
    // (the shards and flags sit at their work positions, by segment: only the counts have sides)
    DecodeSides::Side so, sr;
    so.recv = d->orig_recv, sr.recv = d->rec_recv;
    const DecodeGeom g = DecodeSides(d->high, d->k, d->m, so, sr).g;
    // Received flags of the two segments -> device (bytes, one per row), out
    // of the page-locked staging (written once the previous round's copies
    // out of it are done).
    if (!d->host_round) RS16_HIP(d->dev.in_done.wait());
    RS16_HIP(d->dev.h_flags.reserve(GF_ORDER * 2));
    uint8_t* hf = (uint8_t*)d->dev.h_flags.p;
    memcpy(hf, d->received.data(), g.a_count);
    memcpy(hf + GF_ORDER, d->received.data() + g.chunk, g.b_count);
    uint8_t* fl = (uint8_t*)d->dev.flags.p;
    RS16_HIP(hipMemcpyAsync(fl, hf, g.a_count, hipMemcpyHostToDevice, e->stream));
    RS16_HIP(hipMemcpyAsync(fl + GF_ORDER, hf + GF_ORDER, g.b_count, hipMemcpyHostToDevice, e->stream));
    RS16_HIP(d->dev.in_done.record(e->stream));
    uint8_t* w = (uint8_t*)d->dev.work.p;
    DecodeSegs v;
    v.seg_a = w, v.fl_a = fl;
    v.seg_b = w + (size_t)g.chunk * d->S, v.fl_b = fl + GF_ORDER;
    v.rest = w + d->orig_base * d->S;
    v.S_user = d->S;
    if (int rc = e->decode_fused(g, d->S, v, w, (uint8_t*)d->dev.ubuf.p, e->stream, err)) return rc;
    e->forget_decode();
    if (int rc = e->scratch_done(e->stream, err)) return rc;
    if (d->host_round)
        if (int rc = decoder_fetch(d, err)) return rc;
    d->decoded = true;
    return set_error(err, RS16_OK);
}
extern "C" const void* rs16_decoder_restored_original_device(rs16_decoder* d, size_t index) {
    const size_t pos = d->orig_base + index;
    if (d->eng && d->decoded && index < d->k && !d->received[pos]) return (const uint8_t*)d->dev.work.p + pos * d->S;
    return nullptr;
}
extern "C" const void* rs16_decoder_restored_original(rs16_decoder* d, size_t index, rs16_error* err) {
    return result_host(d, rs16_decoder_restored_original_device(d, index), index, decoder_fetch, err);
}
extern "C" int rs16_decoder_restored_original_copy(rs16_decoder* d, size_t index, void* dst, size_t len,
                                                   rs16_error* err) {
    return result_copy(d, rs16_decoder_restored_original_device(d, index), index, dst, len, decoder_fetch, err);
}
extern "C" void rs16_decoder_result_drop(rs16_decoder* d) {  // DecoderWork::reset_received
    decoder_new_round(d);
}
extern "C" int rs16_decoder_is_high_rate(const rs16_decoder* d) { return d->high; }
