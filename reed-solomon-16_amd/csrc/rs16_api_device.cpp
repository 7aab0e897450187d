// rs16_api_device.cpp -- C ABI (include/rs16.h): the device-resident one-shot
// codec: single stripe, prepared (split) decode, batches with shared and with
// per-stripe losses.
#include "rs16_api.hpp"

using namespace rs16;

// ---------------------------------------------------------------------------
// Device-resident one-shot codec.
// ---------------------------------------------------------------------------
int rs16::encode_dev(rs16_engine* e, bool high, size_t k, size_t m, size_t S, const uint8_t* d_orig, uint8_t* d_rec,
                     uint8_t* Z, uint8_t* U, hipStream_t s, rs16_error* err, const VerifySink* vs) {
    const EncodeForm f = e->encode_form(high, k, m, S, 1);
    if (f.one_chunk) return e->encode_high_fused(f, k, m, S, S, d_orig, d_rec, Z, s, err, 1, 0, 0, vs);
    return high ? e->encode_high_multi(f, k, m, S, S, d_orig, d_rec, Z, s, err, vs)
                : e->encode_low_multi(f, k, m, S, S, d_orig, d_rec, Z, U, s, err, vs);
}
int rs16::engine_u(rs16_engine* e, bool high, size_t k, size_t S, uint8_t** U, rs16_error* err) {
    *U = nullptr;
    if (high) return RS16_OK;
    RS16_HIP(e->ws_u.reserve(next_pow2(k) * S));
    *U = (uint8_t*)e->ws_u.p;
    return RS16_OK;
}
int rs16::encode_stripes(rs16_engine* e, bool high, size_t k, size_t m, size_t S, size_t nstripes,
                         const uint8_t* d_orig, size_t bs_orig, uint8_t* d_rec, size_t bs_rec, hipStream_t s,
                         rs16_error* err, const VerifySink* vs) {
    const EncodeForm f = e->encode_form(high, k, m, S, nstripes);
    if (f.one_chunk) {
        RS16_HIP(e->ws_z.reserve(nstripes * f.chunk * S));
        return e->encode_high_fused(f, k, m, S, S, d_orig, d_rec, (uint8_t*)e->ws_z.p, s, err, nstripes, bs_orig,
                                    bs_rec, vs);
    }
    RS16_HIP(e->ws_z.reserve(rs16_encoder_work_count(high, k, m) * S));
    uint8_t *Z = (uint8_t*)e->ws_z.p, *U;
    if (int rc = engine_u(e, high, k, S, &U, err)) return rc;
    for (size_t i = 0; i < nstripes; i++) {
        const uint8_t* oi = d_orig + i * bs_orig;
        if (!vs) {
            if (int rc = encode_dev(e, high, k, m, S, oi, d_rec + i * bs_rec, Z, U, s, err)) return rc;
            continue;
        }
        VerifySink v = *vs;
        v.cmp += i * v.bs_cmp;
        v.rows += i * v.bs_rows;
        if (v.cols) v.cols += i * v.bs_cols;
        if (int rc = encode_dev(e, high, k, m, S, oi, nullptr, Z, U, s, err, &v)) return rc;
    }
    return RS16_OK;
}

extern "C" int rs16_encode_device(rs16_engine* e, size_t k, size_t m, size_t S, const void* d_original,
                                  void* d_recovery, void* stream, rs16_error* err) {
    bool high;
    if (int rc = resolve_rate(RS16_RATE_DEFAULT, k, m, S, &high, err)) return rc;
    if (!shard_aligned(d_original) || !shard_aligned(d_recovery)) return set_error(err, RS16_INVALID_ARGUMENT);
    hipStream_t s;
    if (int rc = begin_ordered(e, stream, &s, err)) return rc;
    const size_t wc = rs16_encoder_work_count(high, k, m);
    RS16_HIP(e->ws_z.reserve(wc * S));
    const int n = e->encode_form(high, k, m, S, 1).one_chunk ? e->slice_count(S) : 1;
    if (n == 1) {
        uint8_t* U;
        if (int rc = engine_u(e, high, k, S, &U, err)) return rc;
        if (int rc = encode_dev(e, high, k, m, S, (const uint8_t*)d_original, (uint8_t*)d_recovery,
                                (uint8_t*)e->ws_z.p, U, s, err))
            return rc;
    } else if (int rc = for_column_slices(e, S, n, s, err, [&](int j, size_t off, size_t w) {
                   // on the engine's slice streams (work space: wc x width each)
                   return e->encode_high_fused(e->encode_form(high, k, m, w, 1), k, m, w, S,
                                               (const uint8_t*)d_original + off,
                                               (uint8_t*)d_recovery + off, (uint8_t*)e->ws_z.p + wc * off,
                                               e->sl_stream[j], err);
               })) {
        return rc;
    }
    if (int rc = e->scratch_done(s, err)) return rc;
    return set_error(err, RS16_OK);
}

// Many independent stripes of one geometry in one call: stripe i's originals
// at d_original + i original_stride, its recovery at d_recovery + i
// recovery_stride.  High-rate stripes with k <= chunk (every k <= m) run
// batched -- each pass launch covers all stripes -- so small stripes fill the
// chip; other shapes encode stripe by stripe.
extern "C" int rs16_encode_device_batch(rs16_engine* e, size_t k, size_t m, size_t S, size_t nstripes,
                                        const void* d_original, size_t original_stride, void* d_recovery,
                                        size_t recovery_stride, void* stream, rs16_error* err) {
    bool high;
    if (int rc = resolve_rate(RS16_RATE_DEFAULT, k, m, S, &high, err)) return rc;
    if (nstripes == 0) return set_error(err, RS16_OK);
    if (!d_original || !d_recovery || !shard_aligned(d_original) || !shard_aligned(d_recovery) ||
        !batch_layout_ok(k, m, S, nstripes, original_stride, recovery_stride))
        return set_error(err, RS16_INVALID_ARGUMENT);
    hipStream_t s;
    if (int rc = begin_ordered(e, stream, &s, err)) return rc;
    if (int rc = encode_stripes(e, high, k, m, S, nstripes, (const uint8_t*)d_original, original_stride,
                                (uint8_t*)d_recovery, recovery_stride, s, err))
        return rc;
    if (int rc = e->scratch_done(s, err)) return rc;
    return set_error(err, RS16_OK);
}

// A decode with nothing to restore (every original received) launches no
// kernel that counts the flags: the flags are copied, as they are at the
// decode's place in stream order, into the engine's ws_flags (segment A at
// 0, B at GF_ORDER), and rs16_decode_check counts that copy -- the caller may
// free or reuse its arrays after the call.  A NULL flag array counts as no
// received rows (the kernels read NULL flags as "none received" too).
static int note_flags_only(rs16_engine* e, const DecodeSides& ds, void* stream, rs16_error* err) {
    e->forget_decode();
    hipStream_t s;
    if (int rc = begin_ordered(e, stream, &s, err)) return rc;
    RS16_HIP(e->ws_flags.reserve(2 * (size_t)GF_ORDER));
    uint8_t* f = (uint8_t*)e->ws_flags.p;
    if (ds.fl_a) RS16_HIP(hipMemcpyAsync(f, ds.fl_a, ds.g.a_count, hipMemcpyDeviceToDevice, s));
    else RS16_HIP(hipMemsetAsync(f, 0, ds.g.a_count, s));
    if (ds.fl_b) RS16_HIP(hipMemcpyAsync(f + GF_ORDER, ds.fl_b, ds.g.b_count, hipMemcpyDeviceToDevice, s));
    else RS16_HIP(hipMemsetAsync(f + GF_ORDER, 0, ds.g.b_count, s));
    if (int rc = e->scratch_done(s, err)) return rc;
    e->last_dec = ds.g;
    e->last_dec_flags_only = true;
    return set_error(err, RS16_OK);
}

// The passes of a device decode whose eval_poly is in ev_main (decode_eval
// on stream s or a preparation ordered before s, either one's plan), per
// column slice.
static int decode_device_passes(rs16_engine* e, const DecodeSides& ds, const rs16_engine::DecodePlan& plan, size_t S,
                                int n, hipStream_t s, rs16_error* err) {
    const size_t rows = ds.g.n;
    RS16_HIP(e->ws_z.reserve(rows * S));
    RS16_HIP(e->ws_u.reserve(rows * S));
    uint8_t* Z = (uint8_t*)e->ws_z.p;
    uint8_t* U = (uint8_t*)e->ws_u.p;
    if (n == 1) {
        if (int rc = ds.passes(e, plan, S, S, 0, Z, U, e->ev_main.rcount.p, s, err)) return rc;
    } else if (int rc = for_column_slices(e, S, n, s, err, [&](int j, size_t off, size_t w) {
                   // (decode_eval was told the slices are narrower than S: no column
                   // decode evaluates the polynomial itself; with identity multipliers
                   // the first slice's passes count the received rows)
                   void* rc_j = j == 0 && plan.ident ? e->ev_main.rcount.p : nullptr;
                   return ds.passes(e, plan, w, S, off, Z + rows * off, U + rows * off, rc_j, e->sl_stream[j], err);
               })) {
        return rc;
    }
    if (int rc = e->scratch_done(s, err)) return rc;
    return set_error(err, RS16_OK);
}

extern "C" int rs16_decode_device(rs16_engine* e, size_t k, size_t m, size_t S, void* d_original,
                                  const uint8_t* d_original_received, const void* d_recovery,
                                  const uint8_t* d_recovery_received, size_t orig_recv, size_t rec_recv, void* stream,
                                  rs16_error* err) {
    bool high;
    if (int rc = resolve_rate(RS16_RATE_DEFAULT, k, m, S, &high, err)) return rc;
    e->forget_decode();  // (whatever happens below, the previous decode is not checked again)
    if (orig_recv > k || rec_recv > m) return set_error(err, RS16_INVALID_ARGUMENT);
    if (int rc = check_received(k, orig_recv, rec_recv, err)) return rc;
    if (!shard_aligned(d_original) || !shard_aligned(d_recovery)) return set_error(err, RS16_INVALID_ARGUMENT);
    const DecodeSides ds(high, k, m, {d_original, d_original_received, orig_recv},
                         {d_recovery, d_recovery_received, rec_recv});
    if (orig_recv == k) return note_flags_only(e, ds, stream, err);
    hipStream_t s;
    if (int rc = begin_ordered(e, stream, &s, err)) return rc;
    // erasure logs once, then the passes per column slice on the slice streams
    // (one slice: the column codec may compute them itself, decode_eval)
    const int n = e->slice_count(S);
    rs16_engine::DecodePlan plan;
    if (int rc = ds.eval(e, e->ev_main, &plan, s, err, n == 1 ? S : 0)) return rc;
    return decode_device_passes(e, ds, plan, S, n, s, err);
}

// Split decode (include/rs16.h): the flag-dependent half of
// rs16_decode_device -- validation and eval_poly of the received pattern
// (src/rate/rate_high.rs:168-202, src/engine.rs:207-218) -- on one stream,
// the passes on another.  The received pattern of a decode is known before
// its shards are (a storage system knows which devices failed), so the
// erasure locator can be computed while the shards are still being produced
// or copied.  The preparation waits for the engine's earlier
// work (a previous decode still reads the eval outputs) but does not become
// the engine's last call: an encode issued after it on the engine stream runs
// concurrently with it.
extern "C" int rs16_decode_prepare(rs16_engine* e, size_t k, size_t m, size_t S, const uint8_t* d_original_received,
                                   const uint8_t* d_recovery_received, size_t orig_recv, size_t rec_recv,
                                   void* stream, rs16_error* err) {
    bool high;
    e->prep.valid = false;
    if (int rc = resolve_rate(RS16_RATE_DEFAULT, k, m, S, &high, err)) return rc;
    e->forget_decode();
    if (orig_recv > k || rec_recv > m) return set_error(err, RS16_INVALID_ARGUMENT);
    if (int rc = check_received(k, orig_recv, rec_recv, err)) return rc;
    const DecodeSides ds(high, k, m, {nullptr, d_original_received, orig_recv},
                         {nullptr, d_recovery_received, rec_recv});
    rs16_engine::Prepared p;
    p.k = k, p.m = m, p.S = S;
    p.g = ds.g, p.fl_a = ds.fl_a, p.fl_b = ds.fl_b;
    p.nslices = e->slice_count(S);
    p.nothing = orig_recv == k;
    if (!p.nothing) {
        hipStream_t s;
        if (int rc = begin_ordered(e, stream, &s, err)) return rc;
        if (int rc = e->guard_eval(s, false, err)) return rc;  // (an earlier, unconsumed preparation)
        if (int rc = ds.eval(e, e->ev_main, &p.plan, s, err, p.nslices == 1 ? S : 0, 1, 0, true)) return rc;
        RS16_HIP(e->prep_ev.get());
        RS16_HIP(hipEventRecord(e->prep_ev, s));
        e->prep_pending = true;
    }
    p.valid = true;
    e->prep = p;
    return set_error(err, RS16_OK);
}

extern "C" int rs16_decode_device_prepared(rs16_engine* e, size_t k, size_t m, size_t S, void* d_original,
                                           const void* d_recovery, void* stream, rs16_error* err) {
    const rs16_engine::Prepared p = e->prep;
    if (!p.valid || p.k != k || p.m != m || p.S != S) return set_error(err, RS16_INVALID_ARGUMENT);
    // (misaligned shard arrays: refused like a wrong geometry, the preparation stays)
    if (!shard_aligned(d_original) || !shard_aligned(d_recovery)) return set_error(err, RS16_INVALID_ARGUMENT);
    e->prep.valid = false;
    // the preparation kept its flags and counts by segment: back to the sides, now with their shard arrays
    const auto fl = DecodeSides::by_segment(p.g.high, p.fl_a, p.fl_b);
    const auto recv = DecodeSides::by_segment(p.g.high, p.g.a_recv, p.g.b_recv);
    const DecodeSides ds(p.g.high, k, m, {d_original, fl.first, recv.first}, {d_recovery, fl.second, recv.second});
    if (p.nothing) return note_flags_only(e, ds, stream, err);
    hipStream_t s;
    if (int rc = begin_ordered(e, stream, &s, err)) return rc;
    if (int rc = e->guard_eval(s, true, err)) return rc;  // after the preparation's eval_poly
    return decode_device_passes(e, ds, p.plan, S, p.nslices, s, err);
}

// rs16_decode_device for nstripes independent stripes that lost the same
// shards (one failed device holds the same shard index of every stripe):
// one eval_poly from the shared flags, every pass launch covering all
// stripes; stripe i's originals at d_original + i original_stride (restored
// in place), its recovery at d_recovery + i recovery_stride.
extern "C" int rs16_decode_device_batch(rs16_engine* e, size_t k, size_t m, size_t S, size_t nstripes,
                                        void* d_original, size_t original_stride, const uint8_t* d_original_received,
                                        const void* d_recovery, size_t recovery_stride,
                                        const uint8_t* d_recovery_received, size_t orig_recv, size_t rec_recv,
                                        void* stream, rs16_error* err) {
    bool high;
    if (int rc = resolve_rate(RS16_RATE_DEFAULT, k, m, S, &high, err)) return rc;
    e->forget_decode();
    if (orig_recv > k || rec_recv > m) return set_error(err, RS16_INVALID_ARGUMENT);
    if (int rc = check_received(k, orig_recv, rec_recv, err)) return rc;
    if (nstripes == 0) return set_error(err, RS16_OK);
    if (!shard_aligned(d_original) || !shard_aligned(d_recovery)) return set_error(err, RS16_INVALID_ARGUMENT);
    const DecodeSides ds(high, k, m, {d_original, d_original_received, orig_recv, original_stride},
                         {d_recovery, d_recovery_received, rec_recv, recovery_stride});
    if (orig_recv == k) return note_flags_only(e, ds, stream, err);
    if (!d_original || !d_recovery || !batch_layout_ok(k, m, S, nstripes, original_stride, recovery_stride))
        return set_error(err, RS16_INVALID_ARGUMENT);
    hipStream_t s;
    if (int rc = begin_ordered(e, stream, &s, err)) return rc;
    if (int rc = ds.decode_batch(e, S, nstripes, 0, s, err)) return rc;
    if (int rc = e->scratch_done(s, err)) return rc;
    return set_error(err, RS16_OK);
}

// rs16_decode_device for `nstripes` independent stripes, each with its own
// received set (reed_solomon_16::decode, src/lib.rs:287-344, once per stripe;
// src/rate/decoder_work.rs:62-139 counts every call's own received shards):
// stripe i's flags at d_*_received + i * *_received_stride bytes, its counts
// in the host arrays.  One launch of the eval kernels with a grid row per
// stripe (per-stripe erasure logs, received bitmaps, zero tiles, lost
// ranges), then the pass launches shared by all stripes, each workgroup
// reading its stripe's metadata.  Stripes go in groups of at most 256 (the
// scratch is sized for one group).  Path, per group: the half-transform
// decode when no stripe of it received an original, else the general decode
// for all of them; the first-pass tiles launched are the union over the
// group's stripes.
extern "C" int rs16_decode_device_batch_varied(rs16_engine* e, size_t k, size_t m, size_t S, size_t nstripes,
                                               void* d_original, size_t original_stride,
                                               const uint8_t* d_original_received, size_t original_received_stride,
                                               const void* d_recovery, size_t recovery_stride,
                                               const uint8_t* d_recovery_received, size_t recovery_received_stride,
                                               const size_t* original_received_counts,
                                               const size_t* recovery_received_counts, void* stream, rs16_error* err) {
    bool high;
    if (int rc = resolve_rate(RS16_RATE_DEFAULT, k, m, S, &high, err)) return rc;
    e->forget_decode();
    if (nstripes == 0) return set_error(err, RS16_OK);
    if (!d_original || !d_recovery || !d_original_received || !d_recovery_received || !original_received_counts ||
        !recovery_received_counts || !batch_layout_ok(k, m, S, nstripes, original_stride, recovery_stride) ||
        !shard_aligned(d_original) || !shard_aligned(d_recovery) || original_received_stride < k ||
        recovery_received_stride < m || nstripes > ((size_t)1 << 16))
        return set_error(err, RS16_INVALID_ARGUMENT);
    for (size_t i = 0; i < nstripes; i++) {
        const size_t o = original_received_counts[i], r = recovery_received_counts[i];
        if (o > k || r > m) return set_error(err, RS16_INVALID_ARGUMENT);
        if (int rc = check_received(k, o, r, err)) return rc;  // (the first such stripe)
    }
    hipStream_t s;
    if (int rc = begin_ordered(e, stream, &s, err)) return rc;
    // Groups of at most VARY_GROUP stripes: the per-stripe metadata (erasure
    // logs, received bitmaps, ... 0.5 MiB a stripe) and the work rows (2 n S
    // bytes a stripe) are reserved for one group, not for the whole call.
    constexpr size_t VARY_GROUP = 256;
    for (size_t g0 = 0; g0 < nstripes; g0 += VARY_GROUP) {
        const size_t ns = std::min(VARY_GROUP, nstripes - g0);
        size_t max_o = 0, max_r = 0;
        bool any_lost = false;
        for (size_t i = g0; i < g0 + ns; i++) {
            max_o = std::max(max_o, original_received_counts[i]);
            max_r = std::max(max_r, recovery_received_counts[i]);
            any_lost |= original_received_counts[i] < k;
        }
        if (!any_lost) continue;  // nothing to restore in any stripe of the group
        // (a segment counts as received when any stripe received a shard of it)
        const DecodeSides ds(high, k, m,
                             {(uint8_t*)d_original + g0 * original_stride,
                              d_original_received + g0 * original_received_stride, max_o, original_stride,
                              original_received_stride},
                             {(const uint8_t*)d_recovery + g0 * recovery_stride,
                              d_recovery_received + g0 * recovery_received_stride, max_r, recovery_stride,
                              recovery_received_stride});
        if (int rc = ds.decode_batch(e, S, ns, ns > 1 ? (uint32_t)ns : 0, s, err)) return rc;
    }
    e->forget_decode();
    if (int rc = e->scratch_done(s, err)) return rc;
    return set_error(err, RS16_OK);
}
