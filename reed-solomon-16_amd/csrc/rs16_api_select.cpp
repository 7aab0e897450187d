// rs16_api_select.cpp -- C ABI (include/rs16.h): the selective decode of a
// stripe, the degraded read -- only the lost originals of the caller's read
// set are restored (single stripe and batch with one shared pattern and one
// shared read set), and the host hook that shows its path choice.
#include "rs16_api.hpp"

using namespace rs16;

// The path of a selective decode (include/rs16.h).  Host arithmetic only: the
// entry points below call it, and so can a test.
extern "C" int rs16_host_select_path(size_t k, size_t m, size_t orig_recv, size_t rec_recv, size_t wanted_count) {
    const int high = rs16_use_high_rate(k, m, nullptr);
    if (high < 0 || orig_recv > k || rec_recv > m || wanted_count > k - orig_recv || orig_recv + rec_recv < k)
        return -1;
    if (orig_recv == k || wanted_count == 0) return 0;
    return wanted_count == k - orig_recv ? 1 : 2;
}

// Both forms: nstripes stripes with one pattern and one read set, stripe i's
// arrays at + i o_stride / r_stride (the single call: one stripe, strides 0).
static int decode_select(rs16_engine* e, size_t k, size_t m, size_t S, bool batched, size_t nstripes, void* d_original,
                         size_t o_stride, const uint8_t* fl_o, const uint8_t* wanted, const void* d_recovery,
                         size_t r_stride, const uint8_t* fl_r, size_t orig_recv, size_t rec_recv, size_t wanted_count,
                         void* stream, rs16_error* err) {
    bool high;
    if (int rc = resolve_rate(RS16_RATE_DEFAULT, k, m, S, &high, err)) return rc;
    e->forget_decode();  // (whatever happens below, the previous decode is not checked again)
    if (!d_original || !d_recovery || !fl_o || !fl_r || !wanted || !shard_aligned(d_original) ||
        !shard_aligned(d_recovery))
        return set_error(err, RS16_INVALID_ARGUMENT);
    if (batched && !batch_layout_ok(k, m, S, nstripes, o_stride, r_stride)) return set_error(err, RS16_INVALID_ARGUMENT);
    if (orig_recv > k || rec_recv > m || wanted_count > k - orig_recv) return set_error(err, RS16_INVALID_ARGUMENT);
    if (int rc = check_received(k, orig_recv, rec_recv, err)) return rc;
    if (nstripes == 0) return set_error(err, RS16_OK);
    const int path = rs16_host_select_path(k, m, orig_recv, rec_recv, wanted_count);
    if (path == 0) return set_error(err, RS16_OK);  // everything received or nothing wanted: nothing launched
    if (path == 1) {
        // the read set covers every lost original: the decode, unchanged (every form of it)
        if (!batched)
            return rs16_decode_device(e, k, m, S, d_original, fl_o, d_recovery, fl_r, orig_recv, rec_recv, stream, err);
        return rs16_decode_device_batch(e, k, m, S, nstripes, d_original, o_stride, fl_o, d_recovery, r_stride, fl_r,
                                        orig_recv, rec_recv, stream, err);
    }
    hipStream_t s;
    if (int rc = begin_ordered(e, stream, &s, err)) return rc;
    // The general decode's sequence with the lost rows' interval, the reveal and
    // the stores narrowed to the read set (DecodeGeom::select); one column slice
    // whatever rs16_engine_set_slices says.
    DecodeSides ds(high, k, m, {d_original, fl_o, orig_recv, o_stride}, {d_recovery, fl_r, rec_recv, r_stride});
    ds.g.select = true;
    ds.g.wanted = wanted;
    ds.g.wanted_count = wanted_count;
    if (int rc = ds.decode_batch(e, S, nstripes, 0, s, err)) return rc;
    if (int rc = e->scratch_done(s, err)) return rc;
    return set_error(err, RS16_OK);
}

extern "C" int rs16_decode_device_select(rs16_engine* e, size_t k, size_t m, size_t S, void* d_original,
                                         const uint8_t* d_original_received, const uint8_t* d_original_wanted,
                                         const void* d_recovery, const uint8_t* d_recovery_received, size_t orig_recv,
                                         size_t rec_recv, size_t wanted_count, void* stream, rs16_error* err) {
    return decode_select(e, k, m, S, false, 1, d_original, 0, d_original_received, d_original_wanted, d_recovery, 0,
                         d_recovery_received, orig_recv, rec_recv, wanted_count, stream, err);
}

extern "C" int rs16_decode_device_select_batch(rs16_engine* e, size_t k, size_t m, size_t S, size_t nstripes,
                                               void* d_original, size_t original_stride,
                                               const uint8_t* d_original_received, const uint8_t* d_original_wanted,
                                               const void* d_recovery, size_t recovery_stride,
                                               const uint8_t* d_recovery_received, size_t orig_recv, size_t rec_recv,
                                               size_t wanted_count, void* stream, rs16_error* err) {
    return decode_select(e, k, m, S, true, nstripes, d_original, original_stride, d_original_received,
                         d_original_wanted, d_recovery, recovery_stride, d_recovery_received, orig_recv, rec_recv,
                         wanted_count, stream, err);
}
