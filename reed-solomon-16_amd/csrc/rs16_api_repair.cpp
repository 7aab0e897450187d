// rs16_api_repair.cpp -- C ABI (include/rs16.h): the repair of a stripe, which
// restores lost recovery shards along with lost originals (single stripe and
// batch with one shared pattern), and the host hook that shows its path choice.
#include "rs16_api.hpp"

using namespace rs16;

// The path of a repair and the last pass's launch range (include/rs16.h).
// Host arithmetic only: the entry points below call it, and so can a test.
extern "C" int rs16_host_repair_path(size_t k, size_t m, size_t orig_recv, size_t rec_recv, uint32_t* lo,
                                     uint32_t* first_tile, uint32_t* tiles) {
    if (lo) *lo = 0;
    if (first_tile) *first_tile = 0;
    if (tiles) *tiles = 0;
    const int high = rs16_use_high_rate(k, m, nullptr);
    if (high < 0 || orig_recv > k || rec_recv > m || orig_recv + rec_recv < k) return -1;
    if (orig_recv == k && rec_recv == m) return 0;
    if (rec_recv == m) return 1;
    if (orig_recv == k) return 2;
    const RepairTiles rt = repair_tiles(decode_geom(high == 1, k, m));
    if (lo) *lo = rt.lo;
    // (two launches when whole tiles lie between the segments: tiles [0, a_tiles)
    // and [b_first, b_first + b_tiles); one range from tile 0: b_first = a_tiles = 0)
    if (first_tile) *first_tile = rt.b_first;
    if (tiles) *tiles = rt.a_tiles + rt.b_tiles;
    return 3;
}

// Both forms: nstripes stripes with one pattern, stripe i's arrays at + i
// o_stride / r_stride (the single call: one stripe, strides 0).
static int repair(rs16_engine* e, size_t k, size_t m, size_t S, bool batched, size_t nstripes, void* d_original,
                  size_t o_stride, const uint8_t* fl_o, void* d_recovery, size_t r_stride, const uint8_t* fl_r,
                  size_t orig_recv, size_t rec_recv, void* stream, rs16_error* err) {
    bool high;
    if (int rc = resolve_rate(RS16_RATE_DEFAULT, k, m, S, &high, err)) return rc;
    e->forget_decode();  // (whatever happens below, the previous decode is not checked again)
    if (!d_original || !d_recovery || !fl_o || !fl_r || !shard_aligned(d_original) || !shard_aligned(d_recovery))
        return set_error(err, RS16_INVALID_ARGUMENT);
    if (batched && !batch_layout_ok(k, m, S, nstripes, o_stride, r_stride)) return set_error(err, RS16_INVALID_ARGUMENT);
    if (orig_recv > k || rec_recv > m) return set_error(err, RS16_INVALID_ARGUMENT);
    if (int rc = check_received(k, orig_recv, rec_recv, err)) return rc;
    if (nstripes == 0) return set_error(err, RS16_OK);
    const int path = rs16_host_repair_path(k, m, orig_recv, rec_recv, nullptr, nullptr, nullptr);
    if (path == 0) return set_error(err, RS16_OK);  // everything received: nothing launched
    if (path == 1) {
        // no recovery shard lost: the decode, unchanged (every form of it)
        if (!batched)
            return rs16_decode_device(e, k, m, S, d_original, fl_o, d_recovery, fl_r, orig_recv, rec_recv, stream, err);
        return rs16_decode_device_batch(e, k, m, S, nstripes, d_original, o_stride, fl_o, d_recovery, r_stride, fl_r,
                                        orig_recv, rec_recv, stream, err);
    }
    hipStream_t s;
    if (int rc = begin_ordered(e, stream, &s, err)) return rc;
    if (path == 2) {
        // No original lost: every input of the encode is there, and the general
        // decode costs about twice an encode.  The engine's encode of the
        // stripe(s) into a buffer of its own, then the rows whose flag is 0
        // copied into the caller's array (received rows are not written).
        e->prep.valid = false;  // (a pending preparation is dropped, as by a decode)
        const size_t rs = m * S;
        RS16_HIP(e->ws_rep.reserve(nstripes * rs));
        uint8_t* rep = (uint8_t*)e->ws_rep.p;
        if (int rc = encode_stripes(e, high, k, m, S, nstripes, (const uint8_t*)d_original, o_stride, rep, rs, s, err))
            return rc;
        if (int rc = e->profiled(PROF_REPAIR_COPY, s, err, [&](uint64_t*) {
                return launch_repair_copy((uint8_t*)d_recovery, rep, fl_r, (uint32_t)m, S, r_stride, rs,
                                          (uint32_t)nstripes, s);
            }))
            return rc;
        if (int rc = e->scratch_done(s, err)) return rc;
        return set_error(err, RS16_OK);
    }
    // Both kinds lost: the general decode's sequence with the reveal and the
    // stores of its last pass extended to both segments (DecodeGeom::repair).
    DecodeSides ds(high, k, m, {d_original, fl_o, orig_recv, o_stride}, {d_recovery, fl_r, rec_recv, r_stride});
    ds.g.repair = true;
    if (int rc = ds.decode_batch(e, S, nstripes, 0, s, err)) return rc;
    if (int rc = e->scratch_done(s, err)) return rc;
    return set_error(err, RS16_OK);
}

extern "C" int rs16_repair_device(rs16_engine* e, size_t k, size_t m, size_t S, void* d_original,
                                  const uint8_t* d_original_received, void* d_recovery,
                                  const uint8_t* d_recovery_received, size_t orig_recv, size_t rec_recv, void* stream,
                                  rs16_error* err) {
    return repair(e, k, m, S, false, 1, d_original, 0, d_original_received, d_recovery, 0, d_recovery_received,
                  orig_recv, rec_recv, stream, err);
}

extern "C" int rs16_repair_device_batch(rs16_engine* e, size_t k, size_t m, size_t S, size_t nstripes,
                                        void* d_original, size_t original_stride,
                                        const uint8_t* d_original_received, void* d_recovery, size_t recovery_stride,
                                        const uint8_t* d_recovery_received, size_t orig_recv, size_t rec_recv,
                                        void* stream, rs16_error* err) {
    return repair(e, k, m, S, true, nstripes, d_original, original_stride, d_original_received, d_recovery,
                  recovery_stride, d_recovery_received, orig_recv, rec_recv, stream, err);
}
