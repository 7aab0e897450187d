// rs16_api_verify.cpp -- C ABI (include/rs16.h): the scrub of a stripe, which
// tells whether the stored recovery shards still equal the encode of the stored
// originals and, if not, which shards and which 64-byte column blocks differ
// (single stripe and batch with one shared check set), and the host hook that
// shows its path choice.
#include "rs16_api.hpp"

using namespace rs16;

// The default path of a scrub whose encode ends in a pass with a comparing
// form (EncodeForm::verify_fusable): the fused path only where it measured
// faster than encode + compare in every alternating pair of every run, clean and
// corrupted (include/rs16.h, "When to prefer it"; profiles/r18_verify.txt).
// That is the batch form of the one-chunk high rate at 1024-row chunks (513 ..
// 1024 recovery shards, as many originals at most) from 4 stripes on -- the
// batches too wide for the column codec: 4 / 8 / 32 x 1000:1000 x 1 KiB 23.1 /
// 28.8 / 68.3 against 25.5 / 30.0 / 75.8 us.  The compare kernel's second sweep
// over the recovery costs more there than the compare loads of the last pass.
// Not one such stripe through the passes (20.3 against 22.0 us, but 7 of 9 pairs
// in one of three runs), not at 8192 rows and above nor in the multi-chunk
// rates, where the two paths lie within 2 % of each other and the fused one lost
// pairs.  Sizes in between are not measured.
static bool fused_by_default(const EncodeForm& f, size_t nstripes) {
    return f.one_chunk && f.chunk == 1024 && nstripes >= 4;
}

// 0: encode + compare, 1: the fused path (include/rs16.h); -1: unsupported shape.
// Host arithmetic only: the entry points below call it, and so can a test.
static int verify_path(const rs16_engine* e, bool high, size_t k, size_t m, size_t S, size_t nstripes) {
    // (encode_form counts the stripes of one launch: nstripes for the one-chunk high rate, else one)
    const EncodeForm f = e->encode_form(high, k, m, S, nstripes);
    if ((e->diag & DIAG_NO_FUSED_VERIFY) || !f.verify_fusable()) return 0;
    return (e->diag & DIAG_FORCE_FUSED_VERIFY) || fused_by_default(f, nstripes) ? 1 : 0;
}

// Both forms: nstripes stripes with one check set, stripe i's arrays at + i
// o_stride / r_stride and its flags at + i rf_stride / cf_stride (the single
// call: one stripe).
static int verify(rs16_engine* e, size_t k, size_t m, size_t S, bool batched, size_t nstripes, const void* d_original,
                  size_t o_stride, const void* d_recovery, size_t r_stride, const uint8_t* checked,
                  uint8_t* row_flags, size_t rf_stride, uint8_t* col_flags, size_t cf_stride, void* stream,
                  rs16_error* err) {
    bool high;
    if (int rc = resolve_rate(RS16_RATE_DEFAULT, k, m, S, &high, err)) return rc;
    if (!d_original || !d_recovery || !row_flags || !shard_aligned(d_original) || !shard_aligned(d_recovery))
        return set_error(err, RS16_INVALID_ARGUMENT);
    const size_t blocks = S / 64;
    if (batched && (!batch_layout_ok(k, m, S, nstripes, o_stride, r_stride) || rf_stride < m ||
                    (col_flags && cf_stride < blocks)))
        return set_error(err, RS16_INVALID_ARGUMENT);
    if (nstripes == 0) return set_error(err, RS16_OK);
    hipStream_t s;
    if (int rc = begin_ordered(e, stream, &s, err)) return rc;
    // Both paths only ever store the byte 1: the used range of each stripe's
    // flag arrays is cleared first, the bytes between the strides stay.
    if (nstripes == 1 || rf_stride == m) RS16_HIP(hipMemsetAsync(row_flags, 0, (nstripes - 1) * rf_stride + m, s));
    else RS16_HIP(hipMemset2DAsync(row_flags, rf_stride, 0, m, nstripes, s));
    if (col_flags) {
        if (nstripes == 1 || cf_stride == blocks)
            RS16_HIP(hipMemsetAsync(col_flags, 0, (nstripes - 1) * cf_stride + blocks, s));
        else RS16_HIP(hipMemset2DAsync(col_flags, cf_stride, 0, blocks, nstripes, s));
    }
    const uint8_t* o = (const uint8_t*)d_original;
    const uint8_t* r = (const uint8_t*)d_recovery;
    // (the encode's work space: the engine's buffers, never the caller's shards)
    if (verify_path(e, high, k, m, S, nstripes) == 1) {
        // The encode's sequence up to its last launch, which compares with the
        // stored rows instead of storing: no second recovery array.
        const VerifySink vs{r, S, r_stride, row_flags, col_flags, checked, rf_stride, cf_stride};
        if (int rc = encode_stripes(e, high, k, m, S, nstripes, o, o_stride, nullptr, 0, s, err, &vs)) return rc;
    } else {
        // The engine's encode of the stripe(s) into a buffer of its own, then
        // one compare kernel over it and the stored shards.
        const size_t rs = m * S;
        RS16_HIP(e->ws_rep.reserve(nstripes * rs));
        uint8_t* rep = (uint8_t*)e->ws_rep.p;
        if (int rc = encode_stripes(e, high, k, m, S, nstripes, o, o_stride, rep, rs, s, err)) return rc;
        if (int rc = e->profiled(PROF_VERIFY_CMP, s, err, [&](uint64_t*) {
                return launch_verify_cmp(rep, r, checked, row_flags, col_flags, (uint32_t)m, S, rs, r_stride,
                                         rf_stride, cf_stride, (uint32_t)nstripes, s);
            }))
            return rc;
    }
    if (int rc = e->scratch_done(s, err)) return rc;
    return set_error(err, RS16_OK);
}

extern "C" int rs16_verify_device(rs16_engine* e, size_t k, size_t m, size_t S, const void* d_original,
                                  const void* d_recovery, const uint8_t* d_recovery_checked,
                                  uint8_t* d_recovery_mismatch, uint8_t* d_column_mismatch, void* stream,
                                  rs16_error* err) {
    return verify(e, k, m, S, false, 1, d_original, 0, d_recovery, 0, d_recovery_checked, d_recovery_mismatch, m,
                  d_column_mismatch, S / 64, stream, err);
}

extern "C" int rs16_verify_device_batch(rs16_engine* e, size_t k, size_t m, size_t S, size_t nstripes,
                                        const void* d_original, size_t original_stride, const void* d_recovery,
                                        size_t recovery_stride, const uint8_t* d_recovery_checked,
                                        uint8_t* d_recovery_mismatch, size_t recovery_mismatch_stride,
                                        uint8_t* d_column_mismatch, size_t column_mismatch_stride, void* stream,
                                        rs16_error* err) {
    return verify(e, k, m, S, true, nstripes, d_original, original_stride, d_recovery, recovery_stride,
                  d_recovery_checked, d_recovery_mismatch, recovery_mismatch_stride, d_column_mismatch,
                  column_mismatch_stride, stream, err);
}

// The path of a scrub (include/rs16.h) on an engine with the diagnostic
// switches `diag` and the default column-codec limits: 0 encode + compare, 1
// fused, -1 unsupported counts or shard size.  Host arithmetic only (an engine
// object that is never activated: no device call).
extern "C" int rs16_host_verify_path(size_t k, size_t m, size_t S, size_t nstripes, int diag) {
    bool high;
    rs16_error err;
    if (resolve_rate(RS16_RATE_DEFAULT, k, m, S, &high, &err)) return -1;
    rs16_engine e;
    e.diag = diag;
    return verify_path(&e, high, k, m, S, nstripes ? nstripes : 1);
}
