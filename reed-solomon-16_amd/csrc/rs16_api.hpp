// rs16_api.hpp -- what the C-ABI units (rs16_api*.cpp) share (internal):
// the helpers that cross units, the decode's segment order (DecodeSides) and
// the column slicing of a device call.
#pragma once
#include <algorithm>
#include <cstring>
#include <new>
#include <tuple>
#include <vector>

#include "rs16_engine.hpp"

namespace rs16 {

// Resolve the rate of a (rate kind, k, m) request and validate it, the way
// DefaultRate{En,De}coder::new / reset and {High,Low}Rate*::reset_work do.
int resolve_rate(int rate, size_t k, size_t m, size_t S, bool* high, rs16_error* err);

// A caller's device shard array starts on a 64-byte boundary (include/rs16.h,
// "Conventions"): the kernels load rows as 16-byte vectors and derive row
// addresses from the base, and 64 bytes is the layout's block, as for shard
// sizes and strides.  Checked by the extern "C" wrappers only, before any
// launch; the engine's own methods pass base + 64 j to themselves.
inline bool shard_aligned(const void* p) { return ((uintptr_t)p & 63) == 0; }

// The start of a call that uses the engine's scratch on the caller's stream
// (NULL: the engine's): *s, ordered after the engine's previous such call.
inline int begin_ordered(rs16_engine* e, void* stream, hipStream_t* s, rs16_error* err) {
    if (int rc = e->activate(err)) return rc;
    return e->order(*s = e->pick(stream), err);
}

// Objects created on an engine (rs16_engine::encoders / decoders /
// update_plans / locate_plans / comms) keep what they hold on the device and in
// page-locked memory in one member, `dev`: detach empties it (the holders free
// what they own; the engine's device is current, the object's work done) and
// clears the object's engine; the object's free() forgets it in its engine's list.
template <class T> void detach(T* x) {
    x->dev = {};
    x->eng = nullptr;
}
// (instantiated in the unit that defines the type: the engine's destructor sees none of them whole)
extern template void detach(rs16_encoder*);
extern template void detach(rs16_decoder*);
extern template void detach(rs16_update_plan*);
extern template void detach(rs16_locate_plan*);
void detach(rs16_comm* comm);  // first destroys its RCCL communicator (rs16_comm.cpp)
template <class V, class T> void forget(V& v, T* x) { v.erase(std::remove(v.begin(), v.end(), x), v.end()); }
template <class T> void free_attached(T* x, std::vector<T*> rs16_engine::*list) {
    if (!x) return;
    if (rs16_engine* e = x->eng) {
        (void)hipSetDevice(e->device);
        (void)hipStreamSynchronize(e->stream);
        detach(x);
        forget(e->*list, x);
    }
    delete x;
}

// Device encode of one stripe (or column slice) with work space Z of
// work_count x S bytes, on stream s.
// Z: work_count x S, U: next_pow2(k) x S for the low rate (the transformed
// originals) -- both owned by stream s for the call: the engine's ws_z /
// ws_u on the engine-ordered paths (order() / scratch_done()), a slot's own
// buffers on concurrent slots.
// Which encoder runs is the engine's one decision (rs16_engine::encode_form).
// vs: the scrub's fused path (rs16_engine::encode_high_fused).
int encode_dev(rs16_engine* e, bool high, size_t k, size_t m, size_t S, const uint8_t* d_orig, uint8_t* d_rec,
               uint8_t* Z, uint8_t* U, hipStream_t s, rs16_error* err, const VerifySink* vs = nullptr);
// The engine's own low-rate scratch for an engine-ordered call (*U = nullptr for the high rate: none needed).
int engine_u(rs16_engine* e, bool high, size_t k, size_t S, uint8_t** U, rs16_error* err);
// Device encode of nstripes stripes on the engine's scratch, on the
// engine-ordered stream s: stripe i's originals at d_orig + i bs_orig, its
// recovery to d_rec + i bs_rec.  Which launches encode them and how much
// scratch they take follows the encode form: the one-chunk high rate runs
// batched -- each pass launch covers all stripes, a chunk of work rows per
// stripe -- other shapes stripe by stripe in one stripe's work space.
// vs: the scrub's fused path -- every stripe's last launch compares on the sink
// (its cmp / rows / cols moved on by their stripe strides) and d_rec is not
// used; only for the forms of EncodeForm::verify_fusable.
int encode_stripes(rs16_engine* e, bool high, size_t k, size_t m, size_t S, size_t nstripes, const uint8_t* d_orig,
                   size_t bs_orig, uint8_t* d_rec, size_t bs_rec, hipStream_t s, rs16_error* err,
                   const VerifySink* vs = nullptr);

// What the layout of a batch of one geometry must satisfy: every stripe's
// shards fit inside its stride, the strides are whole 64-byte blocks, as shard
// sizes (every row stays aligned), and the stripes are few enough -- one
// launch holds < 2^32 tiles; stay far below.
constexpr size_t MAX_BATCH_STRIPES = (size_t)1 << 20;
inline bool batch_layout_ok(size_t k, size_t m, size_t S, size_t nstripes, size_t o_stride, size_t r_stride) {
    return o_stride >= k * S && r_stride >= m * S && o_stride % 64 == 0 && r_stride % 64 == 0 &&
           nstripes <= MAX_BATCH_STRIPES;
}

// The decode's two sides.  The kernels know segments: A = work rows [0,
// a_count), B = rows [chunk, chunk + b_count).  The callers know originals
// and recovery.  The high rate uses recovery as A and originals as B, the low
// rate the other way round -- decided here and nowhere else: every decode
// entry point hands over its originals-side and recovery-side values once and
// passes the members on (the kernels' view, DecodeSegs, is the base).
struct DecodeSides : DecodeSegs {
    // One side as the caller has it: the shard array, its received flags, the
    // received count, and for batches the byte strides from stripe to stripe.
    struct Side {
        const void* shards = nullptr;
        const uint8_t* flags = nullptr;
        size_t recv = 0, stride = 0, flag_stride = 0;
    };
    // (originals', recovery's) -> (A's, B's); the swap is its own inverse, so
    // the same call takes (A's, B's) back to (originals', recovery's).
    template <class T> static std::pair<T, T> by_segment(bool high, T orig, T rec) {
        return high ? std::pair<T, T>(rec, orig) : std::pair<T, T>(orig, rec);
    }

    DecodeGeom g;  // a_recv / b_recv set
    size_t fs_a, fs_b;
    // (rest / bs_rest: the originals' array and its stripe stride)
    size_t orig_recv, rec_recv;
    size_t orig_base, rec_base;  // first work row of the originals / the recovery (rate_{high,low}.rs:279-299)

    DecodeSides(bool high, size_t k, size_t m, const Side& orig, const Side& rec) : g(decode_geom(high, k, m)) {
        const std::pair<const Side&, const Side&> ab = by_segment<const Side&>(high, orig, rec);
        const Side &a = ab.first, &b = ab.second;
        g.a_recv = a.recv, g.b_recv = b.recv;
        seg_a = (const uint8_t*)a.shards, seg_b = (const uint8_t*)b.shards;
        fl_a = a.flags, fl_b = b.flags;
        bs_a = a.stride, bs_b = b.stride, fs_a = a.flag_stride, fs_b = b.flag_stride;
        rest = (uint8_t*)orig.shards, bs_rest = orig.stride;
        orig_recv = orig.recv, rec_recv = rec.recv;
        std::tie(orig_base, rec_base) = by_segment<size_t>(high, 0, g.chunk);
    }
    // rs16_engine::decode_eval / decode_passes with the members in their places:
    // eval writes to ev and fills *plan, which the passes of that evaluation get.
    // off: the byte column the shard arrays are entered at (a column slice).
    using EvalBufs = rs16_engine::EvalBufs;
    using DecodePlan = rs16_engine::DecodePlan;
    int eval(rs16_engine* e, EvalBufs& ev, DecodePlan* plan, hipStream_t s, rs16_error* err, size_t S = 0,
             size_t nstripes = 1, uint32_t vary = 0, bool prepare = false) const {
        return e->decode_eval(g, fl_a, fl_b, ev, plan, s, err, S, nstripes, vary, fs_a, fs_b, prepare);
    }
    int passes(rs16_engine* e, const DecodePlan& plan, size_t S, size_t S_user, size_t off, void* Z, void* U,
               void* rcount, hipStream_t s, rs16_error* err, size_t nstripes = 1) const {
        DecodeSegs v = *this;
        v.S_user = S_user;
        // (the repair restores the lost rows of both segments, each in its own array)
        if (g.repair) v.rest = (uint8_t*)seg_a, v.bs_rest = bs_a, v.rest_b = (uint8_t*)seg_b, v.bs_rest_b = bs_b;
        v.seg_a += off, v.seg_b += off, v.rest += off;
        return e->decode_passes(g, S, v, (uint8_t*)Z, (uint8_t*)U, plan, (uint32_t*)rcount, nstripes, s, err);
    }
    // A batched decode on the engine's scratch, on the engine-ordered stream s:
    // n work rows of Z and of U per stripe, the eval kernels, then the passes
    // (vary: eval's -- stripes with losses of their own).
    int decode_batch(rs16_engine* e, size_t S, size_t nstripes, uint32_t vary, hipStream_t s, rs16_error* err) const {
        RS16_HIP(e->ws_z.reserve(nstripes * g.n * S));
        RS16_HIP(e->ws_u.reserve(nstripes * g.n * S));
        DecodePlan plan;
        if (int rc = eval(e, e->ev_main, &plan, s, err, S, nstripes, vary)) return rc;
        return passes(e, plan, S, S, 0, e->ws_z.p, e->ws_u.p, e->ev_main.rcount.p, s, err, nstripes);
    }
};

// Received shards of one side, from host flag bytes (nonzero = received).
inline size_t count_received(const uint8_t* flags, size_t n) {
    size_t c = 0;
    for (size_t i = 0; i < n; i++) c += flags[i] != 0;
    return c;
}
// decode_begin (src/rate/decoder_work.rs:120-139): fewer than k shards in all.
int check_received(size_t k, size_t orig_recv, size_t rec_recv, rs16_error* err);

// A device call on stream s cut into the engine's n column slices: slice j
// covers the byte columns [off, off + w) (whole 64-byte blocks, the last
// slices the wider ones -- not rs16_column_slice's partition, which makes the
// first ones wider) and runs on e->sl_stream[j], forked from s and joined
// back into it.
template <class F> int for_column_slices(rs16_engine* e, size_t S, int n, hipStream_t s, rs16_error* err, F slice) {
    if (int rc = e->fork(s, n, err)) return rc;
    const size_t blocks = S / 64;
    for (size_t j = 0, b0 = 0; j < (size_t)n; j++) {
        const size_t b1 = blocks * (j + 1) / n;
        if (int rc = slice((int)j, b0 * 64, (b1 - b0) * 64)) return rc;
        b0 = b1;
    }
    return e->join(s, n, err);
}

}  // namespace rs16
