// rs16_api_host.cpp -- C ABI (include/rs16.h): the one-shot codec on shards
// in host memory: column slices through two slots, pipelined stripes, and
// the columns of one stripe over several engines.
#include "rs16_api.hpp"

using namespace rs16;

// ---------------------------------------------------------------------------
// Host-resident one-shot codec: shards start and end in host memory.
// ---------------------------------------------------------------------------
int rs16_engine::host_slots(rs16_error* err) {
    for (auto& sl : hslot)
        RS16_HIP(sl.s.get());
    RS16_HIP(hev.get());
    if (int rc = order(stream, err)) return rc;
    // start after the caller's earlier work on the engine stream
    RS16_HIP(hipEventRecord(hev, stream));
    for (auto& sl : hslot) RS16_HIP(hipStreamWaitEvent(sl.s, hev, 0));
    return RS16_OK;
}

// Column slice width: a multiple of 64 (every 64-byte column block is an
// independent codeword, src/algorithm.md:6-32); default: the whole shard.
// Measured on MI355X at 32768:32768 x 1 KiB (scripts/host_slices.py):
// 1024 / 512 / 256 / 128-byte slices take 1.33 / 1.40 / 1.97 / 3.16 ms per
// encode -- the pitched (2-D) pinned copies lose more than the overlap wins.
static size_t host_slice(size_t S, size_t slice) {
    if (slice == 0) slice = S;
    slice = std::max<size_t>(64, slice / 64 * 64);
    return std::min(slice, S);
}

using HostSlot = rs16_engine::HostSlot;

// A slot's device buffers for encodes / decodes of k:m shards of W bytes.
static int reserve_encode(HostSlot& sl, size_t k, size_t m, size_t W, bool high, rs16_error* err) {
    RS16_HIP(sl.orig.reserve(k * W));
    RS16_HIP(sl.rec.reserve(m * W));
    RS16_HIP(sl.z.reserve(rs16_encoder_work_count(high, k, m) * W));
    if (!high) RS16_HIP(sl.u.reserve(next_pow2(k) * W));  // (of its own: the slots run concurrently)
    return RS16_OK;
}
static int reserve_decode(HostSlot& sl, size_t k, size_t m, size_t W, const DecodeGeom& g, rs16_error* err) {
    RS16_HIP(sl.orig.reserve(k * W));
    RS16_HIP(sl.rec.reserve(m * W));
    RS16_HIP(sl.z.reserve((size_t)g.n * W));
    RS16_HIP(sl.u.reserve((size_t)g.n * W));
    RS16_HIP(sl.rcount.reserve(GF_ORDER / 64 * 8));
    return RS16_OK;
}
// The low rate's second work array of an encode on a slot.
static uint8_t* slot_u(HostSlot& sl, bool high) { return high ? nullptr : (uint8_t*)sl.u.p; }

// The byte columns [off, off + w) of a host stripe (rows of S bytes) through
// slot sl on stream s: pitched copy in, codec, pitched copy out.
static int encode_host_slice(rs16_engine* e, HostSlot& sl, hipStream_t s, bool high, size_t k, size_t m, size_t S,
                             size_t off, size_t w, const void* h_original, void* h_recovery, rs16_error* err) {
    RS16_HIP(hipMemcpy2DAsync(sl.orig.p, w, (const uint8_t*)h_original + off, S, w, k, hipMemcpyHostToDevice, s));
    if (int rc = encode_dev(e, high, k, m, w, (const uint8_t*)sl.orig.p, (uint8_t*)sl.rec.p, (uint8_t*)sl.z.p,
                            slot_u(sl, high), s, err))
        return rc;
    RS16_HIP(hipMemcpy2DAsync((uint8_t*)h_recovery + off, S, sl.rec.p, w, w, m, hipMemcpyDeviceToHost, s));
    return RS16_OK;
}
// ds: the decode with sl's rows as its shard arrays (host_decode_sides); plan: its evaluation's.
static int decode_host_slice(rs16_engine* e, HostSlot& sl, hipStream_t s, const DecodeSides& ds,
                             const rs16_engine::DecodePlan& plan, size_t k, size_t m, size_t S, size_t off, size_t w,
                             void* h_original, const void* h_recovery, rs16_error* err) {
    if (ds.rec_recv)
        RS16_HIP(hipMemcpy2DAsync(sl.rec.p, w, (const uint8_t*)h_recovery + off, S, w, m, hipMemcpyHostToDevice, s));
    if (ds.orig_recv)
        RS16_HIP(hipMemcpy2DAsync(sl.orig.p, w, (const uint8_t*)h_original + off, S, w, k, hipMemcpyHostToDevice, s));
    if (int rc = ds.passes(e, plan, w, w, 0, sl.z.p, sl.u.p, sl.rcount.p, s, err)) return rc;
    // restored originals land in place; received rows come back unchanged
    RS16_HIP(hipMemcpy2DAsync((uint8_t*)h_original + off, S, sl.orig.p, w, w, k, hipMemcpyDeviceToHost, s));
    return RS16_OK;
}

// The received counts of one stripe's host flags, and NotEnoughShards.
static int host_received(size_t k, size_t m, const uint8_t* original_received, const uint8_t* recovery_received,
                         size_t* orig_recv, size_t* rec_recv, rs16_error* err) {
    *orig_recv = count_received(original_received, k);
    *rec_recv = count_received(recovery_received, m);
    return check_received(k, *orig_recv, *rec_recv, err);
}
// Received flags of one host stripe -> the engine's hflags (originals' at
// d_flags, recovery's behind them) on the engine stream.
static int upload_host_flags(rs16_engine* e, size_t k, size_t m, const uint8_t* original_received,
                             const uint8_t* recovery_received, rs16_error* err) {
    RS16_HIP(e->hflags.reserve(k + m));
    uint8_t* d_of = (uint8_t*)e->hflags.p;
    RS16_HIP(hipMemcpyAsync(d_of, original_received, k, hipMemcpyHostToDevice, e->stream));
    RS16_HIP(hipMemcpyAsync(d_of + k, recovery_received, m, hipMemcpyHostToDevice, e->stream));
    return RS16_OK;
}
// A decode whose shard arrays are slot sl's rows and whose flags are the k + m bytes at d_flags.
static DecodeSides host_decode_sides(bool high, size_t k, size_t m, const HostSlot& sl, const uint8_t* d_flags,
                                     size_t orig_recv, size_t rec_recv) {
    return DecodeSides(high, k, m, {sl.orig.p, d_flags, orig_recv}, {sl.rec.p, d_flags + k, rec_recv});
}

extern "C" int rs16_encode_host(rs16_engine* e, size_t k, size_t m, size_t S, const void* h_original,
                                void* h_recovery, size_t slice_bytes, rs16_error* err) {
    bool high;
    if (int rc = resolve_rate(RS16_RATE_DEFAULT, k, m, S, &high, err)) return rc;
    if (int rc = e->activate(err)) return rc;
    const size_t W = host_slice(S, slice_bytes);
    for (auto& sl : e->hslot)
        if (int rc = reserve_encode(sl, k, m, W, high, err)) return rc;
    if (int rc = e->host_slots(err)) return rc;
    for (size_t off = 0, j = 0; off < S; off += W, j++) {
        auto& sl = e->hslot[j & 1];
        if (int rc = encode_host_slice(e, sl, sl.s, high, k, m, S, off, std::min(W, S - off), h_original, h_recovery,
                                       err))
            return rc;
    }
    for (auto& sl : e->hslot) RS16_HIP(hipStreamSynchronize(sl.s));
    if (int rc = e->scratch_done(e->stream, err)) return rc;
    return set_error(err, RS16_OK);
}

extern "C" int rs16_decode_host(rs16_engine* e, size_t k, size_t m, size_t S, void* h_original,
                                const uint8_t* original_received, const void* h_recovery,
                                const uint8_t* recovery_received, size_t slice_bytes, rs16_error* err) {
    bool high;
    if (int rc = resolve_rate(RS16_RATE_DEFAULT, k, m, S, &high, err)) return rc;
    size_t orig_recv, rec_recv;
    if (int rc = host_received(k, m, original_received, recovery_received, &orig_recv, &rec_recv, err)) return rc;
    if (orig_recv == k) return set_error(err, RS16_OK);
    if (int rc = e->activate(err)) return rc;
    const size_t W = host_slice(S, slice_bytes);
    for (auto& sl : e->hslot)
        if (int rc = reserve_decode(sl, k, m, W, decode_geom(high, k, m), err)) return rc;
    // received flags -> device; erasure logs once, shared by every slice
    if (int rc = e->order(e->stream, err)) return rc;
    if (int rc = upload_host_flags(e, k, m, original_received, recovery_received, err)) return rc;
    const uint8_t* d_flags = (const uint8_t*)e->hflags.p;
    const DecodeSides ds[2] = {host_decode_sides(high, k, m, e->hslot[0], d_flags, orig_recv, rec_recv),
                               host_decode_sides(high, k, m, e->hslot[1], d_flags, orig_recv, rec_recv)};
    rs16_engine::DecodePlan plan;
    if (int rc = ds[0].eval(e, e->ev_main, &plan, e->stream, err, W)) return rc;
    if (int rc = e->host_slots(err)) return rc;
    for (size_t off = 0, j = 0; off < S; off += W, j++) {
        auto& sl = e->hslot[j & 1];
        if (int rc = decode_host_slice(e, sl, sl.s, ds[j & 1], plan, k, m, S, off, std::min(W, S - off), h_original,
                                       h_recovery, err))
            return rc;
    }
    for (auto& sl : e->hslot) RS16_HIP(hipStreamSynchronize(sl.s));
    if (int rc = e->scratch_done(e->stream, err)) return rc;
    // (the counts came from the host flags themselves: nothing for rs16_decode_check)
    e->forget_decode();
    return set_error(err, RS16_OK);
}

// ---------------------------------------------------------------------------
// Host-resident stripes, pipelined.  Two lanes, each a stream with device
// buffers and codec scratch of its own (hslot[b]: rows, Z, U; ev_lane[b]:
// the decode's eval_poly outputs): stripe i runs on lane i & 1 as
// H2D -> codec -> D2H in stream order, so while one lane copies a stripe's
// outputs back the other copies the next stripe's inputs in -- both link
// directions busy -- and no event crosses between streams (the copy engines'
// waits on other queues' events stalled the pipeline for milliseconds at a
// time, profiles/r05_hostbatch_trace.txt).
// ---------------------------------------------------------------------------
namespace {
// Contiguous runs of rows whose flag equals `want` (rows [0, n)), each one
// copy; more than max_runs of them: one copy of the span from the first to
// the last such row.
template <class F>
int copy_runs(const uint8_t* flags, size_t n, bool want, size_t max_runs, F copy) {
    size_t runs = 0, first = n, last = 0;
    for (size_t i = 0; i < n; i++) {
        if ((flags[i] != 0) != want) continue;
        if (i == 0 || (flags[i - 1] != 0) != want) runs++;
        first = std::min(first, i);
        last = i + 1;
    }
    if (runs == 0) return RS16_OK;
    if (runs > max_runs) return copy(first, last - first);
    for (size_t i = 0; i < n;) {
        if ((flags[i] != 0) != want) {
            i++;
            continue;
        }
        size_t j = i;
        while (j < n && (flags[j] != 0) == want) j++;
        if (int rc = copy(i, j - i)) return rc;
        i = j;
    }
    return RS16_OK;
}
constexpr size_t HP_MAX_RUNS = 64;
}  // namespace

int rs16_engine::host_pipe_events(rs16_error* err) {
    for (auto& ev : hp_ev) RS16_HIP(ev.get());
    RS16_HIP(hp_off.get());
    return RS16_OK;
}

extern "C" int rs16_encode_host_batch(rs16_engine* e, size_t k, size_t m, size_t S, size_t nstripes,
                                      const void* h_original, size_t original_stride, void* h_recovery,
                                      size_t recovery_stride, rs16_error* err) {
    bool high;
    if (int rc = resolve_rate(RS16_RATE_DEFAULT, k, m, S, &high, err)) return rc;
    if (nstripes == 0) return set_error(err, RS16_OK);
    if (!h_original || !h_recovery || original_stride < k * S || recovery_stride < m * S)
        return set_error(err, RS16_INVALID_ARGUMENT);
    if (int rc = e->activate(err)) return rc;
    for (auto& sl : e->hslot)
        if (int rc = reserve_encode(sl, k, m, S, high, err)) return rc;
    if (int rc = e->host_pipe_events(err)) return rc;
    if (int rc = e->host_slots(err)) return rc;  // (lanes after the engine stream's earlier work)
    for (size_t i = 0; i < nstripes; i++) {
        auto& sl = e->hslot[i & 1];
        uint8_t* d_o = (uint8_t*)sl.orig.p;
        uint8_t* d_r = (uint8_t*)sl.rec.p;
        // lane 1 starts half a period late (its first H2D after lane 0's), so
        // that from then on one lane's D2H meets the other's H2D, not its D2H
        if (i == 1) RS16_HIP(hipStreamWaitEvent(sl.s, e->hp_off, 0));
        RS16_HIP(hipMemcpyAsync(d_o, (const uint8_t*)h_original + i * original_stride, k * S, hipMemcpyHostToDevice,
                                sl.s));
        if (i == 0) RS16_HIP(hipEventRecord(e->hp_off, sl.s));
        if (int rc = encode_dev(e, high, k, m, S, d_o, d_r, (uint8_t*)sl.z.p, slot_u(sl, high), sl.s, err)) return rc;
        RS16_HIP(hipMemcpyAsync((uint8_t*)h_recovery + i * recovery_stride, d_r, m * S, hipMemcpyDeviceToHost, sl.s));
    }
    for (auto& sl : e->hslot) RS16_HIP(hipStreamSynchronize(sl.s));
    if (int rc = e->scratch_done(e->stream, err)) return rc;
    return set_error(err, RS16_OK);
}

extern "C" int rs16_decode_host_batch(rs16_engine* e, size_t k, size_t m, size_t S, size_t nstripes,
                                      void* h_original, size_t original_stride, const uint8_t* original_received,
                                      size_t original_received_stride, const void* h_recovery,
                                      size_t recovery_stride, const uint8_t* recovery_received,
                                      size_t recovery_received_stride, rs16_error* err) {
    bool high;
    if (int rc = resolve_rate(RS16_RATE_DEFAULT, k, m, S, &high, err)) return rc;
    if (nstripes == 0) return set_error(err, RS16_OK);
    if (!h_original || !h_recovery || !original_received || !recovery_received || original_stride < k * S ||
        recovery_stride < m * S || original_received_stride < k || recovery_received_stride < m)
        return set_error(err, RS16_INVALID_ARGUMENT);
    // every stripe's counts first (src/rate/decoder_work.rs:120-139): a stripe
    // with too few shards fails the call before anything moves
    std::vector<size_t> ocnt(nstripes), rcnt(nstripes);
    for (size_t i = 0; i < nstripes; i++)
        if (int rc = host_received(k, m, original_received + i * original_received_stride,
                                   recovery_received + i * recovery_received_stride, &ocnt[i], &rcnt[i], err))
            return rc;
    if (int rc = e->activate(err)) return rc;
    for (auto& sl : e->hslot)
        if (int rc = reserve_decode(sl, k, m, S, decode_geom(high, k, m), err)) return rc;
    RS16_HIP(e->hflags.reserve(2 * (k + m)));
    RS16_HIP(e->hp_flags.reserve(2 * (k + m)));
    if (int rc = e->host_pipe_events(err)) return rc;
    if (int rc = e->host_slots(err)) return rc;
    auto& ev = e->hp_ev;
    int first_lane = -1;  // (lane offset: see rs16_encode_host_batch)
    bool offset_pending = true;
    for (size_t i = 0; i < nstripes; i++) {
        if (ocnt[i] == k) continue;  // nothing lost: nothing moves, nothing runs
        const int b = (int)(i & 1);
        if (first_lane >= 0 && offset_pending && b != first_lane) {
            RS16_HIP(hipStreamWaitEvent(e->hslot[b].s, e->hp_off, 0));
            offset_pending = false;
        }
        auto& sl = e->hslot[b];
        uint8_t* d_o = (uint8_t*)sl.orig.p;
        uint8_t* d_r = (uint8_t*)sl.rec.p;
        uint8_t* d_of = (uint8_t*)e->hflags.p + b * (k + m);  // the recovery's flags behind the originals'
        const uint8_t* fo = original_received + i * original_received_stride;
        const uint8_t* fr = recovery_received + i * recovery_received_stride;
        uint8_t* ho = (uint8_t*)h_original + i * original_stride;
        const uint8_t* hr = (const uint8_t*)h_recovery + i * recovery_stride;
        // rows [r0, r0 + nr) of a shard array, one copy on the lane's stream
        auto rows = [&](uint8_t* dst, const uint8_t* src, hipMemcpyKind kind) {
            return [=, &sl](size_t r0, size_t nr) -> int {
                RS16_HIP(hipMemcpyAsync(dst + r0 * S, src + r0 * S, nr * S, kind, sl.s));
                return RS16_OK;
            };
        };
        // ---- in: the flags (through page-locked staging: a pageable source
        // would make the copy synchronous; the lane's staging slot was last
        // read by its previous stripe's copy) and the received rows
        uint8_t* hf = (uint8_t*)e->hp_flags.p + b * (k + m);
        RS16_HIP(hipEventSynchronize(ev[b]));
        memcpy(hf, fo, k);
        memcpy(hf + k, fr, m);
        RS16_HIP(hipMemcpyAsync(d_of, hf, k + m, hipMemcpyHostToDevice, sl.s));
        RS16_HIP(hipEventRecord(ev[b], sl.s));
        if (int rc = copy_runs(fr, m, true, HP_MAX_RUNS, rows(d_r, hr, hipMemcpyHostToDevice))) return rc;
        if (int rc = copy_runs(fo, k, true, HP_MAX_RUNS, rows(d_o, ho, hipMemcpyHostToDevice))) return rc;
        if (first_lane < 0) {
            RS16_HIP(hipEventRecord(e->hp_off, sl.s));
            first_lane = b;
        }
        // ---- codec, with the lane's own eval_poly outputs
        const DecodeSides ds = host_decode_sides(high, k, m, sl, d_of, ocnt[i], rcnt[i]);
        rs16_engine::DecodePlan plan;
        if (int rc = ds.eval(e, e->ev_lane[b], &plan, sl.s, err, S)) return rc;
        if (int rc = ds.passes(e, plan, S, S, 0, sl.z.p, sl.u.p, sl.rcount.p, sl.s, err)) return rc;
        // ---- out: the restored originals (in place in the lane's rows)
        if (int rc = copy_runs(fo, k, false, HP_MAX_RUNS, rows(ho, d_o, hipMemcpyDeviceToHost))) return rc;
    }
    for (auto& sl : e->hslot) RS16_HIP(hipStreamSynchronize(sl.s));
    if (int rc = e->scratch_done(e->stream, err)) return rc;
    e->forget_decode();  // (the counts came from the host flags: nothing for rs16_decode_check)
    return set_error(err, RS16_OK);
}

// ---------------------------------------------------------------------------
// Several GPUs in one process: the byte columns of one stripe are split over
// the engines (every 64-byte column block is an independent codeword,
// src/algorithm.md:18-32); each engine copies its column
// slice in with a pitched DMA copy, runs the device codec on it and copies
// it back, all engines concurrently.  No exchange between the GPUs.
// ---------------------------------------------------------------------------
// Column slice of engine j of n: rs16_column_slice (rs16_comm.cpp), the
// partition the RCCL scatter / gather and rs16/columns.py use.
static void multi_slice(size_t S, int n, int j, size_t* off, size_t* w) { (void)rs16_column_slice(S, n, j, off, w); }
static int multi_check(rs16_engine* const* engines, int n, rs16_error* err) {
    if (!engines || n < 1) return set_error(err, RS16_INVALID_ARGUMENT);
    for (int j = 0; j < n; j++)
        if (!engines[j]) return set_error(err, RS16_INVALID_ARGUMENT);
    return RS16_OK;
}
static int multi_sync(rs16_engine* const* engines, int n, rs16_error* err) {
    for (int j = 0; j < n; j++) {
        rs16_engine* e = engines[j];
        if (int rc = e->activate(err)) return rc;
        RS16_HIP(hipStreamSynchronize(e->stream));
        if (int rc = e->scratch_done(e->stream, err)) return rc;
    }
    return RS16_OK;
}

extern "C" int rs16_encode_host_multi(rs16_engine* const* engines, int n, size_t k, size_t m, size_t S,
                                      const void* h_original, void* h_recovery, rs16_error* err) {
    if (int rc = multi_check(engines, n, err)) return rc;
    bool high;
    if (int rc = resolve_rate(RS16_RATE_DEFAULT, k, m, S, &high, err)) return rc;
    for (int j = 0; j < n; j++) {
        size_t off, w;
        multi_slice(S, n, j, &off, &w);
        if (w == 0) continue;
        rs16_engine* e = engines[j];
        if (int rc = e->activate(err)) return rc;
        if (int rc = e->order(e->stream, err)) return rc;
        auto& sl = e->hslot[0];
        if (int rc = reserve_encode(sl, k, m, w, high, err)) return rc;
        if (int rc = encode_host_slice(e, sl, e->stream, high, k, m, S, off, w, h_original, h_recovery, err)) return rc;
    }
    if (int rc = multi_sync(engines, n, err)) return rc;
    return set_error(err, RS16_OK);
}

extern "C" int rs16_decode_host_multi(rs16_engine* const* engines, int n, size_t k, size_t m, size_t S,
                                      void* h_original, const uint8_t* original_received, const void* h_recovery,
                                      const uint8_t* recovery_received, rs16_error* err) {
    if (int rc = multi_check(engines, n, err)) return rc;
    bool high;
    if (int rc = resolve_rate(RS16_RATE_DEFAULT, k, m, S, &high, err)) return rc;
    size_t orig_recv, rec_recv;
    if (int rc = host_received(k, m, original_received, recovery_received, &orig_recv, &rec_recv, err)) return rc;
    if (orig_recv == k) return set_error(err, RS16_OK);
    for (int j = 0; j < n; j++) {
        size_t off, w;
        multi_slice(S, n, j, &off, &w);
        if (w == 0) continue;
        rs16_engine* e = engines[j];
        if (int rc = e->activate(err)) return rc;
        if (int rc = e->order(e->stream, err)) return rc;
        auto& sl = e->hslot[0];
        if (int rc = reserve_decode(sl, k, m, w, decode_geom(high, k, m), err)) return rc;
        // (every engine its own flags and erasure logs, on its own stream, ahead of its slice)
        if (int rc = upload_host_flags(e, k, m, original_received, recovery_received, err)) return rc;
        const DecodeSides ds = host_decode_sides(high, k, m, sl, (const uint8_t*)e->hflags.p, orig_recv, rec_recv);
        rs16_engine::DecodePlan plan;
        if (int rc = ds.eval(e, e->ev_main, &plan, e->stream, err, w)) return rc;
        if (int rc = decode_host_slice(e, sl, e->stream, ds, plan, k, m, S, off, w, h_original, h_recovery, err))
            return rc;
    }
    if (int rc = multi_sync(engines, n, err)) return rc;
    for (int j = 0; j < n; j++) engines[j]->forget_decode();  // (host flags: nothing to check)
    return set_error(err, RS16_OK);
}
