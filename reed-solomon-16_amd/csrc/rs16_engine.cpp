// rs16_engine.cpp -- engine object: tables in HBM, engine-level transforms
// as HBM passes, and the fused encode/decode pass sequences.
#include <cstdlib>
#include "rs16_engine.hpp"

#include <algorithm>
#include <cstring>

namespace rs16 {

hipError_t DevBuf::reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
}
void DevBuf::release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
}

hipError_t HostBuf::reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    hipError_t e = hipHostMalloc(&p, bytes, hipHostMallocPortable);
    if (e == hipSuccess) cap = bytes;
    return e;
}
void HostBuf::release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
}

void Event::release() {
    if (ev) (void)hipEventDestroy(ev);
    ev = nullptr;
}
void Stream::release() {
    if (s) (void)hipStreamDestroy(s);
    s = nullptr;
}

hipError_t Pending::record(hipStream_t s) {
    if (hipError_t e = ev.get()) return e;
    hipError_t e = hipEventRecord(ev, s);
    busy = e == hipSuccess;
    return e;
}
hipError_t Pending::wait() {
    if (!busy) return hipSuccess;
    busy = false;
    return hipEventSynchronize(ev);
}

int set_error(rs16_error* err, int code, uint64_t v0, uint64_t v1, uint64_t v2) {
    if (err) {
        err->code = code;
        err->v0 = v0;
        err->v1 = v1;
        err->v2 = v2;
    }
    return code;
}
int hip_fail(rs16_error* err, hipError_t e) { return set_error(err, RS16_DEVICE_ERROR, (uint64_t)e); }

size_t next_pow2(size_t x) {
    size_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

DecodeGeom decode_geom(bool high, size_t k, size_t m) {
    DecodeGeom g;
    g.high = high;
    g.a_count = (uint32_t)(high ? m : k);
    g.b_count = (uint32_t)(high ? k : m);
    g.chunk = (uint32_t)next_pow2(g.a_count);
    g.n = (uint32_t)next_pow2((size_t)g.chunk + g.b_count);
    return g;
}

RepairTiles repair_tiles(const DecodeGeom& g) {
    const int L = ilog2(g.n);
    if (L <= 8) return {0, 0, 0, 1};
    RepairTiles t;
    t.lo = (uint32_t)(L / 2);
    const uint32_t tile = 1u << t.lo;
    t.a_tiles = (g.a_count + tile - 1) >> t.lo;
    t.b_first = g.chunk >> t.lo;
    const uint32_t b_end = (uint32_t)(((size_t)g.chunk + g.b_count + tile - 1) >> t.lo);
    if (t.b_first <= t.a_tiles) t.a_tiles = 0, t.b_first = 0;  // one range from tile 0
    t.b_tiles = b_end - t.b_first;
    return t;
}

static PassArgs base_args(const rs16_engine* e, size_t S) {
    PassArgs a;
    std::memset(&a, 0, sizeof a);
    a.skew_tab = e->d_skew_tab.as<uint32_t>();
    a.mul_tab = e->d_mul_tab.as<uint32_t>();
    a.zero = e->d_zero_sink.as<uint8_t>();
    a.S_in = a.S_out = a.S_seg = a.S_rest = S;
    a.qrow = (uint32_t)(S / 8);
    a.diag = (uint32_t)e->diag;
    a.z_form = Z_SHARD;  // (only the sequences that ask z_form_sequence set another form: z_form_args)
    return a;
}

}  // namespace rs16

using namespace rs16;

int rs16_engine::activate(rs16_error* err) {
    RS16_HIP(hipSetDevice(device));
    return RS16_OK;
}

int rs16_engine::slice_count(size_t S) const {
    const int n = slices;
    return (int)std::max<size_t>(1, std::min<size_t>(std::min(n, MAX_SLICES), S / 64));
}

// Slice 0 runs on the caller's stream s itself; slices 1.. on sl_stream[1..]
// (sl_stream[0] = s while a sliced call is being issued).
int rs16_engine::fork(hipStream_t s, int n, rs16_error* err) {
    RS16_HIP(sl_fork.get());
    if (n > 1) RS16_HIP(hipEventRecord(sl_fork, s));
    for (int j = 1; j < n; j++) {
        RS16_HIP(sl_own[j].get());
        RS16_HIP(hipStreamWaitEvent(sl_own[j], sl_fork, 0));
    }
    sl_stream[0] = s;
    for (int j = 1; j < MAX_SLICES; j++) sl_stream[j] = sl_own[j];
    return RS16_OK;
}

int rs16_engine::join(hipStream_t s, int n, rs16_error* err) {
    for (int j = 1; j < n; j++) {
        RS16_HIP(sl_join[j].get());
        RS16_HIP(hipEventRecord(sl_join[j], sl_own[j]));
        RS16_HIP(hipStreamWaitEvent(s, sl_join[j], 0));
    }
    return RS16_OK;
}

int rs16_engine::order(hipStream_t s, rs16_error* err) {
    if (last == LAST_ENGINE && s != stream) {
        RS16_HIP(order_ev.get());
        RS16_HIP(hipEventRecord(order_ev, stream));
        RS16_HIP(hipStreamWaitEvent(s, order_ev, 0));
    } else if (last == LAST_CALLER) {
        RS16_HIP(hipStreamWaitEvent(s, order_ev, 0));  // (recorded by scratch_done)
    }
    return RS16_OK;
}

int rs16_engine::scratch_done(hipStream_t s, rs16_error* err) {
    if (s == stream) {
        last = LAST_ENGINE;
        return RS16_OK;
    }
    RS16_HIP(order_ev.get());
    RS16_HIP(hipEventRecord(order_ev, s));
    last = LAST_CALLER;
    return RS16_OK;
}

// A timing event out of the pool (a new one when the pool is empty), recorded on s.
static hipError_t pooled_record(std::vector<Event>& pool, Event* ev, hipStream_t s) {
    if (!pool.empty()) *ev = std::move(pool.back()), pool.pop_back();
    if (hipError_t e = ev->get(hipEventDefault)) return e;
    return hipEventRecord(*ev, s);
}

int rs16_engine::prof_begin(hipStream_t s, Event* ev, rs16_error* err) {
    if (profiling) RS16_HIP(pooled_record(ev_pool, ev, s));
    return RS16_OK;
}

int rs16_engine::prof_end(int id, hipStream_t s, Event ev, rs16_error* err) {
    if (!ev) return RS16_OK;
    Event b;
    RS16_HIP(pooled_record(ev_pool, &b, s));
    prof_pending.push_back({id, std::move(ev), std::move(b)});
    if (prof_pending.size() > 4096) return prof_collect(err);  // bound the event pool
    return RS16_OK;
}

int rs16_engine::prof_collect(rs16_error* err) {
    for (ProfRec& r : prof_pending) {
        RS16_HIP(hipEventSynchronize(r.b));
        float ms = 0.f;
        RS16_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        prof_ms[r.id] += ms;
        prof_n[r.id] += 1;
        ev_pool.push_back(std::move(r.a));
        ev_pool.push_back(std::move(r.b));
    }
    prof_pending.clear();
    return RS16_OK;
}

int rs16_engine::pass(int prog, int T, const PassArgs& a, uint32_t tiles, hipStream_t s, rs16_error* err, int prof) {
    return profiled(prof < 0 ? prog : prof, s, err, [&](uint64_t* stamps) {
        if (!stamps) return launch_pass(prog, T, a, tiles, s);
        PassArgs b = a;
        b.stamps = stamps;
        return launch_pass(prog, T, b, tiles, s);
    });
}

bool rs16_engine::col_ok(int L, size_t S, size_t nstripes, bool gen) const {
    const bool rows = col_rows_ok((uint32_t)L) || (gen && L == (int)COL_LGEN);
    if (!rows || (diag & DIAG_NO_COLUMN)) return false;
    return (S / 8) * nstripes <= col_max_quads || (diag & DIAG_FORCE_COLUMN);
}

// the radix-2 multi-chunk encodes (launch_col, COL_ENC_IFFT / COL_ENC_FFTX /
// COL_ENC with nch > 1): 2^8 .. 2^10-row chunks, 2 or more of them and at
// most col_max_chunk_rows rows (the high rate's 256 / 512-row chunks: up to
// 8192 rows, which still beat the passes there: 8000:300 30.1 against 33.7
// us, 8000:200 34.0 against 40.9, profiles/r04_probe_chunks.txt)
bool rs16_engine::col_chunks_ok(int L, uint32_t nch, size_t S, bool high) const {
    const size_t rows_max = high && L <= 9 ? std::max<size_t>(col_max_chunk_rows, 8192) : col_max_chunk_rows;
    return L >= (int)COL_LCHUNK && L <= (int)COL_LMAX && nch > 1 && nch <= COL_MAX_CHUNKS &&
           (((size_t)nch << L) <= rows_max || (diag & DIAG_FORCE_COLUMN)) &&
           nch < col_img_count((uint32_t)L) && col_ok(L, S, 1);
}

ColArgs rs16_engine::col_args(const uint8_t* in, size_t S_in, uint8_t* out, size_t S_out, size_t S, size_t in_rows,
                              size_t out_rows, size_t skew_ifft, size_t skew_fft) const {
    ColArgs a;
    std::memset(&a, 0, sizeof a);
    a.skew_tab = d_skew_tab.as<uint32_t>();
    a.mul_tab = d_mul_tab.as<uint32_t>();
    a.zero = d_zero_sink.as<uint8_t>();
    a.nstripes = 1;
    a.diag = (uint32_t)diag;
    a.in = in;
    a.S_in = S_in;
    a.out = out;
    a.S_out = S_out;
    a.qrow = (uint32_t)(S / 8);
    a.in_rows = (uint32_t)in_rows;
    a.out_rows = (uint32_t)out_rows;
    a.skew_ifft = (uint32_t)skew_ifft;
    a.skew_fft = (uint32_t)skew_fft;
    return a;
}

// The one decision of how a shape is encoded: the branches of the three
// encoders below, in the order they are tested here.
EncodeForm rs16_engine::encode_form(bool high, size_t k, size_t m, size_t S, size_t nstripes) const {
    EncodeForm f;
    f.chunk = next_pow2(high ? m : k);
    f.one_chunk = high && k <= f.chunk;
    f.nch = (uint32_t)(((high ? k : m) + f.chunk - 1) / f.chunk);
    const int L = f.L = ilog2(f.chunk);
    f.lo = L <= 8 ? L : L / 2;  // (row_split above 2^8 rows; up to there one pass over all L bits)
    f.hi = L - f.lo;
    if (f.one_chunk) f.kind = col_ok(L, S, nstripes) ? f.COL : (L <= 8 ? f.ONE_PASS : f.THREE_PASS);
    else if (L == 0) f.kind = f.ROWS;
    else if (!high && f.nch == 1) f.kind = col_ok(L, S, 1) ? f.COL : f.PASSES;
    else if (L == (int)COLM_L && f.nch <= COLM_MAX_CHUNKS && col_ok(L, S, 1)) f.kind = f.COLM;
    else f.kind = col_chunks_ok(L, f.nch, S, high) ? f.COL_CHUNKS : f.PASSES;
    return f;
}

// The column codec's tables (HostTables::col_img / col_v), uploaded on the
// engine's first column launch: engines that never run it allocate nothing.
int rs16_engine::col_tables(hipStream_t s, rs16_error* err) {
    if (d_col_img.p) return RS16_OK;
    const HostTables& t = host_tables();
    DevBuf img, v;  // (the members only once both are whole)
    RS16_HIP(img.reserve(COL_IMG_DWORDS * 4));
    RS16_HIP(v.reserve(t.col_v.size() * 4));
    RS16_HIP(hipMemcpyAsync(img.p, t.col_img.data(), COL_IMG_DWORDS * 4, hipMemcpyHostToDevice, s));
    RS16_HIP(hipMemcpyAsync(v.p, t.col_v.data(), t.col_v.size() * 4, hipMemcpyHostToDevice, s));
    RS16_HIP(hipStreamSynchronize(s));  // (pageable sources: keep no pending copy)
    d_col_img = std::move(img);
    d_col_v = std::move(v);
    return RS16_OK;
}

int rs16_engine::col(const ColArgs& args, int L, int mode, hipStream_t s, rs16_error* err) {
    const bool sel = mode == COL_DEC_GEN_SEL;
    const bool dec = mode == COL_DEC_EWORK || mode == COL_DEC_EVAL || mode == COL_DEC_GEN || sel;
    if (int rc = col_tables(s, err)) return rc;
    // the table images of the two transforms (skew deltas 0 / 2^L; the
    // kernel adds the chunk index of a multi-chunk encode to the delta)
    ColArgs a = args;
    const uint32_t N = 1u << L;
    if ((a.skew_ifft != 0 && a.skew_ifft != N) || (a.skew_fft != 0 && a.skew_fft != N) ||
        (a.nch > 1 && a.nch >= col_img_count((uint32_t)L)))
        return hip_fail(err, hipErrorInvalidValue);  // (unreachable: every caller passes 0 or 2^L)
    const uint32_t *img = d_col_img.as<uint32_t>(), *vt = d_col_v.as<uint32_t>();
    a.img_ifft = (const uint8_t*)(img + col_img_offset((uint32_t)L, a.skew_ifft ? 1 : 0));
    a.img_fft = (const uint8_t*)(img + col_img_offset((uint32_t)L, a.skew_fft ? 1 : 0));
    if (mode == COL_DEC_EVAL) a.vtab = vt + col_v_offset(2u << L);  // (2^(L+1) work rows)
    if (mode == COL_DEC_GEN || sel) a.vtab = vt + col_v_offset(1u << L);  // (2^L work rows)
    return profiled(sel ? PROF_COL_DEC_SEL : (dec ? PROF_COL_DEC : PROF_COL_ENC), s, err, [&](uint64_t* stamps) {
        if (stamps) a.stamps = stamps;
        return launch_col(a, (uint32_t)L, mode, s);
    });
}

// The multi-chunk encodes of 128-row chunks in one launch (colm_kernel,
// rs16_col.hip): nch chunks of originals (high) or of recovery (low).
int rs16_engine::col_multi(size_t k, size_t m, size_t S, size_t S_user, const uint8_t* d_orig, uint8_t* d_rec,
                           uint32_t nch, bool high, hipStream_t s, rs16_error* err) {
    ColArgs c = col_args(d_orig, S_user, d_rec, S_user, S, k, m, 0, 0);
    c.nch = nch;
    // (colm_kernel records no timeline: the stamps pointer is not passed on)
    return profiled(PROF_COL_ENC, s, err, [&](uint64_t*) { return launch_col_multi(c, high, s); });
}

// The three launches of a sequence that keeps the work buffer in form f: the
// form, and their twiddle table (a tower sequence: in tower coordinates).
void rs16_engine::z_form_args(PassArgs& a, ZForm f) const {
    a.z_form = f;
    a.skew_tab = (f == Z_TOWER ? d_skew_tab_tower : d_skew_tab).as<uint32_t>();
}

// Engine::fft over 2^L rows: L <= 8 in one pass; otherwise the high
// (L - L/2) row bits as a strided pass, then the low L/2 bits contiguous.
int rs16_engine::fft(uint8_t* data, size_t S, size_t pos, size_t size, size_t skew_delta, hipStream_t s,
                     rs16_error* err) {
    const int L = ilog2(size);
    if (L == 0) return RS16_OK;
    PassArgs a = base_args(this, S);
    a.in = a.out = data + pos * S;
    a.skew_fft = (uint32_t)skew_delta;
    if (L <= 8) {
        RS16_PASS(GEN_FFT, L, a, 1, s);
        return RS16_OK;
    }
    const int lo = row_split(L).lo, hi = row_split(L).hi;
    a.lo = lo;
    RS16_PASS(GEN_FFT, hi, a, 1u << lo, s);
    a.lo = 0;
    RS16_PASS(GEN_FFT, lo, a, 1u << hi, s);
    return RS16_OK;
}

int rs16_engine::ifft(uint8_t* data, size_t S, size_t pos, size_t size, size_t skew_delta, hipStream_t s,
                      rs16_error* err) {
    const int L = ilog2(size);
    if (L == 0) return RS16_OK;
    PassArgs a = base_args(this, S);
    a.in = a.out = data + pos * S;
    a.skew_ifft = (uint32_t)skew_delta;
    if (L <= 8) {
        RS16_PASS(GEN_IFFT, L, a, 1, s);
        return RS16_OK;
    }
    const int lo = row_split(L).lo, hi = row_split(L).hi;
    a.lo = 0;
    RS16_PASS(GEN_IFFT, lo, a, 1u << hi, s);
    a.lo = lo;
    RS16_PASS(GEN_IFFT, hi, a, 1u << lo, s);
    return RS16_OK;
}

// The last launch of an encode as the scrub's comparing program: nothing is
// stored to a recovery array (out stays null), the stored rows are read at the
// addresses the recovery stores would take.
static void sink_args(PassArgs& a, const VerifySink& v) {
    a.out = nullptr;
    a.S_out = 0;
    a.vfy_cmp = v.cmp;
    a.vfy_S = v.S_cmp;
    a.bs_vfy_cmp = v.bs_cmp;
    a.vfy_rows = v.rows;
    a.vfy_cols = v.cols;
    a.vfy_checked = v.checked;
    a.bs_vfy_rows = v.bs_rows;
    a.bs_vfy_cols = v.bs_cols;
    a.bs_vfy_checked = 0;  // (one check set for all stripes)
}

// HighRateEncoder::encode for original_count <= chunk (src/rate/rate_high.rs:44-83):
//   recovery = FFT(IFFT(originals zero-padded to chunk, skew = chunk), skew = 0)[0..m)
// as three passes over the 2-D row factorisation (contiguous low bits /
// strided high bits); IFFT-high and FFT-high share the strided pass.
int rs16_engine::encode_high_fused(const EncodeForm& f, size_t k, size_t m, size_t S, size_t S_user,
                                   const uint8_t* d_orig, uint8_t* d_rec, uint8_t* Z, hipStream_t s, rs16_error* err,
                                   size_t nst, size_t bs_orig, size_t bs_rec, const VerifySink* vs) {
    const size_t chunk = f.chunk;
    const int L = f.L, lo = f.lo, hi = f.hi;
    // (a verify sink: the forms whose last launch compares -- never the column codec's)
    if (vs && !f.verify_fusable()) return set_error(err, RS16_INVALID_ARGUMENT);
    if (f.kind == f.COL) {
        // 512 / 1024-row chunks: the whole encode in one launch (rs16_col.hip)
        ColArgs c = col_args(d_orig, S_user, d_rec, S_user, S, k, m, chunk, 0);
        c.nstripes = (uint32_t)nst;
        c.bs_in = bs_orig;
        c.bs_out = bs_rec;
        return col(c, L, COL_ENC, s, err);
    }
    PassArgs a = base_args(this, S);
    a.seg_a = d_orig;
    a.S_seg = S_user;
    a.a_count = (uint32_t)k;
    a.skew_ifft = (uint32_t)chunk;
    a.skew_fft = 0;
    a.out_rows = (uint32_t)m;
    // nst > 1: independent stripes batched in each launch (PassArgs::stripe_tiles);
    // stripe i's originals / recovery at d_orig / d_rec + i bs_orig / bs_rec,
    // its work rows at Z + i chunk S
    const uint32_t ns = (uint32_t)nst;
    auto batch = [&](uint32_t tiles, size_t bs_in, size_t bs_out, size_t bs_seg) {
        a.stripe_tiles = ns > 1 ? tiles : 0;
        a.bs_in = bs_in;
        a.bs_out = bs_out;
        a.bs_seg = bs_seg;
        return tiles * ns;
    };
    if (f.kind == f.ONE_PASS) {
        a.out = d_rec;
        a.S_out = S_user;
        if (vs) sink_args(a, *vs);
        RS16_PASS(vs ? ENC_SINGLE_VFY : ENC_SINGLE, L, a, batch(1, 0, bs_rec, bs_orig), s);
        return RS16_OK;
    }
    const size_t zs = chunk * S;
    // the form of Z between the three passes, one decision for all of them
    // (a verify sink: the work rows in the shards' own form -- the comparing
    // last pass has the general kernel only)
    const ZForm zf = vs ? Z_SHARD : z_form_sequence((uint32_t)chunk, S, S_user, a.a_count, a.chunk, a.row_base_in, diag);
    a.out = Z;
    a.lo = 0;
    z_form_args(a, zf);
    RS16_PASS(ENC_FIRST, lo, a, batch(1u << hi, 0, zs, bs_orig), s);
    a.in = Z;
    a.lo = lo;
    RS16_PASS(ENC_MID, hi, a, batch(1u << lo, zs, zs, 0), s);
    a.in = Z;
    a.out = d_rec;
    a.S_out = S_user;
    a.lo = 0;
    const uint32_t tiles = (uint32_t)((m + ((size_t)1 << lo) - 1) >> lo);
    if (vs) sink_args(a, *vs);
    RS16_PASS(vs ? ENC_LAST_VFY : ENC_LAST, lo, a, batch(tiles, zs, bs_rec, 0), s);
    return RS16_OK;
}

// {High,Low}RateDecoder::decode (src/rate/rate_high.rs:168-247,
// src/rate/rate_low.rs:168-247), all in HBM:
//   e     = eval_poly(erasure vector)                       (3 small kernels)
//   z     = IFFT_low(received * e)                          (pass 1, contiguous)
//   u     = FFT_high((I + H) IFFT_high(z))                  (pass 2, strided)
//   y     = u + L z,  out = reveal(FFT_low(y))              (pass 3, contiguous)
// where the formal derivative FD = I + L + H is split into its low-bit part L
// and high-bit part H (L commutes with the high-bit layers and
// FFT_high o IFFT_high = I), so no separate derivative pass is needed.
int rs16_engine::decode_fused(const DecodeGeom& g, size_t S, const DecodeSegs& v, uint8_t* Z, uint8_t* U,
                              hipStream_t s, rs16_error* err) {
    DecodePlan plan;
    if (int rc = decode_eval(g, v.fl_a, v.fl_b, ev_main, &plan, s, err, S)) return rc;
    return decode_passes(g, S, v, Z, U, plan, (uint32_t*)ev_main.rcount.p, 1, s, err);
}

int rs16_engine::guard_eval(hipStream_t s, bool consume, rs16_error* err) {
    if (!prep_pending) return RS16_OK;
    RS16_HIP(hipStreamWaitEvent(s, prep_ev, 0));
    prep_pending = false;
    if (!consume) prep.valid = false;
    return RS16_OK;
}

// Erasure logs e = eval_poly(erasure vector) into ev.elog (2-3 small kernels);
// *plan: what the passes that follow need to know of it.
int rs16_engine::decode_eval(const DecodeGeom& g, const uint8_t* flags_a, const uint8_t* flags_b, EvalBufs& ev,
                             DecodePlan* plan, hipStream_t s, rs16_error* err, size_t S, size_t nstripes,
                             uint32_t vary, size_t bs_fa, size_t bs_fb, bool prepare) {
    // (a prepared decode's outputs in ev_main are about to be overwritten)
    if (&ev == &ev_main && !prepare)
        if (int rc = guard_eval(s, false, err)) return rc;
    // Any evaluation other than the preparation itself drops the preparation,
    // whichever buffers it writes to (the pipelined host path's lanes use
    // their own).  A contract of the split decode (include/rs16.h), no longer
    // a necessity: the preparation's plan is a value of its own.
    if (!prepare) prep.valid = false;
    const size_t nv = vary > 1 ? vary : 1;
    RS16_HIP(ev.work32.reserve(nv * VARY_WORK * 4));
    RS16_HIP(ev.elog.reserve(nv * VARY_WORK * 4));
    RS16_HIP(ev.zflag.reserve(nv * VARY_ZFLAGS));
    RS16_HIP(ev.rbits.reserve(nv * VARY_RBITS * 4));
    RS16_HIP(ev.lost.reserve(nv * VARY_LOST * 4));
    RS16_HIP(ev.rcount.reserve(GF_ORDER / 64 * 8));
    DecodePlan& p = *plan = DecodePlan{};
    p.ev = &ev;
    p.var_ns = vary > 1 ? vary : 0;
    p.var_bs_fa = vary > 1 ? bs_fa : 0;
    p.var_bs_fb = vary > 1 ? bs_fb : 0;
    ErasureSpec es{};
    es.flags_a = flags_a;
    es.flags_b = flags_b;
    es.a_count = g.a_count;
    es.chunk = g.chunk;
    es.b_count = g.b_count;
    es.pad_fill = g.high ? 1 : 0;
    es.tail_fill = g.high ? 0 : 1;
    // the pass metadata: received bitmap, and zero flags of the first pass's
    // tiles (2^lo rows, lo = L/2) when the decode takes more than one pass
    const int L = ilog2(g.n);
    es.rbits = (uint32_t*)ev.rbits.p;
    es.zflags = L > 8 ? (uint8_t*)ev.zflag.p : nullptr;
    es.n = g.n;
    es.zlo = (uint32_t)(L / 2);
    // the lost originals' row range prunes the general multi-pass decode
    // (the half-transform decode restores every original: not needed)
    const bool prune = !half_decode(g) && L > 8;
    es.lostpart = prune ? (uint32_t*)ev.lost.p : nullptr;
    es.lostrange = prune ? (uint32_t*)ev.lost.p + 512 : nullptr;
    es.orig_b = g.high ? 1 : 0;
    es.lost_all = g.repair ? 1 : 0;  // (the repair stores the lost rows of both segments)
    es.wanted = g.select ? g.wanted : nullptr;  // (the selective decode: the interval of the wanted rows)
    es.rcount = (uint32_t*)ev.rcount.p;
    es.diag = (uint32_t)diag;
    last_dec = g;
    last_dec_valid = true;
    if (p.var_ns) {
        // every stripe's own metadata; no received counts (rs16_decode_check
        // covers the single-pattern calls)
        es.nstripes = p.var_ns;
        es.bs_fa = p.var_bs_fa;
        es.bs_fb = p.var_bs_fb;
        es.bs_work = es.bs_elog = VARY_WORK;
        es.bs_rbits = VARY_RBITS;
        es.bs_zflags = VARY_ZFLAGS;
        es.bs_lost = VARY_LOST;
        es.rcount = nullptr;
        last_dec_valid = false;
    }
    // A whole-half erasure: every log is 0, nothing to evaluate (the passes
    // count the received rows for rs16_decode_check)
    p.ident = identity_logs(g, vary);
    if (p.ident) return RS16_OK;
    // High-rate half decodes of 2^9 / 2^10-row halves through the column
    // codec: it evaluates the polynomial itself (an n-point XOR convolution,
    // rs16_col.hip) and writes rcount; no kernel here.
    // (the repair takes the pass codec at every size: COL_DEC_GEN restores originals only)
    p.eval_in_col = S && !g.repair && (half_decode(g) ? g.high && col_ok(ilog2(g.n) - 1, S, nstripes)
                                                      : col_ok(ilog2(g.n), S, nstripes, true));
    if (p.eval_in_col) return RS16_OK;
    // The decode passes that read erasure logs finish eval_poly's last
    // 256-point FWHT themselves, for the 256-row block of their tile's rows
    // (one kernel less) -- except the one-pass half-transform decode, whose
    // gather and reveal rows lie in different blocks.
    // (the column codec's half decodes of 2^9 / 2^10 rows finish it too)
    p.elog_fused = !(half_decode(g) && ilog2(g.n) - 1 <= 8);
    uint32_t *work = (uint32_t*)ev.work32.p, *elog = (uint32_t*)ev.elog.p;
    return profiled(PROF_EVAL_POLY, s, err, [&](uint64_t* stamps) {
        es.stamps = stamps;
        // (the form -- small, fused, two-kernel -- is the launcher's choice, rs16_eval.hip)
        return launch_eval_poly_from_flags(es, work, elog, d_log_walsh.as<uint16_t>(), s, !p.elog_fused);
    });
}

// Half-transform decode.  When every original is lost and the originals'
// segment is one half of the n work rows (high rate: rows [n/2, n) with
// n = 2 chunk; low rate: rows [0, n/2)), the input of the transform is zero
// on that half and only that half of its output is needed.  Then the top
// layer's butterflies and every formal-derivative term cancel on the needed
// half (see DESIGN.md "Half-transform decode"; checked against the
// sequential oracle by tests/test_half_decode.py):
//     FFT(FD(IFFT(x)))[dst half] = FFT_dst(IFFT_src(x[src half]))
// with IFFT_src / FFT_dst the n/2-row transforms over the low L-1 row bits
// with the twiddles of their half (skew_delta = its first row).  So the
// decode is an encode-shaped pipeline on n/2 rows: gather x e -> IFFT ->
// FFT -> reveal, with no formal derivative.
bool rs16_engine::half_decode(const DecodeGeom& g) {
    if (g.repair) return false;  // (a lost recovery shard: the other half's input is not whole, DecodeGeom::repair)
    if (g.select) return false;  // (the half pipelines store every original, DecodeGeom::select)
    const bool orig_lost = g.high ? g.b_recv == 0 : g.a_recv == 0;
    return orig_lost && g.n >= 2 && g.n == 2 * (size_t)g.chunk;
}

// Identity multipliers.  When the erased rows are exactly one half of the n
// = 2^(L+1) work rows and the other half is received whole (k = m = n / 2,
// every original lost, every recovery shard received; the low rate adds the
// tail [n, 65536), rate_low.rs:183-197), the erasure log of every work row,
// eval_poly(e)[i] = sum_{j erased} log(i ^ j) mod 65535 (src/engine.rs:207-218
// as an XOR convolution with H(LogWalsh) = log), is the log of the
// subspace polynomial of the erased half at i: 0 for every i (the Cantor
// basis normalizes it to 1 on the complementary coset; checked against the
// oracle for every L in tests/test_eval_identity.py).  Then "MULTIPLY
// SHARDS" (rate_high.rs:203-228) and REVEAL ERASURES (:236-242) multiply by
// exp(0) = 1 and exp(65535) = 1: the passes take the rows as they are.  Only
// the pass form of the half decode (halves of 2^11 rows and more) uses it;
// the counts the caller gave pick it, as they pick the half decode.
bool rs16_engine::identity_logs(const DecodeGeom& g, uint32_t vary) const {
    if ((diag & DIAG_NO_IDENTITY) || vary > 1 || !half_decode(g) || ilog2(g.n) - 1 < 11) return false;
    if (g.a_count != g.chunk || g.b_count != g.chunk) return false;
    return g.high ? g.a_recv == g.a_count : g.b_recv == g.b_count;
}

int rs16_engine::mid_tables(int L, const uint32_t** out, rs16_error* err) {
    DevBuf& b = mid_tab[L];
    if (!b.p) {
        const HostTables& t = host_tables();
        const std::vector<uint32_t> ent = mid_matrix_entries(t, L);
        std::vector<uint32_t> tabs(ent.size() * 20);
        for (size_t i = 0; i < ent.size(); i++)
            std::copy_n(&t.mul_tab[(size_t)ent[i] * TAB_DWORDS], 20, &tabs[i * 20]);
        DevBuf up;  // (the member only once the table is whole)
        RS16_HIP(up.reserve(tabs.size() * 4));
        RS16_HIP(hipMemcpy(up.p, tabs.data(), tabs.size() * 4, hipMemcpyHostToDevice));
        b = std::move(up);
    }
    *out = (const uint32_t*)b.p;
    return RS16_OK;
}

// The pass sequence of a decode, given the plan of its decode_eval and what that
// left in the plan's buffers: elog / work32 (erasure logs), rbits (received
// rows) and zflag (zero tiles).
int rs16_engine::decode_passes(const DecodeGeom& g, size_t S, const DecodeSegs& v, uint8_t* Z, uint8_t* U,
                               const DecodePlan& plan, uint32_t* rcount, size_t nst, hipStream_t s, rs16_error* err) {
    const EvalBufs& ev = *plan.ev;
    PassArgs a = base_args(this, S);
    a.S_seg = a.S_rest = v.S_user;
    a.seg_a = v.seg_a;
    a.seg_b = v.seg_b;
    a.flags_a = v.fl_a;
    a.flags_b = v.fl_b;
    a.a_count = g.a_count;
    a.chunk = g.chunk;
    a.b_count = g.b_count;
    a.elog = (const uint32_t*)ev.elog.p;
    a.ework = plan.elog_fused ? (const uint32_t*)ev.work32.p : nullptr;
    a.rest = v.rest;
    a.rest_seg_b = g.high ? 1 : 0;
    a.rbits = (const uint32_t*)ev.rbits.p;
    a.skew_ifft = a.skew_fft = 0;
    if (plan.var_ns) {  // stripes with losses of their own (decode_eval's per-stripe metadata)
        a.bs_fa = plan.var_bs_fa;
        a.bs_fb = plan.var_bs_fb;
        a.bs_elog = VARY_WORK;
        a.bs_rbits = VARY_RBITS;
        a.bs_zflags = VARY_ZFLAGS;
        a.bs_lost = VARY_LOST;
        rcount = nullptr;
    }
    // nst > 1: independent stripes with one erasure pattern (rs16_decode_device_batch):
    // every launch covers all of them (PassArgs::stripe_tiles); stripe i's
    // segments / restored originals at + i bs_a / bs_b / bs_rest, its work
    // rows at Z / U + i n S
    const uint32_t ns = (uint32_t)nst;
    const size_t zs = (size_t)g.n * S;
    a.bs_seg = v.bs_a;
    a.bs_seg_b = v.bs_b;
    a.bs_rest = v.bs_rest;
    a.rest_b = v.rest_b;
    a.bs_rest_b = v.bs_rest_b;
    auto batch = [&](uint32_t tiles, size_t bs_in, size_t bs_in2, size_t bs_out) {
        a.stripe_tiles = ns > 1 ? tiles : 0;
        a.bs_in = bs_in;
        a.bs_in2 = bs_in2;
        a.bs_out = bs_out;
        return tiles * ns;
    };
    // a column launch of the decode: col_args and what the two forms below share
    auto col_dec = [&](const uint8_t* in, size_t bs_in, uint32_t in_rows, uint32_t out_rows, uint32_t src,
                       uint32_t dst) {
        ColArgs c = col_args(in, v.S_user, v.rest, v.S_user, S, in_rows, out_rows, src, dst);
        c.elog = (const uint32_t*)ev.elog.p;
        c.nstripes = ns;
        c.bs_in = bs_in;
        c.bs_out = v.bs_rest;
        c.chunk = g.chunk;
        c.bs_flags_o = plan.var_bs_fb;
        return c;
    };
    const int L = ilog2(g.n);
    if (half_decode(g)) {
        const uint32_t half = g.n / 2, src = g.high ? 0 : half, dst = g.high ? half : 0;
        const uint32_t orig = g.high ? g.b_count : g.a_count;
        a.row_base_in = a.skew_ifft = src;
        a.row_base_out = a.skew_fft = dst;
        const int Lh = L - 1;
        if (plan.ident) {
            // Identity multipliers (identity_logs): gather the received half
            // as it is -> IFFT -> FFT -> its rows are the restored originals,
            // i.e. the encoder's three passes with the half's twiddles; the
            // first and last count the received flags for rs16_decode_check
            const int lo = row_split(Lh).lo, hi = row_split(Lh).hi;
            a.seg_a = g.high ? v.seg_a : v.seg_b;
            a.bs_seg = g.high ? v.bs_a : v.bs_b;
            a.a_count = half;
            a.rcount = rcount;
            a.cnt_flags = g.high ? v.fl_a : v.fl_b;
            a.cnt_base = src;
            a.cnt_seg = g.high ? 0 : 1;
            // (the form of Z between these three passes, as in the encode)
            const ZForm zf = z_form_sequence(half, S, v.S_user, a.a_count, a.chunk, a.row_base_in, diag);
            a.lo = 0;
            a.out = Z;
            z_form_args(a, zf);
            RS16_PASS_AS(PROF_DEC_HALF_FIRST, ENC_FIRST, lo, a, batch(1u << hi, 0, 0, zs), s);
            a.rcount = nullptr;
            a.lo = lo;
            a.in = Z;
            RS16_PASS_AS(PROF_DEC_HALF_MID, ENC_MID, hi, a, batch(1u << lo, zs, 0, zs), s);
            a.lo = 0;
            a.out = v.rest;
            a.S_out = v.S_user;
            a.out_rows = orig;
            a.rcount = rcount;
            a.cnt_flags = g.high ? v.fl_b : v.fl_a;
            a.cnt_base = dst;
            a.cnt_seg = g.high ? 1 : 0;
            RS16_PASS_AS(DEC_HALF_LAST, ENC_LAST, lo, a, batch((orig + (1u << lo) - 1) >> lo, zs, 0, v.bs_rest), s);
            return RS16_OK;
        }
        // 2^6 .. 2^10-row halves: the whole decode in one launch (rs16_col.hip)
        // -- high rate with the polynomial in the kernel; the low rate from
        // 2^9 rows on, on eval_poly's output
        const bool col_eval = plan.eval_in_col && g.high;
        if (!col_eval && Lh <= 8) {
            a.ework = nullptr;  // (decode_eval did the whole eval_poly)
            RS16_PASS(DEC_HALF_SINGLE, Lh, a, batch(1, 0, 0, 0), s);
            return RS16_OK;
        }
        if (col_eval || col_ok(Lh, S, ns)) {
            ColArgs c = g.high ? col_dec(v.seg_a, v.bs_a, g.a_count, orig, src, dst)
                               : col_dec(v.seg_b, v.bs_b, g.b_count, orig, src, dst);
            c.flags = g.high ? v.fl_a : v.fl_b;
            c.base_in = src;
            c.base_out = dst;
            c.e_pad = 1;  // (high rate: padding rows erased, nothing above the originals)
            c.bs_flags = g.high ? plan.var_bs_fa : plan.var_bs_fb;
            c.bs_elog = plan.var_ns ? VARY_WORK : 0;
            if (col_eval) {
                // eval_poly in the kernel (decode_eval launched nothing)
                c.flags_o = v.fl_b;
                c.o_rows = g.b_count;
                c.vtab = nullptr;  // (col(): d_col_v + col_v_offset(2^(L+1)))
                c.rcount = rcount;
                return col(c, Lh, COL_DEC_EVAL, s, err);
            }
            c.elog = (const uint32_t*)ev.work32.p;  // (eval_poly without its last H_lo: plan.elog_fused)
            return col(c, Lh, COL_DEC_EWORK, s, err);
        }
        const int lo = row_split(Lh).lo, hi = row_split(Lh).hi;
        // (form 0 throughout: this ENC_MID reads the rows a decoder pass wrote)
        a.lo = 0;
        a.out = Z;
        RS16_PASS_AS(PROF_DEC_HALF_FIRST, DEC_FIRST, lo, a, batch(1u << hi, 0, 0, zs), s);
        a.lo = lo;
        a.in = Z;
        RS16_PASS_AS(PROF_DEC_HALF_MID, ENC_MID, hi, a, batch(1u << lo, zs, 0, zs), s);
        a.lo = 0;
        a.out = nullptr;
        RS16_PASS(DEC_HALF_LAST, lo, a, batch((orig + (1u << lo) - 1) >> lo, zs, 0, 0), s);
        return RS16_OK;
    }
    if (plan.eval_in_col) {
        // up to 2^11 work rows: the whole general decode in one launch,
        // polynomial and formal derivative in the kernel (rs16_col.hip);
        // segment A / B = recovery / originals (high rate) or originals /
        // recovery (low rate, rate_low.rs:168-247)
        ColArgs c = col_dec(v.seg_a, v.bs_a, g.a_count, g.high ? g.b_count : g.a_count, 0, 0);
        c.flags = v.fl_a;
        c.in_b = v.seg_b;
        c.bs_in_b = v.bs_b;
        c.flags_o = v.fl_b;
        c.o_rows = g.b_count;
        c.rev_a = g.high ? 0 : 1;
        c.e_pad = g.high ? 1 : 0;
        c.e_tail = g.high ? 0 : 1;
        c.e_k = g.high ? 0 : host_tables().col_k[L];
        c.rcount = rcount;
        c.bs_flags = plan.var_bs_fa;
        c.wanted = g.select ? g.wanted : nullptr;  // (lost[] = lost and wanted; the polynomial follows the flags)
        return col(c, L, g.select ? COL_DEC_GEN_SEL : COL_DEC_GEN, s, err);
    }
    a.wanted = g.select ? g.wanted : nullptr;  // (read by the select programs alone)
    if (L <= 8) {
        RS16_PASS(g.repair ? DEC_SINGLE_ALL : (g.select ? DEC_SINGLE_SEL : DEC_SINGLE), L, a, batch(1, 0, 0, 0), s);
        return RS16_OK;
    }
    const int lo = L / 2, hi = L - lo;
    // One flag per DEC_FIRST tile (2^hi <= 256): tiles without a received
    // row are skipped by DEC_FIRST and read as zero by DEC_MID / DEC_LAST.
    a.zflags = (const uint8_t*)ev.zflag.p;
    a.lostrange = (const uint32_t*)ev.lost.p + 512;  // (written by decode_eval)
    // Launch only the tiles that can hold a received row: a segment with no
    // received shard contributes none (its tiles are flagged by block 0).
    const uint32_t tile = 1u << lo, ntiles = 1u << hi;
    uint32_t t0z = ntiles, t1z = 0;
    if (g.a_recv) t0z = 0, t1z = (g.a_count + tile - 1) / tile;
    if (g.b_recv) {
        t0z = std::min(t0z, g.chunk / tile);
        t1z = std::max(t1z, std::min(ntiles, (uint32_t)(((size_t)g.chunk + g.b_count + tile - 1) / tile)));
    }
    if (t1z <= t0z) t0z = 0, t1z = 1;  // (unreachable: a decode has received shards) keep one launch
    a.tile_base = t0z;
    a.lo = 0;
    a.out = Z;
    RS16_PASS(DEC_FIRST, lo, a, batch(t1z - t0z, 0, 0, zs), s);
    a.tile_base = 0;
    if (g.repair) {
        // The repair: the last pass's tiles of both segments are consumed, so
        // DEC_MID keeps the U rows of tiles [0, end of segment B) (narrowed on
        // the device by the lost rows' interval, lostrange -- of both segments,
        // ErasureSpec::lost_all); no direct middle pass, no tile_last kernel
        // (mid_direct = tl_max = 0).  The last pass is DEC_LAST_ALL over the
        // tiles of both segments (repair_tiles); each workgroup returns at
        // once when its tile holds no lost row.
        const RepairTiles rt = repair_tiles(g);
        a.lo = lo;
        a.in = Z;
        a.out = U;
        a.need_lo = 0;
        a.need_hi = rt.b_first + rt.b_tiles;
        RS16_PASS(DEC_MID, hi, a, batch(1u << lo, zs, 0, zs), s);
        a.need_lo = a.need_hi = 0;
        a.lo = 0;
        a.in = Z;
        a.in2 = U;
        a.out = nullptr;
        if (rt.a_tiles) RS16_PASS(DEC_LAST_ALL, lo, a, batch(rt.a_tiles, zs, zs, 0), s);
        a.tile_base = rt.b_first;
        RS16_PASS(DEC_LAST_ALL, lo, a, batch(rt.b_tiles, zs, zs, 0), s);
        return RS16_OK;
    }
    // Only tiles that contain original rows are needed in the last pass,
    // so DEC_MID computes and stores only U rows of those tiles (its tile
    // row k is row bits [lo, L) = the last pass's tile index).
    const uint32_t ob = g.high ? g.chunk : 0;
    const uint32_t oc = g.high ? g.b_count : g.a_count;
    const uint32_t t0 = ob >> lo, t1 = (uint32_t)(((size_t)ob + oc + ((size_t)1 << lo) - 1) >> lo);
    a.lo = lo;
    a.in = Z;
    a.out = U;
    a.need_lo = t0;
    a.need_hi = t1;
    // (the selective decode: the lost originals of the read set stand for the
    // lost ones in both gates below; the device decides by lostrange, which the
    // eval kernels took over the same rows)
    const size_t lost = g.select ? g.wanted_count
                                 : (g.high ? (size_t)g.b_count - g.b_recv : (size_t)g.a_count - g.a_recv);
    // Few lost originals: the middle pass's consumed rows may be few enough
    // for the direct product (mid_direct_kernel; DEC_MID then returns for
    // the stripes it covered -- decided on the device from lostrange)
    // (grid z = the stripe: at most 65535 of them in one launch)
    if (!(diag & DIAG_NO_MID_DIRECT) && lost <= ((size_t)MID_DIRECT_MAX << lo) && ns <= 65535) {
        const uint32_t* mt = nullptr;
        if (int rc = mid_tables(L, &mt, err)) return rc;
        batch(1u << lo, zs, 0, zs);  // (stripe displacements of the launch)
        if (int rc = profiled(PROF_DEC_MID_DIRECT, s, err, [&](uint64_t* stamps) {
                a.stamps = stamps;
                const hipError_t e = launch_mid_direct(a, mt, (uint32_t)hi, ns, s);
                a.stamps = nullptr;
                return e;
            }))
            return rc;
        a.mid_direct = MID_DIRECT_MAX;
    }
    RS16_PASS(DEC_MID, hi, a, batch(1u << lo, zs, 0, zs), s);
    a.mid_direct = 0;
    a.need_lo = a.need_hi = 0;
    a.lo = 0;
    a.in = Z;
    a.in2 = U;
    a.out = nullptr;
    a.tile_base = t0;
    // Lost originals in few tiles (lost-range pruning leaves a handful of
    // tiles to this pass): one wave per quad column of each tile
    // (tile_last_kernel) instead of one 8-wave item per 32 quads, whose
    // latency was the pass.  Over more tiles the items win (scattered
    // losses: 128 tiles 81 -> 37 us; break-even 16-32 tiles,
    // scripts/probe_general.py).  How many tiles the lost originals span is
    // known on the device only (lostrange): with <= 2048 lost both kernels
    // are launched and each returns at once where the other one applies.
    const bool tile_last = lo == 8 && !(diag & DIAG_NO_TILE_LAST) && (lost <= 2048 || (diag & DIAG_TILE_LAST));
    if (tile_last) {
        a.tl_max = (diag & DIAG_TILE_LAST) ? (1u << hi) : TILE_LAST_MAX;
        // (the grid: tl_max tiles from the first lost original's, the kernel
        // reads that tile from lostrange; a launch that returns at once costs
        // per workgroup)
        const uint32_t tiles = batch(std::min(t1 - t0, a.tl_max), zs, zs, 0);
        if (int rc = profiled(g.select ? PROF_DEC_TILE_LAST_SEL : PROF_DEC_TILE_LAST, s, err, [&](uint64_t* stamps) {
                a.stamps = stamps;
                const hipError_t e = g.select ? launch_tile_last_sel(a, tiles, s) : launch_tile_last(a, tiles, s);
                a.stamps = nullptr;
                return e;
            }))
            return rc;
        if (diag & DIAG_TILE_LAST) return RS16_OK;  // (every span is tile_last's)
    }
    RS16_PASS(g.select ? DEC_LAST_SEL : DEC_LAST, lo, a, batch(t1 - t0, zs, zs, 0), s);
    return RS16_OK;
}

// The FFT half of the multi-chunk encoders: FFT of nch chunks of Z (batched
// like the IFFTs below, skew_delta applied to absolute rows), recovery rows
// [0, m) stored to d_rec.
int rs16_engine::fft_to_recovery(const EncodeForm& f, size_t m, size_t S, size_t S_user, const uint8_t* src,
                                 uint8_t* Z, uint8_t* d_rec, uint32_t nch, uint32_t skew, hipStream_t s,
                                 rs16_error* err, const VerifySink* vs) {
    const size_t chunk = f.chunk;
    const int lo = f.lo, hi = f.hi;
    PassArgs a = base_args(this, S);
    a.skew_fft = skew;
    // src != Z: every chunk's FFT reads the one chunk at src (the first pass only)
    const uint32_t mask = src != Z ? (uint32_t)(chunk - 1) : 0u;
    a.in = src;
    a.in_rows_mask = mask;
    if (hi) {
        a.out = Z;
        a.lo = lo;
        RS16_PASS(GEN_FFT, hi, a, nch << lo, s);
        a.in = Z;
        a.in_rows_mask = 0;
    }
    a.out = d_rec;
    a.S_out = S_user;
    a.lo = 0;
    a.out_rows = (uint32_t)m;
    if (vs) sink_args(a, *vs);
    RS16_PASS(vs ? ENC_LAST_VFY : ENC_LAST, lo, a, (uint32_t)((m + ((size_t)1 << lo) - 1) >> lo), s);
    return RS16_OK;
}

// HighRateEncoder::encode with more originals than one chunk
// (src/rate/rate_high.rs:44-83): IFFT of every chunk c of the zero-padded
// originals with skew_delta = c chunk + chunk (pos = c chunk), XOR of all of
// them into chunk 0 (xor_within, :56-74), FFT of chunk 0 with skew 0.  The
// twiddle of a layer at relative row r is skew[r + skew_delta + d - 1] =
// skew[(c chunk + r) + chunk + d - 1]: the per-chunk transforms are one
// transform over absolute rows with skew_delta = chunk whose layers stay
// inside a chunk, so every chunk's IFFT runs in the same launches (tiles over
// all chunks; the first pass gathers the originals, rows >= k read as zero),
// then one XOR reduction, then the FFT.
int rs16_engine::encode_high_multi(const EncodeForm& f, size_t k, size_t m, size_t S, size_t S_user,
                                   const uint8_t* d_orig, uint8_t* d_rec, uint8_t* Z, hipStream_t s, rs16_error* err,
                                   const VerifySink* vs) {
    const size_t chunk = f.chunk;
    const uint32_t nch = f.nch;
    const int L = f.L, lo = f.lo, hi = f.hi;
    // (a verify sink: the passes only -- none of the forms before them)
    if (vs && !f.verify_fusable()) return set_error(err, RS16_INVALID_ARGUMENT);
    if (f.kind == f.ROWS) {  // one-row chunks: the single recovery row is the XOR of the originals
        if (Z != d_orig) RS16_HIP(hipMemcpy2DAsync(Z, S, d_orig, S_user, S, k, hipMemcpyDeviceToDevice, s));
        RS16_HIP(launch_xor_chunks(Z, S, nch, s));
        if (d_rec != Z) RS16_HIP(hipMemcpyAsync(d_rec, Z, S, hipMemcpyDeviceToDevice, s));
        return RS16_OK;
    }
    if (f.kind == f.COLM) return col_multi(k, m, S, S_user, d_orig, d_rec, nch, true, s, err);
    if (f.kind == f.COL_CHUNKS) {
        // 256 / 512 / 1024-row chunks: every chunk's IFFT into Z (one
        // workgroup per quad column and chunk), then the FFT of their XOR
        ColArgs c = col_args(d_orig, S_user, Z, S, S, k, nch * chunk, chunk, 0);
        c.nch = nch;
        if (int rc = col(c, L, COL_ENC_IFFT, s, err)) return rc;
        c = col_args(Z, S, d_rec, S_user, S, nch * chunk, m, 0, 0);
        c.nch = nch;
        return col(c, L, COL_ENC_FFTX, s, err);
    }
    PassArgs a = base_args(this, S);
    a.seg_a = d_orig;
    a.S_seg = S_user;
    a.a_count = (uint32_t)k;
    a.skew_ifft = (uint32_t)chunk;
    a.out = Z;
    a.lo = 0;
    RS16_PASS(ENC_FIRST, lo, a, nch << hi, s);
    if (hi) {
        a.in = a.out = Z;
        a.lo = lo;
        RS16_PASS(GEN_IFFT, hi, a, nch << lo, s);
    }
    RS16_HIP(launch_xor_chunks(Z, chunk * S, nch, s));
    return fft_to_recovery(f, m, S, S_user, Z, Z, d_rec, 1, 0, s, err, vs);
}

// LowRateEncoder::encode (src/rate/rate_low.rs:44-83): IFFT of the
// zero-padded originals (one chunk, skew 0), copied into every recovery chunk
// c, FFT of each with skew_delta = c chunk + chunk -- batched as above
// (absolute rows, skew_delta = chunk), recovery = rows [0, m).  The copies
// are not made: the transformed chunk goes to the scratch U and the FFT's
// first pass reads it for every chunk (PassArgs::in_rows_mask).
int rs16_engine::encode_low_multi(const EncodeForm& f, size_t k, size_t m, size_t S, size_t S_user,
                                  const uint8_t* d_orig, uint8_t* d_rec, uint8_t* Z, uint8_t* U, hipStream_t s,
                                  rs16_error* err, const VerifySink* vs) {
    const size_t chunk = f.chunk;
    const uint32_t nch = f.nch;
    const int L = f.L, lo = f.lo, hi = f.hi;
    // (a verify sink: the passes only -- none of the forms before them)
    if (vs && !f.verify_fusable()) return set_error(err, RS16_INVALID_ARGUMENT);
    if (f.kind == f.ROWS) {  // one original: every transform is the identity, every recovery row a copy
        if (Z != d_orig) RS16_HIP(hipMemcpyAsync(Z, d_orig, S, hipMemcpyDeviceToDevice, s));
        RS16_HIP(launch_copy_chunks(Z, S, nch, s));
        if (d_rec != Z) RS16_HIP(hipMemcpy2DAsync(d_rec, S_user, Z, S, S, m, hipMemcpyDeviceToDevice, s));
        return RS16_OK;
    }
    // one recovery chunk of 512 / 1024 rows: one launch (rs16_col.hip)
    if (f.kind == f.COL) return col(col_args(d_orig, S_user, d_rec, S_user, S, k, m, 0, chunk), L, COL_ENC, s, err);
    if (f.kind == f.COLM) return col_multi(k, m, S, S_user, d_orig, d_rec, nch, false, s, err);
    if (f.kind == f.COL_CHUNKS) {
        // 256 / 512 / 1024-row chunks: one launch, one workgroup per (quad
        // column, recovery chunk), each running the originals' IFFT itself.
        // Every chunk's workgroups read the originals, and chunk 0's write
        // recovery rows [0, chunk): when the two arrays overlap (the Rate
        // API's work buffer, rate_low.rs:44-83) chunk 0 could overwrite
        // originals other chunks have not loaded yet, so the originals are
        // read from a copy in U then (U: next_pow2(k) rows, pitch S).
        const uint8_t* src = d_orig;
        size_t s_in = S_user;
        const uint8_t *o0 = d_orig, *o1 = d_orig + (k - 1) * S_user + S;
        const uint8_t *r0 = d_rec, *r1 = d_rec + (m - 1) * S_user + S;
        if (o0 < r1 && r0 < o1) {
            if (!U) return set_error(err, RS16_INVALID_ARGUMENT);
            RS16_HIP(hipMemcpy2DAsync(U, S, d_orig, S_user, S, k, hipMemcpyDeviceToDevice, s));
            src = U;
            s_in = S;
        }
        ColArgs c = col_args(src, s_in, d_rec, S_user, S, k, m, 0, chunk);
        c.nch = nch;
        return col(c, L, COL_ENC, s, err);
    }
    // U belongs to the caller's stream (no engine-wide fallback: two calls
    // on concurrent streams sharing one buffer restored wrong data, round 3)
    if (!U) return set_error(err, RS16_INVALID_ARGUMENT);
    PassArgs a = base_args(this, S);
    a.seg_a = d_orig;
    a.S_seg = S_user;
    a.a_count = (uint32_t)k;
    a.skew_ifft = 0;
    a.out = U;
    a.lo = 0;
    RS16_PASS(ENC_FIRST, lo, a, 1u << hi, s);
    if (hi) {
        a.in = a.out = U;
        a.lo = lo;
        RS16_PASS(GEN_IFFT, hi, a, 1u << lo, s);
    }
    return fft_to_recovery(f, m, S, S_user, U, Z, d_rec, nch, (uint32_t)chunk, s, err, vs);
}
