// rs16_api.cpp -- C ABI (include/rs16.h): errors, the test hooks, rate
// selection, engine lifecycle, engine ops, diagnostics and the memory / stream
// helpers.  The rest of the C ABI: rs16_api_coders.cpp (rs16_encoder /
// rs16_decoder), rs16_api_device.cpp and rs16_api_host.cpp (the one-shot
// codec on device / host shards), rs16_api_update.cpp (the delta update).
#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>
#include <rccl/rccl.h>

#include <cstdio>

#include "rs16_api.hpp"
#include "rs16_pass_common.hpp"

using namespace rs16;

// ---------------------------------------------------------------------------
// Errors -- Display of src/lib.rs:130-222.
// ---------------------------------------------------------------------------
extern "C" size_t rs16_error_message(const rs16_error* e, char* buf, size_t len) {
    char tmp[256];
    unsigned long long a = e->v0, b = e->v1, c = e->v2;
    switch (e->code) {
    case RS16_OK: snprintf(tmp, sizeof tmp, "ok"); break;
    case RS16_DIFFERENT_SHARD_SIZE:
        snprintf(tmp, sizeof tmp, "different shard size: expected %llu bytes, got %llu bytes", a, b);
        break;
    case RS16_DUPLICATE_ORIGINAL_SHARD_INDEX: snprintf(tmp, sizeof tmp, "duplicate original shard index: %llu", a); break;
    case RS16_DUPLICATE_RECOVERY_SHARD_INDEX: snprintf(tmp, sizeof tmp, "duplicate recovery shard index: %llu", a); break;
    case RS16_INVALID_ORIGINAL_SHARD_INDEX:
        snprintf(tmp, sizeof tmp, "invalid original shard index: %llu >= original_count %llu", b, a);
        break;
    case RS16_INVALID_RECOVERY_SHARD_INDEX:
        snprintf(tmp, sizeof tmp, "invalid recovery shard index: %llu >= recovery_count %llu", b, a);
        break;
    case RS16_INVALID_SHARD_SIZE:
        snprintf(tmp, sizeof tmp, "invalid shard size: %llu bytes (must non-zero and multiple of 64)", a);
        break;
    case RS16_NOT_ENOUGH_SHARDS:
        snprintf(tmp, sizeof tmp, "not enough shards: %llu original + %llu recovery < %llu original_count", b, c, a);
        break;
    case RS16_TOO_FEW_ORIGINAL_SHARDS:
        snprintf(tmp, sizeof tmp, "too few original shards: got %llu shards while original_count is %llu", b, a);
        break;
    case RS16_TOO_MANY_ORIGINAL_SHARDS:
        snprintf(tmp, sizeof tmp, "too many original shards: got more than original_count (%llu) shards", a);
        break;
    case RS16_UNSUPPORTED_SHARD_COUNT:
        snprintf(tmp, sizeof tmp, "unsupported shard count: %llu original shards with %llu recovery shards", a, b);
        break;
    case RS16_DEVICE_ERROR:
        // v0 = hipError_t, or 1000 + ncclResult_t for an RCCL call (rs16_comm.cpp)
        if (a >= 1000)
            snprintf(tmp, sizeof tmp, "device error: RCCL: %s", ncclGetErrorString((ncclResult_t)(a - 1000)));
        else
            snprintf(tmp, sizeof tmp, "device error: %s", hipGetErrorString((hipError_t)a));
        break;
    case RS16_INVALID_ARGUMENT: snprintf(tmp, sizeof tmp, "invalid argument"); break;
    default: snprintf(tmp, sizeof tmp, "unknown error %d", e->code); break;
    }
    size_t n = strlen(tmp);
    if (buf && len) {
        size_t c2 = std::min(n, len - 1);
        memcpy(buf, tmp, c2);
        buf[c2] = 0;
    }
    return n;
}

template <class F> static void host_mul_table(const void* in, void* out, size_t bytes, const uint32_t* t, F mul) {
    const uint8_t* src = (const uint8_t*)in;
    uint8_t* dst = (uint8_t*)out;
    for (size_t q = 0; q < bytes / 8; q++) {
        const size_t off = (q >> 3) * 64 + (q & 7) * 4;
        uint32_t yl, yh, ol = 0, oh = 0;
        memcpy(&yl, src + off, 4);
        memcpy(&yh, src + off + 32, 4);
        mul(ol, oh, yl, yh, t);
        memcpy(dst + off, &ol, 4);
        memcpy(dst + off + 32, &oh, 4);
    }
}
template <class Mul> static void host_mul(const void* in, void* out, size_t bytes, uint16_t log_m, Mul mul) {
    host_mul_table(in, out, bytes, &host_tables().mul_tab[(size_t)log_m * TAB_DWORDS], mul);
}
extern "C" void rs16_host_mul(const void* in, void* out, size_t bytes, uint16_t log_m) {
    host_mul(in, out, bytes, log_m, mul_xor);
}
extern "C" void rs16_host_mul_narrow(const void* in, void* out, size_t bytes, uint16_t log_m) {
    host_mul(in, out, bytes, log_m, mul_xor_narrow);
}
extern "C" uint32_t rs16_host_twiddle(uint32_t index, uint32_t* log_m, uint32_t* table20) {
    const HostTables& t = host_tables();
    if (index >= GF_MODULUS) return ~0u;
    if (log_m) *log_m = t.skew[index];
    if (table20) memcpy(table20, &t.skew_tab[(size_t)index * TAB_DWORDS], 20 * sizeof(uint32_t));
    // (the sentinel's log 65535 is the log of the element 0: log[0] = 65535, while exp[65535] = exp[0])
    return t.skew[index] == GF_MODULUS ? 0u : t.exp[t.skew[index]];
}
extern "C" int rs16_host_twiddle_narrow(uint32_t index) { return twiddle_narrow(index) ? 1 : 0; }
extern "C" uint64_t rs16_host_fast_div_check(uint32_t divisor, uint32_t n0, uint32_t count, uint32_t step) {
    const FastDiv f = fast_div_of(divisor);
    uint64_t bad = 0;
    for (uint64_t i = 0, n = n0; i < count && n < ((uint64_t)1 << 32); i++, n += step)
        bad += fast_div((uint32_t)n, f.mul, f.one) != (uint32_t)n / divisor;
    return bad;
}

static int host_pass_consts(int prog, int T, uint32_t lo, size_t n, const uint64_t* s_in, const uint64_t* s_out,
                            const uint64_t* s_seg, const uint64_t* s_rest, const uint32_t* qrow, uint32_t chunk,
                            uint32_t row_base_in, uint32_t in_rows_mask, uint32_t a_count, int diag,
                            rs16_pass_consts* out) {
    // (the scrub's programs lie behind the profiling ids, as the repair's and the select's)
    if (prog < 0 || (prog >= NUM_PROGS && !verify_prog(prog)) || T < 0 || T > 8 || !out) return 0;
    const PassKernel& k = pass_kernel_of(prog, T);
    if (!k.fn) return 0;
    PassArgs a{};
    a.lo = lo, a.chunk = chunk, a.row_base_in = row_base_in, a.in_rows_mask = in_rows_mask;
    a.diag = (uint32_t)diag;
    a.a_count = a_count;
    for (size_t i = 0; i < n; i++) {
        a.S_in = s_in[i], a.S_out = s_out[i], a.S_seg = s_seg[i], a.S_rest = s_rest[i], a.qrow = qrow[i];
        const PassConsts c = pass_launch_consts(k, T, a);  // (the function launch_pass calls)
        rs16_pass_consts& o = out[i];
        o.voff32 = c.voff32, o.full_lanes = c.full_lanes, o.nslab = c.nslab;
        o.quads = (uint32_t)k.quads, o.threads = (uint32_t)k.threads;
        o.load_shb = (uint32_t)k.load_shb, o.store_shb = (uint32_t)k.store_shb;
        o.reg_bits = (uint32_t)k.reg_bits, o.row_sets = k.quads >= 64 ? 1u : 64u / (uint32_t)k.quads;
        o.rs_in = c.rs_in, o.rs_seg = c.rs_seg, o.rs_out = c.rs_out;
        o.late_rows = c.late_rows;
    }
    return 1;
}
// (a gather with row limit 0: every wave reads the zero page, none is cut)
extern "C" int rs16_host_pass_consts_many(int prog, int T, uint32_t lo, size_t n, const uint64_t* s_in,
                                          const uint64_t* s_out, const uint64_t* s_seg, const uint64_t* s_rest,
                                          const uint32_t* qrow, uint32_t chunk, uint32_t row_base_in,
                                          uint32_t in_rows_mask, int diag, rs16_pass_consts* out) {
    return host_pass_consts(prog, T, lo, n, s_in, s_out, s_seg, s_rest, qrow, chunk, row_base_in, in_rows_mask, 0, diag,
                            out);
}
extern "C" int rs16_host_pass_consts_rows(int prog, int T, uint32_t lo, uint64_t s_in, uint64_t s_out, uint64_t s_seg,
                                          uint64_t s_rest, uint32_t qrow, uint32_t chunk, uint32_t row_base_in,
                                          uint32_t in_rows_mask, uint32_t a_count, int diag, rs16_pass_consts* out) {
    return host_pass_consts(prog, T, lo, 1, &s_in, &s_out, &s_seg, &s_rest, &qrow, chunk, row_base_in, in_rows_mask,
                            a_count, diag, out);
}
extern "C" int rs16_host_pass_consts(int prog, int T, uint32_t lo, uint64_t s_in, uint64_t s_out, uint64_t s_seg,
                                     uint64_t s_rest, uint32_t qrow, uint32_t chunk, uint32_t row_base_in,
                                     uint32_t in_rows_mask, int diag, rs16_pass_consts* out) {
    return rs16_host_pass_consts_many(prog, T, lo, 1, &s_in, &s_out, &s_seg, &s_rest, &qrow, chunk, row_base_in,
                                      in_rows_mask, diag, out);
}
extern "C" int rs16_host_paired_rows(uint32_t chunk_rows, uint64_t S, uint64_t S_user, uint32_t a_count,
                                     uint32_t seg_chunk, uint32_t row_base_in, int diag) {
    // (the function encode_high_fused and decode_passes call)
    return z_form_sequence(chunk_rows, S, S_user, a_count, seg_chunk, row_base_in, diag) >= Z_PAIRED ? 1 : 0;
}
extern "C" int rs16_host_tower_rows(uint32_t chunk_rows, uint64_t S, uint64_t S_user, uint32_t a_count,
                                    uint32_t seg_chunk, uint32_t row_base_in, int diag) {
    // (the function encode_high_fused and decode_passes call)
    return z_form_sequence(chunk_rows, S, S_user, a_count, seg_chunk, row_base_in, diag) == Z_TOWER ? 1 : 0;
}
extern "C" uint32_t rs16_host_tower_basis(uint32_t i) { return i < 8 ? host_tables().tower_a[i] : ~0u; }
extern "C" void rs16_host_tower_conv(const void* in, void* out, size_t bytes) {
    // (the kernels' code path: B's pools through tower_conv, v_perm emulated)
    TowerB tb;
    memcpy(tb.p, host_tables().tower_b, sizeof tb.p);
    const uint8_t* src = (const uint8_t*)in;
    uint8_t* dst = (uint8_t*)out;
    for (size_t q = 0; q < bytes / 8; q++) {
        const size_t off = (q >> 3) * 64 + (q & 7) * 4;
        uint32_t l, h;
        memcpy(&l, src + off, 4);
        memcpy(&h, src + off + 32, 4);
        tower_conv(l, h, tb);
        memcpy(dst + off, &l, 4);
        memcpy(dst + off + 32, &h, 4);
    }
}
extern "C" int rs16_host_tower_twiddle(uint32_t index, uint32_t* table20) {
    if (index >= GF_MODULUS) return 0;
    if (table20) memcpy(table20, &host_tables().skew_tab_tower[(size_t)index * TAB_DWORDS], 20 * sizeof(uint32_t));
    return 1;
}
// (form: 0 the 12-lookup multiply, 1 the 6-lookup narrow one, 2 the 9-lookup wide one, 3 the wide one with c1 = 1)
static void host_mul_tower(const void* in, void* out, size_t bytes, uint32_t index, int form) {
    const uint32_t* t = &host_tables().skew_tab_tower[(size_t)(index < GF_MODULUS ? index : GF_MODULUS) * TAB_DWORDS];
    if (form == 2) host_mul_table(in, out, bytes, t, mul_xor_tower_wide);
    else if (form == 3) host_mul_table(in, out, bytes, t, mul_xor_tower_beta);
    else host_mul_table(in, out, bytes, t, form == 1 ? mul_xor_tower_narrow : mul_xor);
}
extern "C" void rs16_host_mul_tower(const void* in, void* out, size_t bytes, uint32_t index, int form) {
    host_mul_tower(in, out, bytes, index, form);
}
extern "C" uint64_t rs16_host_tower_sweep(const uint32_t* index, size_t n, int form, const void* in, const void* want,
                                          size_t bytes) {
    // (index i on its own: multiply, convert, compare; the indices shared out over a few threads)
    std::atomic<uint64_t> bad{0};
    std::atomic<size_t> next{0};
    auto work = [&] {
        std::vector<uint8_t> prod(bytes), shard(bytes);
        for (size_t i; (i = next.fetch_add(1)) < n;) {
            host_mul_tower(in, prod.data(), bytes, index[i], form);
            rs16_host_tower_conv(prod.data(), shard.data(), bytes);
            const uint8_t* w = (const uint8_t*)want + i * bytes;
            uint64_t b = 0;
            for (size_t blk = 0; blk < bytes / 64; blk++)
                for (size_t e = 0; e < 32; e++)
                    b += shard[blk * 64 + e] != w[blk * 64 + e] || shard[blk * 64 + 32 + e] != w[blk * 64 + 32 + e];
            bad += b;
        }
    };
    const size_t nthr = std::min<size_t>({n, 16, std::max(1u, std::thread::hardware_concurrency())});
    std::vector<std::thread> thr;
    for (size_t i = 1; i < nthr; i++) thr.emplace_back(work);
    work();
    for (auto& th : thr) th.join();
    return bad.load();
}
extern "C" int rs16_host_update_consts(uint32_t rows, uint64_t shard_bytes, uint32_t n, uint32_t* quads_per_lane,
                                       uint32_t* nslab, uint32_t* rows_per_wave, uint64_t* blocks) {
    // (the checks of rs16_update_device)
    if (shard_bytes == 0 || (shard_bytes & 63) != 0 || shard_bytes / 8 > 0xFFFFFFFFu) return 0;
    UpdateArgs a{};
    a.S = shard_bytes, a.qrow = (uint32_t)(shard_bytes / 8), a.rows = rows;
    uint64_t nb;
    if (!update_launch_consts(a, n, &nb)) return 0;  // (the function launch_update calls)
    if (quads_per_lane) *quads_per_lane = a.quads_per_lane;
    if (nslab) *nslab = a.nslab;
    if (rows_per_wave) *rows_per_wave = a.rows_per_wave;
    if (blocks) *blocks = nb;
    return 1;
}
extern "C" int rs16_host_update_batch_consts(uint32_t rows, uint64_t width, uint32_t n, uint32_t nstripes,
                                             uint32_t out[6]) {
    // (the checks of rs16_update_device_batch)
    if (width == 0 || (width & 63) != 0 || width > 0xFFFFFFFFu || nstripes > 65535 || !out) return 0;
    UpdateBatchArgs a{};
    a.qrow = (uint32_t)(width / 8), a.rows = rows, a.nstripes = nstripes;
    uint64_t nb;
    if (!update_batch_launch_consts(a, n, &nb)) return 0;  // (the function launch_update_batch calls)
    out[0] = a.quads_per_lane, out[1] = a.nslab, out[2] = a.rows_per_wave, out[3] = a.stripes_per_wave;
    out[4] = a.waves, out[5] = (uint32_t)nb;
    return 1;
}

extern "C" int rs16_engine_set_profiling(rs16_engine* e, int enable, rs16_error* err) {
    if (int rc = e->activate(err)) return rc;
    if (int rc = e->prof_collect(err)) return rc;
    e->profiling = enable != 0;
    return set_error(err, RS16_OK);
}
extern "C" int rs16_engine_profile_read(rs16_engine* e, int prog, double* total_ms, uint64_t* launches,
                                        rs16_error* err) {
    if (prog < 0 || prog >= NUM_PROF) return set_error(err, RS16_INVALID_ARGUMENT);
    if (int rc = e->activate(err)) return rc;
    if (int rc = e->prof_collect(err)) return rc;
    if (total_ms) *total_ms = e->prof_ms[prog];
    if (launches) *launches = e->prof_n[prog];
    return set_error(err, RS16_OK);
}
extern "C" void rs16_engine_profile_reset(rs16_engine* e) {
    rs16_error err;
    (void)e->activate(&err);
    (void)e->prof_collect(&err);
    for (int i = 0; i < NUM_PROF; i++) e->prof_ms[i] = 0, e->prof_n[i] = 0;
}
extern "C" int rs16_engine_set_stamps(rs16_engine* e, void* d_buf, int prog, rs16_error* err) {
    if (prog < -1 || prog >= NUM_PROF) return set_error(err, RS16_INVALID_ARGUMENT);
    e->stamp_buf = d_buf;
    e->stamp_prof = prog;
    return set_error(err, RS16_OK);
}
extern "C" int rs16_engine_set_slices(rs16_engine* e, int n, rs16_error* err) {
    if (n < 1 || n > rs16_engine::MAX_SLICES) return set_error(err, RS16_INVALID_ARGUMENT);
    e->slices = n;
    return set_error(err, RS16_OK);
}
// The received counts of the engine's last decode against the device flags
// (the eval_poly kernels count the received rows per 64-row chunk).
extern "C" int rs16_decode_check(rs16_engine* e, void* stream, rs16_error* err) {
    if (!e->last_dec_valid && !e->last_dec_flags_only) return set_error(err, RS16_OK);
    if (int rc = e->activate(err)) return rc;
    RS16_HIP(hipStreamSynchronize(e->pick(stream)));
    const DecodeGeom& g = e->last_dec;
    uint64_t a = 0, b = 0;
    if (e->last_dec_flags_only) {
        // nothing was restored and no kernel counted: count the copy of the
        // flags the decode took (note_flags_only; segment A / B sizes)
        std::vector<uint8_t> f(2 * (size_t)GF_ORDER);
        RS16_HIP(hipMemcpy(f.data(), e->ws_flags.p, f.size(), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < g.a_count; i++) a += f[i] != 0;
        for (uint32_t i = 0; i < g.b_count; i++) b += f[GF_ORDER + i] != 0;
    } else {
        const size_t chunks = ((size_t)g.n + 63) / 64;
        std::vector<uint32_t> c(2 * chunks);
        RS16_HIP(hipMemcpy(c.data(), e->ev_main.rcount.p, c.size() * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < chunks; i++) a += c[2 * i], b += c[2 * i + 1];
    }
    // (orig_recv, rec_recv) as the caller gave them to rs16_decode_device
    const auto want = DecodeSides::by_segment<uint64_t>(g.high, g.a_recv, g.b_recv);
    const auto got = DecodeSides::by_segment<uint64_t>(g.high, a, b);
    if (got != want) return set_error(err, RS16_INVALID_ARGUMENT, got.first, got.second);
    return set_error(err, RS16_OK);
}
static constexpr int DIAG_ALL = DIAG_FORCE_VOFF64 | DIAG_EVAL_TWO_KERNEL | DIAG_EVAL_FULL | DIAG_NO_COLUMN |
                                DIAG_FORCE_COLUMN | DIAG_TILE_LAST | DIAG_NO_TILE_LAST | DIAG_FD_LDS |
                                DIAG_COL_RADIX4 | DIAG_NO_IDENTITY | DIAG_NO_MID_DIRECT | DIAG_WIDE_TWIDDLES |
                                DIAG_NO_LATE_ROWS | DIAG_NO_PAIRED_ROWS | DIAG_NO_TOWER_ROWS |
                                DIAG_NO_FUSED_VERIFY | DIAG_FORCE_FUSED_VERIFY;
extern "C" int rs16_engine_set_diagnostics(rs16_engine* e, int flags) {
    const int old = e->diag;
    e->diag = flags & DIAG_ALL;
    return old;
}
// Deprecated process-wide form (the round-4 ABI): the flags every engine
// created afterwards starts with.  Existing engines keep their own.
static std::atomic<int> g_default_diag{0};
extern "C" int rs16_set_diagnostics(int flags) { return g_default_diag.exchange(flags & DIAG_ALL); }
extern "C" int rs16_prog_count(void) { return NUM_PROF; }
extern "C" const char* rs16_prog_name(int prog) {
    static const char* names[] = {"GEN_FFT",   "GEN_IFFT",   "ENC_FIRST",     "ENC_MID",
                                  "ENC_LAST",  "ENC_SINGLE", "DEC_FIRST",     "DEC_MID",
                                  "DEC_LAST",  "DEC_SINGLE", "DEC_HALF_LAST", "DEC_HALF_SINGLE",
                                  "DEC_HALF_FIRST", "DEC_HALF_MID", "EVAL_POLY", "COL_ENC", "COL_DEC",
                                  "DEC_MID_DIRECT", "DEC_TILE_LAST",
                                  "DEC_LAST_SEL", "DEC_SINGLE_SEL", "DEC_TILE_LAST_SEL", "COL_DEC_SEL",
                                  "ENC_LAST_VFY", "ENC_SINGLE_VFY", "VERIFY_CMP",
                                  "LOCATE_SCAN", "LOCATE_DECIDE", "LOCATE_CONFIRM", "LOCATE_APPLY",
                                  "DEC_LAST_ALL", "DEC_SINGLE_ALL", "REPAIR_COPY"};
    static_assert(sizeof names / sizeof names[0] == NUM_PROF, "profiling names");
    return (prog >= 0 && prog < NUM_PROF) ? names[prog] : "?";
}

extern "C" const char* rs16_version(void) { return "rs16-mi355x 0.1 gfx950 (v_perm GF(2^16) engine)"; }

// ---------------------------------------------------------------------------
// Rates.
// ---------------------------------------------------------------------------
static bool high_supports(size_t k, size_t m) {  // src/rate/rate_high.rs:19-25
    return k > 0 && m > 0 && k < GF_ORDER && m < GF_ORDER && next_pow2(m) + k <= GF_ORDER;
}
static bool low_supports(size_t k, size_t m) {  // src/rate/rate_low.rs:19-25
    return k > 0 && m > 0 && k < GF_ORDER && m < GF_ORDER && next_pow2(k) + m <= GF_ORDER;
}

extern "C" int rs16_use_high_rate(size_t k, size_t m, rs16_error* err) {  // rate_default.rs:15-64
    if (k > GF_ORDER || m > GF_ORDER) return set_error(err, RS16_UNSUPPORTED_SHARD_COUNT, k, m), -1;
    const size_t kp = next_pow2(k), mp = next_pow2(m);
    const size_t smaller = std::min(kp, mp), larger = std::max(k, m);
    if (k == 0 || m == 0 || smaller + larger > GF_ORDER) return set_error(err, RS16_UNSUPPORTED_SHARD_COUNT, k, m), -1;
    set_error(err, RS16_OK);
    if (kp < mp) return 0;
    if (kp > mp) return 1;
    return k <= m ? 1 : 0;
}

extern "C" int rs16_supports(int rate, size_t k, size_t m) {
    if (rate == RS16_RATE_HIGH) return high_supports(k, m);
    if (rate == RS16_RATE_LOW) return low_supports(k, m);
    return rs16_use_high_rate(k, m, nullptr) >= 0;
}

extern "C" int rs16_validate(int rate, size_t k, size_t m, size_t S, rs16_error* err) {  // src/rate.rs:91-106
    if (!rs16_supports(rate, k, m)) return set_error(err, RS16_UNSUPPORTED_SHARD_COUNT, k, m);
    // (from 4 GiB on the kernels' 32-bit stride arithmetic would wrap: not supported)
    if (S == 0 || (S & 63) != 0 || (uint64_t)S >> 32) return set_error(err, RS16_INVALID_SHARD_SIZE, S);
    return set_error(err, RS16_OK);
}

extern "C" size_t rs16_encoder_work_count(int high, size_t k, size_t m) {
    const size_t chunk = high ? next_pow2(m) : next_pow2(k);
    const size_t n = high ? k : m;
    return (n + chunk - 1) / chunk * chunk;
}
extern "C" size_t rs16_decoder_work_count(int high, size_t k, size_t m) {
    return decode_geom(high != 0, k, m).n;
}

int rs16::resolve_rate(int rate, size_t k, size_t m, size_t S, bool* high, rs16_error* err) {
    if (rate == RS16_RATE_DEFAULT) {
        int h = rs16_use_high_rate(k, m, err);
        if (h < 0) return err ? err->code : RS16_UNSUPPORTED_SHARD_COUNT;
        *high = h == 1;
    } else if (rate == RS16_RATE_HIGH || rate == RS16_RATE_LOW) {
        *high = rate == RS16_RATE_HIGH;
    } else {
        return set_error(err, RS16_INVALID_ARGUMENT);
    }
    return rs16_validate(*high ? RS16_RATE_HIGH : RS16_RATE_LOW, k, m, S, err);
}
int rs16::check_received(size_t k, size_t orig_recv, size_t rec_recv, rs16_error* err) {
    if (orig_recv + rec_recv < k) return set_error(err, RS16_NOT_ENOUGH_SHARDS, k, orig_recv, rec_recv);
    return RS16_OK;
}

// ---------------------------------------------------------------------------
// Engine.
// ---------------------------------------------------------------------------
extern "C" rs16_engine* rs16_engine_new(int device, rs16_error* err) { return rs16_engine_new_ex(device, 0, err); }

extern "C" rs16_engine* rs16_engine_new_ex(int device, int flags, rs16_error* err) {
    if (flags & ~RS16_ENGINE_OWN_QUEUE) return set_error(err, RS16_INVALID_ARGUMENT), nullptr;
    int ndev = 0;
    hipError_t he = hipGetDeviceCount(&ndev);
    if (he != hipSuccess) return hip_fail(err, he), nullptr;
    if (device < 0 || device >= ndev) return set_error(err, RS16_INVALID_ARGUMENT), nullptr;
    rs16_engine* e = new (std::nothrow) rs16_engine();
    if (!e) return set_error(err, RS16_INVALID_ARGUMENT), nullptr;
    e->device = device;
    e->diag = g_default_diag.load();
    e->flags = flags;
    if (e->upload_tables(err)) {
        delete e;
        return nullptr;
    }
    set_error(err, RS16_OK);
    return e;
}

// The engine's stream and the tables every engine has.
int rs16_engine::upload_tables(rs16_error* err) {
    const HostTables& t = host_tables();
    RS16_HIP(hipSetDevice(device));
    if (flags & RS16_ENGINE_OWN_QUEUE) {
        // A stream with a CU mask gets a hardware queue of its own (the HIP
        // runtime shares its GPU_MAX_HW_QUEUES queues only among unmasked
        // streams); the mask enables every CU.
        int cus = 0;
        RS16_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        std::vector<uint32_t> mask(((size_t)cus + 31) / 32, 0xFFFFFFFFu);
        if (cus % 32) mask.back() = (1u << (cus % 32)) - 1;
        hipStream_t masked = nullptr;
        RS16_HIP(hipExtStreamCreateWithCUMask(&masked, (uint32_t)mask.size(), mask.data()));
        stream.adopt(masked);
    } else {
        RS16_HIP(stream.get());
    }
    RS16_HIP(d_skew_tab.reserve((size_t)GF_ORDER * TAB_DWORDS * 4));
    RS16_HIP(d_skew_tab_tower.reserve((size_t)GF_ORDER * TAB_DWORDS * 4));
    RS16_HIP(d_mul_tab.reserve(t.mul_tab.size() * 4));
    RS16_HIP(d_log_walsh.reserve(GF_ORDER * 2));
    RS16_HIP(d_zero_sink.reserve(RS16_ZERO_BYTES));
    RS16_HIP(hipMemset(d_zero_sink.p, 0, RS16_ZERO_BYTES));
    RS16_HIP(hipMemcpy(d_skew_tab.p, t.skew_tab.data(), t.skew_tab.size() * 4, hipMemcpyHostToDevice));
    RS16_HIP(hipMemcpy(d_skew_tab_tower.p, t.skew_tab_tower.data(), t.skew_tab_tower.size() * 4, hipMemcpyHostToDevice));
    RS16_HIP(hipMemcpy(d_mul_tab.p, t.mul_tab.data(), t.mul_tab.size() * 4, hipMemcpyHostToDevice));
    RS16_HIP(hipMemcpy(d_log_walsh.p, t.log_walsh.data(), GF_ORDER * 2, hipMemcpyHostToDevice));
    return RS16_OK;
}

rs16_engine::~rs16_engine() {
    (void)hipSetDevice(device);
    // The streams this engine's work can be on: its own, the slice and
    // host-pipeline streams, and the last caller stream that used its scratch
    // (through order_ev).  Other engines and unrelated work are not waited for.
    if (stream) (void)hipStreamSynchronize(stream);
    for (auto& s : sl_own)
        if (s) (void)hipStreamSynchronize(s);
    for (auto& sl : hslot)
        if (sl.s) (void)hipStreamSynchronize(sl.s);
    if (last == LAST_CALLER && order_ev) (void)hipEventSynchronize(order_ev);
    for (rs16_encoder* c : encoders) detach(c);
    for (rs16_decoder* c : decoders) detach(c);
    for (rs16_update_plan* c : update_plans) detach(c);
    for (rs16_locate_plan* c : locate_plans) detach(c);
    for (rs16_comm* c : comms) detach(c);
}

extern "C" void rs16_engine_free(rs16_engine* e) {
    if (e) delete e;  // (~rs16_engine)
}

extern "C" int rs16_engine_device(const rs16_engine* e) { return e->device; }
extern "C" void* rs16_engine_stream(const rs16_engine* e) { return (void*)e->stream.s; }
extern "C" int rs16_engine_synchronize(rs16_engine* e, void* stream, rs16_error* err) {
    if (int rc = e->activate(err)) return rc;
    RS16_HIP(hipStreamSynchronize(e->pick(stream)));
    return set_error(err, RS16_OK);
}

// ---- engine ops -----------------------------------------------------------
static bool is_pow2(size_t x) { return x && !(x & (x - 1)); }

static int check_transform(size_t shard_count, size_t S, size_t pos, size_t size, size_t trunc, size_t skew_delta,
                           rs16_error* err) {
    if (S == 0 || (S & 63) || !is_pow2(size) || size > GF_ORDER || trunc > size || pos + size > shard_count)
        return set_error(err, RS16_INVALID_ARGUMENT);
    // largest twiddle index touched: (size - 2) + skew_delta must be < GF_MODULUS
    if (size >= 2 && size - 2 + skew_delta >= GF_MODULUS) return set_error(err, RS16_INVALID_ARGUMENT);
    return RS16_OK;
}

extern "C" int rs16_engine_fft(rs16_engine* e, void* data, size_t shard_count, size_t S, size_t pos, size_t size,
                               size_t trunc, size_t skew_delta, void* stream, rs16_error* err) {
    if (int rc = check_transform(shard_count, S, pos, size, trunc, skew_delta, err)) return rc;
    if (!shard_aligned(data)) return set_error(err, RS16_INVALID_ARGUMENT);
    if (int rc = e->activate(err)) return rc;
    if (int rc = e->fft((uint8_t*)data, S, pos, size, skew_delta, e->pick(stream), err)) return rc;
    return set_error(err, RS16_OK);
}
extern "C" int rs16_engine_fft_skew_end(rs16_engine* e, void* data, size_t shard_count, size_t S, size_t pos,
                                        size_t size, size_t trunc, void* stream, rs16_error* err) {
    return rs16_engine_fft(e, data, shard_count, S, pos, size, trunc, pos + size, stream, err);
}
extern "C" int rs16_engine_ifft(rs16_engine* e, void* data, size_t shard_count, size_t S, size_t pos, size_t size,
                                size_t trunc, size_t skew_delta, void* stream, rs16_error* err) {
    if (int rc = check_transform(shard_count, S, pos, size, trunc, skew_delta, err)) return rc;
    if (!shard_aligned(data)) return set_error(err, RS16_INVALID_ARGUMENT);
    if (int rc = e->activate(err)) return rc;
    if (int rc = e->ifft((uint8_t*)data, S, pos, size, skew_delta, e->pick(stream), err)) return rc;
    return set_error(err, RS16_OK);
}
extern "C" int rs16_engine_ifft_skew_end(rs16_engine* e, void* data, size_t shard_count, size_t S, size_t pos,
                                         size_t size, size_t trunc, void* stream, rs16_error* err) {
    return rs16_engine_ifft(e, data, shard_count, S, pos, size, trunc, pos + size, stream, err);
}
extern "C" int rs16_engine_fwht(rs16_engine* e, uint16_t* d, size_t trunc, void* stream, rs16_error* err) {
    if (trunc > GF_ORDER) return set_error(err, RS16_INVALID_ARGUMENT);
    if (int rc = e->activate(err)) return rc;
    if (int rc = e->order(e->pick(stream), err)) return rc;
    if (int rc = e->guard_eval(e->pick(stream), false, err)) return rc;
    RS16_HIP(e->ev_main.work32.reserve(GF_ORDER * 4));
    RS16_HIP(launch_fwht_u16(d, (uint32_t*)e->ev_main.work32.p, e->pick(stream)));
    if (int rc = e->scratch_done(e->pick(stream), err)) return rc;
    return set_error(err, RS16_OK);
}
extern "C" int rs16_engine_eval_poly(rs16_engine* e, uint16_t* d, size_t trunc, void* stream, rs16_error* err) {
    if (trunc > GF_ORDER) return set_error(err, RS16_INVALID_ARGUMENT);
    if (int rc = e->activate(err)) return rc;
    if (int rc = e->order(e->pick(stream), err)) return rc;
    if (int rc = e->guard_eval(e->pick(stream), false, err)) return rc;
    RS16_HIP(e->ev_main.work32.reserve(GF_ORDER * 4));
    RS16_HIP(launch_eval_poly_u16(d, (uint32_t*)e->ev_main.work32.p, e->d_log_walsh.as<uint16_t>(), e->pick(stream)));
    if (int rc = e->scratch_done(e->pick(stream), err)) return rc;
    return set_error(err, RS16_OK);
}
extern "C" int rs16_engine_mul(rs16_engine* e, void* x, size_t bytes, uint16_t log_m, void* stream, rs16_error* err) {
    if ((bytes & 63) || !shard_aligned(x)) return set_error(err, RS16_INVALID_ARGUMENT);
    if (int rc = e->activate(err)) return rc;
    RS16_HIP(launch_mul((uint8_t*)x, bytes, log_m, e->d_mul_tab.as<uint32_t>(), e->pick(stream)));
    return set_error(err, RS16_OK);
}
extern "C" int rs16_engine_xor(rs16_engine* e, void* x, const void* y, size_t bytes, void* stream, rs16_error* err) {
    if ((bytes & 63) || !shard_aligned(x) || !shard_aligned(y)) return set_error(err, RS16_INVALID_ARGUMENT);
    if (int rc = e->activate(err)) return rc;
    RS16_HIP(launch_xor((uint8_t*)x, (const uint8_t*)y, bytes, e->pick(stream)));
    return set_error(err, RS16_OK);
}
extern "C" int rs16_engine_xor_within(rs16_engine* e, void* data, size_t shard_count, size_t S, size_t x, size_t y,
                                      size_t count, void* stream, rs16_error* err) {
    if ((S & 63) || x + count > shard_count || y + count > shard_count || (x < y ? x + count > y : y + count > x))
        return set_error(err, RS16_INVALID_ARGUMENT);
    uint8_t* d = (uint8_t*)data;  // (rs16_engine_xor checks the alignment: x S and y S are multiples of 64)
    return rs16_engine_xor(e, d + x * S, d + y * S, count * S, stream, err);
}
extern "C" int rs16_engine_formal_derivative(rs16_engine* e, void* data, size_t n, size_t S, void* stream,
                                             rs16_error* err) {
    if ((S & 63) || S == 0 || !is_pow2(n) || !shard_aligned(data)) return set_error(err, RS16_INVALID_ARGUMENT);
    hipStream_t s;
    if (int rc = begin_ordered(e, stream, &s, err)) return rc;
    RS16_HIP(e->ws_fd.reserve(n * S));
    RS16_HIP(launch_formal_derivative((uint8_t*)e->ws_fd.p, (const uint8_t*)data, n, S, s));
    RS16_HIP(hipMemcpyAsync(data, e->ws_fd.p, n * S, hipMemcpyDeviceToDevice, s));
    if (int rc = e->scratch_done(s, err)) return rc;
    return set_error(err, RS16_OK);
}

// ---------------------------------------------------------------------------
// Device memory helpers.
// ---------------------------------------------------------------------------
// A device / page-locked allocation or a stream, made on the engine's device.
template <class T, class F> static void* made(rs16_engine* e, rs16_error* err, F make) {
    if (e->activate(err)) return nullptr;
    T p = nullptr;
    if (hipError_t he = make(&p)) return hip_fail(err, he), nullptr;
    set_error(err, RS16_OK);
    return p;
}
extern "C" void* rs16_device_alloc(rs16_engine* e, size_t bytes, rs16_error* err) {
    return made<void*>(e, err, [&](void** p) { return hipMalloc(p, bytes ? bytes : 1); });
}
extern "C" void rs16_device_free(rs16_engine* e, void* p) {
    if (!e || !p) return;
    (void)hipSetDevice(e->device);
    (void)hipFree(p);
}
extern "C" void* rs16_stream_create(rs16_engine* e, rs16_error* err) {
    return made<hipStream_t>(e, err, [](hipStream_t* p) { return hipStreamCreateWithFlags(p, hipStreamNonBlocking); });
}
extern "C" void rs16_stream_destroy(rs16_engine* e, void* st) {
    if (!e || !st) return;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize((hipStream_t)st);
    (void)hipStreamDestroy((hipStream_t)st);
}
extern "C" void* rs16_host_alloc(rs16_engine* e, size_t bytes, rs16_error* err) {
    return made<void*>(e, err, [&](void** p) { return hipHostMalloc(p, bytes ? bytes : 1, hipHostMallocPortable); });
}
extern "C" void rs16_host_free(rs16_engine* e, void* p) {
    if (!e || !p) return;
    (void)hipSetDevice(e->device);
    (void)hipHostFree(p);
}
// One copy on the call's stream, complete on return.
template <class F> static int copy_sync(rs16_engine* e, void* stream, rs16_error* err, F copy) {
    if (int rc = e->activate(err)) return rc;
    hipStream_t s = e->pick(stream);
    RS16_HIP(copy(s));
    RS16_HIP(hipStreamSynchronize(s));
    return set_error(err, RS16_OK);
}
extern "C" int rs16_memcpy_htod(rs16_engine* e, void* dst, const void* src, size_t bytes, void* stream,
                                rs16_error* err) {
    return copy_sync(e, stream, err,
                     [&](hipStream_t s) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s); });
}
extern "C" int rs16_memcpy_dtoh(rs16_engine* e, void* dst, const void* src, size_t bytes, void* stream,
                                rs16_error* err) {
    return copy_sync(e, stream, err,
                     [&](hipStream_t s) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s); });
}
extern "C" int rs16_memcpy2d_htod(rs16_engine* e, void* dst, size_t d_pitch, const void* src, size_t h_pitch,
                                  size_t width, size_t rows, void* stream, rs16_error* err) {
    if (width > d_pitch || width > h_pitch) return set_error(err, RS16_INVALID_ARGUMENT);
    return copy_sync(e, stream, err, [&](hipStream_t s) {
        return hipMemcpy2DAsync(dst, d_pitch, src, h_pitch, width, rows, hipMemcpyHostToDevice, s);
    });
}
extern "C" int rs16_memcpy2d_dtoh(rs16_engine* e, void* dst, size_t h_pitch, const void* src, size_t d_pitch,
                                  size_t width, size_t rows, void* stream, rs16_error* err) {
    if (width > d_pitch || width > h_pitch) return set_error(err, RS16_INVALID_ARGUMENT);
    return copy_sync(e, stream, err, [&](hipStream_t s) {
        return hipMemcpy2DAsync(dst, h_pitch, src, d_pitch, width, rows, hipMemcpyDeviceToHost, s);
    });
}
extern "C" int rs16_memset_device(rs16_engine* e, void* dst, int value, size_t bytes, void* stream, rs16_error* err) {
    if (int rc = e->activate(err)) return rc;
    RS16_HIP(hipMemsetAsync(dst, value, bytes, e->pick(stream)));
    return set_error(err, RS16_OK);
}
