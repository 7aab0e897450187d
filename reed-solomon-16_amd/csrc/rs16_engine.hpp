// rs16_engine.hpp -- host-side engine object and pass drivers (internal).
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rs16.h"
#include "rs16_internal.hpp"

namespace rs16 {

// The five holders of what the host side owns on the GPU.  Each frees its
// resource in its destructor (on the device it was made on, current then),
// cannot be copied and is empty after a move: a member or a local of these
// types needs no release list.  release() is for freeing early on purpose.
//
// Grow-only device buffer.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept { return release(), std::swap(p, o.p), std::swap(cap, o.cap), *this; }
    ~DevBuf() { if (p) release(); }
    hipError_t reserve(size_t bytes);
    void release();
    template <class T> T* as() const { return (T*)p; }  // a table that kernels read as T
};
// Grow-only page-locked host buffer (hipHostMalloc): DMA-rate H2D / D2H.
struct HostBuf {
    void* p = nullptr;
    size_t cap = 0;
    HostBuf() = default;
    HostBuf(HostBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    HostBuf& operator=(HostBuf&& o) noexcept { return release(), std::swap(p, o.p), std::swap(cap, o.cap), *this; }
    ~HostBuf() { if (p) release(); }
    hipError_t reserve(size_t bytes);
    void release();
};
// An event, made by the first get() (hipEventDefault: the profiling pool's timing flavour).
struct Event {
    hipEvent_t ev = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : ev(std::exchange(o.ev, nullptr)) {}
    Event& operator=(Event&& o) noexcept { return release(), std::swap(ev, o.ev), *this; }
    ~Event() { if (ev) release(); }  // (inline: an empty one costs a test)
    hipError_t get(unsigned flags = hipEventDisableTiming) {
        return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags);
    }
    void release();
    operator hipEvent_t() const { return ev; }
};
// A stream, made by the first get() (non-blocking) or made elsewhere and handed over (adopt).
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(std::exchange(o.s, nullptr)) {}
    Stream& operator=(Stream&& o) noexcept { return release(), std::swap(s, o.s), *this; }
    ~Stream() { if (s) release(); }
    hipError_t get() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    void adopt(hipStream_t made) { release(), s = made; }
    void release();
    operator hipStream_t() const { return s; }
};
// An event recorded on a stream and not yet waited for on the host.
struct Pending {
    Event ev;
    bool busy = false;
    Pending() = default;
    Pending(Pending&& o) noexcept : ev(std::move(o.ev)), busy(std::exchange(o.busy, false)) {}
    Pending& operator=(Pending&& o) noexcept {
        return ev = std::move(o.ev), busy = std::exchange(o.busy, false), *this;
    }
    hipError_t record(hipStream_t s);
    hipError_t wait();  // host-side: returns once the recorded work is done
};
template <class T>
constexpr bool owns = !std::is_copy_constructible<T>::value && !std::is_copy_assignable<T>::value &&
                      std::is_nothrow_move_constructible<T>::value;
static_assert(owns<DevBuf> && owns<HostBuf> && owns<Event> && owns<Stream> && owns<Pending>, "holders: move only");

// Status helper: every internal call returns an rs16 code and fills err.
int set_error(rs16_error* err, int code, uint64_t v0 = 0, uint64_t v1 = 0, uint64_t v2 = 0);
int hip_fail(rs16_error* err, hipError_t e);
#define RS16_HIP(call)                                 \
    do {                                               \
        hipError_t _e = (call);                        \
        if (_e != hipSuccess) return hip_fail(err, _e); \
    } while (0)
#define RS16_PASS(...)                                       \
    do {                                                     \
        if (int _rc = this->pass(__VA_ARGS__, err)) return _rc; \
    } while (0)
// the same under profiling id PROF
#define RS16_PASS_AS(PROF, ...)                                     \
    do {                                                            \
        if (int _rc = this->pass(__VA_ARGS__, err, PROF)) return _rc; \
    } while (0)

size_t next_pow2(size_t x);
inline int ilog2(size_t x) { int l = 0; while (((size_t)1 << l) < x) l++; return l; }

// Geometry of a decode (both rates): segment A = rows [0, a_count),
// segment B = rows [chunk, chunk + b_count), transform of n rows.
struct DecodeGeom {
    bool high;
    uint32_t a_count, chunk, b_count, n;
    // Received shard counts of the two segments when the caller knows them
    // (0: the whole segment is lost, so its first-pass tiles need no launch).
    size_t a_recv = 1, b_recv = 1;
    // The repair (rs16_repair_device, general path): the lost rows of both
    // segments are restored, each to its own array.  The pass codec at every
    // size -- no half-transform or identity decode (a recovery shard is lost,
    // so the transform's input is not zero on a half even when every original
    // is lost), no column codec, no mid_direct / tile_last kernels.
    bool repair = false;
    // The selective decode (rs16_decode_device_select, path 2): only the lost
    // originals of the read set are restored -- `wanted`, a device array of one
    // byte per original (nonzero: wanted), of which `wanted_count` are lost.
    // No half-transform or identity decode: every original may be lost while
    // only some are wanted, and those pipelines store every row below
    // out_rows (their counts would qualify: the trap the repair documents for
    // 3:5).  An all-lost stripe takes the general path, whose DEC_FIRST
    // launches the received segment's tiles only; up to 2^11 work rows the
    // column codec's COL_DEC_GEN_SEL.  The row interval that prunes the passes
    // (lostrange) is taken over the wanted rows; the erasure locator comes from
    // the received flags alone.  wanted_count stands for the lost count in the
    // host's gates (mid_direct, tile_last).  One column slice.
    bool select = false;
    const uint8_t* wanted = nullptr;
    size_t wanted_count = 0;
};
DecodeGeom decode_geom(bool high, size_t k, size_t m);
// The last pass of the general repair (DEC_LAST_ALL, 2^lo-row tiles, lo = L / 2
// of the n = 2^L > 2^8 work rows): segment A's tiles [0, a_tiles) and segment
// B's [b_first, b_first + b_tiles), whole tiles between them left out -- one
// launch when the two ranges touch or overlap (then a_tiles = 0 and B's range
// starts at tile 0), else two.  n <= 2^8: lo = 0 and one tile, the one-pass
// kernel's.  Host arithmetic only (rs16_host_repair_path shows it to tests).
struct RepairTiles {
    uint32_t lo, a_tiles, b_first, b_tiles;
};
RepairTiles repair_tiles(const DecodeGeom& g);

// The scrub (rs16_verify_device, fused path): where the last launch of an
// encode compares instead of storing -- the stored recovery shards (row stride
// S_cmp), the row flags, the column flags (nullptr: none) and the check set
// (nullptr: every row), with the byte strides from stripe to stripe of a
// batched launch.  The check set is shared by the stripes.
struct VerifySink {
    const uint8_t* cmp;
    size_t S_cmp, bs_cmp;
    uint8_t* rows;
    uint8_t* cols;
    const uint8_t* checked;
    size_t bs_rows, bs_cols;
};

// The decode's view of its two segments (decode_passes, decode_fused): the
// gather sources with their device flags and where the lost rows go.
// S_user: the row stride of seg_a / seg_b / rest / rest_b; bs_*: the byte
// strides from stripe to stripe of a batched launch.
struct DecodeSegs {
    const uint8_t *seg_a = nullptr, *seg_b = nullptr, *fl_a = nullptr, *fl_b = nullptr;
    size_t bs_a = 0, bs_b = 0;
    uint8_t* rest = nullptr;  // where the restored originals go, stripe stride bs_rest
    size_t bs_rest = 0;
    // g.repair: rest / bs_rest are segment A's array and stripe stride, rest_b
    // / bs_rest_b segment B's; the lost rows of both are restored
    uint8_t* rest_b = nullptr;
    size_t bs_rest_b = 0;
    size_t S_user = 0;
};

// How a shape is encoded (rs16_engine::encode_form): the chunk geometry -- nch
// chunks of chunk = 2^L rows, the passes' row split lo + hi = L -- and which
// branch of the encoders runs.  one_chunk: the one-chunk high rate (k <= chunk:
// encode_high_fused, the shape with batched launches and column slices), whose
// kinds are COL, ONE_PASS (L <= 8) and THREE_PASS; the multi-chunk high rate
// and the low rate have ROWS (L == 0: the XOR of the rows / the copies), COL
// (the low rate's one recovery chunk in one column launch), COLM, COL_CHUNKS
// and PASSES.
struct EncodeForm {
    enum Kind { COL, ONE_PASS, THREE_PASS, ROWS, COLM, COL_CHUNKS, PASSES } kind;
    bool one_chunk;
    size_t chunk;
    uint32_t nch;
    int L, lo, hi;
    // The encode ends in a pass-codec store pass that has a comparing form
    // (ENC_SINGLE_VFY at T >= 1, ENC_LAST_VFY at T >= 4, fft_to_recovery's last
    // pass at T = lo): the shapes a VerifySink may be given for.
    bool verify_fusable() const {
        return kind == ONE_PASS ? L >= 1 : kind == THREE_PASS || (kind == PASSES && lo >= 4);
    }
};

}  // namespace rs16

struct rs16_encoder;
struct rs16_decoder;
struct rs16_update_plan;
struct rs16_locate_plan;
struct rs16_comm;

struct rs16_engine {
    int device = 0;
    int flags = 0;  // rs16_engine_new_ex flags (RS16_ENGINE_OWN_QUEUE)
    rs16::Stream stream;
    // diagnostic switches of this engine (rs16::DiagFlags, rs16_engine_set_diagnostics)
    int diag = 0;
    rs16::DevBuf d_skew_tab;        // v_perm table per twiddle index (8 MiB)
    rs16::DevBuf d_skew_tab_tower;  // the same in tower coordinates: the passes of a tower sequence
    rs16::DevBuf d_mul_tab;
    rs16::DevBuf d_col_img;    // column codec table images (HostTables::col_img)
    rs16::DevBuf d_col_v;      // column codec eval_poly tables (HostTables::col_v)
    rs16::DevBuf d_log_walsh;  // (uint16_t)
    rs16::DevBuf d_zero_sink;  // zero page (PassArgs::zero, ColArgs::zero)
    int upload_tables(rs16_error* err);  // the five of them every engine has (rs16_engine_new_ex)
    // scratch
    rs16::DevBuf ws_z, ws_u, ws_fd, ws_flags;
    // the repair's recovery-only path: the re-encoded recovery shards of the
    // call's stripes (recovery_count x shard_bytes each), reserved on first use
    rs16::DevBuf ws_rep;
    // rs16_locate_device / _batch, rs16_heal_device / _batch, per stripe of the
    // call: the candidate errors of the originals (k x S), their encode (m x S),
    // the per-element (count, row sum) pairs of the scan, the per-block
    // candidates (for a heal also the status and shard entries the caller did
    // not ask for) and the heal's fix (B x 64).  ws_loc_e and the pairs are all
    // zero as a whole between calls (loc_clean), whatever the stripes of the
    // next call: the kernels put back what they wrote, and a call that finds the
    // buffers regrown or a previous call cut short clears them whole.
    rs16::DevBuf ws_loc_e, ws_loc_rep, ws_loc_acc, ws_loc_cand, ws_loc_fix;
    bool loc_clean = false;
    // the general decode's middle pass as v_perm tables of its matrix, per
    // transform size L (mid_tables; built on first use)
    rs16::DevBuf mid_tab[17];
    // The decode's eval_poly outputs / pass metadata (written by decode_eval,
    // read by decode_passes): ev_main, or one of the pipelined host path's
    // per-lane sets (so that two lanes' decodes never share them).
    struct EvalBufs {
        rs16::DevBuf work32, elog;
        rs16::DevBuf zflag;   // per DEC_FIRST tile, 1 = no received row (tile skipped, rows zero)
        rs16::DevBuf rbits;   // received-row bitmap (65536 bits)
        rs16::DevBuf lost;    // lost-original row range per 256-row block (2 KiB) + overall (8 B)
        rs16::DevBuf rcount;  // received rows per 64-row chunk and segment (ErasureSpec::rcount)
    };
    EvalBufs ev_main, ev_lane[2];
    // What one decode_eval left behind, the value decode_passes works from: the
    // buffers it wrote to and what it decided about them.
    struct DecodePlan {
        EvalBufs* ev = nullptr;
        bool ident = false;        // every erasure log is 0 (identity_logs): no eval_poly kernel ran
        bool elog_fused = false;   // the final 256-point FWHT is left to the passes (ev->work32)
        bool eval_in_col = false;  // eval_poly is left to the column codec (COL_DEC_EVAL / COL_DEC_GEN)
        uint32_t var_ns = 0;       // stripes with losses of their own (0: shared) ...
        uint64_t var_bs_fa = 0, var_bs_fb = 0;  // ... and their flags' strides
    };
    // Split decode (rs16_decode_prepare / rs16_decode_device_prepared): the
    // prepared received pattern, whose eval_poly went to ev_main on the
    // prepare's stream; prep_ev marks its end.  While prep_pending, any other
    // use of ev_main first orders itself after prep_ev (guard_eval).
    struct Prepared {
        bool valid = false, nothing = false;
        size_t k = 0, m = 0, S = 0;
        rs16::DecodeGeom g{};
        const uint8_t* fl_a = nullptr;
        const uint8_t* fl_b = nullptr;
        int nslices = 1;
        DecodePlan plan;  // of its evaluation, which the prepared decode's passes get
    } prep;
    rs16::Event prep_ev;
    bool prep_pending = false;
    // order stream s after a pending preparation's eval_poly (whose outputs
    // the caller is about to overwrite or read) and drop the preparation
    // unless it is the one being consumed
    int guard_eval(hipStream_t s, bool consume, rs16_error* err);
    // the last decode's geometry and the received counts it was given (rs16_decode_check)
    rs16::DecodeGeom last_dec{};
    bool last_dec_valid = false;
    // ... or, when that decode had nothing to restore (every original
    // received: no kernel counted anything), a copy of its flags in ws_flags
    // (segment A at 0, B at GF_ORDER), which rs16_decode_check counts itself
    bool last_dec_flags_only = false;
    void forget_decode() { last_dec_valid = last_dec_flags_only = false; }
    // Host-resident pipeline (rs16_encode_host / rs16_decode_host): column
    // slices alternate between two slots, each with its own stream and the
    // device buffers of one slice, so copies and compute of different slices
    // overlap.  hflags: the received flags of a host decode; hev orders the
    // slots after the engine stream.
    struct HostSlot {
        rs16::Stream s;
        rs16::DevBuf orig, rec, z, u;
        rs16::DevBuf rcount;  // the slot's column decodes' received counts (never ws_rcount)
    };
    HostSlot hslot[2];
    // Column slices of the device-resident one-shot codec: a stripe's shard
    // columns are split into `slices` slices (multiples of 64 bytes; every
    // 64-byte column block is an independent codeword) that run on internal
    // streams forked from and joined back into the caller's stream.  Default
    // 1: measured on MI355X (scripts/probe_fork.py), the fork/join events
    // cost ~8 us of host time each and the cross-queue dependencies erase the
    // overlap (32768:32768 x 1 KiB encode 97 us at 1 slice, 101 us at 2);
    // only fully independent streams (two stripes) gain (+10 %).
    static constexpr int MAX_SLICES = 4;
    int slices = 1;
    hipStream_t sl_stream[MAX_SLICES] = {};  // per call: [0] = caller's stream, [j] = sl_own[j] (borrowed)
    rs16::Stream sl_own[MAX_SLICES];
    rs16::Event sl_fork, sl_join[MAX_SLICES];
    int slice_count(size_t S) const;
    int fork(hipStream_t s, int n, rs16_error* err);
    int join(hipStream_t s, int n, rs16_error* err);
    rs16::DevBuf hflags;
    rs16::Event hev;
    // pipelined host stripes (rs16_{en,de}code_host_batch): per lane, the
    // flag bytes' copy out of hp_flags is done
    rs16::Event hp_ev[2];
    rs16::Event hp_off;  // the first stripe's H2D is done: the other lane's first H2D starts then
    rs16::HostBuf hp_flags;  // page-locked staging of the decode's flag bytes (2 x (k + m))
    int host_pipe_events(rs16_error* err);
    int host_slots(rs16_error* err);

    hipStream_t pick(void* s) const { return s ? (hipStream_t)s : stream.s; }
    int activate(rs16_error* err);

    // The scratch buffers (ws_*) belong to the engine, not to a stream: a
    // call that uses them on stream s first waits for the engine's previous
    // such call when that ran on another stream, so calls on different
    // streams cannot overwrite each other's scratch.  order(s) at the start
    // of such a call, scratch_done(s) at its end.  A call on a caller's
    // stream records order_ev there before it returns (the stream is never
    // touched again: the caller may destroy it); a call on the engine's own
    // stream records nothing unless a later call on another stream needs it
    // (then it is recorded on the engine stream, which the engine owns), so
    // the one-stream case costs no event.
    enum { LAST_NONE, LAST_ENGINE, LAST_CALLER } last = LAST_NONE;
    rs16::Event order_ev;
    int order(hipStream_t s, rs16_error* err);
    int scratch_done(hipStream_t s, rs16_error* err);

    // The five kinds of object created on this engine.  Its destructor detaches
    // them (rs16::detach, rs16_api.hpp: the object's device and page-locked
    // memory freed, its eng cleared): a detached object answers every call with
    // RS16_INVALID_ARGUMENT and its free() only frees host memory.
    std::vector<rs16_encoder*> encoders;
    std::vector<rs16_decoder*> decoders;
    std::vector<rs16_update_plan*> update_plans;
    std::vector<rs16_locate_plan*> locate_plans;
    std::vector<rs16_comm*> comms;
    // Waits for the engine's work and detaches those objects; the members free
    // themselves.  The one ordering rule: all waiting happens in the destructor's
    // body, before any member is destroyed, so the order of the members is free.
    ~rs16_engine();

    // Pass launch (with optional hipEvent timing on the launch stream under
    // profiling id `prof` (rs16::ProfId; -1 = the program's own id).
    int pass(int prog, int T, const rs16::PassArgs& a, uint32_t tiles, hipStream_t s, rs16_error* err,
             int prof = -1);
    int prof_begin(hipStream_t s, rs16::Event* ev, rs16_error* err);
    int prof_end(int id, hipStream_t s, rs16::Event ev, rs16_error* err);
    // One kernel launch under profiling id `prof`: launch(stamps) returns the
    // launch's hipError_t; stamps = stamp_buf when `prof` is the stamped id,
    // else nullptr.  The only caller of prof_begin / prof_end.
    template <class F> int profiled(int prof, hipStream_t s, rs16_error* err, F launch) {
        rs16::Event ev;  // (stays empty unless profiling is on)
        if (int rc = prof_begin(s, &ev, err)) return rc;
        const hipError_t he = launch(stamp_buf && prof == stamp_prof ? (uint64_t*)stamp_buf : nullptr);
        return he == hipSuccess ? prof_end(prof, s, std::move(ev), err) : rs16::hip_fail(err, he);
    }
    bool profiling = false;
    // diagnostic timelines (rs16_engine_set_stamps): passes under profiling
    // id stamp_prof get stamp_buf (RS16_STAMPS builds record into it)
    void* stamp_buf = nullptr;
    int stamp_prof = -1;
    struct ProfRec {
        int id;
        rs16::Event a, b;
    };
    std::vector<ProfRec> prof_pending;
    std::vector<rs16::Event> ev_pool;  // timing events not in use
    double prof_ms[rs16::NUM_PROF] = {};
    uint64_t prof_n[rs16::NUM_PROF] = {};
    int prof_collect(rs16_error* err);

    // Engine ops on device shard arrays (validated by the C ABI layer).
    // the form field and twiddle table of the launches of a three-pass sequence (z_form_sequence)
    void z_form_args(rs16::PassArgs& a, rs16::ZForm f) const;
    int fft(uint8_t* data, size_t S, size_t pos, size_t size, size_t skew_delta, hipStream_t s, rs16_error* err);
    int ifft(uint8_t* data, size_t S, size_t pos, size_t size, size_t skew_delta, hipStream_t s, rs16_error* err);

    // The one decision of how a shape is encoded (EncodeForm): nstripes is the
    // stripes of one batched launch, which only the one-chunk high rate has
    // (other shapes run stripe by stripe: their column limits count one stripe).
    rs16::EncodeForm encode_form(bool high, size_t k, size_t m, size_t S, size_t nstripes) const;
    // Fused HighRate single-chunk encode (f.one_chunk): originals rows [0,k) of
    // d_orig -> recovery rows [0,m) of d_rec, using Z (chunk rows) as work.
    // S = row width worked on (a column slice of the caller's arrays when
    // S < S_user), S_user = row stride of d_orig / d_rec (Z: stride S).
    // f (here and in the multi-chunk encoders): encode_form of the call's shape.
    int encode_high_fused(const rs16::EncodeForm& f, size_t k, size_t m, size_t S, size_t S_user, const uint8_t* d_orig,
                          uint8_t* d_rec, uint8_t* Z, hipStream_t s, rs16_error* err, size_t nstripes = 1,
                          size_t bs_orig = 0, size_t bs_rec = 0, const rs16::VerifySink* vs = nullptr);
    // vs (here and in the multi-chunk encoders): the last launch is the
    // comparing program (ENC_SINGLE_VFY / ENC_LAST_VFY) on the sink, d_rec is
    // not used, and the work rows keep the shards' form; only for the forms of
    // EncodeForm::verify_fusable (others: RS16_INVALID_ARGUMENT, nothing launched).
    // Fused decode (both rates) of one stripe: v's seg_a / seg_b gather
    // sources with device flags; lost originals written to v.rest; Z, U work
    // (n rows each; Z may alias the sources when they live at their work
    // positions).  S = row width (Z, U: stride S)
    int decode_fused(const rs16::DecodeGeom& g, size_t S, const rs16::DecodeSegs& v, uint8_t* Z, uint8_t* U,
                     hipStream_t s, rs16_error* err);
    // decode_fused = decode_eval (erasure logs into ev.elog, what it decided
    // into *plan) + decode_passes (given that plan).
    // S / nstripes: the width of the decode_passes launches that follow (0:
    // unknown); when the column codec will run them as a high-rate half
    // decode it computes eval_poly itself and no kernel is launched here.
    // vary > 1: nstripes = vary stripes with losses of their own, stripe i's
    // flags at flags_a / flags_b + i bs_fa / bs_fb bytes: one grid row of the
    // eval kernels per stripe, per-stripe metadata (VARY_* strides below).
    // prepare: the evaluation of rs16_decode_prepare, which keeps the
    // preparation it is making.
    // Every erasure log of the decode is 0 (a whole-half erasure, DESIGN.md
    // 3.13): the multipliers are identities and eval_poly is not launched.
    bool identity_logs(const rs16::DecodeGeom& g, uint32_t vary) const;
    // Device tables of the L-bit general decode's middle-pass matrix
    // (mid_matrix_entries), uploaded on first use.
    int mid_tables(int L, const uint32_t** out, rs16_error* err);
    int decode_eval(const rs16::DecodeGeom& g, const uint8_t* flags_a, const uint8_t* flags_b, EvalBufs& ev,
                    DecodePlan* plan, hipStream_t s, rs16_error* err, size_t S = 0, size_t nstripes = 1,
                    uint32_t vary = 0, size_t bs_fa = 0, size_t bs_fb = 0, bool prepare = false);
    // per-stripe decode metadata of a batch with losses of its own
    static constexpr uint32_t VARY_WORK = rs16::GF_ORDER, VARY_RBITS = rs16::GF_ORDER / 32, VARY_ZFLAGS = 256,
                              VARY_LOST = 520;
    // rcount: where a column decode that evaluates the polynomial itself
    // writes the received counts (ErasureSpec::rcount layout): ev_main.rcount on
    // the call's own stream, a buffer of their own for concurrent slots.
    int decode_passes(const rs16::DecodeGeom& g, size_t S, const rs16::DecodeSegs& v, uint8_t* Z, uint8_t* U,
                      const DecodePlan& plan, uint32_t* rcount, size_t nstripes, hipStream_t s, rs16_error* err);
    // The half-transform decode applies (every original lost, originals
    // segment = one half of the work rows).
    static bool half_decode(const rs16::DecodeGeom& g);
    // One-launch codec (rs16_col.hip) for transforms of 2^9 / 2^10 rows:
    // used when the launch has at most col_max_quads quad columns (x
    // stripes); wider launches take the pass codec, whose tiles share each
    // twiddle table over 32 quad columns.
    uint32_t col_max_quads = 256;  // (measured: scripts/probe_col.py)
    bool col_ok(int L, size_t S, size_t nstripes, bool gen = false) const;  // gen: the general decode (up to 2^11 rows)
    // Multi-chunk encodes of 2^8 .. 2^10-row chunks in the column codec: at
    // most col_max_chunk_rows rows in all (more take the passes: every
    // workgroup stages its own twiddle tables, and the low rate's repeats the
    // IFFT, so the column form's cost grows faster with the chunk count;
    // break-even 6-8 chunks of 1024 rows, scripts/probe_chunks.py)
    uint32_t col_max_chunk_rows = 6144;
    bool col_chunks_ok(int L, uint32_t nch, size_t S, bool high) const;
    int col(const rs16::ColArgs& a, int L, int mode, hipStream_t s, rs16_error* err);
    int col_multi(size_t k, size_t m, size_t S, size_t S_user, const uint8_t* d_orig, uint8_t* d_rec, uint32_t nch,
                  bool high, hipStream_t s, rs16_error* err);
    int col_tables(hipStream_t s, rs16_error* err);
    // A column launch of one stripe and one chunk: in_rows rows at `in` (pitch
    // S_in) -> out_rows rows at `out` (pitch S_out), S bytes of each, the two
    // transforms' skew deltas.  The callers add what differs (stripes, chunks,
    // the decodes' flags and logs).
    rs16::ColArgs col_args(const uint8_t* in, size_t S_in, uint8_t* out, size_t S_out, size_t S, size_t in_rows,
                           size_t out_rows, size_t skew_ifft, size_t skew_fft) const;
    // Multi-chunk encoders (high rate with k > chunk, low rate): every chunk's
    // transform in one batched set of launches.  d_orig rows have pitch
    // S_user, Z is the work space (work_count x S; may be d_orig), the
    // recovery rows [0, m) go to d_rec (pitch S_user; may be Z).
    int encode_high_multi(const rs16::EncodeForm& f, size_t k, size_t m, size_t S, size_t S_user, const uint8_t* d_orig,
                          uint8_t* d_rec, uint8_t* Z, hipStream_t s, rs16_error* err,
                          const rs16::VerifySink* vs = nullptr);
    // U: chunk x S bytes for the transformed originals, owned by the call's
    // stream (the engine's ws_u on the engine-ordered paths, a slot's own
    // buffer on concurrent slots); required -- there is no fallback.
    int encode_low_multi(const rs16::EncodeForm& f, size_t k, size_t m, size_t S, size_t S_user, const uint8_t* d_orig,
                         uint8_t* d_rec, uint8_t* Z, uint8_t* U, hipStream_t s, rs16_error* err,
                         const rs16::VerifySink* vs = nullptr);
    int fft_to_recovery(const rs16::EncodeForm& f, size_t m, size_t S, size_t S_user, const uint8_t* src, uint8_t* Z,
                        uint8_t* d_rec, uint32_t nch, uint32_t skew, hipStream_t s, rs16_error* err,
                        const rs16::VerifySink* vs = nullptr);
};
