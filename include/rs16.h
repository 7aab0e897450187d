/*
 * rs16.h -- C ABI of the MI355X-native GF(2^16) Reed-Solomon codec.
 *
 * This is the drop-in boundary for the hot path of malaire/reed-solomon-16
 * v0.1.0 (a Rust crate).  Each entry point names the reference interface it
 * replaces (file:line in the reference tree).  A Rust `impl Engine` /
 * FFI stub binding these symbols is shown in INTEGRATION.md.
 *
 * Conventions
 *  - Every fallible call returns 0 (RS16_OK) or an error code and, if `err`
 *    is non-NULL, fills it with the code and the payload fields of the
 *    reference's `Error` variant (src/lib.rs:31-125) in declaration order.
 *  - Shard arrays are the reference's flat layout (ShardsRefMut,
 *    src/engine/shards.rs:60-66): shard i starts at byte i*shard_bytes;
 *    every 64-byte block holds 32 low bytes then 32 high bytes
 *    (src/algorithm.md:6-32).
 *  - `_device` / `d_` pointers are HIP device pointers on the engine's
 *    device; `stream` is a hipStream_t (NULL = the engine's own stream).
 *    Device-pointer calls are asynchronous on that stream.
 *  - Received flags: a flag byte means "received" when it is nonzero -- any
 *    nonzero value (1, 2, 0x80, 0xFF ...), in device and host flag arrays
 *    alike; only 0 means "not received".  Flag arrays need no alignment, and
 *    no byte outside [0, count) of a flag array is read as a flag
 *    (tests/test_gpu_flag_bytes.py).
 *  - Device shard arrays handed to the codec (the originals / recovery of the
 *    one-shot, batch, prepared and update calls, the arrays of the engine
 *    shard ops fft / ifft / mul / xor / xor_within / formal_derivative) must
 *    start on a 64-byte boundary, else RS16_INVALID_ARGUMENT before anything
 *    is launched.  64 is the layout's block size, not a measured number:
 *    shard sizes and strides are already multiples of it, so every row then
 *    starts on a block.  (The add_*_shard_device calls copy their shard and
 *    take any address; the u16 arrays of fwht / eval_poly and the RCCL
 *    buffers are not shard arrays of the codec.)
 *  - One engine must not be used from two threads at once (it owns scratch
 *    workspace); create one engine per device/thread.  It may be used on
 *    several streams: a call that needs the engine's scratch on stream s
 *    first makes s wait (hipStreamWaitEvent) for the engine's previous such
 *    call when that was issued on another stream, so two streams never
 *    share the scratch concurrently (calls on one engine serialise; use one
 *    engine per stream for concurrent codecs).
 *  - rs16_engine_free waits for the engine's work (its own streams and the
 *    last caller stream it ran on, through an event), releases what every
 *    object created on the engine holds on the device and in page-locked
 *    memory -- rs16_encoder, rs16_decoder, rs16_update_plan,
 *    rs16_locate_plan, rs16_comm (whose RCCL communicator it destroys) -- and
 *    detaches them.  These objects may outlive their engine: a detached one
 *    fails every call with RS16_INVALID_ARGUMENT (rs16_comm_rank / _size,
 *    which return no status: -RS16_INVALID_ARGUMENT), and its free() only
 *    frees its host memory (safe in any order at process exit).  Device
 *    memory, page-locked memory and streams from rs16_device_alloc /
 *    rs16_host_alloc / rs16_stream_create are the caller's: free them
 *    while the engine is alive.
 */
#ifndef RS16_H
#define RS16_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- Error -- reed_solomon_16::Error, src/lib.rs:31-125 ---------------- */
typedef enum rs16_error_code {
    RS16_OK = 0,
    RS16_DIFFERENT_SHARD_SIZE = 1,           /* v0 shard_bytes, v1 got */
    RS16_DUPLICATE_ORIGINAL_SHARD_INDEX = 2, /* v0 index */
    RS16_DUPLICATE_RECOVERY_SHARD_INDEX = 3, /* v0 index */
    RS16_INVALID_ORIGINAL_SHARD_INDEX = 4,   /* v0 original_count, v1 index */
    RS16_INVALID_RECOVERY_SHARD_INDEX = 5,   /* v0 recovery_count, v1 index */
    RS16_INVALID_SHARD_SIZE = 6,             /* v0 shard_bytes */
    RS16_NOT_ENOUGH_SHARDS = 7,              /* v0 original_count, v1 original_received_count,
                                                v2 recovery_received_count */
    RS16_TOO_FEW_ORIGINAL_SHARDS = 8,        /* v0 original_count, v1 original_received_count */
    RS16_TOO_MANY_ORIGINAL_SHARDS = 9,       /* v0 original_count */
    RS16_UNSUPPORTED_SHARD_COUNT = 10,       /* v0 original_count, v1 recovery_count */
    /* Not in the reference (it has no device and panics on misuse): */
    RS16_DEVICE_ERROR = 100,                 /* HIP runtime failure, v0 = hipError_t (RCCL: 1000 + ncclResult_t) */
    RS16_INVALID_ARGUMENT = 101              /* engine-op misuse the reference would panic on */
} rs16_error_code;

typedef struct rs16_error {
    int32_t code;
    uint64_t v0, v1, v2;
} rs16_error;

/* `impl Display for Error` (src/lib.rs:130-222): writes the exact message,
 * returns its length (excluding NUL); truncates to len-1 bytes. */
size_t rs16_error_message(const rs16_error* err, char* buf, size_t len);

/* ---- Engine -- trait Engine (src/engine.rs:140-260) ---------------------
 * rs16_engine_new plays NoSimd::new (src/engine/engine_nosimd.rs:27-35):
 * it builds the GF tables (src/engine/tables.rs) once per process and
 * uploads them to the device's HBM. */
typedef struct rs16_engine rs16_engine;
rs16_engine* rs16_engine_new(int device, rs16_error* err);
/* rs16_engine_new with creation flags (0 = rs16_engine_new).
 * RS16_ENGINE_OWN_QUEUE: the engine's stream gets a hardware queue of its
 * own (a stream with a CU mask enabling every CU; the HIP runtime shares its
 * GPU_MAX_HW_QUEUES queues among unmasked streams only).  Two engines whose
 * streams share a queue run one after the other; serving callers that keep
 * two stripes in flight on two engines create the second one this way so the
 * pair overlaps deterministically (profiles/r05_queues.txt).
 * Unknown flags: RS16_INVALID_ARGUMENT. */
enum { RS16_ENGINE_OWN_QUEUE = 1 };
rs16_engine* rs16_engine_new_ex(int device, int flags, rs16_error* err);
void rs16_engine_free(rs16_engine* eng);
int rs16_engine_device(const rs16_engine* eng);
void* rs16_engine_stream(const rs16_engine* eng);     /* hipStream_t owned by the engine */
int rs16_engine_synchronize(rs16_engine* eng, void* stream, rs16_error* err);

/* Engine::fft (src/engine.rs:158-165): in-place DIT FFT on shards
 * [pos, pos+size) of `data` (shard_count x shard_bytes, device).  Outputs
 * [pos, pos+truncated_size) are exact for any input.  */
int rs16_engine_fft(rs16_engine* eng, void* data, size_t shard_count, size_t shard_bytes, size_t pos, size_t size,
                    size_t truncated_size, size_t skew_delta, void* stream, rs16_error* err);
/* Engine::fft_skew_end (src/engine.rs:222-230): skew_delta = pos + size. */
int rs16_engine_fft_skew_end(rs16_engine* eng, void* data, size_t shard_count, size_t shard_bytes, size_t pos,
                             size_t size, size_t truncated_size, void* stream, rs16_error* err);
/* Engine::ifft (src/engine.rs:188-195).  As in the reference contract,
 * shards [pos+truncated_size, pos+size) must be zero on input. */
int rs16_engine_ifft(rs16_engine* eng, void* data, size_t shard_count, size_t shard_bytes, size_t pos, size_t size,
                     size_t truncated_size, size_t skew_delta, void* stream, rs16_error* err);
/* Engine::ifft_skew_end (src/engine.rs:242-250). */
int rs16_engine_ifft_skew_end(rs16_engine* eng, void* data, size_t shard_count, size_t shard_bytes, size_t pos,
                              size_t size, size_t truncated_size, void* stream, rs16_error* err);
/* Engine::fwht (src/engine.rs:175) on a device u16[65536]; data beyond
 * truncated_size must be zero (the only way eval_poly uses it).  Bit-exact
 * u16 outputs: the engine-level op runs the reference's layer order with its
 * add_mod / sub_mod (src/engine.rs:90-100), so 0 and 65535 come out where the
 * reference has them (tests/test_gpu_engine.py).  The decoders' internal
 * erasure-log kernels only need the residue mod 65535 and use a faster order
 * (both values mean the same log, exp[65535] == exp[0], src/engine/tables.rs:118). */
int rs16_engine_fwht(rs16_engine* eng, uint16_t* d_data, size_t truncated_size, void* stream, rs16_error* err);
/* Engine::eval_poly (src/engine.rs:207-218) on a device u16[65536]; bit-exact
 * as rs16_engine_fwht. */
int rs16_engine_eval_poly(rs16_engine* eng, uint16_t* d_erasures, size_t truncated_size, void* stream,
                          rs16_error* err);
/* Engine::mul (src/engine.rs:198): x[] *= log_m, bytes % 64 == 0. */
int rs16_engine_mul(rs16_engine* eng, void* d_x, size_t bytes, uint16_t log_m, void* stream, rs16_error* err);
/* Engine::xor (src/engine.rs:201): x[] ^= y[], bytes % 64 == 0. */
int rs16_engine_xor(rs16_engine* eng, void* d_x, const void* d_y, size_t bytes, void* stream, rs16_error* err);
/* Engine::xor_within (src/engine.rs:256-259), ranges must not overlap. */
int rs16_engine_xor_within(rs16_engine* eng, void* data, size_t shard_count, size_t shard_bytes, size_t x, size_t y,
                           size_t count, void* stream, rs16_error* err);
/* Engine::formal_derivative (src/engine.rs:233-238); shard_count must be a
 * power of two (the reference panics on slice bounds otherwise). */
int rs16_engine_formal_derivative(rs16_engine* eng, void* data, size_t shard_count, size_t shard_bytes, void* stream,
                                  rs16_error* err);

/* ---- Rates -- src/rate.rs:51-107, src/rate/rate_default.rs:15-64 --------- */
typedef enum rs16_rate { RS16_RATE_DEFAULT = 0, RS16_RATE_HIGH = 1, RS16_RATE_LOW = 2 } rs16_rate;
/* Rate::supports / ReedSolomonEncoder::supports (src/reed_solomon.rs:76-84). */
int rs16_supports(int rate, size_t original_count, size_t recovery_count);
/* Rate::validate (src/rate.rs:91-106).  Shards of 4 GiB or more are an
 * invalid shard size here (the kernels keep row strides in 32 bits). */
int rs16_validate(int rate, size_t original_count, size_t recovery_count, size_t shard_bytes, rs16_error* err);
/* use_high_rate (src/rate/rate_default.rs:15-64): 1 high, 0 low, -1 error. */
int rs16_use_high_rate(size_t original_count, size_t recovery_count, rs16_error* err);
/* {High,Low}Rate{Encoder,Decoder}::work_count (rate_high.rs:131-137,301-305; rate_low.rs:131-137,301-305). */
size_t rs16_encoder_work_count(int high, size_t original_count, size_t recovery_count);
size_t rs16_decoder_work_count(int high, size_t original_count, size_t recovery_count);

/* ---- Encoder -- RateEncoder (src/rate.rs:113-173) with the Rate chosen
 *      by `rate`; RS16_RATE_DEFAULT == ReedSolomonEncoder (src/reed_solomon.rs:13-85).
 *      Work space lives in HBM (EncoderWork, src/rate/encoder_work.rs). */
typedef struct rs16_encoder rs16_encoder;
rs16_encoder* rs16_encoder_new(rs16_engine* eng, int rate, size_t original_count, size_t recovery_count,
                               size_t shard_bytes, rs16_error* err);
void rs16_encoder_free(rs16_encoder* enc);
int rs16_encoder_reset(rs16_encoder* enc, size_t original_count, size_t recovery_count, size_t shard_bytes,
                       rs16_error* err);
/* add_original_shard (src/rate/encoder_work.rs:49-69); shard in host memory.
 * The shard is copied (host memcpy, no device call) into a page-locked image
 * of the work buffer; consecutive shards stream to HBM in 1 MiB DMA copies
 * while the caller keeps adding, so the caller may reuse its buffer at once. */
int rs16_encoder_add_original_shard(rs16_encoder* enc, const void* shard, size_t len, rs16_error* err);
/* same, shard in device memory (copied on the engine stream). */
int rs16_encoder_add_original_shard_device(rs16_encoder* enc, const void* d_shard, size_t len, rs16_error* err);
/* encode (rate_high.rs:44-83 / rate_low.rs:44-83); on success the
 * EncoderResult (src/encoder_result.rs) is valid until rs16_encoder_result_drop.
 * Returns once the work is enqueued on the engine stream: the last staged
 * rows go to HBM, the passes run, and when any original came from host
 * memory the recovery rows come back in one DMA copy to page-locked memory
 * (rs16_encoder_recovery waits for it).
 * The encode works in place: calling it again while the result is held
 * returns RS16_INVALID_ARGUMENT (the reference's &mut borrow makes that a
 * compile error, src/rate.rs:157-166); add_original_shard in that state
 * returns TooManyOriginalShards, as every original is in. */
int rs16_encoder_encode(rs16_encoder* enc, rs16_error* err);
/* EncoderResult::recovery (src/encoder_result.rs:16-19): host pointer to
 * recovery shard `index` (shard_bytes, page-locked, valid until the result is
 * dropped), NULL if index >= recovery_count (or on a device error, err set).
 * The first call waits for the recovery rows to be in host memory. */
const void* rs16_encoder_recovery(rs16_encoder* enc, size_t index, rs16_error* err);
/* The same shard in HBM: device pointer, NULL if index >= recovery_count. */
const void* rs16_encoder_recovery_device(rs16_encoder* enc, size_t index);
/* Copy recovery shard `index` to host memory; returns 1 if it exists, 0 if not, <0 on error. */
int rs16_encoder_recovery_copy(rs16_encoder* enc, size_t index, void* dst, size_t len, rs16_error* err);
/* Drop for EncoderResult (src/encoder_result.rs:48-52). */
void rs16_encoder_result_drop(rs16_encoder* enc);
int rs16_encoder_is_high_rate(const rs16_encoder* enc);

/* ---- Decoder -- RateDecoder (src/rate.rs:179-250); RS16_RATE_DEFAULT ==
 *      ReedSolomonDecoder (src/reed_solomon.rs:93-183). */
typedef struct rs16_decoder rs16_decoder;
rs16_decoder* rs16_decoder_new(rs16_engine* eng, int rate, size_t original_count, size_t recovery_count,
                               size_t shard_bytes, rs16_error* err);
void rs16_decoder_free(rs16_decoder* dec);
int rs16_decoder_reset(rs16_decoder* dec, size_t original_count, size_t recovery_count, size_t shard_bytes,
                       rs16_error* err);
/* add_original_shard / add_recovery_shard (src/rate/decoder_work.rs:62-116).
 * Host shards are staged like the encoder's (page-locked image of the work
 * layout, runs of consecutive positions streamed to HBM while adding). */
int rs16_decoder_add_original_shard(rs16_decoder* dec, size_t index, const void* shard, size_t len, rs16_error* err);
int rs16_decoder_add_recovery_shard(rs16_decoder* dec, size_t index, const void* shard, size_t len, rs16_error* err);
int rs16_decoder_add_original_shard_device(rs16_decoder* dec, size_t index, const void* d_shard, size_t len,
                                           rs16_error* err);
int rs16_decoder_add_recovery_shard_device(rs16_decoder* dec, size_t index, const void* d_shard, size_t len,
                                           rs16_error* err);
/* decode (rate_high.rs:168-247 / rate_low.rs:168-247); DecoderResult valid until drop.
 * The decode restores in place: decode or add_*_shard while the result is
 * held returns RS16_INVALID_ARGUMENT (a compile error in the reference). */
int rs16_decoder_decode(rs16_decoder* dec, rs16_error* err);
/* DecoderResult::restored_original (src/decoder_result.rs:16-19): host
 * pointer to restored original `index` (page-locked, valid until the result
 * is dropped), NULL if it was received or index >= original_count (or on a
 * device error, err set).  After a decode with host shards the restored rows
 * come back in one DMA copy; the first call waits for it. */
const void* rs16_decoder_restored_original(rs16_decoder* dec, size_t index, rs16_error* err);
/* The same shard in HBM: device pointer or NULL. */
const void* rs16_decoder_restored_original_device(rs16_decoder* dec, size_t index);
/* Copy restored original `index` to host; returns 1 if restored, 0 if None, <0 on error. */
int rs16_decoder_restored_original_copy(rs16_decoder* dec, size_t index, void* dst, size_t len, rs16_error* err);
/* Drop for DecoderResult (src/decoder_result.rs:44-48). */
void rs16_decoder_result_drop(rs16_decoder* dec);
int rs16_decoder_is_high_rate(const rs16_decoder* dec);

/* ---- Device-resident one-shot codec (the benchmark path) -----------------
 * reed_solomon_16::encode (src/lib.rs:242-279) with originals and recovery
 * already in HBM: d_original = original_count shards, d_recovery receives
 * recovery_count shards.  Default rate selection as ReedSolomonEncoder. */
int rs16_encode_device(rs16_engine* eng, size_t original_count, size_t recovery_count, size_t shard_bytes,
                       const void* d_original, void* d_recovery, void* stream, rs16_error* err);
/* rs16_encode_device for `nstripes` independent stripes of one geometry in
 * one call (many objects, each its own codeword set; SURVEY.md 8(f)3
 * "batched independent codewords"): stripe i's original_count shards at
 * d_original + i * original_stride bytes, its recovery_count shards written
 * at d_recovery + i * recovery_stride (strides >= count * shard_bytes and
 * multiples of 64, else RS16_INVALID_ARGUMENT).
 * Every stripe's result equals rs16_encode_device on it alone.  High-rate
 * stripes with original_count <= next_pow2(recovery_count) -- every stripe
 * with original_count <= recovery_count -- run batched, each pass launch
 * covering all stripes, so stripes far below the chip's size (100:100,
 * 1000:1000) still fill it; other shapes run stripe after stripe.  The
 * reference encodes one stripe per call (src/lib.rs:242-279). */
int rs16_encode_device_batch(rs16_engine* eng, size_t original_count, size_t recovery_count, size_t shard_bytes,
                             size_t nstripes, const void* d_original, size_t original_stride, void* d_recovery,
                             size_t recovery_stride, void* stream, rs16_error* err);
/* reed_solomon_16::decode (src/lib.rs:287-344), device-resident: d_original
 * holds original_count shard slots (received ones valid, flagged by the
 * device byte array d_original_received); d_recovery holds recovery_count
 * slots flagged by d_recovery_received.  The host passes the number of
 * received shards of each kind: they give the reference's NotEnoughShards /
 * nothing-to-do checks AND select the launch -- a count of 0 means "no
 * shard of this kind was received", and the first pass then launches no
 * tile of that segment.  The counts MUST equal the number of nonzero flags
 * (a 0 count with set flags drops those shards and restores wrong data
 * without an error; rs16_decode_check detects it after the fact).  Lost
 * originals are restored in place into d_original.  Default rate selection
 * as ReedSolomonDecoder. */
int rs16_decode_device(rs16_engine* eng, size_t original_count, size_t recovery_count, size_t shard_bytes,
                       void* d_original, const uint8_t* d_original_received, const void* d_recovery,
                       const uint8_t* d_recovery_received, size_t original_received_count,
                       size_t recovery_received_count, void* stream, rs16_error* err);
/* rs16_decode_device for `nstripes` independent stripes that lost the same
 * shards -- the case of a failed device, which holds the same shard index of
 * every stripe: the received flags and counts are shared, stripe i's
 * original slots at d_original + i * original_stride bytes (lost ones
 * restored in place), its recovery at d_recovery + i * recovery_stride
 * (strides as for rs16_encode_device_batch).
 * One eval_poly for all, every pass launch covering all stripes.  Every
 * stripe's result equals rs16_decode_device on it alone. */
int rs16_decode_device_batch(rs16_engine* eng, size_t original_count, size_t recovery_count, size_t shard_bytes,
                             size_t nstripes, void* d_original, size_t original_stride,
                             const uint8_t* d_original_received, const void* d_recovery, size_t recovery_stride,
                             const uint8_t* d_recovery_received, size_t original_received_count,
                             size_t recovery_received_count, void* stream, rs16_error* err);
/* rs16_decode_device for `nstripes` independent stripes, EACH WITH ITS OWN
 * received set (the reference decodes one stripe per call with that call's
 * received shards: src/lib.rs:287-344, src/rate/decoder_work.rs:62-139):
 * stripe i's flags at d_original_received + i * original_received_stride and
 * d_recovery_received + i * recovery_received_stride (strides >= the counts),
 * its received counts in the HOST arrays original_received_counts[i] /
 * recovery_received_counts[i] (which must equal its flags, as for
 * rs16_decode_device), its shards as for rs16_decode_device_batch.  Errors are
 * the per-stripe ones (NotEnoughShards with the first failing stripe's
 * numbers).  One eval_poly launch with a grid row per stripe, then pass
 * launches shared by all stripes.  Every stripe's result equals
 * rs16_decode_device on it alone.  (rs16_decode_check does not cover it.) */
int rs16_decode_device_batch_varied(rs16_engine* eng, size_t original_count, size_t recovery_count,
                                    size_t shard_bytes, size_t nstripes, void* d_original, size_t original_stride,
                                    const uint8_t* d_original_received, size_t original_received_stride,
                                    const void* d_recovery, size_t recovery_stride,
                                    const uint8_t* d_recovery_received, size_t recovery_received_stride,
                                    const size_t* original_received_counts, const size_t* recovery_received_counts,
                                    void* stream, rs16_error* err);
/* Repair: rs16_decode_device with d_recovery writable.  Lost originals are
 * restored in place, and lost recovery shards are regenerated in place, equal
 * to what rs16_encode_device writes for the full stripe -- the stripe is back
 * at full redundancy without a decode followed by an encode of everything.
 * Received slots of both arrays are not written.  Rate selection, flag bytes
 * (0 = lost, any other value = received), the 64-byte alignment, asynchrony on
 * `stream`, the ordering on the engine's scratch and the discard of a pending
 * rs16_decode_prepare are those of rs16_decode_device; the counts MUST equal
 * the flags, as there.
 * Errors, in this order: UnsupportedShardCount / InvalidShardSize as
 * rs16_validate gives them; InvalidArgument for a NULL or misaligned array
 * (the flag arrays included) and, in the batch form, a bad stride; InvalidArgument
 * for a count above its shard count, NotEnoughShards (with the decode's
 * payload) for fewer than original_count received.  Everything received:
 * RS16_OK, nothing launched.
 * Three paths (rs16_host_repair_path):
 *   1  no recovery shard lost: rs16_decode_device itself, every form of it.
 *   2  no original lost: the engine's encode into a buffer of its own
 *      (recovery_count x shard_bytes per stripe, kept by the engine) and one
 *      copy kernel for the rows whose flag is 0.  Costs the encode plus the
 *      copy, about half a general decode.
 *   3  both kinds lost: the general decode's passes, the last one revealing
 *      and storing the lost rows of both segments (each workgroup of it
 *      returns at once when its tile holds no lost row).  Always the pass
 *      codec: stripes of up to 2048 work rows, which rs16_decode_device runs in
 *      the one-launch column codec, take three launches here.
 * When to prefer it (measured on one MI355X at 1 KiB shards, DESIGN.md 3.16,
 * profiles/r16_repair.txt): at 32768:32768 with both kinds lost it beats
 * rs16_decode_device + rs16_encode_device at every pattern tried -- 177
 * against 206 us with 1 % of each kind lost at random, 134 against 146 with
 * one shard of each, 184 against 202 at 25 %, 143 against 150 with clustered
 * losses (where the decode alone has faster kernels the repair does not
 * take).  At 1000:1000 it LOSES, 30.0-31.6 against 26.1-27.6 us: stripes of up
 * to 2048 work rows decode in one launch of the column codec and the repair
 * takes eval_poly plus three passes, so there decode + encode is the faster
 * way to a whole stripe.  Sizes in between are not measured.  Recovery only:
 * the encode plus 2.4-5.3 us for the copy, and only the lost rows are
 * written.  With no recovery shard lost it IS the decode.
 * rs16_decode_check covers paths 1 and 3 as it covers the decode; after path
 * 2 (no kernel read the originals' flags) it reports RS16_OK.
 * Column slices (rs16_engine_set_slices) apply to path 1 only: paths 2 and 3
 * run one slice whatever the setting (results are the same). */
int rs16_repair_device(rs16_engine* eng, size_t original_count, size_t recovery_count, size_t shard_bytes,
                       void* d_original, const uint8_t* d_original_received, void* d_recovery,
                       const uint8_t* d_recovery_received, size_t original_received_count,
                       size_t recovery_received_count, void* stream, rs16_error* err);
/* rs16_repair_device for `nstripes` stripes that lost the same shards (a failed
 * device holds the same index of every stripe): one shared pattern, arrays and
 * strides as for rs16_decode_device_batch.  Every stripe's result equals
 * rs16_repair_device on it alone. */
int rs16_repair_device_batch(rs16_engine* eng, size_t original_count, size_t recovery_count, size_t shard_bytes,
                             size_t nstripes, void* d_original, size_t original_stride,
                             const uint8_t* d_original_received, void* d_recovery, size_t recovery_stride,
                             const uint8_t* d_recovery_received, size_t original_received_count,
                             size_t recovery_received_count, void* stream, rs16_error* err);
/* Selective decode, the degraded read: rs16_decode_device restoring only the
 * lost originals the caller asks for.  d_original_wanted is the read set, a
 * device array of original_count bytes: a byte other than 0 means "wanted" (any
 * nonzero value, as for the received flags).  The array needs no alignment, and
 * no byte outside [0, original_count) is read as a flag.
 *   - a lost original (flag 0) whose wanted byte is nonzero is restored in
 *     place, bit-equal to what rs16_decode_device writes there;
 *   - a lost original whose wanted byte is 0 is NOT written: its slot keeps
 *     its bytes;
 *   - wanted bytes of received originals are ignored; received slots are never
 *     written; d_recovery is read only.
 * wanted_count is the number of lost originals in the read set (rows with flag
 * 0 and a nonzero wanted byte).  Like the received counts it comes from the
 * host, MUST equal what the device arrays say, and selects the launches:
 *   - 0: nothing is launched (RS16_OK), whatever the read set holds;
 *   - original_count - original_received_count: the call IS the plain decode,
 *     the read set is not read and every lost original is restored;
 *   - values in between only steer two host gates (whether the direct middle
 *     pass and the per-column last pass are launched beside the general ones).
 *     The device decides by the row interval of the lost-and-wanted originals,
 *     which it computes itself from the two arrays, and restores exactly the
 *     rows the arrays name: a wrong value in this range costs time, not
 *     correctness.  rs16_decode_check does not verify it.
 * The erasure locator still comes from ALL erasures -- only the row interval
 * that prunes the passes, the reveal and the stores follow the read set.
 * Rate selection, the 64-byte alignment of the shard arrays, asynchrony on
 * `stream`, the ordering on the engine's scratch, the discard of a pending
 * rs16_decode_prepare and rs16_decode_check afterwards are those of
 * rs16_decode_device.
 * Errors, in this order: UnsupportedShardCount / InvalidShardSize as
 * rs16_validate gives them; InvalidArgument for a NULL or misaligned shard
 * array, a NULL flag or wanted array and, in the batch form, a bad stride;
 * InvalidArgument for a count above its shard count or wanted_count above
 * original_count - original_received_count; NotEnoughShards (with the decode's
 * payload) for fewer than original_count received.  Then: everything received
 * or wanted_count == 0 gives RS16_OK with nothing launched.
 * Paths (rs16_host_select_path): 1 = rs16_decode_device itself, every form of
 * it; 2 = the selective decode -- never the half-transform or identity decode
 * (they store every original), one launch of the column codec up to 2048 work
 * rows, else eval_poly and the general decode's passes with the middle pass
 * as a direct product and the last pass on the wanted rows' tiles only.
 * Column slices (rs16_engine_set_slices) apply to path 1 only.
 * When to prefer it (measured on one MI355X at 1 KiB shards with every recovery
 * shard received, DESIGN.md 3.17, profiles/r17_select.txt; the other candidate
 * is rs16_decode_device on the same stripe and pattern): when the rows wanted
 * lie in few 256-row tiles of a large stripe that has received originals.  At
 * 32768:32768 one row read out of a 1 % loss scattered over every tile takes
 * 90.4 us against the decode's 148.5 (0.61 x; the select's median burst lies
 * below the decode's fastest), out of a random 50 % loss 87.9 against 146.9, 16
 * rows of one tile 89.1 against 146.6.  What remains is the locator, the gather
 * and the first transform of every received row, which no read set shortens.
 * It does NOT win where the read set is spread over every tile -- every second
 * lost row: 147.9 against 148.8 and 145.8 against 147.4 us, the decode's cost --
 * and it LOSES where every original is lost: the plain call then takes the
 * half-transform / identity decode, which stores every original and which a
 * selective call cannot take, 62.1 against 56.6 us for one row and 107.8
 * against 56.5 for every second row at 32768:32768, 13.2-14.6 against 11.1 at
 * 1000:1000.  There, decode into a scratch array if the other slots must keep
 * their bytes.  At 1000:1000 with received originals the call is one launch
 * either way and there is little to prune: 17.6-19.5 against 19.1-19.7 us.
 * Sizes in between are not measured. */
int rs16_decode_device_select(rs16_engine* eng, size_t original_count, size_t recovery_count, size_t shard_bytes,
                              void* d_original, const uint8_t* d_original_received,
                              const uint8_t* d_original_wanted, const void* d_recovery,
                              const uint8_t* d_recovery_received, size_t original_received_count,
                              size_t recovery_received_count, size_t wanted_count, void* stream, rs16_error* err);
/* rs16_decode_device_select for `nstripes` stripes that lost the same shards
 * and are read at the same indices: one shared pattern and one shared read
 * set, arrays and strides as for rs16_decode_device_batch.  Every stripe's
 * result equals rs16_decode_device_select on it alone. */
int rs16_decode_device_select_batch(rs16_engine* eng, size_t original_count, size_t recovery_count,
                                    size_t shard_bytes, size_t nstripes, void* d_original, size_t original_stride,
                                    const uint8_t* d_original_received, const uint8_t* d_original_wanted,
                                    const void* d_recovery, size_t recovery_stride,
                                    const uint8_t* d_recovery_received, size_t original_received_count,
                                    size_t recovery_received_count, size_t wanted_count, void* stream,
                                    rs16_error* err);
/* Scrub: verify a stripe's stored recovery shards on the device.  Tells whether
 * the recovery shards in d_recovery still equal the encode of the originals in
 * d_original and, if not, which recovery shards and which byte columns differ.
 * d_original holds all original_count shards, d_recovery recovery_count slots;
 * both are READ ONLY and 64-byte aligned like every other device shard array.
 * Rate selection is that of rs16_encode_device.
 * The check set d_recovery_checked: NULL means every recovery shard is checked;
 * otherwise recovery_count bytes, 0 = "do not compare this slot" (the shard may
 * be missing: the slot's bytes are never read as data that matters), any nonzero
 * byte = "compare".  It needs no alignment, and no byte outside [0,
 * recovery_count) is read.
 * Outputs: d_recovery_mismatch[j] is written for every j < recovery_count,
 * whatever it held before: 1 when shard j is checked and differs in at least one
 * byte from what rs16_encode_device would write there for these originals, else
 * 0.  d_column_mismatch may be NULL; if given it is shard_bytes / 64 bytes, and
 * byte c is 1 when some checked recovery shard differs within bytes [64 c, 64 c
 * + 64), else 0.  Every 64-byte column block is an independent codeword, so the
 * pair of arrays tells "one recovery shard rotted" (one row, few columns) from
 * "an original rotted" (many rows at the same columns).  Neither output array
 * needs alignment; no byte outside them is written.  There is no count and no
 * "which original is bad" here: rs16_locate_device below names the one corrupt
 * shard of each column block.
 * The call is asynchronous on `stream` and ordered on the engine's scratch like
 * an encode.  Like rs16_encode_device it is not a decode: it neither discards a
 * pending rs16_decode_prepare nor changes what rs16_decode_check reports.
 * Column slices (rs16_engine_set_slices) do not apply.
 * Errors, in this order: UnsupportedShardCount / InvalidShardSize as
 * rs16_validate gives them; InvalidArgument for a NULL or misaligned shard
 * array, a NULL d_recovery_mismatch and, in the batch form, a bad stride or
 * nstripes > 2^20.  nstripes == 0: RS16_OK, nothing launched.
 * Two paths (rs16_host_verify_path), both starting with a clear of the flag arrays
 * on the stream; the kernels only ever store the byte 1:
 *   1 = fused: the encode's own launches up to the last one, whose place a
 *       comparing form of it takes (ENC_LAST_VFY / ENC_SINGLE_VFY): it loads the
 *       stored row where the encode would store the computed one and writes
 *       flag bytes where they differ.  No second recovery array, no store sweep,
 *       no compare launch.  Exists where the engine's encode of the shape ends
 *       in a pass-codec store pass: not for stripes the column codec encodes
 *       (512 / 1024-row chunks up to 2 KiB of quad columns, the multi-chunk
 *       column forms) nor for chunks below 16 rows in the multi-chunk rates or
 *       one-row chunks.  Its three-pass sequence keeps the work rows in the
 *       shards' form (as under RS16_DIAG_NO_PAIRED_ROWS).
 *   0 = encode + compare: the engine's encode into a buffer of its own
 *       (recovery_count x shard_bytes per stripe, reserved on first use), then
 *       one compare kernel (VERIFY_CMP) over it and the stored shards.
 * RS16_DIAG_NO_FUSED_VERIFY / RS16_DIAG_FORCE_FUSED_VERIFY force either path
 * wherever it exists; the flags are identical under both.
 * When to prefer it (measured on one MI355X per run at 1 KiB shards, clean and
 * with one original corrupted, DESIGN.md 3.18, profiles/r18_verify.txt; the
 * other candidate is an encode into a second array plus a compare kernel of the
 * caller's own, which is what path 0 does inside the library): a scrub costs an
 * encode plus 4-17 us, and never a second recovery array of the caller's.  Over
 * rs16_encode_device alone, on the default path: +15.7 to +16.8 us at
 * 32768:32768 (76 against 60 us), +6.5 to +7.2 at 8000:8000 (41 against 34),
 * +8.1 to +8.3 at 60000:3000 (107 against 98), +10.0 to +11.6 at 5:3000 (18.7
 * against 7.3), +7.5 to +8.1 at 1000:1000 (15.6 against 7.8), +3.8 to +7.4 for
 * the batches below.  The default path is the fused one only where it was faster than
 * encode + compare in every alternating pair of every run, clean and corrupted:
 * batches of 4 or more one-chunk high-rate stripes of 1024-row chunks (513 ..
 * 1024 recovery shards, at most as many originals), which are too wide for the
 * column codec -- 4 / 8 / 32 x 1000:1000: 23.1 / 28.8 / 68.3 us against 25.5 /
 * 30.0 / 75.8 (0.91 / 0.96 / 0.90 x).  Everywhere else the default is encode +
 * compare and the fused kernels stay reachable through the force flag: at
 * 32768:32768 the fused path is 0.4-1.3 us faster in the median (75.7 against
 * 76.1 us) but lost 1 to 3 of 9 pairs per run -- its three passes keep the work
 * rows in the shards' form (the middle pass 32.5 against 27.6 us in tower form)
 * and its last pass takes 26.2 us against 19.4, which together give back most of
 * the 14.2 us compare kernel; at 8000:8000 it is 0.2-0.8 us SLOWER (41.3 against
 * 40.8) and at 60000:3000 1.2-1.6 us slower (107.9 against 106.7), losing every
 * pair but two; one 1000:1000 stripe forced through the passes
 * (RS16_DIAG_NO_COLUMN) is 1.4-1.7 us faster fused (20.3 against 22.0) but won
 * only 7 of 9 pairs in one of three runs.  Stripes the column codec encodes and
 * chunks below 16 rows in the multi-chunk rates have no fused kernel.  Sizes in
 * between are not measured. */
int rs16_verify_device(rs16_engine* eng, size_t original_count, size_t recovery_count, size_t shard_bytes,
                       const void* d_original, const void* d_recovery, const uint8_t* d_recovery_checked,
                       uint8_t* d_recovery_mismatch, uint8_t* d_column_mismatch, void* stream, rs16_error* err);
/* rs16_verify_device for `nstripes` stripes: stripe i's shards at + i
 * original_stride / recovery_stride (multiples of 64, at least the arrays'
 * sizes), its flags at d_recovery_mismatch + i recovery_mismatch_stride and
 * d_column_mismatch + i column_mismatch_stride (at least recovery_count and
 * shard_bytes / 64; anything smaller is InvalidArgument).  Only each stripe's
 * used range is written: bytes between the strides stay as they were.  The
 * check set is shared by all stripes: a failed device holds the same index of
 * every stripe.  Every stripe's flags equal rs16_verify_device on it alone. */
int rs16_verify_device_batch(rs16_engine* eng, size_t original_count, size_t recovery_count, size_t shard_bytes,
                             size_t nstripes, const void* d_original, size_t original_stride,
                             const void* d_recovery, size_t recovery_stride, const uint8_t* d_recovery_checked,
                             uint8_t* d_recovery_mismatch, size_t recovery_mismatch_stride,
                             uint8_t* d_column_mismatch, size_t column_mismatch_stride, void* stream, rs16_error* err);
/* Locate: which ONE shard of each 64-byte column block is corrupt.  The scrub
 * above says that a stripe is inconsistent; this call says which shard to
 * distrust, per column block, and by what to XOR it to make the block
 * consistent again -- what a caller needs to fix a silently rotted shard in
 * place, or to set the received flags of rs16_repair_device.  The case is one
 * device rotting silently: one corrupt shard per codeword.  No reference
 * counterpart (the reference has erasure decoding only).
 * The encode is GF(2^16)-linear per element position, recovery_j = sum_i
 * M[j][i] original_i, and the code is MDS.  With syndrome_j = encode(stored
 * originals)_j ^ stored recovery_j: one corrupt recovery shard j makes exactly
 * syndrome_j nonzero; one corrupt original i with error e makes every syndrome
 * nonzero, syndrome_j = M[j][i] e, and syndrome_0 / syndrome_1 = M[0][i] /
 * M[1][i] names i, because every 2 x 2 minor of M is nonzero.
 *
 * A plan is per (rate, original_count, recovery_count) and holds rows 0 and 1
 * of M on the device as logs, a table ratio -> i and the field's log / exp
 * tables.  `rate` means what it means for rs16_update_plan_new: the rate the
 * stripe was encoded with, RS16_RATE_DEFAULT = the choice of rs16_encode_device.
 * rs16_locate_plan_new is synchronous: the two rows come from the engine's own
 * encode of unit vectors (exact on every rate path) -- original i carries the
 * element 1 at element position i of a stripe of 64 ceil(original_count / 32)
 * bytes per shard, taken in column chunks of 1 KiB shards (512 originals each,
 * 64 encodes at 32768:32768), of which only recovery rows 0 and 1 are copied
 * back.  Errors, in this order: UnsupportedShardCount as rs16_validate gives it
 * for `rate`; recovery_count < 2: InvalidArgument (distance 2 detects an error
 * and cannot locate it).  Like an update plan, a locate plan is attached to its
 * engine and detached by rs16_engine_free: later calls on it fail with
 * RS16_INVALID_ARGUMENT and rs16_locate_plan_free then frees only host memory.
 * Calls enqueued on a caller's stream must have finished before the plan or its
 * engine is freed (the kernels read the plan's tables).
 *
 * rs16_locate_device fills one entry per 64-byte column block c < B =
 * shard_bytes / 64; every entry is written, whatever it held before:
 *   RS16_LOCATE_CLEAN        every recovery shard equals the encode in this
 *                            block.  d_block_shard[c] = 0xFFFFFFFF, fix = 0.
 *   RS16_LOCATE_RECOVERY     d_block_shard[c] = j: every inconsistent element
 *                            of the block has exactly one nonzero syndrome, in
 *                            the same row j.  The fix is row j's syndrome bytes
 *                            of this block.
 *   RS16_LOCATE_ORIGINAL     d_block_shard[c] = i: every inconsistent element
 *                            of the block is explained by an error in original i
 *                            alone -- verified against all recovery_count
 *                            recovery shards, not only rows 0 and 1.  The fix is
 *                            the error in the shard layout, 32 low bytes then 32
 *                            high bytes.
 *   RS16_LOCATE_UNLOCATABLE  anything else: 2 .. recovery_count - 1 nonzero
 *                            syndromes at an element, a ratio no original has, a
 *                            candidate that fails the check against all rows,
 *                            elements of one block that name different shards.
 *                            d_block_shard[c] = 0xFFFFFFFF, fix = 0.
 * d_block_fix may be NULL; if given it is B x 64 bytes: XOR block c of it into
 * bytes [64 c, 64 c + 64) of the named shard and the block is consistent.
 * Guarantee: a block in which at most recovery_count - 1 shards are corrupt at
 * any one element position is never attributed to a wrong shard -- it is
 * located when that number is 1 and (elements that disagree aside) reported
 * UNLOCATABLE otherwise.  This follows from the code's minimum distance
 * recovery_count + 1: two error patterns with the same syndromes differ by a
 * codeword, which has at least recovery_count + 1 nonzero shards.  At
 * recovery_count = 2 it covers exactly one corrupt shard: two corrupt shards at
 * one element position can look like a third, and the call then names it.
 * Both shard arrays are READ ONLY and 64-byte aligned like every other device
 * shard array.  d_block_status, d_block_shard and d_block_fix need only their
 * natural alignment; no byte outside them is written.
 * The call is asynchronous on `stream` and ordered on the engine's scratch like
 * rs16_verify_device: it is not a decode, it neither discards a pending
 * rs16_decode_prepare nor changes what rs16_decode_check reports.  Column
 * slices (rs16_engine_set_slices) do not apply.
 * Errors, in this order: a NULL or detached plan: InvalidArgument;
 * InvalidShardSize as rs16_validate gives it; a NULL or misaligned shard array,
 * a NULL d_block_status or d_block_shard: InvalidArgument.
 * The sequence on the device: the engine's encode of d_original into a buffer of
 * its own (as the scrub's path 0); a scan of all recovery_count rows that
 * counts, per element position, the rows with a nonzero syndrome element and
 * keeps the smallest such row; a decide kernel that classifies each block and
 * scatters each ORIGINAL candidate's error e = syndrome_0 / M[0][i] into a
 * zeroed original_count x shard_bytes error array E of the engine; the engine's
 * encode of E; and a confirm kernel that downgrades an ORIGINAL block to
 * UNLOCATABLE unless encode(E) equals the syndrome in all recovery_count rows of
 * the block.  The engine keeps E, both encodes and the counts: (original_count +
 * 2 recovery_count) x shard_bytes beside the encode's work space.
 * Not provided: host-memory forms, more than one corrupt shard
 * per codeword, and skipping the second encode when no block names an original
 * (the host would have to wait for the device to know).
 * When to prefer it (measured on one MI355X at 1 KiB shards, clean and with
 * one original corrupted, bursts alternating with rs16_verify_device of the same
 * stripe on the same build; DESIGN.md 3.19, profiles/r19_locate.txt): a locate
 * costs about two encodes plus three sweeps, 1.6-2.0 x a scrub, so scrub with
 * rs16_verify_device and call this for the stripes it flags.  At 32768:32768:
 * 134.4 us clean and 148.4 with one original corrupted, against the scrub's 73.6
 * and 75.0 (1.83 x / 1.98 x; 2.3 / 2.5 x an encode); of that the two encodes are
 * about 118 us (58.9 each alone), the scan 13.9-14.6 (the scrub's compare kernel: 13.5-14.9), the
 * decide kernel 8 and the confirm kernel 6 clean, 15.8 with a block to check
 * (per-kernel figures under profiling, which lengthens short launches).  At
 * 1000:1000: 24.1 us clean and 27.1 corrupted against 15.4 and 15.6 (1.56 x /
 * 1.73 x), the three kernels at the 6-7.5 us floor of a profiled launch.
 * rs16_locate_plan_new costs 6.0 ms of host time at 32768:32768 (64 encodes) and
 * 0.12 ms at 1000:1000: keep the plan of a geometry that is scrubbed.  Sizes in
 * between are not measured. */
typedef struct rs16_locate_plan rs16_locate_plan;
rs16_locate_plan* rs16_locate_plan_new(rs16_engine* eng, int rate, size_t original_count, size_t recovery_count,
                                       rs16_error* err);
void rs16_locate_plan_free(rs16_locate_plan* plan);
/* Diagnostics / tests: out[i] = M[0][i], out[original_count + i] = M[1][i] as
 * field elements (2 x original_count values). */
int rs16_locate_plan_rows(rs16_locate_plan* plan, uint16_t* out, rs16_error* err);
enum { RS16_LOCATE_CLEAN = 0, RS16_LOCATE_ORIGINAL = 1, RS16_LOCATE_RECOVERY = 2, RS16_LOCATE_UNLOCATABLE = 3 };
int rs16_locate_device(rs16_locate_plan* plan, size_t shard_bytes, const void* d_original, const void* d_recovery,
                       uint8_t* d_block_status, uint32_t* d_block_shard, void* d_block_fix, void* stream,
                       rs16_error* err);
/* Heal: fix located blocks in place; locate and heal stripe batches.  The last
 * link of scrub -> locate -> fix, in the form the other operations have: a
 * rotting device holds the same index of every stripe, so a scrub flags many
 * stripes of one geometry at once.
 *
 * rs16_locate_device_batch is rs16_locate_device for nstripes stripes of the
 * plan's geometry: stripe i's originals at d_original + i original_stride, its
 * recovery at d_recovery + i recovery_stride (bytes, as rs16_encode_device_batch
 * takes them), its status at d_block_status + i status_stride (bytes, >= B),
 * its shard entries at d_block_shard + i shard_stride (ENTRIES, >= B) and its
 * fix at d_block_fix + i fix_stride (bytes, >= 64 B; d_block_fix may be NULL).
 * Stripe i's status, shard and fix are what rs16_locate_device gives on stripe i
 * alone.  Every entry of each stripe's used range is written; bytes between the
 * strides are never written.  Both shard arrays are READ ONLY.
 *
 * rs16_heal_device runs the locate's sequence and then XORs, in place, the 64
 * fix bytes of every block that ends RS16_LOCATE_ORIGINAL into the named
 * original when heal_mask has RS16_HEAL_ORIGINAL, and of every block that ends
 * RS16_LOCATE_RECOVERY into the named recovery shard when it has
 * RS16_HEAL_RECOVERY.  "Ends" means after the confirm kernel: a block
 * downgraded to UNLOCATABLE is never written.  CLEAN blocks, UNLOCATABLE blocks
 * and blocks of a kind outside the mask are not written, and no byte of any
 * other shard or block is.  d_block_status and d_block_shard may be NULL; when
 * given they report what was found BEFORE the fix, exactly as the locate would.
 * d_counts (required) gets four uint32: d_counts[RS16_LOCATE_*] = the number of
 * the stripe's blocks with each final status, all four written whatever they
 * held; the host reads 16 bytes per stripe to learn whether anything stayed
 * UNLOCATABLE (a healed stripe scrubs clean exactly when that count is 0).
 * rs16_heal_device_batch is the same for nstripes stripes: the strides above
 * less the fix's, and stripe i's counts at d_counts + i counts_stride (ENTRIES,
 * >= 4).
 * The guarantee is the locate's: with at most recovery_count - 1 corrupt shards
 * per element position a heal never writes a wrong shard.
 *
 * Errors, in this order: those of rs16_locate_device, the NULL or detached plan
 * first (for the heal a NULL d_block_status or d_block_shard is no error); for
 * the heal a heal_mask of 0 or with unknown bits, then a NULL d_counts:
 * InvalidArgument; for the batch forms a stride of a shard array that is no
 * multiple of 64 or smaller than its stripe, then an output stride below its
 * minimum, then nstripes > 65535: InvalidArgument.  nstripes == 0 is RS16_OK
 * with nothing launched and nothing written.
 * Like rs16_locate_device the calls are asynchronous on `stream`, ordered on the
 * engine's scratch, and no decode: a pending rs16_decode_prepare and the report
 * of rs16_decode_check survive them.  Column slices do not apply.
 * Work space: the engine's buffers of the locate, grown to nstripes x
 * (original_count + 2 recovery_count) x shard_bytes, nstripes x the pairs (16
 * copies of shard_bytes / 2 x 8 bytes up to 64 KiB shards, one above),
 * nstripes x B candidates and, for the heal, nstripes x B x 64 bytes of fix
 * (plus nstripes x B x 5 bytes for the status and shard entries the caller did
 * not ask for), beside the encode's work space.  The batch is never grouped or
 * chunked: an allocation failure is RS16_DEVICE_ERROR, and the caller splits.
 * The sequence on the device: both encodes through the engine's batch encode
 * (the one-chunk high rate in launches that cover all stripes, other shapes
 * stripe by stripe), the scan and the confirm kernel with the stripes in grid z
 * (the scan still aims at about 2048 workgroups in all), the decide kernel over
 * all stripes' blocks numbered through, and for the heal a clear of the counts
 * and one more kernel (16 lanes per block, one dword each).
 * When to prefer it (measured on one MI355X at 1 KiB shards, clean and with one
 * original corrupted per stripe, against N rs16_locate_device calls of the
 * library as it was before the batch forms, each build in a process of its
 * own, five alternating pairs; DESIGN.md 3.20, profiles/r20_heal.txt): from 4
 * flagged stripes of one geometry on, locate them in one call.  N x 1000:1000:
 * 48.4 / 58.6 / 130.1 us clean and 52.8 / 62.7 / 138.1 corrupted for N = 4 / 8 /
 * 32 (12.1 / 7.3 / 4.1 us per stripe) against loops of 96.9 / 192.9 / 793.9 and
 * 109.3 / 216.7 / 908.1 -- 2.0 / 3.3 / 6.1 x and 2.1 / 3.5 / 6.6 x, faster in every
 * pair.  4 x 32768:32768: 467.8 and 484.4 us against 530.4 and 583.5 (1.13 x /
 * 1.20 x, every pair): the encodes dominate there and gain nothing from the
 * batch; the four short kernels are paid once.  The batch of 1000:1000 stripes
 * encodes through the pass kernels, not the column codec (three launches for
 * all stripes), so one stripe through the batch call costs what the single call
 * costs (24.3 / 27.3 us) and two or three are not measured.  The heal adds one
 * clear and one kernel: +3.1 .. +4.6 us per CALL over the locate at every size
 * measured, whatever the stripe count, against a download, a host loop and one
 * 64-byte XOR launch per dirty block.  rs16_locate_device itself is unchanged:
 * 24.39 (24.27 .. 24.44) against 24.45 (24.40 .. 24.50) us clean and 27.40
 * against 27.31 corrupted at 1000:1000; at 32768:32768 134.3 against 134.5 clean,
 * and corrupted 142.4 against 143.0 in one geometry of the run and 148.7 against
 * 143.6 in the other (the same call on other buffers).  Its status, shard and
 * fix are byte-equal to the earlier library's.  Sizes in between are not
 * measured. */
int rs16_locate_device_batch(rs16_locate_plan* plan, size_t shard_bytes, size_t nstripes, const void* d_original,
                             size_t original_stride, const void* d_recovery, size_t recovery_stride,
                             uint8_t* d_block_status, size_t status_stride, uint32_t* d_block_shard,
                             size_t shard_stride, void* d_block_fix, size_t fix_stride, void* stream,
                             rs16_error* err);
enum { RS16_HEAL_ORIGINAL = 1, RS16_HEAL_RECOVERY = 2 }; /* which arrays the heal may write */
int rs16_heal_device(rs16_locate_plan* plan, size_t shard_bytes, void* d_original, void* d_recovery, int heal_mask,
                     uint8_t* d_block_status, uint32_t* d_block_shard, uint32_t* d_counts, void* stream,
                     rs16_error* err);
int rs16_heal_device_batch(rs16_locate_plan* plan, size_t shard_bytes, size_t nstripes, void* d_original,
                           size_t original_stride, void* d_recovery, size_t recovery_stride, int heal_mask,
                           uint8_t* d_block_status, size_t status_stride, uint32_t* d_block_shard,
                           size_t shard_stride, uint32_t* d_counts, size_t counts_stride, void* stream,
                           rs16_error* err);
/* Host arithmetic only, for tests: the scan launch's shape {cw, rsub, gx, gy,
 * rows_per_wg} for nstripes stripes -- cw column lanes by rsub rows per
 * workgroup pass, gx workgroups over the columns, gy over the rows of
 * rows_per_wg each.  0, or -1 for a shard size, recovery count or stripe count
 * that no locate takes. */
int rs16_host_locate_scan_shape(size_t shard_bytes, size_t recovery_count, size_t nstripes, uint32_t out[5]);
/* Checked mode of the engine's last decode: waits for `stream` and compares
 * the received counts that decode was given with the rows the device flags
 * mark received (the eval_poly kernels count them per 64-row chunk as they
 * scan the flags, off the host's path).  RS16_OK when they agree (or no
 * decode ran), else RS16_INVALID_ARGUMENT with v0 / v1 = the originals /
 * recovery shards the flags mark received. */
int rs16_decode_check(rs16_engine* eng, void* stream, rs16_error* err);
/* Concurrent column slices of rs16_encode_device / rs16_decode_device (1..4,
 * default 1): the shard columns are split into slices of multiples of 64
 * bytes (each 64-byte column block is an independent codeword, so results
 * are identical) that run on internal streams forked from and joined back
 * into the call's stream.  The calls stay asynchronous and ordered on
 * `stream`.  On MI355X / ROCm 7.2 the fork/join costs more than the overlap
 * gains; independent codecs belong on independent streams. */
int rs16_engine_set_slices(rs16_engine* eng, int slices, rs16_error* err);

/* ---- Host-resident one-shot codec ---------------------------------------
 * reed_solomon_16::encode / decode (src/lib.rs:242-344) with every shard in
 * host memory (page-locked, rs16_host_alloc, for DMA-rate copies; pageable
 * works too).  The shard columns are processed in slices of slice_bytes (a
 * multiple of 64; 0 = the whole shard) that alternate between two streams,
 * so that the host->device copy of one slice, the device codec of another
 * and the device->host copy of a third may overlap (on MI355X the pitched
 * copies of narrow slices cost more than the overlap gains; see
 * DESIGN.md).  Synchronous: returns when the
 * outputs are in host memory.  Decode: received flags are host byte arrays;
 * lost originals are restored in place into h_original. */
int rs16_encode_host(rs16_engine* eng, size_t original_count, size_t recovery_count, size_t shard_bytes,
                     const void* h_original, void* h_recovery, size_t slice_bytes, rs16_error* err);
int rs16_decode_host(rs16_engine* eng, size_t original_count, size_t recovery_count, size_t shard_bytes,
                     void* h_original, const uint8_t* original_received, const void* h_recovery,
                     const uint8_t* recovery_received, size_t slice_bytes, rs16_error* err);

/* ---- Split device decode -------------------------------------------------
 * rs16_decode_device in two halves on two streams.  rs16_decode_prepare
 * takes the received pattern only (the same flags / counts and checks as
 * rs16_decode_device: UnsupportedShardCount, InvalidArgument,
 * NotEnoughShards) and enqueues the erasure locator, eval_poly of the
 * erasure vector (src/rate/rate_high.rs:168-202, src/engine.rs:207-218), on
 * `stream`; rs16_decode_device_prepared then runs the rest of the decode
 * (src/rate/rate_high.rs:203-247) on its own stream, ordered after the
 * preparation.  The pattern of a decode is known before its shards are (a
 * storage system knows which devices failed), so the locator can be computed
 * while the shards are still being produced or copied in: work the caller
 * issues on the engine between the two calls that does not decode -- e.g.
 * the encode of the stripe whose recovery is about to be decoded -- runs
 * concurrently with the preparation.  One preparation per engine, consumed
 * by the next rs16_decode_device_prepared with the same (k, m, shard_bytes)
 * (else InvalidArgument); any other decode on the engine in between orders
 * itself after the preparation and discards it.  The flag arrays must keep
 * their contents until the prepared decode has run.  Results are those of
 * rs16_decode_device; rs16_decode_check covers the prepared decode. */
int rs16_decode_prepare(rs16_engine* eng, size_t original_count, size_t recovery_count, size_t shard_bytes,
                        const uint8_t* d_original_received, const uint8_t* d_recovery_received,
                        size_t original_received_count, size_t recovery_received_count, void* stream,
                        rs16_error* err);
int rs16_decode_device_prepared(rs16_engine* eng, size_t original_count, size_t recovery_count,
                                size_t shard_bytes, void* d_original, const void* d_recovery, void* stream,
                                rs16_error* err);

/* ---- Partial-stripe writes: delta update of the recovery shards ----------
 * Overwriting a few original shards of a stripe that is already encoded.
 * The encode is GF(2^16)-linear per element position (src/algorithm.md:18-32),
 *   recovery_j = sum_i M[j][i] * original_i,
 * so after originals indices[0 .. n) changed from old_e to new_e
 *   recovery_j ^= sum_e M[j][indices[e]] * (old_e ^ new_e).
 * That needs only the n deltas and the recovery shards: the other originals
 * need not be in HBM, and one read-modify-write sweep over the recovery rows
 * replaces the three passes of rs16_encode_device.  No reference counterpart
 * (the reference re-encodes: src/lib.rs:242-279).
 *
 * A plan holds the n columns of M for one (rate, original_count,
 * recovery_count, indices).  `rate` must be the rate the stripe was encoded
 * with: the two rates are different codes with different M.
 * RS16_RATE_DEFAULT means what it means everywhere else in the library, the
 * choice of rs16_use_high_rate -- the rate of rs16_encode_device.  At most
 * RS16_UPDATE_MAX_SHARDS = 32 originals per plan: the plan gets its columns
 * from ONE encode of a 64-byte stripe (the engine's own encode of that rate,
 * so they are exact on every rate path), and a 64-byte block carries 32
 * independent elements -- element e is the field element 1 in shard
 * indices[e] and 0 elsewhere, and recovery row j returns M[j][indices[e]] in
 * element e.  More changed originals: XOR is associative, so apply several
 * plans one after another (each to its own deltas); likewise several updates
 * through one plan compose to the encode of the final stripe.
 *
 * rs16_update_plan_new is synchronous (one small encode on the engine's
 * stream, its result copied to the host, an m x n index array uploaded).
 * Errors, checked in this order: UnsupportedShardCount as rs16_validate gives
 * for `rate`; n == 0 or n > 32: InvalidArgument; an index >= original_count:
 * InvalidOriginalShardIndex (v0 original_count, v1 index); a repeated index:
 * DuplicateOriginalShardIndex.  Like an encoder, a plan is detached by
 * rs16_engine_free: later calls on it fail with RS16_INVALID_ARGUMENT and
 * rs16_update_plan_free then frees only host memory.  Updates enqueued on a
 * caller's stream must have finished before the plan or its engine is freed.
 *
 * rs16_update_device is asynchronous on `stream` and works in place:
 * d_delta = the n shards old ^ new in the order of `indices`, contiguous,
 * read only; d_recovery = recovery shards [recovery_pos, recovery_pos +
 * recovery_n), contiguous (a node that stores only some recovery shards
 * updates only those); recovery_n == 0 does nothing.  shard_bytes 0 or no
 * multiple of 64: InvalidShardSize; a range beyond recovery_count:
 * InvalidArgument.  It uses no engine scratch and no decode state: it may run
 * on any stream beside the engine's other work, and it neither disturbs
 * rs16_decode_check nor a pending rs16_decode_prepare.
 *
 * When to prefer it (MI355X, DESIGN.md 3.15, profiles/r08_update.txt): the
 * update's cost grows with n, rs16_encode_device's does not.  Measured at
 * 32768:32768 x 1 KiB: the encode 69 us, the update 12 / 18 / 33 / 63 us at
 * n = 1 / 4 / 8 / 16; it stops beating the encode at n = 17 (16-18 at 64 and
 * 192-byte shards) and costs twice the encode at n = 32.  So the cap of 32 is
 * above the crossover: with the whole stripe in HBM, re-encode from about 16
 * changed shards on; the update still wins beyond that when the other
 * originals would first have to be fetched.  At 1000:1000 x 1 KiB (8 us
 * encode) the update is 4-5 us up to n = 16 and level with the encode at 32.
 * rs16_update_plan_new costs 1 ms at 32768:32768 and 0.07 ms at 1000:1000
 * (host time, synchronous): keep plans for shards that are rewritten often. */
enum { RS16_UPDATE_MAX_SHARDS = 32 };   /* one 64-byte block carries 32 independent elements */
typedef struct rs16_update_plan rs16_update_plan;
rs16_update_plan* rs16_update_plan_new(rs16_engine* eng, int rate, size_t original_count, size_t recovery_count,
                                       const size_t* indices, size_t n, rs16_error* err);
void rs16_update_plan_free(rs16_update_plan* plan);
size_t rs16_update_plan_count(const rs16_update_plan* plan);
/* Diagnostics / tests: out[j * n + e] = M[j][indices[e]] as a field element
 * (recovery_count x n values). */
int rs16_update_plan_coefficients(rs16_update_plan* plan, uint16_t* out, rs16_error* err);
int rs16_update_device(rs16_update_plan* plan, size_t shard_bytes, const void* d_delta, void* d_recovery,
                       size_t recovery_pos, size_t recovery_n, void* stream, rs16_error* err);
/* rs16_update_device on a column window of the shards, for a batch of stripes
 * of one geometry in one launch.  Every 64-byte column block
 * is a codeword of its own (src/algorithm.md:18-32), so a write that changes
 * bytes [off, off + width) of some originals changes the same bytes of the
 * recovery shards and no others; and the plan's table of (recovery row, delta
 * shard) is the same for every stripe of a geometry.
 *
 * Layout.  `width` = the bytes of every row that are updated, a multiple of
 * 64.  d_delta and d_recovery point at the window's FIRST byte: the caller
 * has added the column offset, a multiple of 64, so they are 64-byte aligned
 * like every shard array.  Delta e (old ^ new of original indices[e], its
 * window) of stripe i lies at d_delta + i delta_stride + e delta_pitch;
 * recovery shard recovery_pos + r of stripe i at d_recovery + i
 * recovery_stride + r recovery_pitch, r < recovery_n.  Bytes of a row outside
 * [0, width), rows outside the range and bytes between strides are neither
 * read as data nor written; the deltas are read only.  Each stripe's result
 * is that of rs16_update_device on the stripe's whole shards with deltas that
 * are zero outside the window -- and so that of a re-encode.  Asynchronous on
 * `stream`, in place.  The strides of a single stripe (nstripes == 1) are not
 * used.
 *
 * Errors, checked in this order: a NULL or detached plan: InvalidArgument;
 * width 0 or no multiple of 64: InvalidShardSize (v0 = width); a range beyond
 * recovery_count: InvalidArgument; recovery_n == 0 or nstripes == 0: RS16_OK,
 * nothing launched; then InvalidArgument for a NULL or misaligned array; a
 * pitch that is no multiple of 64 or below width; for nstripes > 1 a stride
 * that is no multiple of 64, a recovery_stride below (recovery_n - 1)
 * recovery_pitch + width or a delta_stride below (n - 1) delta_pitch + width
 * (stripes would overlap); nstripes > 65535 (the heal's cap); a width or pitch
 * of 4 GiB or more.  Like rs16_update_device it uses no engine scratch and no
 * decode state: any stream, beside the engine's other work; it neither
 * disturbs rs16_decode_check nor a pending rs16_decode_prepare.
 *
 * When to prefer it (MI355X, DESIGN.md 3.22, profiles/r22_update_batch.txt;
 * hipEvent time per call through the Python binding, against the library of
 * the commit before in a process of its own, five alternating pairs):
 * - Stripes: at 1000:1000 x 1 KiB the batch beats a loop of
 *   rs16_update_device calls from 4 stripes on, the fewest measured above
 *   one, in every pair: 4 stripes 4.4 / 4.9 / 11.5 us at n = 1 / 4 / 16
 *   against 14.1 / 15.5 / 19.1 for the loop, 8 stripes 5.2 / 7.9 / 20.0
 *   against 29.3 / 30.8 / 37.7, 32 stripes 11.4 / 19.5 / 53.9 against 121.8 /
 *   125.2 / 148.8.  At 32768:32768 x 1 KiB the sweep dominates: 4 stripes 41.7
 *   / 53.7 / 203.9 against 53.0 / 76.8 / 223.9 (1.27 / 1.43 / 1.10 x).  It
 *   lost to the loop nowhere.
 * - Windows: a 4 KiB window of 64 KiB shards takes 4.3 / 4.9 / 11.3 us at
 *   1000:1000 and 10.6 / 18.5 / 56.7 at 8000:8000, against 21.2 / 31.2 / 106.2
 *   and 227.7 / 229.7 / 730.4 for rs16_update_device on the whole shards with
 *   zero-padded deltas: 4.9 .. 9.4 x and 12.4 .. 21.4 x.
 * - Windows of at most 128 bytes of two stripes or more take a packed form
 *   (8 or 4 stripes a wave): 32 stripes of 64 bytes 4.0 / 4.4 / 7.9 us, of
 *   128 bytes 4.3 / 6.0 / 12.5, against 5.7 / 11.0 / 33.0 and 5.8 / 10.4 /
 *   29.9 with one stripe a wave.
 * - One stripe at full width is the single call's work through a longer
 *   argument list: at 1000:1000 x 1 KiB 4.2 / 4.4 / 5.1 us against 3.5 / 3.9 /
 *   5.0, outside the single call's run-to-run spread at n = 1 and 4 (both are
 *   bound by the launch), inside it at 16; at 32768:32768 12.8 / 19.2 / 56.5
 *   against 12.6 / 19.4 / 58.5, inside it at n = 1 and 4.  For one stripe of
 *   whole shards rs16_update_device stays the call to make.
 * - rs16_update_device itself is unchanged: the same machine code
 *   (scripts/isa_compare.py), this build's median inside the parent's spread
 *   in 21 of 24 rows, 0.11 us slower to 5.8 us faster in the other three.
 * Sizes in between are not measured. */
int rs16_update_device_batch(rs16_update_plan* plan, size_t width, size_t nstripes,
                             const void* d_delta, size_t delta_pitch, size_t delta_stride,
                             void* d_recovery, size_t recovery_pitch, size_t recovery_stride,
                             size_t recovery_pos, size_t recovery_n, void* stream, rs16_error* err);

/* ---- Host-resident stripes, pipelined (full duplex) -----------------------
 * nstripes independent stripes in host memory (stripe i's originals at
 * h_original + i original_stride, its recovery at h_recovery + i
 * recovery_stride; page-locked memory for DMA-rate copies), each encoded /
 * decoded exactly as rs16_encode_host / rs16_decode_host would, with two
 * stripes in flight: the host->device copy of stripe i + 1 and the
 * device->host copy of stripe i - 1 run on two copy streams while stripe i
 * is on the device, so both directions of the link carry data at once (one
 * stripe alone cannot overlap: its outputs exist only after its inputs are
 * all in).  Copies are contiguous row runs, no pitched copies.  The
 * reference's EncoderWork / DecoderWork path (src/rate/encoder_work.rs:49-69,
 * src/encoder_result.rs:31-95) once per stripe.  Synchronous.  Decode: stripe
 * i's host flag bytes at original_received + i original_received_stride /
 * recovery_received + i recovery_received_stride; only received rows travel
 * to the device and only the lost originals come back (restored in place);
 * a stripe with too few shards fails the whole call before any copy
 * (NotEnoughShards, the first such stripe). */
int rs16_encode_host_batch(rs16_engine* eng, size_t original_count, size_t recovery_count, size_t shard_bytes,
                           size_t nstripes, const void* h_original, size_t original_stride, void* h_recovery,
                           size_t recovery_stride, rs16_error* err);
int rs16_decode_host_batch(rs16_engine* eng, size_t original_count, size_t recovery_count, size_t shard_bytes,
                           size_t nstripes, void* h_original, size_t original_stride,
                           const uint8_t* original_received, size_t original_received_stride,
                           const void* h_recovery, size_t recovery_stride, const uint8_t* recovery_received,
                           size_t recovery_received_stride, rs16_error* err);

/* ---- Several GPUs in one process ------------------------
 * reed_solomon_16::encode / decode of ONE stripe with host-resident shards,
 * its byte columns split over the n engines (one per GPU): engine j takes its
 * share of the B = shard_bytes / 64 column blocks (rs16_column_slice; every
 * column block is an independent codeword, src/algorithm.md:18-32), copies
 * them in with a pitched DMA copy, runs the device codec and copies them
 * back; the engines run concurrently, with no exchange between the GPUs.
 * Synchronous.  Results are identical to rs16_encode_host / rs16_decode_host
 * (n = 1 is that call with one whole-width slice).  Decode: host flag byte
 * arrays; lost originals restored in place into h_original. */
int rs16_encode_host_multi(rs16_engine* const* engines, int n, size_t original_count, size_t recovery_count,
                           size_t shard_bytes, const void* h_original, void* h_recovery, rs16_error* err);
int rs16_decode_host_multi(rs16_engine* const* engines, int n, size_t original_count, size_t recovery_count,
                           size_t shard_bytes, void* h_original, const uint8_t* original_received,
                           const void* h_recovery, const uint8_t* recovery_received, rs16_error* err);

/* ---- RCCL over xGMI: column-slice scatter / gather -----
 * For a stripe that lives in ONE GPU's HBM (BASELINE configs[4]): the root's
 * rows x shard_bytes array is split into byte-column slices, rank r getting
 * whole 64-byte column blocks, B / n of them and one more for the first
 * B mod n ranks (B = shard_bytes / 64; rs16_column_slice), as a contiguous
 * rows x width array -- itself a shard
 * array of shard_bytes = width, so every rank runs the device codec on its
 * slice with no further exchange -- and gathered back the same way.  The
 * root packs / unpacks with pitched device copies; the slices move with one
 * grouped ncclSend / ncclRecv per other rank (the root's own slice is one
 * pitched device copy, no RCCL).  Ranks are processes (one
 * rs16_comm_new each, with the root's rs16_comm_unique_id shared out of
 * band) or engines of one process (rs16_comm_init_all).  The collective
 * calls take this process's communicators (n of them, ranks in any order)
 * with one buffer per communicator: d_full is used on the root only,
 * d_slice on every rank.  Asynchronous on `stream` (n == 1) or on each
 * engine's stream.  Like an encoder, a communicator is detached by
 * rs16_engine_free ("Conventions"). */
typedef struct rs16_comm rs16_comm;
int rs16_comm_unique_id(void* id128, rs16_error* err);
rs16_comm* rs16_comm_new(rs16_engine* eng, int nranks, int rank, const void* id128, rs16_error* err);
int rs16_comm_init_all(rs16_engine* const* engines, int n, rs16_comm** comms, rs16_error* err);
void rs16_comm_free(rs16_comm* comm);
int rs16_comm_rank(const rs16_comm* comm);
int rs16_comm_size(const rs16_comm* comm);
/* Column slice of `rank` among `nranks`: byte offset and width (multiples of 64; width may be 0). */
int rs16_column_slice(size_t shard_bytes, int nranks, int rank, size_t* offset, size_t* width);
int rs16_scatter_columns(rs16_comm* const* comms, int n, int root, size_t rows, size_t shard_bytes,
                         const void* const* d_full, void* const* d_slice, void* stream, rs16_error* err);
int rs16_gather_columns(rs16_comm* const* comms, int n, int root, size_t rows, size_t shard_bytes,
                        const void* const* d_slice, void* const* d_full, void* stream, rs16_error* err);
/* Diagnostics: the multi-rank data path of rs16_scatter_columns /
 * rs16_gather_columns on ONE rank.  `comm` is a one-rank communicator; the
 * array is split into `vslices` column slices (rs16_column_slice with nranks =
 * vslices) that are all owned by that rank: slice 0 is the root's own (one
 * pitched copy), every other slice goes through the staging pack, one grouped
 * ncclSend / ncclRecv per slice with the rank itself as the peer, and (gather)
 * the unpack, exactly as another rank's slice would.  d_slices[j] = slice j's
 * rows x width_j buffer.  No reference counterpart (the reference has no
 * multi-GPU path); lets a one-GPU machine run the code the driver's 8-GPU
 * run depends on (tests/test_gpu_rccl.py). */
int rs16_scatter_columns_virtual(rs16_comm* comm, int vslices, size_t rows, size_t shard_bytes, const void* d_full,
                                 void* const* d_slices, void* stream, rs16_error* err);
int rs16_gather_columns_virtual(rs16_comm* comm, int vslices, size_t rows, size_t shard_bytes,
                                const void* const* d_slices, void* d_full, void* stream, rs16_error* err);

/* ---- Device memory helpers (so FFI callers need no HIP headers) ------- */
void* rs16_device_alloc(rs16_engine* eng, size_t bytes, rs16_error* err);
void rs16_device_free(rs16_engine* eng, void* d_ptr);
int rs16_memcpy_htod(rs16_engine* eng, void* d_dst, const void* src, size_t bytes, void* stream, rs16_error* err);
int rs16_memcpy_dtoh(rs16_engine* eng, void* dst, const void* d_src, size_t bytes, void* stream, rs16_error* err);
int rs16_memset_device(rs16_engine* eng, void* d_dst, int value, size_t bytes, void* stream, rs16_error* err);
/* Pitched copies (hipMemcpy2DAsync, then a wait): `rows` rows of `width`
 * bytes, row i at d + i * d_pitch on the device and h + i * h_pitch on the
 * host -- a column block of every row of a wide array in one call. */
int rs16_memcpy2d_htod(rs16_engine* eng, void* d_dst, size_t d_pitch, const void* src, size_t h_pitch, size_t width,
                       size_t rows, void* stream, rs16_error* err);
int rs16_memcpy2d_dtoh(rs16_engine* eng, void* dst, size_t h_pitch, const void* d_src, size_t d_pitch, size_t width,
                       size_t rows, void* stream, rs16_error* err);
/* Streams (hipStream_t, non-blocking) on the engine's device, for callers
 * without HIP headers that run codecs on streams of their own. */
void* rs16_stream_create(rs16_engine* eng, rs16_error* err);
void rs16_stream_destroy(rs16_engine* eng, void* stream);
/* Page-locked host staging memory (hipHostMalloc, portable: usable by every
 * engine of a multi-GPU call): shards that start and end
 * in host memory move over PCIe at DMA rate from/to these buffers (the
 * host-resident path of EncoderWork / DecoderWork, src/rate/encoder_work.rs:49-69). */
void* rs16_host_alloc(rs16_engine* eng, size_t bytes, rs16_error* err);
void rs16_host_free(rs16_engine* eng, void* h_ptr);

/* Diagnostics: per-kernel timing.  When enabled, every HBM pass (and the
 * eval_poly kernel group) is bracketed by hipEvents on its launch stream.
 * rs16_engine_profile_read synchronizes and returns, for pass program
 * `prog` (0 .. rs16_prog_count()-1, named by rs16_prog_name: the pass programs,
 * then the ids of kernel groups such as EVAL_POLY, COL_ENC or REPAIR_COPY; new
 * ids are added and an id's value may move, so look an id up by its name), the summed
 * milliseconds and the number of launches since the last reset. */
int rs16_engine_set_profiling(rs16_engine* eng, int enable, rs16_error* err);
int rs16_engine_profile_read(rs16_engine* eng, int prog, double* total_ms, uint64_t* launches, rs16_error* err);
void rs16_engine_profile_reset(rs16_engine* eng);
int rs16_prog_count(void);
/* Diagnostics: phase timeline.  Library builds made with -DRS16_STAMPS=1
 * (scripts/stamps.py; never the shipped one) make the passes launched under
 * profiling id `prog` write 16 u64 clock stamps per workgroup to d_buf
 * (workgroup b at d_buf[16 b]); prog = -1 or d_buf = NULL turns it off.  Other
 * builds accept the call and record nothing. */
int rs16_engine_set_stamps(rs16_engine* eng, void* d_buf, int prog, rs16_error* err);
const char* rs16_prog_name(int prog);

/* Diagnostics: switches of ONE engine to alternative code paths, for tests
 * and measurements only (results are identical; 0 = the shipped paths, the
 * state of every new engine).  Returns the engine's previous flags.  There is
 * no process-wide state: other engines keep their own flags.  Like every call
 * on an engine, not to be made while another thread issues work on it. */
enum {
    RS16_DIAG_FORCE_VOFF64 = 1,    /* 64-bit per-lane HBM offsets in every pass */
    RS16_DIAG_EVAL_TWO_KERNEL = 2, /* eval_poly: the two-kernel form everywhere */
    RS16_DIAG_EVAL_FULL = 4,       /* eval_poly: the full 65536-point form for n <= 2048 */
    RS16_DIAG_NO_COLUMN = 8,       /* 512 / 1024-row transforms through the pass codec instead of
                                      the one-launch column codec */
    RS16_DIAG_FORCE_COLUMN = 16,   /* ... through the column codec at any shard width / stripe count / chunk count */
    RS16_DIAG_TILE_LAST = 32,      /* the general decode's last pass (65536 work rows) one wave per quad
                                      column of a tile at any loss count (default: <= 2048 lost) */
    RS16_DIAG_NO_TILE_LAST = 64,   /* ... always as 8-wave items of 32 quad columns */
    RS16_DIAG_FD_LDS = 128,        /* the general decode's in-tile formal derivative always through LDS */
    RS16_DIAG_COL_RADIX4 = 256,    /* column codec: 4 rows per thread everywhere (no radix-2 form) */
    RS16_DIAG_NO_IDENTITY = 512,   /* a decode whose erased rows are exactly one half of the work rows (all
                                      originals lost, all recovery received, k = m = 2^j >= 2048): evaluate
                                      the erasure polynomial and multiply anyway (default: every erasure
                                      log is 0, the multipliers are identities and are skipped) */
    RS16_DIAG_NO_MID_DIRECT = 1024, /* the general decode's middle pass always as the 2^hi-point IFFT /
                                      derivative / FFT pass, also when the lost originals lie in at most
                                      4 of its output rows per column (default there: a direct product
                                      with the pass's matrix) */
    RS16_DIAG_WIDE_TWIDDLES = 2048, /* the full 12-lookup multiply in every layer (default: the middle
                                      passes multiply with 9 lookups in the layers whose twiddles all
                                      lie in the GF(2^8) subfield) */
    RS16_DIAG_NO_LATE_ROWS = 4096, /* the T = 7 / 8 encoder-family passes always request all their rows
                                      ahead of the first layer (default: a launch none of whose waves
                                      needs the general row loads requests most of them from inside
                                      the first layer; rs16_pass_consts.late_rows) */
    RS16_DIAG_NO_PAIRED_ROWS = 8192, /* the engine's work buffer keeps the shard layout between the passes
                                      of every sequence (default: the three-pass encode and the identity
                                      decode of 2^14 / 2^15-row chunks, widths a multiple of 512 bytes,
                                      keep a quad's two dwords next to each other there and move a row
                                      with one 8-byte access per lane; rs16_host_paired_rows) */
    RS16_DIAG_NO_TOWER_ROWS = 16384, /* paired rows of the work buffer stay in the shards' coordinates
                                      (default: they are kept as a + b beta over the GF(2^8) subfield, in
                                      which the middle pass multiplies by a subfield twiddle with 6
                                      lookups instead of 9; rs16_host_tower_rows) */
    RS16_DIAG_NO_FUSED_VERIFY = 32768, /* rs16_verify_device always as encode + compare (path 0); wins
                                      over RS16_DIAG_FORCE_FUSED_VERIFY when both are set */
    RS16_DIAG_FORCE_FUSED_VERIFY = 65536 /* ... as the fused path wherever a comparing kernel exists for
                                      the shape's last pass, whatever the default gate says */
};
int rs16_engine_set_diagnostics(rs16_engine* eng, int flags);
/* Deprecated (the round-4 process-wide form, kept for existing callers):
 * sets the flags every engine created AFTER the call starts with and returns
 * the previous default.  Engines that exist keep their own flags. */
int rs16_set_diagnostics(int flags);

/* Diagnostics: host-side evaluation of the device multiply (same v_perm
 * byte-table format and code path as the kernels, with v_perm emulated):
 * out[] = in[] * log_m for `bytes` (multiple of 64) bytes of shard data, with
 * Engine::mul semantics (log_m 65535 == x1).  Lets CPU-only tests check the
 * table format against the reference multiply (NoSimd::mul). */
void rs16_host_mul(const void* in, void* out, size_t bytes, uint16_t log_m);
/* The same through the narrow multiply of the middle passes, which leaves
 * out the lookups from an input's low byte to the output's high byte: equal
 * to rs16_host_mul exactly when the multiplier is an element of the GF(2^8)
 * subfield (as a field element, < 256). */
void rs16_host_mul_narrow(const void* in, void* out, size_t bytes, uint16_t log_m);
/* The FFT / IFFT twiddle of skew index `index` (0 .. 65534) as the engine's
 * tables hold it: returns the field element (0 for the "no multiply"
 * sentinel; ~0 for an index out of range), its log to *log_m (65535 = the
 * sentinel) and its 20-dword v_perm multiply table to table20 (either may
 * be NULL).  rs16_host_twiddle_narrow: 1 when the index rule the pass
 * launches go by calls the twiddle a subfield element, else 0. */
uint32_t rs16_host_twiddle(uint32_t index, uint32_t* log_m, uint32_t* table20);
int rs16_host_twiddle_narrow(uint32_t index);
/* The pass launches divide workgroup indices by launch constants (slabs per
 * row, tiles per stripe) with a host-computed multiply-high constant instead
 * of a division.  This checks that form on the host: the number of n = n0 +
 * i * step, i < count (stopping at 2^32), whose quotient by `divisor` (>= 1)
 * differs from n / divisor. */
uint64_t rs16_host_fast_div_check(uint32_t divisor, uint32_t n0, uint32_t count, uint32_t step);
/* The launch constants by which a pass launch picks its address forms, as
 * the launcher computes them (one host function, which every launch calls;
 * no device needed), and the geometry of the kernel of pass program `prog`
 * (rs16_prog_name: the ids below DEC_HALF_FIRST; the ids from there on are
 * profiling ids, not covered here) at tile bits T:
 *   voff32      1: every lane's byte offset below its wave's row base fits 32
 *               bits (SGPR base + 32-bit lane offset), 0: 64-bit lane offsets
 *   full_lanes  1: the launch's waves may take the full-item fast path
 *   rs_in, rs_seg, rs_out   its byte strides between consecutive row registers
 *   nslab       slabs of `quads` quads per row
 *   quads, threads          quads per tile row, threads per workgroup
 *   load_shb, store_shb     0: rows loaded / stored in layout A, else in layout
 *               B, consecutive row registers 2^shb tile rows apart
 *   reg_bits, row_sets      row bits a thread holds in registers (R), row sets
 *               per wave (HWS): a lane's rows start up to (HWS - 1) 2^R << lo
 *               (layout A) or (HWS - 1) << lo (layout B) rows below its wave's
 * from the stride exponent `lo`, the four row strides (bytes), the slice width
 * `qrow` (quads of 8 bytes), the decoder's segment boundary `chunk` and first
 * gather row `row_base_in`, the plain loads' row mask and the RS16_DIAG_*
 * flags.  Returns 1, or 0 when (prog, T) has no kernel (*out untouched). */
typedef struct rs16_pass_consts {
    uint32_t voff32, full_lanes, nslab;
    uint32_t quads, threads, load_shb, store_shb, reg_bits, row_sets;
    uint64_t rs_in, rs_seg, rs_out;
    uint32_t late_rows; /* 1: the launch runs the late-rows kernel variant (32-bit lane offsets, no
                           row mask, a gather's row limit a multiple of row_sets 2^reg_bits << lo,
                           no RS16_DIAG_NO_LATE_ROWS; the T = 7 / 8 encoder-family passes only) */
} rs16_pass_consts;
int rs16_host_pass_consts(int prog, int T, uint32_t lo, uint64_t s_in, uint64_t s_out, uint64_t s_seg, uint64_t s_rest,
                          uint32_t qrow, uint32_t chunk, uint32_t row_base_in, uint32_t in_rows_mask, int diag,
                          rs16_pass_consts* out);
/* The same for n launches that differ in their strides and slice width only
 * (arrays of n; out[i] for launch i): sweeps of many widths in one call. */
int rs16_host_pass_consts_many(int prog, int T, uint32_t lo, size_t n, const uint64_t* s_in, const uint64_t* s_out,
                               const uint64_t* s_seg, const uint64_t* s_rest, const uint32_t* qrow, uint32_t chunk,
                               uint32_t row_base_in, uint32_t in_rows_mask, int diag, rs16_pass_consts* out);
/* rs16_host_pass_consts for a gathering first pass whose rows at and above
 * `a_count` are absent (the two calls above: a_count = 0, no wave is cut). */
int rs16_host_pass_consts_rows(int prog, int T, uint32_t lo, uint64_t s_in, uint64_t s_out, uint64_t s_seg,
                               uint64_t s_rest, uint32_t qrow, uint32_t chunk, uint32_t row_base_in,
                               uint32_t in_rows_mask, uint32_t a_count, int diag, rs16_pass_consts* out);
/* Whether the three pass launches over a chunk of `chunk_rows` rows (a power
 * of two) of width S bytes -- the three-pass encode, or the identity decode of
 * one half -- keep the engine's work buffer in the paired row form (a quad's
 * low and high dword adjacent: one 8-byte access per row and lane), as the
 * engine decides it (one host function; no device needed).  1 exactly when
 * all three launches (first / middle / last encoder pass at L / 2, L - L / 2
 * and L / 2 row bits) report late_rows and full_lanes in rs16_host_pass_consts_rows,
 * the chunk has 2^14 or 2^15 rows (the chunks whose three passes all have such
 * kernels) and RS16_DIAG_NO_PAIRED_ROWS is not set in `diag`.  S_user: the
 * caller's row stride; a_count: the first pass's row limit; seg_chunk,
 * row_base_in: the decode's segment boundary and first gather row (0, 0 in an
 * encode).  The form never leaves the engine: results are identical. */
int rs16_host_paired_rows(uint32_t chunk_rows, uint64_t S, uint64_t S_user, uint32_t a_count, uint32_t seg_chunk,
                          uint32_t row_base_in, int diag);
/* Tower form of the work buffer's paired rows.  With beta = v_8 of the Cantor
 * basis every element (lo, hi) is a + b beta, a = lo ^ B(hi) and b = hi in the
 * GF(2^8) subfield; v_{8+i} = a_i + v_i beta gives B's columns a_i.
 * rs16_host_tower_rows: rs16_host_paired_rows for the tower form -- 1 exactly
 * when the sequence is paired and RS16_DIAG_NO_TOWER_ROWS is not set.
 * rs16_host_tower_basis: a_i as the tables derived it (i < 8; else ~0).
 * rs16_host_tower_conv: out[] = in[] switched between the two forms (the
 * kernels' lookups, v_perm emulated; its own inverse), `bytes` a multiple of 64.
 * rs16_host_tower_twiddle: the 20-dword table of skew index `index` in tower
 * coordinates, as the passes of a tower sequence stage it (0: out of range).
 * rs16_host_mul_tower: out[] = that table applied to in[] (tower form in and
 * out); `form` = 0: the 12-lookup multiply, 1: the 6-lookup one of the layers
 * whose twiddles are subfield elements, 2: the 9-lookup wide multiply of the
 * T = 7 passes, 3: the one for twiddles s ^ v_8, s in the subfield (the middle
 * pass's wide layer).
 * rs16_host_tower_sweep: the same for the `n` skew indices index[]: the tower
 * table of index[i] applied to in[] (`bytes`, tower form) in form `form`,
 * converted to the shards' coordinates and compared with want[i * bytes ..);
 * returns the number of elements that differ over all i. */
int rs16_host_tower_rows(uint32_t chunk_rows, uint64_t S, uint64_t S_user, uint32_t a_count, uint32_t seg_chunk,
                         uint32_t row_base_in, int diag);
uint32_t rs16_host_tower_basis(uint32_t i);
void rs16_host_tower_conv(const void* in, void* out, size_t bytes);
int rs16_host_tower_twiddle(uint32_t index, uint32_t* table20);
void rs16_host_mul_tower(const void* in, void* out, size_t bytes, uint32_t index, int form);
uint64_t rs16_host_tower_sweep(const uint32_t* index, size_t n, int form, const void* in, const void* want,
                               size_t bytes);
/* The shape of the launch by which rs16_update_device updates `rows` recovery
 * rows of `shard_bytes` from `n` deltas, as the launcher computes it (one host
 * function, which every update calls; no device needed):
 *   quads_per_lane  8-byte quads of a row a lane works on (1 or 2)
 *   nslab           slabs of 64 quads_per_lane quads per row, one wave each
 *   rows_per_wave   consecutive rows a wave updates (the last run may be shorter)
 *   blocks          workgroups of four waves; wave w has slab w mod nslab of
 *                   run w / nslab
 * Any of the four pointers may be NULL.  Returns 1, or 0 where
 * rs16_update_device launches nothing or fails (rows = 0, a shard size that is
 * 0, no multiple of 64 or too large, n = 0 or above RS16_UPDATE_MAX_SHARDS). */
int rs16_host_update_consts(uint32_t rows, uint64_t shard_bytes, uint32_t n, uint32_t* quads_per_lane,
                            uint32_t* nslab, uint32_t* rows_per_wave, uint64_t* blocks);
/* The same for rs16_update_device_batch: `rows` recovery rows of a window of
 * `width` bytes, `n` deltas, `nstripes` stripes (one host function, which the
 * batch launcher calls; no device needed).  out[0 .. 6) =
 *   quads_per_lane, nslab, rows_per_wave   as above, of the window
 *   stripes_per_wave  stripes a wave works on: above 1 is the packed form of
 *                     windows of at most 128 bytes (lane l: quad l mod qrow of
 *                     stripe l / qrow of the wave's group, qrow = width / 8)
 *   waves             waves with work: wave w has slab w mod nslab of stripe
 *                     group (w / nslab) mod ngroups of run w / (nslab ngroups),
 *                     ngroups = ceil(nstripes / stripes_per_wave)
 *   blocks            workgroups of four waves
 * One stripe gives the quads_per_lane, nslab and rows_per_wave of
 * rs16_host_update_consts.  Returns 1, or 0 where rs16_update_device_batch
 * launches nothing or fails (rows = 0, nstripes = 0 or above 65535, a width
 * that is 0, no multiple of 64 or 4 GiB and more, n = 0 or above
 * RS16_UPDATE_MAX_SHARDS). */
int rs16_host_update_batch_consts(uint32_t rows, uint64_t width, uint32_t n, uint32_t nstripes, uint32_t out[6]);
/* The path rs16_repair_device takes, as the entry points decide it (one host
 * function; no device needed): 0 nothing to do, 1 = rs16_decode_device (no
 * recovery shard lost), 2 = encode + copy of the lost recovery rows (no
 * original lost), 3 = general repair; -1 where the call fails (unsupported
 * counts, a count above its shard count, fewer than original_count received).
 * *lo / *first_tile / *tiles (any may be NULL): for path 3 the last pass's
 * tiles of 2^lo rows.  *tiles tiles are launched in all.  Whole tiles that lie
 * between the two segments are not launched: then the launches are segment A's
 * tiles [0, ceil(a_count / 2^lo)) and segment B's from tile *first_tile =
 * chunk / 2^lo on (the rest of *tiles).  Where the two ranges touch or overlap
 * they are one range and *first_tile = 0.  One tile at lo = 0 when the stripe
 * has at most 2^8 work rows (the one-pass kernel).  0, 0, 0 on every other
 * path.  (Segment A: the recovery shards at the high rate, the originals at
 * the low rate; chunk = a_count rounded up to a power of two.) */
int rs16_host_repair_path(size_t original_count, size_t recovery_count, size_t original_received_count,
                          size_t recovery_received_count, uint32_t* lo, uint32_t* first_tile, uint32_t* tiles);
/* The path rs16_verify_device / rs16_verify_device_batch takes for a shape, as
 * the entry points decide it (one host function) on an engine with the
 * diagnostic switches `diag` (RS16_DIAG_*) and the default column-codec limits:
 * 1 = fused, 0 = encode + compare, -1 = the counts or the shard size are not
 * supported.  nstripes: the stripes of the batch form (1: the single call). */
int rs16_host_verify_path(size_t original_count, size_t recovery_count, size_t shard_bytes, size_t nstripes,
                          int diag);
/* The path rs16_decode_device_select takes, as the entry points decide it (one
 * host function; no device needed): 0 nothing to do (every original received,
 * or wanted_count == 0), 1 = rs16_decode_device (the read set covers every lost
 * original), 2 = the selective decode; -1 where the call fails (unsupported
 * counts, a count above its shard count, wanted_count above the lost
 * originals' count, fewer than original_count received). */
int rs16_host_select_path(size_t original_count, size_t recovery_count, size_t original_received_count,
                          size_t recovery_received_count, size_t wanted_count);

/* Library/build identification, e.g. "rs16-mi355x gfx950". */
const char* rs16_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RS16_H */
