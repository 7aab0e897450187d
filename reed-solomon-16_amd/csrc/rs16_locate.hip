// rs16_locate.hip -- the kernels of rs16_locate_device / _batch and
// rs16_heal_device / _batch (include/rs16.h): which one shard of each 64-byte
// column block is corrupt, for one stripe or many of one geometry.  The engine
// encodes the stored originals into a buffer of its own (enc); the syndrome of
// recovery row j is enc[j] ^ rec[j] and is never stored.
//   scan     per element position, over all m rows: how many rows have a
//            nonzero syndrome element there, and the sum of those rows (the
//            row itself when there is one)
//   decide   per block: classify its 32 elements, write status / shard / fix and
//            scatter an ORIGINAL candidate's error into the error array E
//   confirm  after the engine's encode of E: every ORIGINAL block must have
//            encode(E) equal to the syndrome in all m rows, else UNLOCATABLE
//   apply    the heal only: XOR each located block's fix into the named shard
//            and count the stripe's blocks by final status
// A unit of its own, so the kernels of the other units compile as before.
#include "rs16_internal.hpp"

#include "../../include/rs16.h"

namespace rs16 {

namespace {
constexpr uint32_t SCAN_THREADS = 256;
constexpr uint32_t SCAN_WGS = 2048;  // workgroups a scan or confirm launch aims at: 8 per CU
constexpr uint32_t NONE = 0xFFFFFFFFu;
// an element's class in the decide kernel
enum : uint32_t { EL_CLEAN = 0, EL_ORIGINAL = 1, EL_RECOVERY = 2, EL_BAD = 3 };

// byte offset of column lane `col` within a row: low dword 4 l of block c, col = 8 c + l
__device__ __forceinline__ uint64_t lane_offset(uint32_t col) { return (uint64_t)(col >> 3) * 64 + (col & 7) * 4; }

__device__ __forceinline__ uint32_t load32(const uint8_t* p) { return *(const uint32_t*)p; }

// the syndrome's nonzero elements of a lane as a byte mask: low bytes | high bytes
__device__ __forceinline__ uint32_t syn_or(const uint8_t* enc, const uint8_t* rec, uint64_t off) {
    return (load32(enc + off) ^ load32(rec + off)) | (load32(enc + off + 32) ^ load32(rec + off + 32));
}

__device__ __forceinline__ void count_row(uint32_t d, uint32_t r, uint32_t (&cnt)[4], uint32_t (&rsum)[4]) {
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const uint32_t nz = ((d >> (8 * e)) & 0xFFu) != 0;
        cnt[e] += nz;
        rsum[e] += nz ? r : 0;
    }
}
}  // namespace

// Thread t of a workgroup: column lane blockIdx.x * 256 + t % cw, row slot t /
// cw (< rsub); it walks rows r0 + slot, + rsub, ... of the workgroup's row chunk.
// Most rows XOR to zero: four rows are loaded ahead and skipped together on a
// wave-uniform test.  A thread that found something adds (count, sum of the
// rows) to the element's pair with one 64-bit atomic.  When an original is
// corrupt every thread of a column does, so the pairs exist nslots times and
// the row walkers spread over them (one address took 5 ns per atomic:
// profiles/r19_locate.txt); the decide kernel adds the copies up.  Grid z is
// the stripe: the three arrays move on by their stripe strides (bytes, bytes,
// pairs).  MANY = false is the form of one stripe, which does none of that: the
// single call keeps the code it had before the stripe dimension (it measured
// 0.3-0.6 us slower through the batch form; profiles/r20_heal.txt).
template <bool MANY>
__global__ void __launch_bounds__(SCAN_THREADS) locate_scan_kernel(const uint8_t* enc, const uint8_t* rec,
                                                                   unsigned long long* acc, uint32_t nslots,
                                                                   uint64_t S, uint32_t m, uint32_t cols, uint32_t cw,
                                                                   uint32_t rsub, uint32_t rows_per_wg,
                                                                   uint64_t bs_enc, uint64_t bs_rec, uint64_t bs_acc) {
    if (MANY) enc += blockIdx.z * bs_enc, rec += blockIdx.z * bs_rec, acc += blockIdx.z * bs_acc;
    const uint32_t slot = threadIdx.x / cw;
    const uint32_t col = blockIdx.x * SCAN_THREADS + (threadIdx.x - slot * cw);
    if (slot >= rsub || col >= cols) return;
    const uint32_t r0 = blockIdx.y * rows_per_wg;
    const uint32_t r1 = r0 + rows_per_wg < m ? r0 + rows_per_wg : m;
    const uint64_t off = lane_offset(col);
    uint32_t cnt[4] = {0, 0, 0, 0}, rsum[4] = {0, 0, 0, 0};
    uint32_t r = r0 + slot;
    for (; r < r1 && r1 - r > 3 * rsub; r += 4 * rsub) {
        const uint64_t o0 = (uint64_t)r * S + off, o1 = o0 + (uint64_t)rsub * S, o2 = o1 + (uint64_t)rsub * S,
                       o3 = o2 + (uint64_t)rsub * S;
        const uint32_t d0 = syn_or(enc, rec, o0), d1 = syn_or(enc, rec, o1), d2 = syn_or(enc, rec, o2),
                       d3 = syn_or(enc, rec, o3);
        if (__builtin_amdgcn_ballot_w64((d0 | d1 | d2 | d3) != 0) == 0) continue;
        count_row(d0, r, cnt, rsum);
        count_row(d1, r + rsub, cnt, rsum);
        count_row(d2, r + 2 * rsub, cnt, rsum);
        count_row(d3, r + 3 * rsub, cnt, rsum);
    }
    for (; r < r1; r += rsub) {
        const uint32_t d = syn_or(enc, rec, (uint64_t)r * S + off);
        if (__builtin_amdgcn_ballot_w64(d != 0) == 0) continue;
        count_row(d, r, cnt, rsum);
    }
    // (nslots is a power of two; at most 65535 rows: the count stays below 2^17 and the sum below 2^32)
    unsigned long long* mine = acc + (uint64_t)((blockIdx.y * rsub + slot) & (nslots - 1)) * ((uint64_t)cols * 4);
#pragma unroll
    for (int e = 0; e < 4; e++)
        if (cnt[e]) atomicAdd(&mine[(uint64_t)col * 4 + e], (unsigned long long)rsum[e] << 32 | cnt[e]);
}

// 32 lanes per block, two blocks per workgroup.  Lane e classifies element e:
//   no nonzero syndrome               clean
//   one, in row j                     recovery shard j
//   all m                             original i = ratio[log s0 - log s1] with
//                                     error exp[log s0 - log M[0][i]], or bad
//                                     when no original has that ratio
//   2 .. m - 1                        bad
// The block is CLEAN without a dirty element, RECOVERY / ORIGINAL when every
// dirty element names the same shard, else UNLOCATABLE.  Every entry of status,
// shard and fix is written; the element's pairs go back to zero.  The blocks
// of all stripes are numbered through, stripe by stripe: the two halves of a
// workgroup may belong to two stripes (an odd block count), so each half moves
// the arrays on to its own stripe.  MANY = false: one stripe, as in the scan.
template <bool MANY>
__global__ void __launch_bounds__(64) locate_decide_kernel(LocateArgs a) {
    __shared__ uint32_t s_kind[2][32], s_shard[2][32];
    const uint32_t e = threadIdx.x & 31, h = threadIdx.x >> 5;
    const uint32_t g = blockIdx.x * 2 + h;
    uint32_t c = g;
    bool active = c < a.blocks;
    if (MANY) {
        const uint32_t st = g / a.blocks;
        c = g - st * a.blocks;
        active = g < a.blocks * a.nstripes;  // (below 2^31: launch_locate_decide)
        a.enc += st * a.bs_enc, a.rec += st * a.bs_rec, a.E += st * a.bs_E, a.acc += st * a.bs_acc;
        a.cand += st * a.bs_cand, a.status += st * a.bs_status, a.shard += st * a.bs_shard;
        if (a.fix) a.fix += st * a.bs_fix;
    }
    const uint64_t at = (uint64_t)c * 64 + e;  // the element's low byte within a row
    uint32_t kind = EL_CLEAN, shard = NONE, err = 0;
    if (active) {
        const uint64_t p = (uint64_t)c * 32 + e;
        // (every copy is loaded before the first one is cleared: the loads go out together)
        unsigned long long v[LOCATE_MAX_SLOTS], sum = 0;
#pragma unroll
        for (uint32_t q = 0; q < LOCATE_MAX_SLOTS; q++) v[q] = q < a.nslots ? a.acc[(uint64_t)q * (a.S / 2) + p] : 0;
#pragma unroll
        for (uint32_t q = 0; q < LOCATE_MAX_SLOTS; q++) sum += v[q];
#pragma unroll
        for (uint32_t q = 0; q < LOCATE_MAX_SLOTS; q++)
            if (v[q]) a.acc[(uint64_t)q * (a.S / 2) + p] = 0;
        const uint32_t cnt = (uint32_t)sum;
        if (cnt == 1) {
            kind = EL_RECOVERY, shard = (uint32_t)(sum >> 32);  // the sum of one row
        } else if (cnt == a.m) {
            // (m >= 2: rows 0 and 1 exist and both syndromes are nonzero)
            const uint32_t s0 = (uint32_t)(a.enc[at] ^ a.rec[at]) | (uint32_t)(a.enc[at + 32] ^ a.rec[at + 32]) << 8;
            const uint32_t s1 = (uint32_t)(a.enc[a.S + at] ^ a.rec[a.S + at]) |
                                (uint32_t)(a.enc[a.S + at + 32] ^ a.rec[a.S + at + 32]) << 8;
            const uint32_t l0 = a.log[s0], l1 = a.log[s1];
            const uint32_t i = a.ratio[l0 >= l1 ? l0 - l1 : l0 + GF_MODULUS - l1];
            if (i >= a.k) {
                kind = EL_BAD;
            } else {
                const uint32_t lm = a.log_m0[i];
                kind = EL_ORIGINAL, shard = i, err = a.exp[l0 >= lm ? l0 - lm : l0 + GF_MODULUS - lm];
            }
        } else if (cnt) {
            kind = EL_BAD;
        }
    }
    s_kind[h][e] = kind, s_shard[h][e] = shard;
    __syncthreads();
    if (!active) return;
    uint32_t bk = EL_CLEAN, bs = NONE;
    for (uint32_t q = 0; q < 32; q++) {
        const uint32_t kq = s_kind[h][q], sq = s_shard[h][q];
        if (kq == EL_CLEAN) continue;
        if (bk == EL_CLEAN) bk = kq, bs = sq;
        if (kq == EL_BAD || kq != bk || sq != bs) {
            bk = EL_BAD;
            break;
        }
    }
    uint32_t lo = 0, hi = 0;
    if (bk == EL_RECOVERY) {
        const uint64_t o = (uint64_t)bs * a.S + at;
        lo = a.enc[o] ^ a.rec[o], hi = a.enc[o + 32] ^ a.rec[o + 32];
    } else if (bk == EL_ORIGINAL) {
        lo = err & 0xFFu, hi = err >> 8;
        const uint64_t o = (uint64_t)bs * a.S + at;
        a.E[o] = (uint8_t)lo, a.E[o + 32] = (uint8_t)hi;
    }
    if (a.fix) a.fix[at] = (uint8_t)lo, a.fix[at + 32] = (uint8_t)hi;
    if (e == 0) {
        a.status[c] = (uint8_t)(bk == EL_BAD ? RS16_LOCATE_UNLOCATABLE : bk);
        a.shard[c] = bk == EL_BAD ? NONE : bs;
        a.cand[c] = bk == EL_ORIGINAL ? bs : NONE;
    }
}

// Grid x = block, y = row chunk; 8 lanes per row of the block, 32 rows per
// workgroup pass.  Workgroups of blocks without a candidate return at once.  A
// lane that finds encode(E) ^ syndrome nonzero downgrades the block (the stores
// of several such lanes carry the same values).  The first row chunk's
// workgroup puts the candidate's block of E back to zero: E was consumed by the
// encode before this launch.  Grid z is the stripe (MANY = false: one stripe).
template <bool MANY>
__global__ void __launch_bounds__(SCAN_THREADS) locate_confirm_kernel(LocateArgs a, uint32_t rows_per_wg) {
    const uint32_t c = blockIdx.x, st = MANY ? blockIdx.z : 0;
    const uint32_t i = a.cand[st * a.bs_cand + c];
    if (i == NONE) return;
    if (MANY) {
        a.enc += st * a.bs_enc, a.rec += st * a.bs_rec, a.enc2 += st * a.bs_enc2, a.E += st * a.bs_E;
        a.status += st * a.bs_status, a.shard += st * a.bs_shard;
        if (a.fix) a.fix += st * a.bs_fix;
    }
    if (blockIdx.y == 0 && threadIdx.x < 16) ((uint32_t*)(a.E + (uint64_t)i * a.S + (uint64_t)c * 64))[threadIdx.x] = 0;
    const uint32_t r0 = blockIdx.y * rows_per_wg;
    const uint32_t r1 = r0 + rows_per_wg < a.m ? r0 + rows_per_wg : a.m;
    const uint64_t off = (uint64_t)c * 64 + (threadIdx.x & 7) * 4;
    uint32_t bad = 0;
    for (uint32_t r = r0 + (threadIdx.x >> 3); r < r1; r += SCAN_THREADS / 8) {
        const uint64_t o = (uint64_t)r * a.S + off;
        bad |= load32(a.enc + o) ^ load32(a.rec + o) ^ load32(a.enc2 + o);
        bad |= load32(a.enc + o + 32) ^ load32(a.rec + o + 32) ^ load32(a.enc2 + o + 32);
    }
    if (bad) {
        a.status[c] = RS16_LOCATE_UNLOCATABLE;
        a.shard[c] = NONE;
        if (a.fix)
            for (uint32_t b = 0; b < 64; b++) a.fix[(uint64_t)c * 64 + b] = 0;
    }
}

// The heal: 16 lanes per block, one dword each, 16 blocks of one stripe per
// workgroup (grid x), stripes over grid y (strided when there are more stripes
// than grid rows).  A block whose final status is ORIGINAL or RECOVERY and
// whose array is given (orig_w / rec_w, by the heal's mask) gets its fix XORed
// into the named shard; every block is counted in the workgroup's histogram,
// which goes to the stripe's four counters with one atomic per nonzero entry.
__global__ void __launch_bounds__(256) locate_apply_kernel(LocateArgs a) {
    __shared__ uint32_t s_cnt[4];
    const uint32_t lane = threadIdx.x & 15;
    const uint32_t c = blockIdx.x * 16 + (threadIdx.x >> 4);
    for (uint32_t st = blockIdx.y; st < a.nstripes; st += gridDim.y) {
        if (threadIdx.x < 4) s_cnt[threadIdx.x] = 0;
        __syncthreads();
        if (c < a.blocks) {
            const uint32_t status = a.status[st * a.bs_status + c] & 3u;
            const uint32_t i = a.shard[st * a.bs_shard + c];
            uint8_t* dst = nullptr;
            // (an index outside the shard counts is never followed)
            if (status == RS16_LOCATE_ORIGINAL && a.orig_w && i < a.k)
                dst = a.orig_w + st * a.bs_orig + (uint64_t)i * a.S;
            else if (status == RS16_LOCATE_RECOVERY && a.rec_w && i < a.m)
                dst = a.rec_w + st * a.bs_rec + (uint64_t)i * a.S;
            if (dst) {
                uint32_t* d = (uint32_t*)(dst + (uint64_t)c * 64) + lane;
                *d ^= ((const uint32_t*)(a.fix + st * a.bs_fix + (uint64_t)c * 64))[lane];
            }
            if (lane == 0) atomicAdd(&s_cnt[status], 1u);
        }
        __syncthreads();
        if (threadIdx.x < 4 && s_cnt[threadIdx.x])
            atomicAdd(&a.counts[st * a.bs_counts + threadIdx.x], s_cnt[threadIdx.x]);
    }
}

__global__ void __launch_bounds__(256) locate_unit_kernel(uint8_t* buf, uint64_t Sc, uint32_t i0, uint32_t n,
                                                          uint32_t value) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q < n) buf[(uint64_t)(i0 + q) * Sc + 64 * (q >> 5) + (q & 31)] = (uint8_t)value;
}

// rows_per_wg of a launch of about SCAN_WGS workgroups, gx of them side by side
// (over the columns and the stripes), each pass of a workgroup taking `step`
// rows and every thread at least four.
static uint32_t chunk_rows(uint32_t m, uint64_t gx, uint32_t step) {
    uint32_t gy = SCAN_WGS / gx ? (uint32_t)(SCAN_WGS / gx) : 1;
    const uint32_t most = (m + 4 * step - 1) / (4 * step);
    if (gy > most) gy = most;
    const uint32_t rows = (m + gy - 1) / gy;
    return (rows + step - 1) / step * step;
}

LocateScanShape locate_scan_shape(uint64_t S, uint32_t m, uint32_t nstripes) {
    LocateScanShape sh{};
    const uint64_t cols = S / 8;
    if (cols >= SCAN_THREADS) {
        sh.cw = SCAN_THREADS, sh.rsub = 1, sh.gx = (uint32_t)((cols + SCAN_THREADS - 1) / SCAN_THREADS);
    } else {
        sh.cw = (uint32_t)cols, sh.rsub = SCAN_THREADS / (uint32_t)cols, sh.gx = 1;
    }
    sh.rows_per_wg = chunk_rows(m, (uint64_t)sh.gx * nstripes, sh.rsub);
    sh.gy = (m + sh.rows_per_wg - 1) / sh.rows_per_wg;
    return sh;
}

// what every launch asks of the stripe dimension: grid y and z stop at 65535,
// and a stripe's rows of enc and rec lie inside its stride
static bool stripes_ok(const LocateArgs& a) {
    return a.nstripes >= 1 && a.nstripes <= 65535 && a.bs_enc >= a.m * a.S && a.bs_rec >= a.m * a.S;
}

hipError_t launch_locate_scan(const LocateArgs& a, hipStream_t s) {
    if (!a.enc || !a.rec || !a.acc || a.nslots == 0 || (a.nslots & (a.nslots - 1)) || a.S == 0 || a.S % 64 ||
        a.m == 0 || a.m >= 65536 || !stripes_ok(a) || a.bs_acc < a.nslots * (a.S / 2))
        return hipErrorInvalidValue;
    const LocateScanShape sh = locate_scan_shape(a.S, a.m, a.nstripes);
    hipLaunchKernelGGL(a.nstripes > 1 ? locate_scan_kernel<true> : locate_scan_kernel<false>,
                       dim3(sh.gx, sh.gy, a.nstripes), dim3(SCAN_THREADS), 0, s, a.enc, a.rec, a.acc, a.nslots, a.S, a.m,
                       (uint32_t)(a.S / 8), sh.cw, sh.rsub, sh.rows_per_wg, a.bs_enc, a.bs_rec, a.bs_acc);
    return hipGetLastError();
}

hipError_t launch_locate_decide(const LocateArgs& a, hipStream_t s) {
    if (!a.enc || !a.rec || !a.E || !a.acc || a.nslots == 0 || a.nslots > LOCATE_MAX_SLOTS || !a.cand || !a.log || !a.exp || !a.log_m0 || !a.ratio ||
        !a.status || !a.shard || a.m < 2 || a.blocks == 0 || a.blocks != a.S / 64 || !stripes_ok(a) ||
        a.bs_acc < a.nslots * (a.S / 2) || a.bs_E < a.k * a.S || a.bs_cand < a.blocks || a.bs_status < a.blocks ||
        a.bs_shard < a.blocks || (a.fix && a.bs_fix < a.S))
        return hipErrorInvalidValue;
    const uint64_t all = (uint64_t)a.blocks * a.nstripes;  // (numbered in 32 bits by the kernel)
    if (all > 0x7FFFFFFFu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(a.nstripes > 1 ? locate_decide_kernel<true> : locate_decide_kernel<false>,
                       dim3((uint32_t)((all + 1) / 2)), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_locate_confirm(const LocateArgs& a, hipStream_t s) {
    if (!a.enc || !a.rec || !a.enc2 || !a.E || !a.cand || !a.status || !a.shard || a.blocks == 0 ||
        a.blocks != a.S / 64 || !stripes_ok(a) || a.bs_enc2 < a.m * a.S)
        return hipErrorInvalidValue;
    const uint32_t step = SCAN_THREADS / 8;
    const uint32_t gx = a.blocks;
    const uint64_t wide = (uint64_t)gx * a.nstripes;
    const uint32_t rows_per_wg = chunk_rows(a.m, wide < SCAN_WGS ? wide : SCAN_WGS, step);
    hipLaunchKernelGGL(a.nstripes > 1 ? locate_confirm_kernel<true> : locate_confirm_kernel<false>,
                       dim3(gx, (a.m + rows_per_wg - 1) / rows_per_wg, a.nstripes), dim3(SCAN_THREADS), 0, s, a,
                       rows_per_wg);
    return hipGetLastError();
}

hipError_t launch_locate_apply(const LocateArgs& a, hipStream_t s) {
    if (!a.status || !a.shard || !a.fix || !a.counts || (!a.orig_w && !a.rec_w) || a.blocks == 0 ||
        a.blocks != a.S / 64 || !stripes_ok(a) || a.bs_status < a.blocks || a.bs_shard < a.blocks || a.bs_fix < a.S ||
        a.bs_counts < 4 || (a.orig_w && a.bs_orig < a.k * a.S))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(locate_apply_kernel, dim3((a.blocks + 15) / 16, a.nstripes), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_locate_unit(uint8_t* buf, uint64_t Sc, uint32_t i0, uint32_t n, uint32_t value, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (!buf || Sc < 64 * (((uint64_t)n + 31) / 32)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(locate_unit_kernel, dim3((n + 255) / 256), dim3(256), 0, s, buf, Sc, i0, n, value);
    return hipGetLastError();
}

}  // namespace rs16
