// rs16_locate.hip -- the kernels of rs16_locate_device (include/rs16.h): which
// one shard of each 64-byte column block is corrupt.  The engine encodes the
// stored originals into a buffer of its own (enc); the syndrome of recovery row
// j is enc[j] ^ rec[j] and is never stored.
//   scan     per element position, over all m rows: how many rows have a
//            nonzero syndrome element there, and the sum of those rows (the
//            row itself when there is one)
//   decide   per block: classify its 32 elements, write status / shard / fix and
//            scatter an ORIGINAL candidate's error into the error array E
//   confirm  after the engine's encode of E: every ORIGINAL block must have
//            encode(E) equal to the syndrome in all m rows, else UNLOCATABLE
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
// profiles/r19_locate.txt); the decide kernel adds the copies up.
__global__ void __launch_bounds__(SCAN_THREADS) locate_scan_kernel(const uint8_t* enc, const uint8_t* rec,
                                                                   unsigned long long* acc, uint32_t nslots,
                                                                   uint64_t S, uint32_t m, uint32_t cols, uint32_t cw,
                                                                   uint32_t rsub, uint32_t rows_per_wg) {
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
// shard and fix is written; the element's pairs go back to zero.
__global__ void __launch_bounds__(64) locate_decide_kernel(LocateArgs a) {
    __shared__ uint32_t s_kind[2][32], s_shard[2][32];
    const uint32_t e = threadIdx.x & 31, h = threadIdx.x >> 5;
    const uint32_t c = blockIdx.x * 2 + h;
    const bool active = c < a.blocks;
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
// encode before this launch.
__global__ void __launch_bounds__(SCAN_THREADS) locate_confirm_kernel(LocateArgs a, uint32_t rows_per_wg) {
    const uint32_t c = blockIdx.x;
    const uint32_t i = a.cand[c];
    if (i == NONE) return;
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

__global__ void __launch_bounds__(256) locate_unit_kernel(uint8_t* buf, uint64_t Sc, uint32_t i0, uint32_t n,
                                                          uint32_t value) {
    const uint32_t q = blockIdx.x * 256 + threadIdx.x;
    if (q < n) buf[(uint64_t)(i0 + q) * Sc + 64 * (q >> 5) + (q & 31)] = (uint8_t)value;
}

// rows_per_wg of a launch of about SCAN_WGS workgroups, gx of them side by side,
// each pass of a workgroup taking `step` rows and every thread at least four.
static uint32_t chunk_rows(uint32_t m, uint32_t gx, uint32_t step) {
    uint32_t gy = SCAN_WGS / gx ? SCAN_WGS / gx : 1;
    const uint32_t most = (m + 4 * step - 1) / (4 * step);
    if (gy > most) gy = most;
    const uint32_t rows = (m + gy - 1) / gy;
    return (rows + step - 1) / step * step;
}

LocateScanShape locate_scan_shape(uint64_t S, uint32_t m) {
    LocateScanShape sh{};
    const uint64_t cols = S / 8;
    if (cols >= SCAN_THREADS) {
        sh.cw = SCAN_THREADS, sh.rsub = 1, sh.gx = (uint32_t)((cols + SCAN_THREADS - 1) / SCAN_THREADS);
    } else {
        sh.cw = (uint32_t)cols, sh.rsub = SCAN_THREADS / (uint32_t)cols, sh.gx = 1;
    }
    sh.rows_per_wg = chunk_rows(m, sh.gx, sh.rsub);
    sh.gy = (m + sh.rows_per_wg - 1) / sh.rows_per_wg;
    return sh;
}

hipError_t launch_locate_scan(const LocateArgs& a, hipStream_t s) {
    if (!a.enc || !a.rec || !a.acc || a.nslots == 0 || (a.nslots & (a.nslots - 1)) || a.S == 0 || a.S % 64 ||
        a.m == 0 || a.m >= 65536)
        return hipErrorInvalidValue;
    const LocateScanShape sh = locate_scan_shape(a.S, a.m);
    hipLaunchKernelGGL(locate_scan_kernel, dim3(sh.gx, sh.gy), dim3(SCAN_THREADS), 0, s, a.enc, a.rec, a.acc, a.nslots,
                       a.S, a.m, (uint32_t)(a.S / 8), sh.cw, sh.rsub, sh.rows_per_wg);
    return hipGetLastError();
}

hipError_t launch_locate_decide(const LocateArgs& a, hipStream_t s) {
    if (!a.enc || !a.rec || !a.E || !a.acc || a.nslots == 0 || a.nslots > LOCATE_MAX_SLOTS || !a.cand || !a.log || !a.exp || !a.log_m0 || !a.ratio ||
        !a.status || !a.shard || a.m < 2 || a.blocks == 0 || a.blocks != a.S / 64)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(locate_decide_kernel, dim3((a.blocks + 1) / 2), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_locate_confirm(const LocateArgs& a, hipStream_t s) {
    if (!a.enc || !a.rec || !a.enc2 || !a.E || !a.cand || !a.status || !a.shard || a.blocks == 0 ||
        a.blocks != a.S / 64)
        return hipErrorInvalidValue;
    const uint32_t step = SCAN_THREADS / 8;
    const uint32_t gx = a.blocks;
    const uint32_t rows_per_wg = chunk_rows(a.m, gx < SCAN_WGS ? gx : SCAN_WGS, step);
    hipLaunchKernelGGL(locate_confirm_kernel, dim3(gx, (a.m + rows_per_wg - 1) / rows_per_wg), dim3(SCAN_THREADS), 0, s,
                       a, rows_per_wg);
    return hipGetLastError();
}

hipError_t launch_locate_unit(uint8_t* buf, uint64_t Sc, uint32_t i0, uint32_t n, uint32_t value, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (!buf || Sc < 64 * (((uint64_t)n + 31) / 32)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(locate_unit_kernel, dim3((n + 255) / 256), dim3(256), 0, s, buf, Sc, i0, n, value);
    return hipGetLastError();
}

}  // namespace rs16
