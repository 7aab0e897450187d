// rs16_pass_small.hpp -- the two small kernels of the general decode that
// stand in for a pass when the lost originals are few: tile_last_kernel (the
// last pass, DEC_LAST) and mid_direct_kernel (the middle pass, DEC_MID), with
// their launchers.  They share the column codec's in-wave operations
// (rs16_colops.hpp), not the pass template.
//
// Included by rs16_pass_dec.hip alone, which defines them: compiled in a unit
// of its own, tile_last_kernel comes out as other machine code than beside
// the decoder's pass kernels (the Makefile says why).
#pragma once
#include <algorithm>

#include "rs16_pass_common.hpp"
#include "rs16_fwht.hpp"
#include "rs16_colops.hpp"
#include "rs16_diag.hpp"

namespace rs16 {

// tile_last_kernel: the general decode's last pass, one wave per quad column
// of a 256-row tile (the body and its description: rs16_tile_last.inc).
__global__ void __launch_bounds__(256) tile_last_kernel(PassArgs a) {
    constexpr int RULE = ROWS_LOST;
#include "rs16_tile_last.inc"
}

// The grid is num_tiles tiles (x stripes) wide.  With a.lostrange set the
// kernel counts them from the stripe's first lost tile, read from lostrange
// (a.tile_base is not used), and takes the stripe only when its lost tiles
// number at most a.tl_max: tl_max = 0 would restore nothing, so it is an error.
hipError_t launch_tile_last(const PassArgs& a, uint32_t num_tiles, hipStream_t s) {
    if (a.lostrange && a.tl_max == 0) return hipErrorInvalidValue;
    if (num_tiles == 0 || a.qrow == 0) return hipSuccess;
    const uint32_t nwg = num_tiles * ((a.qrow + 3) / 4);
    hipLaunchKernelGGL(tile_last_kernel, dim3(nwg), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The general decode's middle pass as a direct product.  DEC_MID is the same
// linear map u = FFT_hi (I + H) IFFT_hi z on every tile column j (rows
// t << lo | j; its twiddles do not involve j), a 2^hi x 2^hi matrix M over
// GF(2^16) (mid_matrix_entries, rs16_tables.cpp).  When the lost originals
// lie in few last-pass tiles, DEC_LAST consumes only the U rows t in
// [nlo, nhi) -- nhi - nlo <= MID_DIRECT_MAX -- and each is a sum over the
// live z rows (DEC_FIRST tiles with a received row, zflags):
//   u[o << lo | j] = sum over live t of M[o][t] z[t << lo | j]
// -- (nhi - nlo) x (live rows) multiplies per column instead of DEC_MID's
// 2^hi-point IFFT, derivative and output-pruned FFT (at the reference
// bench's 1 % loss: 2 x 129 against ~1300 butterflies, and one dispatch
// round instead of two).  Workgroup = (column j, 64-quad slab, stripe);
// its 8 waves take the rows t = w mod 8 (the zero tiles cluster, so
// interleaved), all of a wave's rows requested at once, and multiply them by
// the tables of rows [nlo, nhi) of M in LDS (one LDS-DMA copy of the
// contiguous v_perm tables), then XOR their partial sums through LDS; wave o
// stores row nlo + o.  A stripe whose consumed rows exceed
// MID_DIRECT_MAX returns here and DEC_MID computes it (PassArgs::mid_direct).
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(512) mid_direct_kernel(PassArgs a, const uint32_t* mtab, uint32_t hi) {
    constexpr uint32_t W = 8, RPW = 256 / W;  // waves; rows per wave at 2^hi = 256
    extern __shared__ __attribute__((aligned(16))) uint8_t mlds[];
    // blockIdx.x = column j x slabs + 64-quad slab (one index: the stamps' workgroup id)
    const uint32_t nslab = (a.qrow + 63) / 64;
    const uint32_t j = blockIdx.x / nslab, slab = blockIdx.x - j * nslab;
    const uint32_t t0 = threadIdx.x, lane = t0 & 63, w = uni(t0 >> 6);
    __builtin_assume(a.lostrange != nullptr);  // (launched for lost-range-pruned decodes only: mid_need reads it)
    if (blockIdx.z) stripe_displace(a, blockIdx.z);  // stripe z
    uint32_t nlo, nhi;
    if (!mid_need(a, nlo, nhi)) return;
    const uint32_t N = 1u << hi, nout = nhi - nlo, rpw = N / W;
    RS16_STAMP(a, 0);
    const uint32_t Qg = slab * 64 + lane;
    const bool active = Qg < a.qrow;
    const uint32_t offL = (Qg >> 3) * 64 + (Qg & 7) * 4;
    const uint8_t* zpage = a.zero + (offL & 0x7FFFu);
    // The wave's rows t = w + 8 u (a dead row -- DEC_FIRST tile without a
    // received row -- reads the zero page) and the tables of rows [nlo, nhi)
    // of M (LDS-DMA, L2-resident after the first workgroups).
    // (lane u reads row u's zero-tile flag: one load and a ballot)
    const bool lv_lane = lane < rpw && !(a.zflags && a.zflags[w + W * lane]);
    const uint64_t live = __ballot(lv_lane);
    const uint8_t* rbase = a.in + ((uint64_t)w << a.lo | j) * a.S_in;
    const uint64_t rstride = ((uint64_t)W << a.lo) * a.S_in;
    // Rows in batches of RPB: batch b + 1 is requested once batch b has
    // landed, before batch b's multiplies.  (All rows requested at once land
    // together at the end of the chip-wide load phase and the VALU idles
    // through it: 14.8 us per workgroup, half of it loads,
    // `profiles/r05_mid_direct.txt`.)
    constexpr uint32_t RPB = 8, NB = RPW / RPB;
    uint32_t zl[2][RPB], zh[2][RPB];
    auto fetch = [&](uint32_t b, uint32_t (&l)[RPB], uint32_t (&h)[RPB]) {
#pragma unroll
        for (uint32_t v = 0; v < RPB; v++) {
            const uint32_t u = b * RPB + v;
            const uint32_t* p = (const uint32_t*)(active && ((live >> u) & 1u) ? rbase + u * rstride + offL : zpage);
            l[v] = p[0];
            h[v] = p[8];
        }
    };
    fetch(0, zl[0], zh[0]);
    uint4* tabs = (uint4*)mlds;
    colops::dma_copy_rt<W * 64>((const uint8_t*)(mtab + (size_t)nlo * N * 20), mlds, nout * N * 80);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();  // tables in LDS
    RS16_STAMP(a, 1);
    uint32_t acc[MID_DIRECT_MAX][2] = {};
    auto multiply = [&](uint32_t b, const uint32_t (&l)[RPB], const uint32_t (&h)[RPB]) {
#pragma unroll
        for (uint32_t v = 0; v < RPB; v++) {
            const uint32_t u = b * RPB + v;
            if (!((live >> u) & 1u)) continue;  // (uniform)
            const uint32_t t = w + W * u;
#pragma unroll
            for (uint32_t o = 0; o < MID_DIRECT_MAX; o++) {
                if (o >= nout) break;
                uint32_t tt[20];
                load_table_lds(tt, tabs + (o * N + t) * 5);
                mul_xor(acc[o][0], acc[o][1], l[v], h[v], tt);
            }
        }
    };
#pragma unroll
    for (uint32_t b = 0; b < NB; b++) {
        if (b * RPB >= rpw) break;  // (uniform: 2^hi < 256)
        if (b + 1 < NB && (b + 1) * RPB < rpw) fetch(b + 1, zl[(b + 1) & 1], zh[(b + 1) & 1]);
        multiply(b, zl[b & 1], zh[b & 1]);
        __builtin_amdgcn_s_waitcnt(vmcnt_wait(0));
    }
    RS16_STAMP(a, 2);
    // XOR the waves' partial sums: row o by wave o
    __syncthreads();  // (the tables are no longer read: the partials reuse their LDS)
    uint2* part = (uint2*)mlds;
#pragma unroll
    for (uint32_t o = 0; o < MID_DIRECT_MAX; o++)
        if (o < nout) part[(w * MID_DIRECT_MAX + o) * 64 + lane] = make_uint2(acc[o][0], acc[o][1]);
    __syncthreads();
    if (w < nout) {
        uint32_t xl = 0, xh = 0;
#pragma unroll
        for (uint32_t v = 0; v < W; v++) {
            const uint2 q = part[(v * MID_DIRECT_MAX + w) * 64 + lane];
            xl ^= q.x;
            xh ^= q.y;
        }
        if (active) {
            uint32_t* p = (uint32_t*)(a.out + ((uint64_t)(nlo + w) << a.lo | j) * a.S_out + offL);
            p[0] = xl;
            p[8] = xh;
        }
    }
    RS16_STAMP_END(a);
}

hipError_t launch_mid_direct(const PassArgs& a, const uint32_t* mtab, uint32_t hi, uint32_t ns, hipStream_t s) {
    if (a.qrow == 0 || ns == 0) return hipSuccess;
    const uint32_t N = 1u << hi;
    // tables of up to MID_DIRECT_MAX rows (bounded by the host's consumed range)
    const uint32_t rows = std::min(MID_DIRECT_MAX, a.need_hi > a.need_lo ? a.need_hi - a.need_lo : 0u);
    if (rows == 0 || hi > 8 || hi < 3) return rows == 0 ? hipSuccess : hipErrorInvalidValue;
    const size_t lds = std::max((size_t)rows * N * 80, (size_t)8 * MID_DIRECT_MAX * 64 * 8);
    if (lds > 65536) {  // (as launch_pass: set on every call, i.e. on the current device)
        hipError_t e = hipFuncSetAttribute((const void*)mid_direct_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(mid_direct_kernel, dim3((1u << a.lo) * ((a.qrow + 63) / 64), 1, ns), dim3(512), lds, s, a, mtab,
                       hi);
    return hipGetLastError();
}

}  // namespace rs16
