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

// ---------------------------------------------------------------------------
// The general decode's last pass (DEC_LAST: y = u + L(z) -> FFT of the tile's
// 8 low row bits -> reveal x (65535 - e) -> store the lost originals,
// rate_high.rs:232-242 / rate_low.rs:232-242) as one wave per quad column of
// a 256-row tile instead of one 8-wave workgroup per (tile, 32-quad slab):
// lane l holds 4 rows of its quad column, the FFT runs in 4 radix-4 blocks
// in registers with in-wave row-bit exchanges (colops, as the column codec
// at 256 rows), the in-tile formal-derivative terms come from registers and
// lane shuffles (no LDS image, no barrier).  Four quad columns per
// workgroup share the tile's 255 twiddle tables (staged by LDS-DMA once) and
// the tile's erasure logs.  A decode that lost few originals needs this pass
// for a handful of tiles only (lost-range pruning): there the 8-wave item's
// latency (two waves per SIMD through 8 layers of 16 rows) was the whole
// pass, 25 us for the reference bench's 1 % loss; here each wave carries a
// quarter of the rows.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) tile_last_kernel(PassArgs a) {
    using namespace colops;
    constexpr int T = 8;
    constexpr uint32_t NTAB = (1u << T) - 1;
    __shared__ __attribute__((aligned(16))) uint8_t tabs[NTAB * 80];
    __shared__ uint32_t elds[256];
    const uint32_t t = threadIdx.x, lane = t & 63, w = uni(t >> 6);
    const uint32_t nq4 = (a.qrow + 3) / 4;
    uint32_t tile = blockIdx.x / nq4;
    const uint32_t qg = blockIdx.x - tile * nq4;
    if (a.stripe_tiles) {
        const uint32_t st = uni(tile / a.stripe_tiles);
        tile -= st * a.stripe_tiles;
        stripe_displace(a, st);
    }
    if (a.lostrange) {
        // The grid covers min(tiles, tl_max) tiles per stripe, counted from
        // the first one with a lost original; lost originals over more than
        // tl_max tiles are DEC_LAST's (its 8-wave items win there:
        // scripts/probe_general.py, break-even 16-32 tiles), and a tile past
        // the last lost original stores nothing.
        uint32_t r0, r1;
        lost_range(a, r0, r1);
        if (!tl_covers<T>(a)) return;
        tile += r0 >> T;
        if (tile > ((r1 - 1) >> T)) return;
    } else {
        tile += a.tile_base;
    }
    RS16_STAMP(a, 0);
    const uint32_t q = qg * 4 + w;
    const bool active = q < a.qrow;
    const uint32_t offL = (q >> 3) * 64 + (q & 7) * 4;
    const bool ztile = a.zflags && tile_is_zero(a, tile);
    // ---- requests: z and u of the lane's rows in the first FFT block's
    // layout (row bits 6, 7 in registers: row k = lane + 64 m), the tile's
    // erasure-log block (wave 0, when eval_poly left its last H_lo to this
    // pass), then the twiddle tables by LDS-DMA
    uint32_t ZL[4], ZH[4], YL[4], YH[4];
    const uint8_t* zpage = a.zero + (offL & 0x7FFFu);
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const uint64_t r = ((uint64_t)tile << T) + lane + 64u * m;
        const uint32_t* pz = (const uint32_t*)(active && !ztile ? a.in + r * a.S_in + offL : zpage);
        const uint32_t* pu = (const uint32_t*)(active ? a.in2 + r * a.S_in + offL : zpage);
        ZL[m] = pz[0];
        ZH[m] = pz[8];
        YL[m] = pu[0];
        YH[m] = pu[8];
    }
    const uint32_t row0 = (tile << T) + a.row_base_out;  // the tile's first decode work row
    uint32_t ev[4] = {0, 0, 0, 0};
    if (a.ework && w == 0) {
#pragma unroll
        for (int j = 0; j < 4; j++) ev[j] = a.ework[(row0 & ~255u) + lane + 64u * j];
    }
#pragma unroll
    for (uint32_t i = 0; i * 256 < NTAB * 5; i++) {
        const uint32_t c = i * 256 + t;
        if (c < NTAB * 5) {
            // chunk c = part c % 5 of table tb = c / 5 (tile-group order: layer
            // kb at groups [2^T - 2^(T-kb), ...), group j = row >> (kb + 1))
            const uint32_t tb = c / 5, part = c - tb * 5;
            const uint32_t kb = (uint32_t)(T - 32 + __clz(NTAB - tb));
            const uint32_t j = tb - ((1u << T) - (1u << (T - kb)));
            const uint32_t idx = (tile << T) + (j << (kb + 1)) + (1u << kb) + a.skew_fft - 1;
            __builtin_amdgcn_global_load_lds((colops::glb_vp)(a.skew_tab + (size_t)idx * TAB_DWORDS + part * 4),
                                             (colops::lds_vp)(tabs + (i * 256 + 64 * w) * 16), 16, 0, 0);
        }
    }
    RS16_STAMP(a, 1);
    __builtin_amdgcn_s_waitcnt(0);
    if (a.ework && w == 0) {
        fwht256_wave(ev);  // the last 256-point FWHT of eval_poly (src/engine.rs:207-218)
#pragma unroll
        for (int j = 0; j < 4; j++) elds[lane + 64 * j] = ev[j];
    }
    __syncthreads();  // tables and logs in LDS
    RS16_STAMP(a, 2);
    // ---- reveal multipliers of the lane's output rows (the last block's
    // layout: row k = 4 lane + m), requested now, used after the FFT
    uint32_t rt[4][20];
    bool lost[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const uint32_t r = row0 + 4 * lane + m;
        lost[m] = active && row_lost_original(a, r);
        const uint32_t e = a.ework ? elds[(4 * lane + m + row0) & 255u] : (lost[m] ? a.elog[r] : 0u);
        glb_table(rt[m], a.mul_tab, lost[m] ? GF_MODULUS - e : ZERO_ENTRY);
    }
    // ---- y = u + L(z): the formal derivative's terms of the tile's row bits
    // (src/engine.rs:233-238 in closed form): y[k] ^= z[k | 2^b] for every
    // bit b < 8 that is 0 in k -- bits 6, 7 are register bits, 0-5 lane bits
    if (!ztile) {
#pragma unroll
        for (int m = 0; m < 4; m++) {
            if (!(m & 1)) YL[m] ^= ZL[m | 1], YH[m] ^= ZH[m | 1];
            if (!(m & 2)) YL[m] ^= ZL[m | 2], YH[m] ^= ZH[m | 2];
        }
#define RS16_FDL(B)                                                                   \
        {                                                                             \
            const bool take = !(lane & (1u << (B)));                                  \
            _Pragma("unroll") for (int m = 0; m < 4; m++) {                           \
                const uint32_t pl = (uint32_t)xshfl<(1 << (B))>((int)ZL[m]);          \
                const uint32_t ph = (uint32_t)xshfl<(1 << (B))>((int)ZH[m]);          \
                YL[m] ^= take ? pl : 0u;                                              \
                YH[m] ^= take ? ph : 0u;                                              \
            }                                                                         \
        }
        RS16_FDL(0) RS16_FDL(1) RS16_FDL(2) RS16_FDL(3) RS16_FDL(4) RS16_FDL(5)
#undef RS16_FDL
    }
    // ---- FFT of the tile's 8 row bits, high layers first: blocks (6, 7),
    // (4, 5), (2, 3), (0, 1)
    auto tabs_of = [&](BlockTabs& bt, auto b0c, auto b1c) {
        constexpr int B0 = decltype(b0c)::value, B1 = decltype(b1c)::value;
        const uint32_t r0 = brow<B0, B1>(lane, 0), r2 = brow<B0, B1>(lane, 2);
        auto off = [](int kb, uint32_t r) { return (((1u << T) - (1u << (T - kb))) + (r >> (kb + 1))) * 80u; };
        lds_table(bt.w0, tabs, off(B0, r0));
        lds_table(bt.w2, tabs, off(B0, r2));
        lds_table(bt.w1, tabs, off(B1, r0));
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    using I3 = std::integral_constant<int, 3>;
    using I4 = std::integral_constant<int, 4>;
    using I5 = std::integral_constant<int, 5>;
    using I6 = std::integral_constant<int, 6>;
    using I7 = std::integral_constant<int, 7>;
    RS16_STAMP(a, 3);
    BlockTabs ta, tb;
    tabs_of(ta, I6(), I7());
    tabs_of(tb, I4(), I5());
    compute<true, true, true>(YL, YH, ta);
    wave_exchange<4, 5>(YL, YH);
    tabs_of(ta, I2(), I3());
    compute<true, true, true>(YL, YH, tb);
    wave_exchange<2, 3>(YL, YH);
    tabs_of(tb, I0(), I1());
    compute<true, true, true>(YL, YH, ta);
    wave_exchange<0, 1>(YL, YH);
    compute<true, true, true>(YL, YH, tb);
    RS16_STAMP(a, 9);
    // ---- reveal (x (65535 - e)) and store the lost originals in place
    // (restored-originals row = work row - the originals' segment start)
    const int64_t shift = (int64_t)a.row_base_out - (a.rest_seg_b ? (int64_t)a.chunk : 0);
#pragma unroll
    for (int m = 0; m < 4; m++) {
        if (!lost[m]) continue;
        uint32_t ol = 0, oh = 0;
        mul_xor(ol, oh, YL[m], YH[m], rt[m]);
        const int64_t rr = (int64_t)(tile << T) + 4 * lane + m + shift;
        uint32_t* p = (uint32_t*)(a.rest + rr * (int64_t)a.S_rest + offL);
        // (plain stores: 32768:32768 1 %-loss decode 103.1 -> 101.5 us against
        // non-temporal ones, same-box A/B x 3)
        p[0] = ol;
        p[8] = oh;
    }
    RS16_STAMP(a, 10);
    RS16_STAMP_END(a);
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
