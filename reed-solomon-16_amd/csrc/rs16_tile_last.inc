// rs16_tile_last.inc -- the body of tile_last_kernel, as text: included inside
// the kernel's two __global__ definitions, tile_last_kernel (rs16_pass_small.hpp,
// in the decoder's unit) and tile_last_sel_kernel (rs16_pass_select.hip, the
// selective decode's), with `a` (the PassArgs parameter) and the constant RULE
// (RowRule, rs16_pass_common.hpp) in scope.  The two differ in the row predicate
// alone (row_wanted<RULE>), which feeds the lost[] array, the choice of the
// reveal table and the stores.  Text and not a function template: with the
// body in a __device__ __forceinline__ function tile_last_kernel compiles to
// other machine code (scripts/isa_compare.py), as the pass kernels do
// (RS16_PASS_HEAD, rs16_pass.hpp).  The includer brings rs16_pass_common.hpp,
// rs16_fwht.hpp, rs16_colops.hpp and rs16_diag.hpp.
//
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
        lost[m] = active && row_wanted<RULE>(a, r);
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
