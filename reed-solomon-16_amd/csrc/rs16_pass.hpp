// rs16_pass.hpp -- the HBM-pass kernel template of the MI355X GF(2^16)
// Reed-Solomon engine: the FFT/IFFT butterflies of the reference `Engine`
// (src/engine/engine_nosimd.rs:190-384, spec src/engine/engine_naive.rs:43-124)
// fused with the Rate-level steps around them (src/rate/rate_high.rs:44-83,
// 168-247; src/rate/rate_low.rs:168-247).
//
// Included only by the units that instantiate pass_kernel<P, T, NV>
// (rs16_pass_enc.hip, rs16_pass_dec.hip; rs16_pass_tower.hip for the tower
// flavours pass_kernel_late_tower; rs16_pass_repair.hip for the repair's
// programs, pass_kernel_repair; rs16_pass_select.hip for the selective
// decode's, pass_kernel_select; rs16_pass_verify.hip for the scrub's,
// pass_kernel_verify); launch_pass (rs16_pass_launch.hip)
// reaches the kernels through their PassKernel lookups.
//
// Structure of one pass
// ---------------------
//   A transform of 2^L rows runs in ceil(L/8) HBM passes.  A pass works on
//   items: an item is a tile of 2^T rows (T <= 8) x Q quads (a quad = 4
//   elements = one lo dword + one hi dword, rs16_gf.hpp), loaded, run
//   through T layers and stored.  Tile t covers rows
//   b_low + (k << lo) + (b_high << (lo+T)), k in [0, 2^T): lo = 0 gives
//   contiguous tiles, lo > 0 strided ones; the slab of an item selects its Q
//   quads of the row.
//
//   One item per workgroup: the twiddle tables of the tile are requested
//   first and the tile's rows right behind them, then staged, computed and
//   stored (a software-pipelined persistent variant
//   measured slower at every T, CHANGELOG.md round 3).
//
//   Lane = quad.  Each thread keeps 16 rows ("a row set") of its quad in
//   VGPRs (8 at T = 5); a wave holds 64/Q row sets (Q = 32 quads per tile row
//   from T = 5 on: 2 row sets per wave).  The 4 layers whose row bits are in registers
//   are radix-16 butterfly networks with no data movement; an LDS transpose
//   switches between layout A (k bits 0-3 in registers) and layout B (k bits
//   T-4..T-1).
//
//   Twiddle tables: a tile needs 2^T - 1 distinct twiddles per transform
//   direction (one per (layer, group)).  Their 80-byte v_perm multiply tables
//   are staged into LDS (one level of loads from skew_tab) and read with ds_read_b128
//   (5 per group, broadcast within each row set), one group ahead of use.
//   Groups are compiled as a straight-line sequence separated by register
//   pins, so a wave holds at most two tables.  The decoder's per-row erasure
//   multipliers (gather and reveal) are staged the same way.
//
//   Butterflies (bit-exact spec, the reference's):
//     FFT  layer d: a ^= b * skew[r + d + skew_delta - 1];  b ^= a
//     IFFT layer d: b ^= a;  a ^= b * skew[r + d + skew_delta - 1]
//   r = group start (row & ~(2d-1)); the GF_MODULUS sentinel ("no multiply",
//   engine_naive.rs:64,116) maps to the all-zero table ZERO_ENTRY.
//
//   Decode zero tiles: a DEC_FIRST tile none of whose rows was received is
//   all zero after the erasure multiply (rate_high.rs:210-228 zero-fills
//   every row it does not multiply) and stays zero through its IFFT layers.
//   It is neither computed nor stored; its flag zflags[tile] = 1 tells
//   DEC_MID to read those rows as zero and to skip the IFFT groups whose rows
//   all are, and DEC_LAST that its z term is zero (y = u + L(z) = u).  At
//   100 % original loss this is the whole original half of the decode work.
//
//   Zero twiddles: the sentinel sits exactly at skew indices 2^i - 1, i.e. at
//   the first group of each layout-B layer of the two-direction passes; those
//   groups run the XOR half of the butterfly only (wave-uniform test).
//
//   Narrow twiddles: a twiddle that is an element of the GF(2^8) subfield
//   multiplies with 9 of the 12 lookups (mul_xor_narrow, rs16_gf.hpp).  The
//   two-direction middle passes exist in compile-time variants that do so
//   from a given layer of each direction on (NarrowVar); launch_pass takes
//   the variant the launch's twiddle indices allow (first_narrow_layer).
//
//   Batched stripes (PassArgs::stripe_tiles): one launch covers independent
//   stripes of one geometry; a workgroup's tile index splits into (stripe,
//   tile within the stripe) and the stripe displaces its array pointers.
#pragma once
#include <type_traits>

#include "rs16_pass_common.hpp"
#include "rs16_fwht.hpp"
#include "rs16_diag.hpp"

namespace rs16 {

enum LoadMode { LD_PLAIN = 0, LD_GATHER_ENC, LD_GATHER_DEC, LD_DEC_LAST };
// ST_RESTORE_ALL (the repair's programs): ST_RESTORE for the lost rows of both
// segments, each stored to its own segment's array (PassArgs::rest / rest_b).
// ST_RESTORE_SEL (the selective decode's programs): ST_RESTORE for the lost
// originals of the read set only (PassArgs::wanted); the addresses are ST_RESTORE's.
// ST_VERIFY (the scrub's programs): ST_RECOVERY's rows and addresses on the
// stored recovery array (PassArgs::vfy_cmp), which is loaded and compared with
// the computed row; only flag bytes are stored (verify_rows).
enum StoreMode { ST_PLAIN = 0, ST_RECOVERY, ST_RESTORE, ST_RESTORE_ALL, ST_RESTORE_SEL, ST_VERIFY };
constexpr bool st_restores(int st) { return st == ST_RESTORE || st == ST_RESTORE_ALL || st == ST_RESTORE_SEL; }
// the row predicate of a restoring store mode (row_wanted)
constexpr int st_row_rule(int st) { return st == ST_RESTORE_ALL ? ROWS_ALL : (st == ST_RESTORE_SEL ? ROWS_SEL : ROWS_LOST); }

// Store cache policy: non-temporal stores in the single-direction passes,
// plain stores in the two-direction passes (same-box A/B, CHANGELOG.md round 3:
// nt / sc1 / sc0 sc1 everywhere and nt loads all measured slower).
template <int P> struct ProgTraits;
#define RS16_PROG(P, LD, I, F, FF, ST)          \
    template <> struct ProgTraits<P> {         \
        static constexpr int LOAD = LD;        \
        static constexpr bool IFFT = I;        \
        static constexpr bool FD = F;          \
        static constexpr bool FFT = FF;        \
        static constexpr int STORE = ST;       \
        static constexpr bool ST_NT = !(I && FF);                                           \
    };
RS16_PROG(GEN_FFT, LD_PLAIN, false, false, true, ST_PLAIN)
RS16_PROG(GEN_IFFT, LD_PLAIN, true, false, false, ST_PLAIN)
RS16_PROG(ENC_FIRST, LD_GATHER_ENC, true, false, false, ST_PLAIN)
RS16_PROG(ENC_MID, LD_PLAIN, true, false, true, ST_PLAIN)
RS16_PROG(ENC_LAST, LD_PLAIN, false, false, true, ST_RECOVERY)
RS16_PROG(ENC_SINGLE, LD_GATHER_ENC, true, false, true, ST_RECOVERY)
RS16_PROG(DEC_FIRST, LD_GATHER_DEC, true, false, false, ST_PLAIN)
RS16_PROG(DEC_MID, LD_PLAIN, true, true, true, ST_PLAIN)
RS16_PROG(DEC_LAST, LD_DEC_LAST, false, false, true, ST_RESTORE)
RS16_PROG(DEC_SINGLE, LD_GATHER_DEC, true, true, true, ST_RESTORE)
RS16_PROG(DEC_HALF_LAST, LD_PLAIN, false, false, true, ST_RESTORE)
RS16_PROG(DEC_HALF_SINGLE, LD_GATHER_DEC, true, false, true, ST_RESTORE)
RS16_PROG(DEC_LAST_ALL, LD_DEC_LAST, false, false, true, ST_RESTORE_ALL)
RS16_PROG(DEC_SINGLE_ALL, LD_GATHER_DEC, true, true, true, ST_RESTORE_ALL)
RS16_PROG(DEC_LAST_SEL, LD_DEC_LAST, false, false, true, ST_RESTORE_SEL)
RS16_PROG(DEC_SINGLE_SEL, LD_GATHER_DEC, true, true, true, ST_RESTORE_SEL)
RS16_PROG(ENC_LAST_VFY, LD_PLAIN, false, false, true, ST_VERIFY)
RS16_PROG(ENC_SINGLE_VFY, LD_GATHER_ENC, true, false, true, ST_VERIFY)
#undef RS16_PROG

// Row bits in registers: 4 (16 rows per thread) from T = 6 on; 3 at T = 5
// (the passes of the n <= 2048 codecs, which are latency-bound: 8 rows per
// thread and 16 quads per tile row give twice the waves, each with half the
// butterfly chain).  At T = 8 a tile row has 32 quads (8-wave workgroups,
// two per CU; 16 quads in 4-wave workgroups measured slower).
template <int T> struct Geo {
    static constexpr int R = T > 4 ? (T == 5 ? 3 : 4) : T;  // row bits held in registers
    static constexpr int NR = 1 << R;                     // rows per thread (a row set)
    static constexpr int SETS = 1 << (T - R);             // row sets per tile
    // Quads per tile row of the T = 7 passes (the encoder's first / last
    // passes and the identity decode's): 64 -- 8-wave workgroups, two per CU,
    // 512 items for a 32768-row stripe, each twiddle table staged once per 64
    // quad columns -- against 32 (4-wave workgroups, four per CU, 1024 items):
    // same-box A/B x 8, 805-815 -> 797-838 GiB/s, mean +1.5 %, 6 of 8 pairs
    // faster (profiles/r06_t7_q64_ab.txt).
    static constexpr int T7_Q = 64;
    // quads per tile row: 32 (two 16-row sets per wave) from T = 6 on, 16
    // (four 8-row sets per wave) at T = 5, 64 (one row set) below
    static constexpr int Q = T > 4 ? (R == 3 ? 16 : (T == 7 ? T7_Q : 32)) : 64;
    static constexpr int HWS = 64 / Q;                    // row sets per wave
    static constexpr int W = SETS / HWS > 0 ? SETS / HWS : 1;  // waves per workgroup
    static constexpr int SHB = T - R;                     // layout B: k = s + (m << SHB)
    static constexpr int THREADS = 64 * W;
    static constexpr int NTAB = (1 << T) - 1;             // twiddle groups per direction
    // Tables of layers kb >= R (layout-B phase) come last: t >= TSPLIT.
    static constexpr int TSPLIT = T > 4 ? (1 << T) - (1 << (T - R)) : 0;
};

template <int P, int T, int QL> struct SmemL;
// The layout switch goes through an LDS image of 2^T rows x QL quads x 8
// bytes, in Q / QL rounds.  One round (4 barriers -> 2 per switch, every
// LDS instruction with all lanes) when the program's whole layout still lets
// two workgroups share a CU (<= 80 KiB: the T = 7 encode passes, 64-quad
// rows); else two rounds of Q / 2 quads (the T = 8 passes, the decoders' T =
// 7 passes with their multiplier tables).  (One round for the T = 7 encode
// passes against two: profiles/r06_t7_one_round_ab.txt.)
constexpr int ONE_ROUND_MAX = 80 * 1024;
// The two-direction middle passes at T = 8 (ENC_MID, also the identity
// decode's middle pass, and DEC_MID): their one-round image (64 KiB) shares
// its LDS with the layout-A twiddle tables, which are dead during both layout
// switches (SmemL::SHARED).  Two rounds with the tables beside the image
// measured slower for both: profiles/r06_mid_shared_ab.txt,
// profiles/r06_dec_mid_shared_ab.txt.
template <int P, int T> struct Rnd {
    static constexpr int NQR = T >= 7 && SmemL<P, T, Geo<T>::Q>::BYTES > ONE_ROUND_MAX ? 2 : 1;
    static constexpr int QL = Geo<T>::Q / NQR;
};

// Dynamic LDS layout of program P at tile bits T (bytes):
//   [image: 2^T x QL x 8][ert: 2^T x 80 (gather multipliers)]
//   [tab1: NTAB x 80 (first direction)][tab2: NTAB x 80 (second direction)]
//   [rvt: 2^T x 80 (reveal multipliers)][lost: 2^T x u32 (row is a lost original)]
//   [elog: 256 x u32]
// Everything but the image is per tile key and stays resident across the
// items of that key.  At T = 8 the largest program (DEC_LAST) needs 75 KiB,
// so two workgroups share a CU.
template <int P, int T, int QL> struct SmemL {
    using PT = ProgTraits<P>;
    static constexpr bool TWO = PT::IFFT && PT::FFT;
    static constexpr int IMG_BYTES = T > 4 ? (1 << T) * QL * 8 : 0;
    // SHARED (ENC_MID and DEC_MID at T = 8, one round): [image 64 KiB,
    // holding the layout-A tables of each direction outside the switches]
    // [IFFT layout-B tables][FFT layout-B tables]
    static constexpr bool SHARED = (P == ENC_MID || P == DEC_MID) && T == 8 && QL == Geo<T>::Q;
    static constexpr int ERT_BYTES = PT::LOAD == LD_GATHER_DEC ? (1 << T) * 80 : 0;
    static constexpr int ERT_OFF = IMG_BYTES;
    static constexpr int TABB_OFF = IMG_BYTES;  // (SHARED: the IFFT's layout-B tables)
    static constexpr int TAB1_BYTES = SHARED ? 0 : Geo<T>::NTAB * 80;
    // Restage (two-direction programs, T > 4): tab2 holds only the second
    // direction's layout-B tables; its layout-A tables are requested before
    // the first layout switch and written over the first direction's (dead
    // by then) in tab1 between its barriers.
    static constexpr bool RESTAGE = TWO && T > 4;
    static constexpr int TAB2_BYTES = TWO ? (RESTAGE ? Geo<T>::NTAB - Geo<T>::TSPLIT : Geo<T>::NTAB) * 80 : 0;
    static constexpr int RVT_BYTES = st_restores(PT::STORE) ? (1 << T) * 80 : 0;
    static constexpr int LOST_BYTES = st_restores(PT::STORE) ? (1 << T) * 4 : 0;
    static constexpr int TAB1_OFF = SHARED ? 0 : ERT_OFF + ERT_BYTES;
    static constexpr int TAB2_OFF = SHARED ? TABB_OFF + (Geo<T>::NTAB - Geo<T>::TSPLIT) * 80 : TAB1_OFF + TAB1_BYTES;
    static constexpr int RVT_OFF = TAB2_OFF + TAB2_BYTES;
    static constexpr int LOST_OFF = RVT_OFF + RVT_BYTES;
    // erasure logs of the tile's rows when the pass finishes eval_poly (ework)
    static constexpr int ELOG_BYTES = (PT::LOAD == LD_GATHER_DEC || st_restores(PT::STORE)) ? 256 * 4 : 0;
    static constexpr int ELOG_OFF = LOST_OFF + LOST_BYTES;
    static constexpr int BYTES = ELOG_OFF + ELOG_BYTES;
};
template <int P, int T> struct Smem : SmemL<P, T, Rnd<P, T>::QL> {};

struct Thr {
    uint32_t lane, w, s;   // lane, wave, row set
    uint32_t qt;           // quad within the tile row
    uint32_t ql, round;    // quad within the LDS round, LDS round
    uint32_t b_low, b_high, offL;
    bool active;
};

template <int T, bool LB> __device__ __forceinline__ uint32_t kidx(const Thr& c, int m) {
    return LB ? c.s + ((uint32_t)m << Geo<T>::SHB) : (c.s << Geo<T>::R) + (uint32_t)m;
}

template <int T> __device__ __forceinline__ uint32_t row_rel(const Thr& c, const PassArgs& a, uint32_t k) {
    return c.b_low + (k << a.lo) + (c.b_high << (a.lo + T));
}
// row_rel(kidx(m)) split into a wave-uniform part (the row of the wave's
// first row set, in SGPRs) and the lane's row-set offset (a VGPR that does
// not depend on m): the HBM row addresses become one scalar multiply-add per
// row plus a per-lane byte offset computed once (PassArgs::voff32).
template <int T, bool LB> __device__ __forceinline__ uint32_t lane_rows(const Thr& c, const PassArgs& a) {
    const uint32_t hs = c.s - c.w * Geo<T>::HWS;  // row set within the wave
    return (LB ? hs : hs << Geo<T>::R) << a.lo;
}
// (the wave's row of row register 0, read into SGPRs once per item: a
// readfirstlane inside the per-row branches would be repeated per row)
template <int T, bool LB> struct WaveRows {
    uint32_t base, lo;
    __device__ __forceinline__ WaveRows(const Thr& c, const PassArgs& a) : lo(a.lo) {
        const uint32_t sw = uni(c.w) * Geo<T>::HWS;
        base = uni(c.b_low + (c.b_high << (a.lo + T)) + ((LB ? sw : sw << Geo<T>::R) << a.lo));
    }
    __device__ __forceinline__ uint32_t operator()(int m) const {
        return base + ((LB ? (uint32_t)m << Geo<T>::SHB : (uint32_t)m) << lo);
    }
};
// A wave-uniform row base address, pinned to SGPRs so that the compiler
// adds the lane offset in the load / store itself (SGPR base + VGPR offset)
// instead of folding the row product into a per-lane 64-bit multiply-add.
typedef __attribute__((address_space(1))) uint8_t gbyte;
typedef __attribute__((address_space(1))) uint32_t gu32;
__device__ __forceinline__ gbyte* sgpr_ptr(const uint8_t* p) {
    const uint64_t v = (uint64_t)p;
    const uint32_t lo = uni((uint32_t)v), hi = uni((uint32_t)(v >> 32));
    return (gbyte*)(((uint64_t)hi << 32) | lo);
}
// r = ur + lr < lim for a uniform ur and a per-lane lr (one vector compare)
__device__ __forceinline__ bool row_below(uint32_t ur, uint32_t lr, uint32_t lim) {
    return ur < lim && lr < lim - ur;
}

// Priority schedule: a wave lowers its issue priority (s_setprio 3 -> 0) as
// its item progresses, so that waves that are behind win the arbitration.
// Hardware age order alone lets the oldest workgroup of a CU run ahead and
// leaves a low-occupancy one-workgroup tail (scripts/stamps.py: 10-16 us
// spread of workgroup end times).  Measured (bench, 2 runs each): this
// schedule 620 / 614 GiB/s; on the two-direction passes only 611 / 611; a
// later schedule 607; none 595 / 594.
// At point `at` of an item (0 staged, 1 first layout-A layers done,
// 2 first direction done, 3 layout-B FFT done, 4 last switch done, 5 stores).
// (A static pair schedule -- slots 0-1 at priority 3 for the whole item,
// slots 2-3 at 0 -- measured no better on the T = 7 passes and 3.5 us worse
// on the T = 8 ones, same-box A/B x 3, round 4.  Round 6, two workgroups per
// CU everywhere: without the schedule, or with a static bias for the younger
// workgroup, ENC_MID runs 2-3 us slower: profiles/r06_prio_schedules_rejected.txt.)
template <int at> __device__ __forceinline__ void prio() {
    constexpr int v[6] = {3, 2, -1, 1, -1, 0};
    if constexpr (v[at] >= 0) __builtin_amdgcn_s_setprio(v[at]);
}

// Row stores / loads at an address that includes the lane's offset (global
// address space from the SGPR base on: base + 32-bit lane offset selects the
// SGPR-base form of global_load / global_store).
template <bool NT> __device__ __forceinline__ void st_ptr(gbyte* p, bool ok, uint32_t L, uint32_t H) {
    if (ok) {
        gu32* g = (gu32*)p;
        if constexpr (NT) {
            __builtin_nontemporal_store(L, g);
            __builtin_nontemporal_store(H, g + 8);
        } else {
            g[0] = L;
            g[8] = H;
        }
    }
}
// Branch-free: a row that is not read is read from the zero page instead
// (PassArgs::zero), so the item's loads are a fixed sequence and the
// compiler's vmcnt waits (for the staged tables and erasure logs, issued
// before the rows) count exactly instead of waiting for every row.
__device__ __forceinline__ void ld_sel(const PassArgs& a, const gbyte* p, bool ok, uint32_t offL, uint32_t& L,
                                       uint32_t& H) {
    // (offL & 0x7FFF: the zero page is RS16_ZERO_BYTES = 64 KiB, rows can be wider)
    const gu32* g = (const gu32*)(ok ? p : (const gbyte*)a.zero + (offL & 0x7FFFu));
    L = g[0];
    H = g[8];
}
// Per-lane byte offset of the lane's quad in the row lane_rows below the
// wave's row: 32 bits (global_load/store with an SGPR base) when the launch
// allows it (PassArgs::voff32), else 64 bits.
template <bool V32> struct LaneOff {
    uint32_t v;
    __device__ __forceinline__ LaneOff(uint32_t lr, uint64_t S, uint32_t offL) : v(lr * (uint32_t)S + offL) {}
    template <class B> __device__ __forceinline__ B* at(B* base) const { return base + v; }
};
template <> struct LaneOff<false> {
    uint64_t v;
    __device__ __forceinline__ LaneOff(uint32_t lr, uint64_t S, uint32_t offL) : v((uint64_t)lr * S + offL) {}
    template <class B> __device__ __forceinline__ B* at(B* base) const { return base + v; }
};

// ---------------------------------------------------------------------------
// Full-item fast path.  The general row addressing above decides per row and
// per lane: a 64-bit product row x stride, a compare against the row limit,
// a select of the zero page (which turns the address into a VGPR pair) or an
// exec branch around the store.  In a launch whose lanes all hold a quad
// (PassArgs::full_lanes) a wave whose rows all lie below the row limit needs
// none of that: one base address per array (one product), the rows of
// consecutive row registers a launch-constant stride apart (PassArgs::rs_in,
// rs_seg, rs_out), every load and store in SGPR base + 32-bit lane offset
// form.  One wave-uniform test per item picks the path; partial tiles and
// slabs, absent rows, in_rows_mask and 64-bit lane offsets take the general
// one.  The plain and encoder-gather loads and the plain and recovery stores
// have it (T > 4: the passes of stripes above 2048 rows); DEC_MID's zero rows
// and pruned stores, the decoder's gathers and the reveal stores do not.
// ---------------------------------------------------------------------------
template <int P, int T> struct FastRows {
    using PT = ProgTraits<P>;
    static constexpr bool LOAD = T > 4 && P != DEC_MID && (PT::LOAD == LD_PLAIN || PT::LOAD == LD_GATHER_ENC);
    static constexpr bool STORE = T > 4 && P != DEC_MID && (PT::STORE == ST_PLAIN || PT::STORE == ST_RECOVERY);
};
// one past the last row of the wave (rows grow with the tile row k)
template <int T, bool LB> __device__ __forceinline__ uint32_t wave_rows_end(const WaveRows<T, LB>& wr) {
    using G = Geo<T>;
    constexpr uint32_t kmax = LB ? (G::HWS - 1) + ((uint32_t)(G::NR - 1) << G::SHB) : ((uint32_t)G::HWS << G::R) - 1;
    return wr.base + (kmax << wr.lo) + 1;
}
// The row requests of the full-item form: row register m of the wave at base
// + m x row stride, every load SGPR base + 32-bit lane offset.  `rows` false
// (wave-uniform): 2 NR dwords of the zero page instead (row stride 0, the
// lane's offset within the page as in ld_sel).  CLAMP: a lane without a quad
// (partial last slab) requests the first quad of its slab -- a lane is a quad
// column, nothing of it reaches another lane, and its stores are masked.
template <int P, int T, bool CLAMP>
__device__ __forceinline__ void request_rows(const PassArgs& a, const Thr& c, bool rows, uint32_t (&L)[Geo<T>::NR],
                                             uint32_t (&H)[Geo<T>::NR]) {
    constexpr bool START_B = !ProgTraits<P>::IFFT;
    constexpr bool GATHER = ProgTraits<P>::LOAD == LD_GATHER_ENC;
    const WaveRows<T, START_B> wr(c, a);
    const uint64_t S = GATHER ? a.S_seg : a.S_in, rs = rows ? (GATHER ? a.rs_seg : a.rs_in) : 0;
    // (offL = (Qg >> 3) * 64 + (Qg & 7) * 4 of the lane's quad Qg = slab * Q + qt, Q a multiple of 8)
    const uint32_t offL = CLAMP && !c.active ? ((c.offL >> 6) - (c.qt >> 3)) * 64 : c.offL;
    const uint32_t voff = rows ? lane_rows<T, START_B>(c, a) * (uint32_t)S + offL : (c.offL & 0x7FFFu);
    uint64_t p = rows ? (uint64_t)(GATHER ? a.seg_a : a.in) + (uint64_t)wr.base * S : (uint64_t)a.zero;
#pragma unroll
    for (int m = 0; m < Geo<T>::NR; m++) {
        const gu32* g = (const gu32*)(sgpr_ptr((const uint8_t*)p) + voff);
        L[m] = g[0];
        H[m] = g[8];
        p += rs;
    }
    // (a block of its own: without the marker the compiler sinks the loads of
    // this and the general paths into one shared block behind them, which
    // takes its addresses as 64-bit VGPR pairs from whichever path ran)
    asm volatile("; full-item rows requested");
}
template <int P, int T>
__device__ __forceinline__ bool load_rows_fast(const PassArgs& a, const Thr& c, uint32_t (&L)[Geo<T>::NR],
                                               uint32_t (&H)[Geo<T>::NR]) {
    constexpr bool START_B = !ProgTraits<P>::IFFT;
    constexpr bool GATHER = ProgTraits<P>::LOAD == LD_GATHER_ENC;
    const WaveRows<T, START_B> wr(c, a);
    if (!a.full_lanes || (GATHER && wave_rows_end<T, START_B>(wr) > a.a_count)) return false;
    // (request_rows<P, T, false>(a, c, true, L, H) written out: through the
    // call, 20 kernels outside the wave-staged ones compile to other code)
    const uint64_t S = GATHER ? a.S_seg : a.S_in, rs = GATHER ? a.rs_seg : a.rs_in;
    const uint32_t voff = lane_rows<T, START_B>(c, a) * (uint32_t)S + c.offL;
    uint64_t p = (uint64_t)(GATHER ? a.seg_a : a.in) + (uint64_t)wr.base * S;
#pragma unroll
    for (int m = 0; m < Geo<T>::NR; m++) {
        const gu32* g = (const gu32*)(sgpr_ptr((const uint8_t*)p) + voff);
        L[m] = g[0];
        H[m] = g[8];
        p += rs;
    }
    asm volatile("; full-item rows requested");  // (a block of its own, see request_rows)
    return true;
}
// How a wave of a wave-staged pass (pass_kernel) gets its rows.  Those passes
// issue request_rows on every path, so the form covers what it can: DIRECT,
// the rows themselves -- any launch with 32-bit lane offsets and no row mask,
// partial slabs included (CLAMP), when the wave's rows lie below the gather's
// row limit; ZERO, a gather wave wholly at or above the limit: the zero page,
// which is its data; GENERAL, the rest (a wave that straddles the limit,
// 64-bit lane offsets, in_rows_mask): the zero page, then load_rows on top.
enum RowsMode { ROWS_DIRECT = 0, ROWS_ZERO, ROWS_GENERAL };
template <int P, int T>
__device__ __forceinline__ uint32_t wave_rows_mode(const PassArgs& a, const Thr& c) {
    constexpr bool START_B = !ProgTraits<P>::IFFT;
    constexpr bool GATHER = ProgTraits<P>::LOAD == LD_GATHER_ENC;
    const WaveRows<T, START_B> wr(c, a);
    const bool below = !GATHER || wave_rows_end<T, START_B>(wr) <= a.a_count;
    const bool above = GATHER && wr.base >= a.a_count;  // (the wave's lowest row)
    const bool direct = (a.voff32 != 0) & (a.in_rows_mask == 0) & below;
    return direct ? ROWS_DIRECT : (above ? ROWS_ZERO : ROWS_GENERAL);
}
// ---------------------------------------------------------------------------
// Late rows (pass_kernel_late).  In a launch none of whose waves can be
// ROWS_GENERAL (launch_pass decides: PassConsts::late_rows) the row requests
// need no guarded block, so they can stand anywhere in straight-line code: the
// wave requests the first D pairs of its first layer ahead of the table
// commit (prologue) and pair q + D right before butterfly q of that layer
// (operator(), GroupLoop's PRE hook).  The VALU starts on pair 0 once D pairs
// are accepted by the memory pipeline instead of all NR / 2 -- at D < NR / 2,
// which is a diagnostic build (RS16_LATE_DEPTH, rs16_diag.hpp); the shipped
// depth requests every pair in the prologue (LateDepth on why).
// Pair q of the first layer: layout A (IFFT layer 0) rows (2q, 2q + 1), layout
// B (ENC_LAST: the FFT's top register bit) rows (q, q + NR / 2).
// Addressing as request_rows: row register m at the wave's SGPR base + m x row
// stride (launch_pass: 15 strides fit 32 bits) + one 32-bit lane offset;
// a gather wave at or above the row limit reads the zero page with stride 0.
// ---------------------------------------------------------------------------
template <int P> struct LateDepth {
    // Pairs requested ahead of the table commit.  Shipped: all 8 in every
    // program, i.e. no request inside the layer -- what the variant keeps is
    // the straight-line prologue (no general block) and ENC_LAST's pair
    // order.  Depths 1 / 2 / 4 bring wave 0's first butterfly ~1 us forward on
    // every box but win or lose the step by box (2: +6 % on one, -1.5 % on
    // another; 4 in ENC_LAST slower than 8 everywhere); 8 was faster than the
    // parent in every pair on every box: profiles/r11_late_rows_depth.txt.
    static constexpr int SHIPPED = 8;
    static constexpr int value = RS16_LATE_DEPTH > 0 ? RS16_LATE_DEPTH : SHIPPED;
};
// PAIR (paired rows): the rows are in the paired form of the work buffer Z
// (quad Qg of a row at bytes [8 Qg, 8 Qg + 8), low dword
// first) and a request is one 8-byte load into (L[m], H[m]).  Paired launches
// are full_lanes launches of the plain loads (launch_pass): every lane has a
// quad and no wave reads the zero page.
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) u32x2 gu32x2;
typedef __attribute__((address_space(1))) uint64_t gu64;
// byte offset of the lane's quad in a paired row, from its offset offL =
// (Qg >> 3) * 64 + (Qg & 7) * 4 in the reference form: 8 Qg
__device__ __forceinline__ uint32_t pair_off(uint32_t offL) { return offL + (offL & 28u); }
template <int P, int T, bool PAIR = false> struct LateRows {
    using G = Geo<T>;
    static constexpr bool START_B = !ProgTraits<P>::IFFT;
    static constexpr bool GATHER = ProgTraits<P>::LOAD == LD_GATHER_ENC;
    static constexpr int RB = START_B ? G::R - 1 : 0;  // the first layer's register bit
    static constexpr int NP = G::NR / 2;               // its pairs
    static constexpr int D = LateDepth<P>::value < NP ? LateDepth<P>::value : NP;
    static_assert(D >= 1 && G::R == 4, "late rows: 16-row sets");
    static_assert(!PAIR || !GATHER, "paired rows: the work buffer, not the caller's shards");
    uint64_t p;         // the wave's row register 0 (uniform)
    uint32_t rs, voff;  // stride of consecutive row registers (uniform), the lane's offset
    __device__ __forceinline__ LateRows(const PassArgs& a, const Thr& c) {
        const WaveRows<T, START_B> wr(c, a);
        // (no wave of the launch straddles the limit: below it or the zero page)
        const bool rows = !GATHER || wr.base < a.a_count;
        const uint64_t S = GATHER ? a.S_seg : a.S_in;
        if constexpr (PAIR) {
            rs = (uint32_t)a.rs_in;
            voff = lane_rows<T, START_B>(c, a) * (uint32_t)S + pair_off(c.offL);
            p = (uint64_t)a.in + (uint64_t)wr.base * S;
            return;
        }
        // (a lane without a quad requests the first quad of its slab: request_rows' CLAMP)
        const uint32_t offL = !c.active ? ((c.offL >> 6) - (c.qt >> 3)) * 64 : c.offL;
        rs = rows ? (uint32_t)(GATHER ? a.rs_seg : a.rs_in) : 0u;
        voff = rows ? lane_rows<T, START_B>(c, a) * (uint32_t)S + offL : (c.offL & 0x7FFFu);
        p = rows ? (uint64_t)(GATHER ? a.seg_a : a.in) + (uint64_t)wr.base * S : (uint64_t)a.zero;
    }
    __device__ __forceinline__ void pair(uint32_t (&L)[G::NR], uint32_t (&H)[G::NR], int q) const {
        const int m = ((q >> RB) << (RB + 1)) + (q & ((1 << RB) - 1));
        // (the lane offset as a 32-bit value of the block the request stands
        // in: extended to 64 bits in the prologue's block, it reaches the
        // layer code as a VGPR pair and the loads lose their SGPR-base form)
        uint32_t v = voff;
        asm volatile("" : "+v"(v));
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int mi = m + (i << RB);
            if constexpr (PAIR) {
                const u32x2 x = *(const gu32x2*)(sgpr_ptr((const uint8_t*)(p + (uint32_t)mi * rs)) + v);
                L[mi] = x.x;
                H[mi] = x.y;
                continue;
            }
            const gu32* g = (const gu32*)(sgpr_ptr((const uint8_t*)(p + (uint32_t)mi * rs)) + v);
            L[mi] = g[0];
            H[mi] = g[8];
        }
    }
    __device__ __forceinline__ void prologue(uint32_t (&L)[G::NR], uint32_t (&H)[G::NR]) const {
#pragma unroll
        for (int q = 0; q < D; q++) pair(L, H, q);
        asm volatile("; late rows: prologue requested");
    }
    // before butterfly q of the first layer: pair q + D, fenced so that the
    // scheduler leaves the request between butterflies q - 1 and q
    __device__ __forceinline__ void operator()(uint32_t (&L)[G::NR], uint32_t (&H)[G::NR], int q) const {
        if (q + D < NP) {
            __builtin_amdgcn_sched_barrier(0);
            pair(L, H, q + D);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
};

// The stores' side: row register m at base + m x rs_out (launch_pass: the
// offsets of all row registers fit 32 bits when full_lanes is set), in any
// order -- the early stores come from inside the last layer block.
// PAIR: the rows go out in the paired form, one 8-byte store per row (a
// paired launch is a full_lanes launch of the plain stores: `on` in every wave).
template <int P, int T, bool PAIR = false> struct FastStore {
    static_assert(!PAIR || (FastRows<P, T>::STORE && ProgTraits<P>::STORE == ST_PLAIN),
                  "paired rows: the plain stores' full-item form");
    static constexpr bool END_B = !ProgTraits<P>::FFT && T > 4;
    const PassArgs& a;
    const Thr& cs;
    bool on;
    uint64_t p;
    __device__ __forceinline__ FastStore(const PassArgs& a_, const Thr& cs_) : a(a_), cs(cs_), on(false), p(0) {
        if constexpr (FastRows<P, T>::STORE) {
            const WaveRows<T, END_B> wr(cs, a);
            on = a.full_lanes &&
                 (ProgTraits<P>::STORE != ST_RECOVERY || wave_rows_end<T, END_B>(wr) <= a.out_rows);
            p = (uint64_t)a.out + (uint64_t)wr.base * a.S_out;
        }
    }
    __device__ __forceinline__ void row(int m, uint32_t L, uint32_t H) const {
        // (the lane offset from cs.offL at each store, as the general path
        // forms it: kept across the early stores' layer block it costs a VGPR)
        if constexpr (PAIR) {
            const uint32_t voff = lane_rows<T, END_B>(cs, a) * (uint32_t)a.S_out + pair_off(cs.offL);
            gu64* g = (gu64*)(sgpr_ptr((const uint8_t*)(p + (uint32_t)m * (uint32_t)a.rs_out)) + voff);
            // (as one 64-bit value: built as the vector {L, H}, the kernels
            // keep their row registers in scratch, 72 bytes per lane)
            const uint64_t x = ((uint64_t)H << 32) | L;
            if constexpr (ProgTraits<P>::ST_NT) __builtin_nontemporal_store(x, g);
            else *g = x;
            return;
        }
        const uint32_t voff = lane_rows<T, END_B>(cs, a) * (uint32_t)a.S_out + cs.offL;
        gu32* g = (gu32*)(sgpr_ptr((const uint8_t*)(p + (uint32_t)m * (uint32_t)a.rs_out)) + voff);
        if constexpr (ProgTraits<P>::ST_NT) {
            __builtin_nontemporal_store(L, g);
            __builtin_nontemporal_store(H, g + 8);
        } else {
            g[0] = L;
            g[8] = H;
        }
    }
};

// ---------------------------------------------------------------------------
// Table staging.  N tables of 5 x 16 B, table i taken from mul_tab entry
// entry(i), spread over the workgroup's threads.  Split into issue (global
// loads into registers, issued next to the tile's own loads so that their
// latencies overlap) and commit (ds_write, before the barrier that
// publishes the tables).
// ---------------------------------------------------------------------------
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
template <int T, int N> struct Stager {
    static constexpr int PER = (N * 5 + Geo<T>::THREADS - 1) / Geo<T>::THREADS;
    u32x4 v[PER > 0 ? PER : 1];

    // table i = entry(i) of `tabs` (TAB_DWORDS dwords per entry)
    template <class F> __device__ __forceinline__ void issue(const uint32_t* tabs, F entry) {
        const u32x4* tab = (const u32x4*)tabs;
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int idx = (int)threadIdx.x + i * Geo<T>::THREADS;
            if (idx < N * 5) v[i] = tab[(size_t)entry(idx / 5) * (TAB_DWORDS / 4) + idx % 5];
        }
    }
    __device__ __forceinline__ void commit(uint4* dst) const {
        u32x4* d = (u32x4*)dst;
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int idx = (int)threadIdx.x + i * Geo<T>::THREADS;
            if (idx < N * 5) d[idx] = v[i];
        }
    }
};

// Wave-private staging (the encoder-family passes at T >= 7, the cut of the
// slot-priority code in pass_kernel): no workgroup barrier stands between a
// wave's row loads and its first layers.  The tables of the first layer block
// are requested and committed by the wave that reads them -- in layout A the
// 2^R - 1 tables of each of its own row sets (group_table: t = offset(kb) +
// (s << (R-1-kb)) + gi), in layout B (ENC_LAST) the block's shared tables,
// which every wave writes with the same values -- and ordered by
// wave_lds_publish().  Every other table is committed by the thread that
// requested it without a barrier of its own: its first reader stands behind
// the barriers of the first layout switch.
template <int P, int T> struct WaveStaged {
    static constexpr bool value = (P == ENC_FIRST || P == ENC_MID || P == ENC_LAST) && T >= 7;
};
// N tables per wave, spread over its 64 lanes: table i = entry(i) of `tabs`,
// committed to table slot slot(i) of dst.
template <int N> struct WaveStager {
    static constexpr int PER = (N * 5 + 63) / 64;
    u32x4 v[PER > 0 ? PER : 1];
    template <class F> __device__ __forceinline__ void issue(const uint32_t* tabs, uint32_t lane, F entry) {
        const u32x4* tab = (const u32x4*)tabs;
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int idx = (int)lane + i * 64;
            if (idx < N * 5) v[i] = tab[(size_t)entry(idx / 5) * (TAB_DWORDS / 4) + idx % 5];
        }
    }
    template <class F> __device__ __forceinline__ void commit(uint4* dst, uint32_t lane, F slot) const {
        u32x4* d = (u32x4*)dst;
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int idx = (int)lane + i * 64;
            if (idx < N * 5) d[slot(idx / 5) * 5 + idx % 5] = v[i];
        }
    }
};
// What a wave's lanes wrote to LDS is visible to the wave's other lanes: the
// LDS executes a wave's instructions in order, the wait retires the writes,
// and the wave-scope fences keep the compiler from moving a lane's table
// reads above its writes (to it they are other addresses).
__device__ __forceinline__ void wave_lds_publish() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0) only
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Twiddle of tile group t (t in [0, 2^T - 1)) as an index of skew_tab (the
// v_perm table of every skew entry, so staging is one load deep): layer kb with
// offset(kb) = 2^T - 2^(T-kb) <= t < offset(kb+1), group j = t - offset(kb)
// covering tile rows k with k >> (kb+1) == j.
template <int T> struct TwiddleEntry {
    const PassArgs& a;
    const Thr& c;
    int t_begin;
    uint32_t skew;
    __device__ __forceinline__ uint32_t operator()(int i) const {
        const int t = t_begin + i;
        // kb = T - 1 - floor(log2(2^T - 1 - t)) (closed form, so the staging
        // loads of a thread issue back to back)
        const int kb = T - 32 + __clz((uint32_t)((1 << T) - 1 - t));
        const uint32_t j = (uint32_t)(t - ((1 << T) - (1 << (T - kb))));
        const uint32_t d = 1u << (a.lo + kb);
        const uint32_t g = (c.b_high << (a.lo + T)) + (j << (kb + 1 + a.lo));
        return g + d + skew - 1;
    }
};

// Decoder rows: pass row r is decode work row r + row_base_in (gather side)
// or r + row_base_out (reveal side) -- non-zero in the half-transform decode.
// Rows [0, a_count) are segment A, [chunk, chunk + b_count) segment B, anything
// else an absent (zero) row; which rows were received: the bitmap a.rbits.
// The erasure log e[r] of a row comes from the tile's LDS copy when the pass
// finished eval_poly itself (el = the tile's 2^T logs), else from HBM.
// "MULTIPLY SHARDS" (rate_high.rs:203-228 / rate_low.rs:203-228: received row
// r x e[r], absent rows x 0) is staged by TileStage::gather.
//
// REVEAL ERASURES (rate_high.rs:236-242 / rate_low.rs:236-242): lost
// original row r -> work[r] * (GF_MODULUS - e[r]).
// (RULE: the repair's programs reveal the lost rows of both segments, the
// selective decode's the lost originals of the read set: row_wanted)
template <int T, int RULE = ROWS_LOST> struct RevealEntry {
    const PassArgs& a;
    const Thr& c;
    const uint32_t* el;
    __device__ __forceinline__ uint32_t operator()(int k) const {
        const uint32_t r = row_rel<T>(c, a, (uint32_t)k) + a.row_base_out;
        return row_wanted<RULE>(a, r) ? GF_MODULUS - (el ? el[k] : a.elog[r]) : ZERO_ENTRY;
    }
};

// Layers for k-bits [KB0, KB1) held in registers of layout LB, as a
// compile-time sequence of twiddle groups (step s, index gi).
// No per-group action (GroupLoop's default).
struct NoFin {
    template <class X> __device__ __forceinline__ void operator()(const X&, const X&, int) const {}
};
// No action before a butterfly of the block's first layer (GroupLoop's
// default; the late-rows kernels pass LateRows).
struct NoPre {
    template <class X> __device__ __forceinline__ void operator()(X&, X&, int) const {}
};

// Breadth-first (layer by layer), except the last FFT block in layout A of
// all 4 register bits: there the groups run depth-first in pre-order (a
// group, then its two halves), so rows m, m + 1 are final right after their
// layer-0 group and can be stored there (EarlyStore).
template <int T, bool LB, int KB0, int KB1, bool FFT> struct LayerSeq {
    static constexpr int SH = LB ? Geo<T>::SHB : 0;
    static constexpr int NR = Geo<T>::NR;
    static constexpr bool DF = FFT && !LB && KB0 == 0 && KB1 == Geo<T>::R && NR >= 8;
    // pre-order of the group tree (node (kb, gi), children (kb-1, 2gi) and
    // (kb-1, 2gi+1)), (kb, gi) packed as kb * 16 + gi; radix 16:
    // (3,0) (2,0) (1,0) (0,0) (0,1) (1,1) (0,2) (0,3) (2,1) (1,2) ...
    static constexpr int df_at(int g) {
        int skb[16] = {}, sgi[16] = {};
        int sp = 0, n = 0;
        skb[sp] = KB1 - 1, sgi[sp] = 0, sp++;
        while (sp > 0) {
            sp--;
            const int kb = skb[sp], gi = sgi[sp];
            if (n++ == g) return kb * 16 + gi;
            if (kb > 0) {
                skb[sp] = kb - 1, sgi[sp] = 2 * gi + 1, sp++;
                skb[sp] = kb - 1, sgi[sp] = 2 * gi, sp++;
            }
        }
        return 0;
    }
    static constexpr int kb_of(int s) { return FFT ? KB1 - 1 - s : KB0 + s; }
    static constexpr int groups_of(int s) { return NR >> (kb_of(s) - SH + 1); }
    static constexpr int total() {
        int n = 0;
        for (int s = 0; s < KB1 - KB0; s++) n += groups_of(s);
        return n;
    }
    static constexpr int step_of(int g) {
        if (DF) return KB1 - 1 - df_at(g) / 16;
        int s = 0;
        while (g >= groups_of(s)) g -= groups_of(s), s++;
        return s;
    }
    static constexpr int index_of(int g) {
        if (DF) return df_at(g) % 16;
        int s = 0;
        while (g >= groups_of(s)) g -= groups_of(s), s++;
        return g;
    }
};

// Where group G's table lives: tile group id t = offset(kb) + j, with
// j = k >> (kb+1) of the group's rows (per row set in layout A, uniform in
// layout B); in two-direction kernels the second direction's tables are in
// tab2.
template <int T, bool LB, int KB0, int KB1, bool FFT, int G, bool IN_TAB2>
__device__ __forceinline__ const uint4* group_table(const Thr& c, const uint4* tab1, const uint4* tab2) {
    using S = LayerSeq<T, LB, KB0, KB1, FFT>;
    constexpr int s = S::step_of(G), gi = S::index_of(G);
    constexpr int kb = S::kb_of(s);
    constexpr int off = (1 << T) - (1 << (T - kb));
    // layout A: k = (s << R) + m  ->  j = (s << (R-1-kb)) + gi ; layout B: j = gi
    const uint32_t j = LB ? (uint32_t)gi : (c.s << (Geo<T>::R - 1 - kb)) + gi;
    const uint32_t t = off + j;
    // tab2 starts at the first layout-B table when the layout-A ones are
    // restaged into tab1 (Smem::RESTAGE); T <= 4 has no layout B (TSPLIT = 0)
    constexpr uint32_t base2 = T > 4 ? Geo<T>::TSPLIT : 0;
    return IN_TAB2 ? tab2 + (t - base2) * 5 : tab1 + t * 5;
}

// Empty volatile asm that "redefines" the data registers: ALU work cannot
// cross it, so group boundaries are real scheduling boundaries.
template <int NR> __device__ __forceinline__ void pin_rows(uint32_t (&L)[NR], uint32_t (&H)[NR]) {
    if constexpr (NR >= 4) {
#pragma unroll
        for (int i = 0; i < NR; i += 4)
            asm volatile("" : "+v"(L[i]), "+v"(L[i + 1]), "+v"(L[i + 2]), "+v"(L[i + 3]), "+v"(H[i]), "+v"(H[i + 1]),
                         "+v"(H[i + 2]), "+v"(H[i + 3]));
    } else {
#pragma unroll
        for (int i = 0; i < NR; i++) asm volatile("" : "+v"(L[i]), "+v"(H[i]));
    }
}

// PRUNE (layout-B groups of DEC_MID; the conditions are uniform):
//   PR_OUT  FFT: a group whose rows [gi << (kb+1), (gi+1) << (kb+1)) miss
//           [need_lo, need_hi) feeds no consumed output and is skipped;
//   PR_ZERO IFFT: a group whose rows are all zero on input stays zero and is
//           skipped.  zmask bit j = tile rows [16j, 16j+16) are all zero.
enum { PR_NONE = 0, PR_OUT, PR_ZERO };
// Narrow-twiddle variants of the two-direction pass kernels (twiddle_narrow,
// rs16_internal.hpp): from which layer kb of the pass on each direction
// multiplies by subfield constants only.  A compile-time choice: the
// unrolled layer code has no branch per group for it.
//   0  none (the 12-lookup multiply everywhere)
//   1  every layer of both directions (stripes of up to 2^14 rows; DEC_MID
//      of the 65536-row general decode)
//   2  all but the IFFT's layer 0 (the encoder's middle pass of a 2^15-row
//      stripe: IFFT at skew 2^15, FFT at skew 0)
//   3  all but the FFT's layer 0 (the identity decode's middle pass: the
//      same with the directions swapped)
// (NARROW_VARIANTS = 4 of them, rs16_pass_common.hpp)
template <int NV> struct NarrowVar {
    static constexpr int NONE = 99;
    static constexpr int IFFT_FROM = NV == 0 ? NONE : (NV == 2 ? 1 : 0);
    static constexpr int FFT_FROM = NV == 0 ? NONE : (NV == 3 ? 1 : 0);
};

// The form of the rows in a block's layers (GroupLoop's TW): shard
// coordinates, or tower form, there with the wide multiplies by 12 lookups
// or by three byte maps.
enum { TW_NONE = 0, TW_ROWS, TW_WIDE3 };
// A wide multiply on a tower table: by three byte maps, or with 12 lookups.
template <bool WIDE3> __device__ __forceinline__ void mul_xor_tower_sel(uint32_t& xL, uint32_t& xH, const MulSel& y,
                                                                      const uint32_t (&t)[20]) {
    if constexpr (WIDE3) mul_xor_tower_wide_sel(xL, xH, y, t);
    else mul_xor_sel<false>(xL, xH, y, t);
}

// NK: the direction's first narrow layer -- the layers kb >= NK multiply
// with mul_xor_narrow (every twiddle of theirs in this launch is a subfield
// constant: launch_pass picks the kernel variant from first_narrow_layer).
// PRE (the late-rows kernels, LateRows): pre(L, H, q) runs before butterfly q
// of the block's first layer -- the q-th pair of that layer, counted over its
// groups -- and requests the rows of a later pair.
// TW (the tower kernels, pass_kernel_late_tower): the rows are in tower form
// in every layer, and every twiddle table is the tower one.  ENC_MID: its
// narrow layers with the 6-lookup multiply of one byte map, the wide layer of
// a narrow variant with the c1 = 1 form (mul_xor_tower_beta; launch_pass
// checks the layer's indices).  ENC_FIRST and ENC_LAST convert at the caller's
// rows: ENC_FIRST in its first layer (pre.tb: B's pools) -- y ^= x in shard
// coordinates, then the multiplicand y ahead of its low selectors, which it
// shares its high ones with, then x -- and ENC_LAST in its last (fin.tb), x
// after the multiply and y from the selectors the multiply took, ahead of y
// ^= x (conv is linear).  TW_WIDE3: they multiply by three byte maps in every
// layer (mul_xor_tower_wide), TW_ROWS: with 12 lookups on the same table.
template <int P, int T, int NK, bool LB, int KB0, int KB1, bool FFT, bool IN_TAB2, int PRUNE, int G, class FIN = NoFin,
          class PRE = NoPre, int TW = TW_NONE>
struct GroupLoop {
    static __device__ __forceinline__ void run(uint32_t (&L)[Geo<T>::NR], uint32_t (&H)[Geo<T>::NR], const Thr& c,
                                               const PassArgs& a, const uint4* tab1, const uint4* tab2,
                                               const uint32_t (&cur)[20], uint32_t zmask, const FIN& fin = FIN(),
                                               const PRE& pre = PRE()) {
        using S = LayerSeq<T, LB, KB0, KB1, FFT>;
        constexpr int s = S::step_of(G), gi = S::index_of(G);
        constexpr int kb = S::kb_of(s);
        constexpr int rb = kb - S::SH;
        constexpr bool more = G + 1 < S::total();
        constexpr bool NARROW = kb >= NK;
        uint32_t nxt[20];
        if constexpr (more)
            load_table_lds(nxt, group_table<T, LB, KB0, KB1, FFT, G + 1, IN_TAB2>(c, tab1, tab2));
        __builtin_amdgcn_sched_barrier(0);  // the prefetch is issued before this group's work
        bool need = true;
        if constexpr (PRUNE == PR_OUT)
            need = ((uint32_t)gi << (kb + 1)) < a.need_hi && ((uint32_t)(gi + 1) << (kb + 1)) > a.need_lo;
        if constexpr (PRUNE == PR_ZERO) {
            static_assert(LB && kb >= 4, "zero pruning works on 16-row blocks of layout B");
            constexpr int nb = 1 << (kb - 3);  // 16-row blocks covered by the group
            constexpr uint32_t all = (uint32_t)((1ull << nb) - 1);
            need = ((zmask >> (gi * nb)) & all) != all;
        }
        // Zero twiddle (the reference's GF_MODULUS sentinel: XOR only, no
        // multiply, engine_naive.rs:64,116).  The sentinel skew entries are
        // exactly the indices 2^i - 1 (rs16_tables.cpp checks this when it
        // builds the tables), which only the first group of a layer-B layer
        // can hit (index = b_high 2^(lo+T) + (2 gi + 1) 2^(lo+kb) + skew - 1):
        // ENC_MID's FFT half and the half decode's IFFT half (skew 0, b_high
        // 0) skip 15 of their 128 multiplies per row set this way.  Layout-B
        // twiddles are uniform, so this is a uniform branch.
        bool mul = true;
        if constexpr (LB && gi == 0 && ProgTraits<P>::IFFT && ProgTraits<P>::FFT) {
            const uint32_t idx = (c.b_high << (a.lo + T)) + (1u << (a.lo + kb)) + (FFT ? a.skew_fft : a.skew_ifft) - 1;
            mul = (idx & (idx + 1)) != 0;
        }
        if (need && mul) {
#pragma unroll
            for (int j = 0; j < (1 << rb); j++) {
                const int m = (gi << (rb + 1)) + j, m2 = m + (1 << rb);
                if constexpr (!std::is_same<PRE, NoPre>::value && s == 0) pre(L, H, (gi << rb) + j);
                if constexpr (TW && P == ENC_FIRST && !LB && kb == 0) {
                    L[m2] ^= L[m];
                    H[m2] ^= H[m];
                    MulSel y = high_selectors(H[m2]);
                    tower_conv_sel(L[m2], y, pre.tb);
                    y = low_selectors(L[m2], y);
                    tower_conv(L[m], H[m], pre.tb);
                    mul_xor_tower_sel<TW == TW_WIDE3>(L[m], H[m], y, cur);
                } else if constexpr (TW && P == ENC_LAST && !LB && kb == 0) {
                    const MulSel y = mul_selectors(L[m2], H[m2]);
                    mul_xor_tower_sel<TW == TW_WIDE3>(L[m], H[m], y, cur);
                    tower_conv_sel(L[m2], y, fin.tb);
                    tower_conv(L[m], H[m], fin.tb);
                    L[m2] ^= L[m];
                    H[m2] ^= H[m];
                } else if constexpr (TW && P != ENC_MID) {
                    if (FFT) {
                        mul_xor_tower_sel<TW == TW_WIDE3>(L[m], H[m], mul_selectors(L[m2], H[m2]), cur);
                        L[m2] ^= L[m];
                        H[m2] ^= H[m];
                    } else {
                        L[m2] ^= L[m];
                        H[m2] ^= H[m];
                        mul_xor_tower_sel<TW == TW_WIDE3>(L[m], H[m], mul_selectors(L[m2], H[m2]), cur);
                    }
                } else if constexpr (TW && P == ENC_MID && !NARROW && NK != NarrowVar<0>::NONE) {
                    if (FFT) {
                        mul_xor_tower_beta(L[m], H[m], L[m2], H[m2], cur);
                        L[m2] ^= L[m];
                        H[m2] ^= H[m];
                    } else {
                        L[m2] ^= L[m];
                        H[m2] ^= H[m];
                        mul_xor_tower_beta(L[m], H[m], L[m2], H[m2], cur);
                    }
                } else if constexpr (TW && P == ENC_MID && NARROW) {
                    if (FFT) {
                        mul_xor_tower_narrow(L[m], H[m], L[m2], H[m2], cur);
                        L[m2] ^= L[m];
                        H[m2] ^= H[m];
                    } else {
                        L[m2] ^= L[m];
                        H[m2] ^= H[m];
                        mul_xor_tower_narrow(L[m], H[m], L[m2], H[m2], cur);
                    }
                } else if (FFT) {
                    mul_xor_t<NARROW>(L[m], H[m], L[m2], H[m2], cur);
                    L[m2] ^= L[m];
                    H[m2] ^= H[m];
                } else {
                    L[m2] ^= L[m];
                    H[m2] ^= H[m];
                    mul_xor_t<NARROW>(L[m], H[m], L[m2], H[m2], cur);
                }
            }
        } else if (need) {
#pragma unroll
            for (int j = 0; j < (1 << rb); j++) {
                const int m = (gi << (rb + 1)) + j, m2 = m + (1 << rb);
                L[m2] ^= L[m];
                H[m2] ^= H[m];
            }
        }
        // (only the group's own rows: a row of a later group may still be
        // in flight from HBM, and pinning it here would make the compiler
        // wait for every row load before the second group of the first layer)
#pragma unroll
        for (int j = 0; j < (1 << rb); j++) {
            const int m = (gi << (rb + 1)) + j, m2 = m + (1 << rb);
            asm volatile("" : "+v"(L[m]), "+v"(H[m]), "+v"(L[m2]), "+v"(H[m2]));
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (S::DF && kb == 0) fin(L, H, gi << 1);  // rows 2 gi, 2 gi + 1 are final
        if constexpr (more)
            GroupLoop<P, T, NK, LB, KB0, KB1, FFT, IN_TAB2, PRUNE, G + 1, FIN, PRE, TW>::run(L, H, c, a, tab1, tab2,
                                                                                              nxt, zmask, fin, pre);
    }
};

// A uniform LDS address held in one VGPR.  Layout-B table addresses are
// compile-time constants; left to the compiler, each ds_read gets its own
// s_add + v_mov to build the address (150 VALU moves per ENC_MID item).
// Through one opaque VGPR base the constant part folds into the ds_read
// offset field instead.  (Against the plain pointer: profiles/r06_lds_vbase_ab.txt.)
__device__ __forceinline__ const uint4* lds_vgpr(const uint4* p) {
    uint32_t v = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint4*)p;
    asm volatile("" : "+v"(v));
    return (const uint4*)(const __attribute__((address_space(3))) uint4*)(uintptr_t)v;
}

// Apply the layers for k-bits [KB0, KB1) held in registers of layout LB.
template <int P, int T, int NK, bool LB, int KB0, int KB1, bool FFT, bool IN_TAB2, int PRUNE = PR_NONE,
          class FIN = NoFin, class PRE = NoPre, int TW = TW_NONE>
__device__ __forceinline__ void layers(uint32_t (&L)[Geo<T>::NR], uint32_t (&H)[Geo<T>::NR], const Thr& c,
                                       const PassArgs& a, const uint4* tab1, const uint4* tab2,
                                       uint32_t zmask = 0, const FIN& fin = FIN(), const PRE& pre = PRE()) {
    if constexpr (KB1 > KB0) {
        if constexpr (LB) {
            if constexpr (IN_TAB2) tab2 = lds_vgpr(tab2);
            else tab1 = lds_vgpr(tab1);
        }
        uint32_t t0[20];
        load_table_lds(t0, group_table<T, LB, KB0, KB1, FFT, 0, IN_TAB2>(c, tab1, tab2));
        GroupLoop<P, T, NK, LB, KB0, KB1, FFT, IN_TAB2, PRUNE, 0, FIN, PRE, TW>::run(L, H, c, a, tab1, tab2, t0, zmask,
                                                                                     fin, pre);
    }
}

// LDS image of the data: row k, quad ql of the current round, as two planes
// (lo dwords, then hi dwords, PLANE dwords apart) so that a row's two dwords
// go through one ds_write2st64_b32 / ds_read2st64_b32 from independent
// registers (an interleaved uint2 image needs register pairs: v_mov copies).
template <int T, int QL> struct Img {
    static constexpr int PLANE = (1 << T) * QL;
    static __device__ __forceinline__ uint32_t* at(uint2* lds, const Thr& c, uint32_t k) {
        return (uint32_t*)lds + k * QL + c.ql;
    }
};

template <int NQR> __device__ __forceinline__ bool my_round(const Thr& c, int r) {
    return NQR == 1 || c.round == (uint32_t)r;
}

template <int T, int QL, bool LB>
__device__ __forceinline__ void put_rows(const uint32_t (&L)[Geo<T>::NR], const uint32_t (&H)[Geo<T>::NR],
                                         const Thr& c, uint2* lds) {
#pragma unroll
    for (int m = 0; m < Geo<T>::NR; m++) {
        uint32_t* p = Img<T, QL>::at(lds, c, kidx<T, LB>(c, m));
        p[0] = L[m];
        p[Img<T, QL>::PLANE] = H[m];
    }
}
template <int T, int QL, bool LB>
__device__ __forceinline__ void get_rows(uint32_t (&L)[Geo<T>::NR], uint32_t (&H)[Geo<T>::NR], const Thr& c,
                                         uint2* lds) {
#pragma unroll
    for (int m = 0; m < Geo<T>::NR; m++) {
        const uint32_t* p = Img<T, QL>::at(lds, c, kidx<T, LB>(c, m));
        L[m] = p[0];
        H[m] = p[Img<T, QL>::PLANE];
    }
}

// y[k] ^= XOR_{b < T, k_b = 0} x[k | 2^b]: the formal derivative restricted
// to the tile's row bits (Engine::formal_derivative, src/engine.rs:233-238,
// in closed form -- step i = (j & ~(2^b-1)) | 2^b XORs row j|2^b into row j,
// and that source row is never written before it is read).
// Terms of row bits held in registers come straight from registers: rows are
// updated in ascending m and a term's source row m | 2^b lies above m, so it
// is read before it is updated and y may alias x.  Terms of row-set bits
// differ between lanes: they are read from the LDS image of x
// unconditionally (for k_b = 1 the address is the row itself) and masked
// with a select, so all reads of a row issue back to back.
template <int T, int QL, bool LB>
__device__ __forceinline__ void fd_rows(uint32_t (&L)[Geo<T>::NR], uint32_t (&H)[Geo<T>::NR],
                                        const uint32_t (&SL)[Geo<T>::NR], const uint32_t (&SH)[Geo<T>::NR],
                                        const Thr& c, uint2* lds) {
    constexpr int R = Geo<T>::R, SHB = Geo<T>::SHB;
#pragma unroll
    for (int m = 0; m < Geo<T>::NR; m++) {
        const uint32_t k = kidx<T, LB>(c, m);
        uint32_t xl = L[m], xh = H[m];
#pragma unroll
        for (int b = 0; b < T; b++) {
            // is bit b of k a register (compile-time) bit?
            const bool reg_bit = LB ? (b >= SHB) : (b < R);
            if (reg_bit) {
                const int mb = LB ? b - SHB : b;
                if (!((m >> mb) & 1)) {
                    xl ^= SL[m | (1 << mb)];
                    xh ^= SH[m | (1 << mb)];
                }
            } else {
                // bit sb of the row set s: above the lane-half bit it is a bit
                // of the (uniform) wave index, and a term not taken is skipped
                constexpr int LOG_HWS = Geo<T>::HWS == 4 ? 2 : (Geo<T>::HWS == 2 ? 1 : 0);
                const int sb = LB ? b : b - R;
                if (sb >= LOG_HWS) {
                    if (!((c.w >> (sb - LOG_HWS)) & 1)) {
                        const uint32_t* p = Img<T, QL>::at(lds, c, k | (1u << b));
                        xl ^= p[0];
                        xh ^= p[Img<T, QL>::PLANE];
                    }
                } else {
                    const uint32_t* p = Img<T, QL>::at(lds, c, k | (1u << b));
                    const uint32_t vl = p[0], vh = p[Img<T, QL>::PLANE];
                    const bool take = !((k >> b) & 1);
                    xl ^= take ? vl : 0u;
                    xh ^= take ? vh : 0u;
                }
            }
        }
        L[m] = xl;
        H[m] = xh;
    }
}

// Layout switch through LDS, in rounds.  `mid` runs after the first barrier.
struct NoMid {
    __device__ __forceinline__ void operator()() const {}
};
// `post` runs in the thread's own round after its rows are read (the image
// of that round is still in place).
template <int T, int NQR, bool FROM_B, class MID = NoMid, class POST = NoMid>
__device__ __forceinline__ void exchange(uint32_t (&L)[Geo<T>::NR], uint32_t (&H)[Geo<T>::NR], const Thr& c,
                                         uint2* lds, MID mid = MID(), POST post = POST()) {
    constexpr int QL = Geo<T>::Q / NQR;
#pragma unroll
    for (int r = 0; r < NQR; r++) {
        if (my_round<NQR>(c, r)) put_rows<T, QL, FROM_B>(L, H, c, lds);
        __syncthreads();
        if (r == 0) mid();
        if (my_round<NQR>(c, r)) {
            get_rows<T, QL, !FROM_B>(L, H, c, lds);
            post();
        }
        __syncthreads();
    }
}

// DEC_MID's second layout switch when its consumed rows lie in the
// layout-B register rows [m0, m0 + ND) (fd_few): only those rows go through
// LDS -- every thread writes ND rows, the threads whose layout-A rows they
// are read them -- in one round with one barrier, instead of all 2^T rows
// in two rounds.  The other threads' rows are not consumed (the layout-A
// FFT layers skip them, the store masks them).
template <int T, int ND>
__device__ __forceinline__ void few_switch(uint32_t (&L)[Geo<T>::NR], uint32_t (&H)[Geo<T>::NR], const Thr& c,
                                           uint2* lds, uint32_t m0) {
    constexpr int Q = Geo<T>::Q, SHB = Geo<T>::SHB, R = Geo<T>::R, NR = Geo<T>::NR;
    constexpr uint32_t ROWS = (uint32_t)ND << SHB, PLANE = ROWS * Q;
    uint32_t* img = (uint32_t*)lds;
    const uint32_t base = m0 << SHB;
#pragma unroll
    for (int m = 0; m < NR; m++) {
        const uint32_t i = (uint32_t)m - m0;  // (uniform)
        if (i < (uint32_t)ND) {
            const uint32_t r = c.s + (i << SHB);  // layout B: k = s + (m << SHB)
            img[r * Q + c.qt] = L[m];
            img[PLANE + r * Q + c.qt] = H[m];
        }
    }
    __syncthreads();
    const uint32_t k0 = c.s << R;  // layout A: k = (s << R) + m
    if (k0 >= base && k0 < base + ROWS) {
#pragma unroll
        for (int m = 0; m < NR; m++) {
            const uint32_t r = k0 - base + (uint32_t)m;
            L[m] = img[r * Q + c.qt];
            H[m] = img[PLANE + r * Q + c.qt];
        }
    }
}

// DEC_MID's formal derivative split by row bits (the two-direction pass's
// layers: IFFT bits [0, R) in layout A, bits [R, T) in layout B, then the
// FFT back).  With w = the rows after the layout-A IFFT layers, z = M_B(w)
// after the layout-B ones, and F_B the layout-B FFT layers (F_B M_B = I:
// same twiddles, inverse butterflies), a term P_b (row k|2^b into row k,
// k_b = 0) of a bit b < R commutes with the butterflies of bits above b, so
//   F_B((I + sum_b P_b) z) = F_B((I + sum_{b >= R} P_b) z) + sum_{b < R} P_b w:
// the terms of the layout-B bits come from registers after the layout-B
// IFFT layers (fd_regs), those of the layout-A bits from the image of w that
// the first layout switch writes anyway (fd_image, read in the switch), and
// they are added to the FFT's rows after its layout-B layers.  No LDS round
// of its own, no barrier.  (DEC_LAST's y = u + L(z) is the same identity one
// pass up: tile_last_kernel.)
template <int T>
__device__ __forceinline__ void fd_regs(uint32_t (&L)[Geo<T>::NR], uint32_t (&H)[Geo<T>::NR]) {
    constexpr int R = Geo<T>::R, SHB = Geo<T>::SHB;
#pragma unroll
    for (int m = 0; m < Geo<T>::NR; m++) {
#pragma unroll
        for (int b = R; b < T; b++) {
            const int mb = b - SHB;  // layout B: k = s + (m << SHB)
            if (!((m >> mb) & 1)) {  // the source row m | 2^mb is updated later
                L[m] ^= L[m | (1 << mb)];
                H[m] ^= H[m | (1 << mb)];
            }
        }
    }
}
// XOR_{b < R, k_b = 0} w[k | 2^b] from the image of w (any layout: the image
// is indexed by tile row)
template <int T, int QL>
__device__ __forceinline__ void fd_image(uint32_t& dl, uint32_t& dh, const Thr& c, const uint2* lds, uint32_t k) {
    dl = dh = 0;
#pragma unroll
    for (int b = 0; b < Geo<T>::R; b++) {
        const uint32_t* p = Img<T, QL>::at((uint2*)lds, c, k | (1u << b));
        const uint32_t vl = p[0], vh = p[Img<T, QL>::PLANE];
        const bool take = !((k >> b) & 1);
        dl ^= take ? vl : 0u;
        dh ^= take ? vh : 0u;
    }
}

// y = x + (in-tile formal derivative part) of the rows in registers, where
// the LDS image is filled from (SL, SH) -- the rows themselves for the
// (I + H) step of DEC_MID, z for DEC_LAST's y = u + L(z).  In rounds; with
// T <= 4 every row bit is a register bit and no LDS is needed.
template <int T, int NQR, bool LB>
__device__ __forceinline__ void tile_fd(uint32_t (&L)[Geo<T>::NR], uint32_t (&H)[Geo<T>::NR],
                                        const uint32_t (&SL)[Geo<T>::NR], const uint32_t (&SH)[Geo<T>::NR],
                                        const Thr& c, uint2* lds) {
    constexpr int QL = Geo<T>::Q / NQR;
    if constexpr (T <= 4) {
        fd_rows<T, QL, LB>(L, H, SL, SH, c, lds);
    } else {
#pragma unroll
        for (int r = 0; r < NQR; r++) {
            if (my_round<NQR>(c, r)) put_rows<T, QL, LB>(SL, SH, c, lds);
            __syncthreads();
            if (my_round<NQR>(c, r)) fd_rows<T, QL, LB>(L, H, SL, SH, c, lds);
            __syncthreads();
        }
    }
}

// One item's rows in registers plus what the item's load learned.
template <int P, int T> struct ItemRegs {
    static constexpr int NR = Geo<T>::NR;
    static constexpr int NZ = ProgTraits<P>::LOAD == LD_DEC_LAST ? NR : 1;
    uint32_t L[NR], H[NR];
    uint32_t zl[NZ], zh[NZ];  // DEC_LAST: z rows for y = u + L(z)
    uint32_t zrow, zmask;     // DEC_MID zero rows (see below)
    bool ztile;               // DEC_LAST: z of this tile is zero (DEC_FIRST skipped it)
};

// Per-item coordinates of this thread: item -> (tile, slab).
__device__ __forceinline__ void set_item(Thr& c, const PassArgs& a, uint32_t item, uint32_t Q, uint32_t& tile,
                                         uint32_t& slab) {
    // One item per workgroup, XCD-aware: workgroups are dealt to the 8 XCDs
    // round-robin (XCD = block mod 8, speed only), so with a tile count that
    // is a multiple of 8 all slabs of a tile run on one XCD (they share the
    // tile's twiddle tables in its L2) and consecutive tiles go to different
    // XCDs (tiles of uneven work spread evenly).
    // (Both forms in one branch-free sequence, the quotient by the launch
    // constant nslab without a division (fast_div): a branch here would split
    // the kernel-argument loads into a round before it and one behind it.)
    const bool x8 = (a.ntiles & 7) == 0;
    const uint32_t i = x8 ? item >> 3 : item;
    const uint32_t q = fast_div(i, a.nslab_mul, a.nslab_one);
    slab = i - q * a.nslab;
    tile = x8 ? q * 8 + (item & 7) : q;
    const uint32_t Qg = slab * Q + c.qt;
    c.active = Qg < a.qrow;
    c.offL = (Qg >> 3) * 64 + (Qg & 7) * 4;
}

// The row loads of an item: row address = SGPR base of the
// wave's row (one scalar multiply-add per row) + the lane's offset.
template <int P, int T, bool V32>
__device__ __forceinline__ void load_rows(const PassArgs& a, const Thr& c, uint32_t tile, ItemRegs<P, T>& d) {
    using PT = ProgTraits<P>;
    using G = Geo<T>;
    constexpr int NR = G::NR, R = G::R;
    constexpr bool START_B = !PT::IFFT;
    const uint32_t lr = lane_rows<T, START_B>(c, a);
    const WaveRows<T, START_B> wr(c, a);
    if constexpr (PT::LOAD == LD_PLAIN) {
        const LaneOff<V32> lo(lr, a.S_in, c.offL);
#pragma unroll
        for (int m = 0; m < NR; m++) {
            // (in_rows_mask: every chunk of the launch reads the one chunk at in)
            const uint32_t ur = a.in_rows_mask ? (wr(m) & a.in_rows_mask) : wr(m);
            ld_sel(a, lo.at(sgpr_ptr(a.in + (uint64_t)ur * a.S_in)), c.active & !((d.zrow >> m) & 1u), c.offL, d.L[m], d.H[m]);
        }
    } else if constexpr (PT::LOAD == LD_GATHER_ENC) {
        // HighRateEncoder::encode: work[0..k) = originals, rest zero (rate_high.rs:50-54)
        const LaneOff<V32> lo(lr, a.S_seg, c.offL);
#pragma unroll
        for (int m = 0; m < NR; m++) {
            const uint32_t ur = wr(m);
            ld_sel(a, lo.at(sgpr_ptr(a.seg_a + (uint64_t)ur * a.S_seg)), c.active & row_below(ur, lr, a.a_count),
                   c.offL, d.L[m], d.H[m]);
        }
    } else if constexpr (PT::LOAD == LD_GATHER_DEC) {
        // received rows (multiplied by their erasure logs in process_item), else
        // zero.  Received bits of the wave's rows: rows [row0, row0 + 16 HWS)
        // of the bitmap (row0 a multiple of 16, of 32 when HWS > 1), scalar loads.
        static_assert(START_B == false && T <= 8, "gather runs in layout A");
        const uint32_t row0 = row_rel<T>(c, a, (c.w * G::HWS) << R) + a.row_base_in;
        const cu32p rb = (cu32p)a.rbits + (row0 >> 5);
        const uint32_t sub = c.s - c.w * G::HWS;
        uint32_t bits;
        // (uni(): each word stays a scalar load; a select of two loads would
        // be folded into one per-lane vector load)
        if constexpr (NR == 8) bits = uni(rb[0]) >> ((row0 & 31) + sub * 8);  // (HWS * 8 <= 32 rows)
        else if constexpr (G::HWS == 4) bits = ((sub >> 1) ? uni(rb[1]) : uni(rb[0])) >> ((sub & 1) * 16);
        else if constexpr (G::HWS == 2) bits = uni(rb[0]) >> (sub * 16);
        else bits = uni(rb[0]) >> (row0 & 31);
        bits &= (1u << NR) - 1;
        const LaneOff<V32> lo(lr, a.S_seg, c.offL);
#pragma unroll
        for (int m = 0; m < NR; m++) {
            const uint32_t ur = wr(m) + a.row_base_in;
            const gbyte* p;
            if constexpr (V32) {
                // (voff32: the wave's rows never straddle the segment boundary)
                p = lo.at(sgpr_ptr(ur >= a.chunk ? a.seg_b + (int64_t)((int64_t)ur - a.chunk) * (int64_t)a.S_seg
                                                 : a.seg_a + (uint64_t)ur * a.S_seg));
            } else {
                const uint32_t r = ur + lr;
                p = (const gbyte*)((r >= a.chunk ? a.seg_b + (uint64_t)(r - a.chunk) * a.S_seg
                                                 : a.seg_a + (uint64_t)r * a.S_seg) +
                                   c.offL);
            }
            ld_sel(a, p, c.active & ((bits >> m) & 1u), c.offL, d.L[m], d.H[m]);
        }
    } else {  // LD_DEC_LAST: u in registers, z for y = u + L(z)
        d.ztile = a.zflags && tile_is_zero(a, tile);
        const LaneOff<V32> lo(lr, a.S_in, c.offL);
#pragma unroll
        for (int m = 0; m < NR; m++) {
            const uint32_t ur = wr(m);
            ld_sel(a, lo.at(sgpr_ptr(a.in + (uint64_t)ur * a.S_in)), c.active & !d.ztile, c.offL, d.zl[m], d.zh[m]);
            ld_sel(a, lo.at(sgpr_ptr(a.in2 + (uint64_t)ur * a.S_in)), c.active, c.offL, d.L[m], d.H[m]);
        }
    }
}

// Issue the HBM loads of one item (and read its decode flags).
template <int P, int T>
__device__ __forceinline__ void load_item(const PassArgs& a, const Thr& c, uint32_t tile, ItemRegs<P, T>& d) {
    using PT = ProgTraits<P>;
    using G = Geo<T>;
    constexpr int NR = G::NR, R = G::R;
    [[maybe_unused]] constexpr bool START_B = !PT::IFFT;
    d.zrow = d.zmask = 0;
    d.ztile = false;
    // ---------------- zero rows of DEC_MID ----------------
    // Row r of this pass came from DEC_FIRST tile r >> lo = k + (b_high << T).
    // zrow bit m: this thread's (layout-A) row m is such a skipped, zero row;
    // zmask bit j: tile rows [16j, 16j+16) all are (uniform, scalar loads).
    if constexpr (P == DEC_MID && T > 4 && R != 4) {
        // (8-row sets: one flag byte per row, per lane; no zmask pruning)
        if (a.zflags) {
            const uint8_t* zt = a.zflags + (c.b_high << T) + (c.s << R);
#pragma unroll
            for (int m = 0; m < NR; m++) d.zrow |= (uint32_t)(zt[m] & 1u) << m;
        }
    } else if constexpr (P == DEC_MID && T > 4) {
        if (a.zflags) {
            const uint8_t* zt = a.zflags + (c.b_high << T);
            // the wave's HWS row sets are 16 * HWS consecutive flag bytes:
            // scalar loads, then each lane picks its row set's 16
            const cu32p zw = (cu32p)(zt + ((c.w * G::HWS) << R));
            const uint32_t sub = c.s - c.w * G::HWS;
            uint32_t fw[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t v = uni(zw[j]);
#pragma unroll
                for (int x = 1; x < G::HWS; x++) v = sub == (uint32_t)x ? uni(zw[4 * x + j]) : v;
                fw[j] = v;
            }
#pragma unroll
            for (int m = 0; m < NR; m++) d.zrow |= ((fw[m >> 2] >> (8 * (m & 3))) & 1u) << m;
            const cu32p zf = (cu32p)zt;
#pragma unroll
            for (int j = 0; j < G::SETS; j++)
                if ((zf[4 * j] & zf[4 * j + 1] & zf[4 * j + 2] & zf[4 * j + 3]) == 0x01010101u) d.zmask |= 1u << j;
        }
    }
    if constexpr (FastRows<P, T>::LOAD) {
        if (load_rows_fast<P, T>(a, c, d.L, d.H)) return;
    }
    if (a.voff32) load_rows<P, T, true>(a, c, tile, d);
    else load_rows<P, T, false>(a, c, tile, d);
}

// Stage everything that depends on the tile key of the thread's current
// item: twiddle tables of both directions, and for the decoder's first /
// last pass the per-row erasure and reveal multipliers (and the last 256-point
// FWHT of eval_poly when the caller left it undone, ework).  In two steps:
// issue() sends the twiddle-table loads (one level deep, from skew_tab), so
// the caller can issue the tile's data loads behind them; finish() stages the
// per-row multipliers, writes everything to LDS and ends with a barrier (the
// wave-staged passes: with wave_lds_publish(), see WaveStaged).  The
// caller must have a barrier between the previous key's last use of these
// LDS regions and finish().
// Reveal multipliers (65535 - e of the lost originals) and lost-row flags of
// the tile; programs with a last layout switch stage them there
// (LateReveal), off the load phase -- they are read only by the stores.
template <int P, int T> struct LateReveal {
    static constexpr bool value = st_restores(ProgTraits<P>::STORE) && ProgTraits<P>::FFT && T > 4;
};
template <int P, int T> struct RevealStage {
    using SM = Smem<P, T>;
    using G = Geo<T>;
    static constexpr int RULE = st_row_rule(ProgTraits<P>::STORE);
    Stager<T, (1 << T)> sr;
    uint32_t lost[((1 << T) + G::THREADS - 1) / G::THREADS];
    __device__ __forceinline__ void issue(const PassArgs& a, const Thr& c, const uint32_t* el) {
        sr.issue(a.mul_tab, RevealEntry<T, RULE>{a, c, el});
#pragma unroll
        for (int i = 0; i < (int)(sizeof lost / sizeof lost[0]); i++) {
            const uint32_t k = threadIdx.x + i * G::THREADS;
            lost[i] = k < (1u << T) && row_wanted<RULE>(a, row_rel<T>(c, a, k) + a.row_base_out);
        }
    }
    __device__ __forceinline__ void commit(uint8_t* smem) const {
        uint32_t* lostf = (uint32_t*)(smem + SM::LOST_OFF);
#pragma unroll
        for (int i = 0; i < (int)(sizeof lost / sizeof lost[0]); i++) {
            const uint32_t k = threadIdx.x + i * G::THREADS;
            if (k < (1u << T)) lostf[k] = lost[i];
        }
        sr.commit((uint4*)(smem + SM::RVT_OFF));
    }
};

template <int P, int T> struct TileStage {
    using PT = ProgTraits<P>;
    using SM = Smem<P, T>;
    using G = Geo<T>;
    // second direction at the start: all of it, or only its layout-B tables
    static constexpr int N2 = !SM::TWO ? 0 : (SM::RESTAGE ? G::NTAB - G::TSPLIT : G::NTAB);
    static constexpr bool S2 = N2 > 0;
    // (SHARED: the first direction's layout-A tables into the image region,
    // its layout-B tables beside it)
    // Wave-private staging (WaveStaged): WS_A, the first block runs in layout
    // A -- the wave stages its row sets' layout-A tables (sw), the workgroup
    // the first direction's layout-B ones (s1b); WS_B, it runs in layout B
    // (ENC_LAST) -- every wave stages the layout-B tables (sw, into the shared
    // slots: a copy per wave would add 4.5 KiB of LDS to a layout that has
    // 6 KiB left under ONE_ROUND_MAX, for values that are the same anyway), the
    // workgroup the layout-A ones (s1).
    static constexpr bool WS = WaveStaged<P, T>::value;
    static constexpr bool WS_A = WS && PT::IFFT, WS_B = WS && !PT::IFFT;
    static_assert(!WS || (T > 4 && G::R == 4 && PT::LOAD != LD_GATHER_DEC && !st_restores(PT::STORE)),
                  "wave-private staging: 16-row sets, twiddle tables only");
    static constexpr int N1 = WS_A ? 0 : (SM::SHARED || WS_B ? G::TSPLIT : G::NTAB);
    static constexpr int N1B = SM::SHARED || WS_A ? G::NTAB - G::TSPLIT : 0;
    static constexpr int NW = WS_A ? G::HWS * (G::NR - 1) : (WS_B ? G::NTAB - G::TSPLIT : 0);
    Stager<T, N1> s1;
    Stager<T, N1B> s1b;
    Stager<T, N2> s2;
    WaveStager<NW> sw;
    // tile group id of the wave's table i
    static __device__ __forceinline__ uint32_t wave_group(const Thr& c, int i) {
        if constexpr (WS_A) {
            // table i15 of row set hs: layer kb = R - 1 - floor(log2(2^R - 1 - i15))
            constexpr int NA = G::NR - 1, R = G::R;
            const int hs = i / NA, i15 = i - hs * NA;
            const int kb = R - 32 + __clz((uint32_t)(NA - i15));
            const uint32_t gi = (uint32_t)(i15 - ((1 << R) - (1 << (R - kb))));
            const uint32_t s = c.w * G::HWS + (uint32_t)hs;
            return (uint32_t)((1 << T) - (1 << (T - kb))) + (s << (R - 1 - kb)) + gi;
        } else {
            return (uint32_t)(G::TSPLIT + i);
        }
    }

    uint32_t ev[4];  // wave 0: the tile's 256-row block of eval_poly's work (ework)
    // decoder gather: the received-bitmap words of this thread's erasure-table
    // rows, loaded before the tile's rows so that the table loads that depend
    // on them issue back to back (a per-row flag load after the rows would
    // wait for all of them, once per table)
    static constexpr int PER_E = ((1 << T) * 5 + G::THREADS - 1) / G::THREADS;
    uint32_t rw[PT::LOAD == LD_GATHER_DEC ? PER_E : 1];

    // the 256-row block holding the tile's decode rows (contiguous tiles of
    // 2^T <= 256 rows at a multiple of 2^T lie in one block)
    __device__ __forceinline__ uint32_t elog_row0(const PassArgs& a, const Thr& c) const {
        const uint32_t base = PT::LOAD == LD_GATHER_DEC ? a.row_base_in : a.row_base_out;
        return row_rel<T>(c, a, 0) + base;
    }
    __device__ __forceinline__ void issue(const PassArgs& a, const Thr& c) {
        if constexpr (SM::ELOG_BYTES > 0) {
            // requested first: the erasure logs head the staging chain
            if (a.ework && c.w == 0) {
                const uint32_t* src = a.ework + (elog_row0(a, c) & ~255u) + c.lane;
#pragma unroll
                for (int j = 0; j < 4; j++) ev[j] = src[64 * j];
            }
        }
        if constexpr (PT::LOAD == LD_GATHER_DEC) {
#pragma unroll
            for (int i = 0; i < PER_E; i++) {
                const uint32_t idx = threadIdx.x + (uint32_t)i * G::THREADS;
                const uint32_t k = min(idx / 5, (1u << T) - 1);
                rw[i] = a.rbits[(row_rel<T>(c, a, k) + a.row_base_in) >> 5];
            }
        }
        // (the wave's own tables first: its first layers wait for them alone)
        if constexpr (WS) {
            const TwiddleEntry<T> tw{a, c, 0, PT::IFFT ? a.skew_ifft : a.skew_fft};
            sw.issue(a.skew_tab, c.lane, [&](int i) { return tw((int)wave_group(c, i)); });
        }
        s1.issue(a.skew_tab, TwiddleEntry<T>{a, c, 0, PT::IFFT ? a.skew_ifft : a.skew_fft});
        if constexpr (N1B > 0) s1b.issue(a.skew_tab, TwiddleEntry<T>{a, c, G::TSPLIT, a.skew_ifft});
        if constexpr (S2) s2.issue(a.skew_tab, TwiddleEntry<T>{a, c, G::NTAB - N2, a.skew_fft});
    }
    // Decoder gather staging, run before the tile's row loads: the erasure
    // logs' last FWHT into LDS, then the "MULTIPLY SHARDS" table loads into
    // se (committed by finish()).
    Stager<T, (PT::LOAD == LD_GATHER_DEC ? (1 << T) : 0)> se;
    const uint32_t* el = nullptr;
    __device__ __forceinline__ void gather(const PassArgs& a, const Thr& c, uint8_t* smem) {
        if constexpr (SM::ELOG_BYTES > 0) {
            if (a.ework) {
                // the last 256-point FWHT of eval_poly, by wave 0 in registers
                uint32_t* elds = (uint32_t*)(smem + SM::ELOG_OFF);
                if (c.w == 0) {
                    fwht256_wave(ev);
#pragma unroll
                    for (int j = 0; j < 4; j++) elds[c.lane + 64 * j] = ev[j];
                }
                __syncthreads();
                el = elds + (elog_row0(a, c) & 255u);
            }
        }
        if constexpr (PT::LOAD == LD_GATHER_DEC) {
            // "MULTIPLY SHARDS" tables (received row r x e[r], absent rows x 0;
            // the received bit from rw)
            static_assert(PER_E == Stager<T, (1 << T)>::PER, "one table chunk per (thread, i)");
            const u32x4* tab = (const u32x4*)a.mul_tab;
            // (two uniform paths: with the logs in LDS every table load issues
            // back to back; only the HBM-logs path waits per row)
            auto gather_rows = [&](auto log_of) {
#pragma unroll
                for (int i = 0; i < PER_E; i++) {
                    const uint32_t idx = threadIdx.x + (uint32_t)i * G::THREADS;
                    const uint32_t k = min(idx / 5, (1u << T) - 1);
                    const uint32_t r = row_rel<T>(c, a, k) + a.row_base_in;
                    const bool rcv = (rw[i] >> (r & 31)) & 1u;
                    const uint32_t e = rcv ? log_of(k, r) : ZERO_ENTRY;
                    if (idx < (1u << T) * 5)
                        se.v[i] = tab[(size_t)e * (TAB_DWORDS / 4) + idx % 5];
                }
            };
            if (el) gather_rows([&](uint32_t k, uint32_t) { return el[k]; });
            else gather_rows([&](uint32_t, uint32_t r) { return a.elog[r]; });
        }
    }
    template <bool GATHERED = false>
    __device__ __forceinline__ void finish(const PassArgs& a, const Thr& c, uint8_t* smem) {
        if constexpr (!GATHERED) gather(a, c, smem);
        if constexpr (PT::LOAD == LD_GATHER_DEC) se.commit((uint4*)(smem + SM::ERT_OFF));
        if constexpr (st_restores(PT::STORE) && !LateReveal<P, T>::value) {
            RevealStage<P, T> rs;
            rs.issue(a, c, el);
            rs.commit(smem);
        }
        if constexpr (WS) {
            // The wave's own tables, then the tables of the later blocks (all
            // requested ahead of the rows: one vmcnt wait that leaves every
            // row load in flight).  The latter are first read behind the
            // barriers of the first layout switch, so this ends without one.
            sw.commit((uint4*)(smem + SM::TAB1_OFF), c.lane, [&](int i) { return wave_group(c, i); });
            if constexpr (S2) s2.commit((uint4*)(smem + SM::TAB2_OFF));
            s1.commit((uint4*)(smem + SM::TAB1_OFF));
            s1b.commit((uint4*)(smem + (SM::SHARED ? SM::TABB_OFF : SM::TAB1_OFF + G::TSPLIT * 80)));
            wave_lds_publish();
            return;
        }
        if constexpr (S2) s2.commit((uint4*)(smem + SM::TAB2_OFF));
        s1.commit((uint4*)(smem + SM::TAB1_OFF));
        if constexpr (N1B > 0) s1b.commit((uint4*)(smem + SM::TABB_OFF));
        __syncthreads();  // staged tables visible
    }
};

// Received counts of a decode with identity multipliers (PassArgs::rcount,
// ENC_FIRST / ENC_LAST launched by decode_passes): wave j of the first
// slab's workgroup counts chunk j of its tile (a tile below 64 rows: the
// chunk's first tile counts it).  Behind uniform branches: the flag bytes
// are the workgroup's first loads (so the compiler's waits for the later
// loads do not change), the ballots run after the tables are staged (the
// bytes are older than the table loads that the staging waited for, with or
// without its barrier) and the counts, in SGPRs, are stored after the item.
template <int P, int T> struct RcvCount {
    static constexpr bool ON = P == ENC_FIRST || P == ENC_LAST;
    static constexpr uint32_t NCH = (1u << T) >= 64 ? (1u << T) / 64 : 1;
    bool go;
    uint32_t r0, f, cnt;
    __device__ __forceinline__ void issue(const PassArgs& a, const Thr& c, bool first) {
        go = false;
        if constexpr (ON) {
            r0 = uni(row_rel<T>(c, a, 0) + 64u * c.w);
            go = first && a.rcount && c.w < NCH && (r0 & 63u) == 0;
            // (the raw byte: it is first looked at in count(), behind the
            // row loads -- a test here would wait for it before they issue,
            // and against a constant 1 the compiler moves count()'s test up
            // to the load, hence the opaque one)
            f = 1;
            asm("" : "+v"(f));
            if (go && a.cnt_flags) f = a.cnt_flags[r0 + c.lane];
        }
    }
    __device__ __forceinline__ void count() {
        if constexpr (ON)
            if (go) cnt = uni((uint32_t)__popcll(__ballot(f != 0)));
    }
    __device__ __forceinline__ void store(const PassArgs& a, const Thr& c) const {
        if constexpr (ON) {
            if (go && c.lane == 0) {
                const uint32_t ch = (r0 + a.cnt_base) >> 6;
                a.rcount[2 * ch + a.cnt_seg] = cnt;
                a.rcount[2 * ch + 1 - a.cnt_seg] = 0;
            }
        }
    }
};

// ST_RESTORE_ALL (the repair's programs): where work row rw + lr of a lane is
// stored -- the row's own segment's array, rest + r S_rest below `chunk`,
// rest_b + (r - chunk) S_rest from there on.  rw: the wave's row of the row
// register, lr: the lane's rows below it, lo: the lane's byte offset.  With
// 32-bit lane offsets the base is one scalar choice by the wave's row: voff32
// is set only when chunk % 2^(T + lo) == 0 (pass_launch_consts, `aligned`), so
// every row of the tile lies on the wave's side of `chunk`.  Else the lane's
// own row chooses (3000:5 at 2^6-row tiles: chunk = 8 lies inside tile 0).
template <bool V32>
__device__ __forceinline__ gbyte* restore_all_ptr(const PassArgs& a, const Thr& cs, uint32_t rw, uint32_t lr,
                                                  const LaneOff<V32>& lo) {
    if constexpr (V32) {
        return lo.at(sgpr_ptr(rw >= a.chunk ? a.rest_b + (uint64_t)(rw - a.chunk) * a.S_rest
                                            : a.rest + (uint64_t)rw * a.S_rest));
    } else {
        const uint32_t r = rw + lr;
        return (gbyte*)((r >= a.chunk ? a.rest_b + (uint64_t)(r - a.chunk) * a.S_rest : a.rest + (uint64_t)r * a.S_rest) +
                        cs.offL);
    }
}
// ST_VERIFY (the scrub's programs): row registers m0 .. m0 + N - 1 of an item
// against the stored recovery rows.  A row is compared when the lane holds a
// quad, the row lies below out_rows and its byte of the check set (if any) is
// nonzero -- the byte is read for rows below out_rows only, and the stored array
// for compared rows only: every other lane reads the zero page in its place
// (ld_sel: the array has out_rows rows and a slab may be wider than the shard),
// so the N requests go out together, ahead of the first compare.  A lane whose
// quad differs stores 1 to its row's flag and to the flag of the quad's 64-byte
// block (offL = (Qg >> 3) * 64 + (Qg & 7) * 4 of quad Qg: block Qg >> 3 = offL
// >> 6).  Several lanes and workgroups may store the same byte, all the value 1.
template <int P, int T, bool V32, int N>
__device__ __forceinline__ void verify_rows(const PassArgs& a, const Thr& cs, const uint32_t (&L)[Geo<T>::NR],
                                            const uint32_t (&H)[Geo<T>::NR], int m0) {
    static_assert(ProgTraits<P>::STORE == ST_VERIFY && ProgTraits<P>::FFT, "the scrub's programs end in layout A");
    const uint32_t lr = lane_rows<T, false>(cs, a);
    const WaveRows<T, false> wr(cs, a);
    const LaneOff<V32> lo(lr, a.vfy_S, cs.offL);
    bool ok[N];
    uint32_t sl[N], sh[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
        const uint32_t ur = wr(m0 + i);
        ok[i] = cs.active & row_below(ur, lr, a.out_rows);
        if (a.vfy_checked) ok[i] = ok[i] && a.vfy_checked[ur + lr] != 0;
        ld_sel(a, lo.at(sgpr_ptr(a.vfy_cmp + (uint64_t)ur * a.vfy_S)), ok[i], cs.offL, sl[i], sh[i]);
    }
#pragma unroll
    for (int i = 0; i < N; i++) {
        if (ok[i] & (((sl[i] ^ L[m0 + i]) | (sh[i] ^ H[m0 + i])) != 0)) {
            a.vfy_rows[wr(m0 + i) + lr] = 1;
            if (a.vfy_cols) a.vfy_cols[cs.offL >> 6] = 1;
        }
    }
}
// The store of row register m of an item (the counterpart of load_rows): recovery / work rows as they are, lost originals revealed
// (x (65535 - e), rate_high.rs:236-242) into the caller's original array.
template <int P, int T, bool V32>
__device__ __forceinline__ void store_row(const PassArgs& a, const Thr& cs, uint32_t L, uint32_t H, int m,
                                          const uint4* rvt, const uint32_t* lostf) {
    using PT = ProgTraits<P>;
    constexpr bool END_B = !PT::FFT && T > 4;
    constexpr bool NT = PT::ST_NT;
    const uint32_t lr = lane_rows<T, END_B>(cs, a);
    const WaveRows<T, END_B> wr(cs, a);
    const uint32_t ur = wr(m);
    if constexpr (PT::STORE == ST_PLAIN) {
        const LaneOff<V32> lo(lr, a.S_out, cs.offL);
        const uint32_t k = kidx<T, END_B>(cs, m);
        st_ptr<NT>(lo.at(sgpr_ptr(a.out + (uint64_t)ur * a.S_out)),
                   cs.active & (P != DEC_MID || (k >= a.need_lo && k < a.need_hi)), L, H);
    } else if constexpr (PT::STORE == ST_RECOVERY) {
        const LaneOff<V32> lo(lr, a.S_out, cs.offL);
        st_ptr<NT>(lo.at(sgpr_ptr(a.out + (uint64_t)ur * a.S_out)), cs.active & row_below(ur, lr, a.out_rows), L, H);
    } else {
        static_assert(st_restores(PT::STORE), "ST_VERIFY stores no row: verify_rows");
        // lost original row r -> restored-originals row r + row_base_out - (segment start)
        const LaneOff<V32> lo(lr, a.S_rest, cs.offL);
        const int64_t shift = (int64_t)a.row_base_out - (a.rest_seg_b ? (int64_t)a.chunk : 0);
        const uint32_t k = kidx<T, END_B>(cs, m);
        // (a row that is not a lost original is neither multiplied nor
        // stored: the branch is per row set, so a wave whose rows were all
        // received skips the reveal -- most rows of a decode with few losses)
        if (cs.active & (lostf[k] != 0)) {
            uint32_t tt[20];
            load_table_lds(tt, rvt + k * 5);
            uint32_t ol = 0, oh = 0;
            mul_xor(ol, oh, L, H, tt);
            if constexpr (PT::STORE == ST_RESTORE_ALL) {
                st_ptr<NT>(restore_all_ptr<V32>(a, cs, ur + a.row_base_out, lr, lo), true, ol, oh);
            } else {
                st_ptr<NT>(lo.at(sgpr_ptr(a.rest + ((int64_t)ur + shift) * (int64_t)a.S_rest)), true, ol, oh);
            }
        }
    }
}
template <int P, int T, bool V32>
__device__ __forceinline__ void store_rows(const PassArgs& a, const Thr& cs, const uint32_t (&L)[Geo<T>::NR],
                                           const uint32_t (&H)[Geo<T>::NR], const uint4* rvt, const uint32_t* lostf) {
    if constexpr (ProgTraits<P>::STORE == ST_VERIFY) {
        verify_rows<P, T, V32, Geo<T>::NR>(a, cs, L, H, 0);
    } else {
#pragma unroll
        for (int m = 0; m < Geo<T>::NR; m++) store_row<P, T, V32>(a, cs, L[m], H[m], m, rvt, lostf);
    }
}
// Early stores: the last FFT block in layout A runs depth-first (LayerSeq),
// so rows m, m + 1 are final as soon as their layer-0 group is done; this
// functor stores them there, spreading the item's stores over the block
// instead of a burst after it.
template <int P, int T, bool PAIR = false> struct EarlyStore {
    const PassArgs& a;
    const Thr& cs;
    const uint4* rvt;
    const uint32_t* lostf;
    const FastStore<P, T, PAIR> fs;
    __device__ __forceinline__ void operator()(const uint32_t (&L)[Geo<T>::NR], const uint32_t (&H)[Geo<T>::NR],
                                               int m) const {
        if constexpr (ProgTraits<P>::STORE == ST_VERIFY) {
            // (the stored quads of both rows requested, then compared)
            if (a.voff32) verify_rows<P, T, true, 2>(a, cs, L, H, m);
            else verify_rows<P, T, false, 2>(a, cs, L, H, m);
        } else if (PAIR || fs.on) {
            fs.row(m, L[m], H[m]);
            fs.row(m + 1, L[m + 1], H[m + 1]);
        } else if (a.voff32) {
            store_row<P, T, true>(a, cs, L[m], H[m], m, rvt, lostf);
            store_row<P, T, true>(a, cs, L[m + 1], H[m + 1], m + 1, rvt, lostf);
        } else {
            store_row<P, T, false>(a, cs, L[m], H[m], m, rvt, lostf);
            store_row<P, T, false>(a, cs, L[m + 1], H[m + 1], m + 1, rvt, lostf);
        }
    }
};

// EarlyStore of the tower form's last pass, with B's pools for the conversion
// in the layer ahead of the stores (GroupLoop).
template <int P, int T, bool PAIR> struct EarlyStoreTower : EarlyStore<P, T, PAIR> {
    TowerB tb;
};

// The same for a pass that ends with its IFFT in layout B (ENC_FIRST, the
// decoders' first pass, GEN_IFFT): the rows with register bit 0 clear and
// those with it set go through the block's layers separately -- the layer of
// register bit 0 (layout-B bit SHB, the first one at T = 8) all in the first
// half, every higher layer's butterfly pairs m, m + 2^rb with m of the half's
// parity -- so the even rows are final after the first half and are stored
// there (fin), and the odd rows' butterflies run while those stores drain.
// Same groups, tables and butterflies as layers<.., LB = true, .., IFFT>,
// in another order; every group's table is read (LDS) one group ahead.
template <int T> struct HalfSeq {
    static constexpr int SH = Geo<T>::SHB, NR = Geo<T>::NR;
    // step g -> half * 256 + kb * 16 + gi
    static constexpr int at(int g) {
        int n = 0;
        for (int half = 0; half < 2; half++)
            for (int kb = Geo<T>::R; kb < T; kb++) {
                const int rb = kb - SH;
                if (rb == 0 && half == 1) continue;  // (bit 0's layer: all in the first half)
                for (int gi = 0; gi < (NR >> (rb + 1)); gi++)
                    if (n++ == g) return half * 256 + kb * 16 + gi;
            }
        return -1;
    }
    static constexpr int total() {
        int g = 0;
        while (at(g) >= 0) g++;
        return g;
    }
};
// TB = TowerMul<WIDE3>: the tower kernels' form of the block (ENC_FIRST, its
// rows in tower form since its first layer): the multiply on a tower table,
// WIDE3 by three byte maps.
struct NoTower {};
template <bool WIDE3> struct TowerMul {};
template <int T, int G, class FIN, class TB = NoTower> struct HalfLoop {
    static __device__ __forceinline__ void run(uint32_t (&L)[Geo<T>::NR], uint32_t (&H)[Geo<T>::NR],
                                               const uint4* tab1, const uint32_t (&cur)[20], const FIN& fin,
                                               const TB& tb = TB()) {
        using S = HalfSeq<T>;
        constexpr int e = S::at(G), half = e >> 8, kb = (e >> 4) & 15, gi = e & 15, rb = kb - S::SH;
        constexpr bool more = G + 1 < S::total();
        uint32_t nxt[20];
        if constexpr (more) {
            constexpr int kb2 = (S::at(G + 1) >> 4) & 15, gi2 = S::at(G + 1) & 15;
            load_table_lds(nxt, tab1 + ((1 << T) - (1 << (T - kb2)) + gi2) * 5);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < (1 << rb); j++) {
            if (rb > 0 && (j & 1) != half) continue;
            const int m = (gi << (rb + 1)) + j, m2 = m + (1 << rb);
            L[m2] ^= L[m];
            H[m2] ^= H[m];
            if constexpr (std::is_same<TB, TowerMul<true>>::value) {
                mul_xor_tower_wide(L[m], H[m], L[m2], H[m2], cur);
            } else {
                mul_xor(L[m], H[m], L[m2], H[m2], cur);
            }
            asm volatile("" : "+v"(L[m]), "+v"(H[m]), "+v"(L[m2]), "+v"(H[m2]));
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (more) {
            if constexpr (half == 0 && (S::at(G + 1) >> 8) == 1) fin(L, H);  // the even rows are final
            HalfLoop<T, G + 1, FIN, TB>::run(L, H, tab1, nxt, fin, tb);
        }
    }
};
template <int T, class FIN, class TB = NoTower>
__device__ __forceinline__ void ifft_b_halves(uint32_t (&L)[Geo<T>::NR], uint32_t (&H)[Geo<T>::NR], const uint4* tab1,
                                              const FIN& fin, const TB& tb = TB()) {
    constexpr int e = HalfSeq<T>::at(0), kb = (e >> 4) & 15, gi = e & 15;
    tab1 = lds_vgpr(tab1);
    uint32_t t0[20];
    load_table_lds(t0, tab1 + ((1 << T) - (1 << (T - kb)) + gi) * 5);
    HalfLoop<T, 0, FIN, TB>::run(L, H, tab1, t0, fin, tb);
}
// fin of ifft_b_halves: the even rows
template <int P, int T, bool PAIR = false> struct EvenStore {
    const PassArgs& a;
    const Thr& cs;
    const FastStore<P, T, PAIR> fs;
    __device__ __forceinline__ void operator()(const uint32_t (&L)[Geo<T>::NR], const uint32_t (&H)[Geo<T>::NR]) const {
        if (PAIR || fs.on) {
#pragma unroll
            for (int m = 0; m < Geo<T>::NR; m += 2) fs.row(m, L[m], H[m]);
            return;
        }
#pragma unroll
        for (int m = 0; m < Geo<T>::NR; m += 2) {
            if (a.voff32) store_row<P, T, true>(a, cs, L[m], H[m], m, nullptr, nullptr);
            else store_row<P, T, false>(a, cs, L[m], H[m], m, nullptr, nullptr);
        }
    }
};

// Compute and store one item whose rows are in d (every thread of the
// workgroup calls it for the same item).
// (PRE: the late-rows kernels' requests inside the first layer block, LateRows;
// PAIR_OUT: the stores write paired rows, FastStore; TOWER: Z's rows are in
// tower form and so are the rows in every layer -- ENC_FIRST converts its rows
// in its first layer, ENC_LAST in its last; pre.tb holds B's pools)
template <int P, int T, int NV, class PRE = NoPre, bool PAIR_OUT = false, bool TOWER = false>
__device__ __forceinline__ void process_item(const PassArgs& a, const Thr& c, uint32_t tile, ItemRegs<P, T>& d,
                                             uint8_t* smem, const PRE& pre = PRE()) {
    using PT = ProgTraits<P>;
    // (a one-direction tower pass has no narrow layers: its NV is the wide multiply, pass_kernel_late_tower)
    constexpr bool WIDE3 = TOWER && !(PT::IFFT && PT::FFT) && NV == 1;
    constexpr int TWF = !TOWER ? TW_NONE : (WIDE3 ? TW_WIDE3 : TW_ROWS);
    constexpr int NKI = NarrowVar<(WIDE3 ? 0 : NV)>::IFFT_FROM, NKF = NarrowVar<(WIDE3 ? 0 : NV)>::FFT_FROM;
    static_assert(NV == 0 || WIDE3 || (PT::IFFT && PT::FFT && T > 4), "narrow variants: two-direction passes only");
    using SM = Smem<P, T>;
    using G = Geo<T>;
    constexpr int NR = G::NR;
    constexpr int R = G::R;
    constexpr int NQR = Rnd<P, T>::NQR;
    constexpr bool TWO = SM::TWO;
    // (DEC_MID runs with T >= 5 only; the 16-row-block pruning needs R = 4)
    constexpr bool ZERO_SKIP = P == DEC_MID && T > 4 && G::R == 4;
    // stores inside the last FFT block (16 rows per lane, not the
    // output-pruned DEC_MID; the reveal stores measured slower inside it)
    constexpr bool EARLY = LayerSeq<T, false, 0, R, true>::DF && P != DEC_MID && !st_restores(PT::STORE) && PT::FFT &&
                           T > 4;
    // the IFFT-only passes: early stores of the even rows (ifft_b_halves;
    // against all stores after the last block: profiles/r05_early_b_ab.txt)
    constexpr bool EARLY_B = PT::IFFT && !PT::FFT && PT::STORE == ST_PLAIN && T > 4 && G::R == 4;
    uint2* lds = (uint2*)smem;
    const uint4* tab1 = (const uint4*)(smem + SM::TAB1_OFF);
    const uint4* tab2 = (const uint4*)(smem + SM::TAB2_OFF);
    const uint4* ert = (const uint4*)(smem + SM::ERT_OFF);
    const uint4* rvt = (const uint4*)(smem + SM::RVT_OFF);
    const uint32_t* lostf = (const uint32_t*)(smem + SM::LOST_OFF);
    uint32_t(&L)[NR] = d.L;
    uint32_t(&H)[NR] = d.H;
    constexpr bool START_B = !PT::IFFT;
    // Final layout: after FFT -> A; after IFFT only -> B (T > 4); T <= 4: A == B.
    [[maybe_unused]] constexpr bool END_B = !PT::FFT && T > 4;
    // DEC_MID whose consumed tile rows (the last pass's tiles with a lost
    // original, [need_lo, need_hi)) lie in few layout-B register rows: the
    // formal derivative split by row bits (fd_regs / fd_image), otherwise
    // through the LDS image (tile_fd).  The layout-A FFT layers make every
    // row of a consumed row's 2^R-row block an input of it: the block's
    // layout-B register rows [fd_m0, fd_m0 + FD_ND) take the fd_image terms.
    constexpr bool SPLIT_FD = P == DEC_MID && T > 4;
    constexpr int FD_PB = 1 << (R - G::SHB);            // register rows per 2^R-row block
    constexpr int FD_ND = FD_PB > 2 ? FD_PB : 2;        // register rows carried
    [[maybe_unused]] bool fd_few = false;
    [[maybe_unused]] uint32_t fd_m0 = 0;
    [[maybe_unused]] uint32_t dl[FD_ND], dh[FD_ND];
    if constexpr (SPLIT_FD) {
        const uint32_t lo = uni(a.need_lo), hi = uni(min(a.need_hi, 1u << T));
        const uint32_t m0 = (lo >> R) * FD_PB, m1 = hi <= lo ? m0 : (((hi - 1) >> R) + 1) * FD_PB;
        fd_few = !a.fd_lds && m1 - m0 <= (uint32_t)FD_ND;
        fd_m0 = hi <= lo ? 0u : min(m0, (uint32_t)(NR - FD_ND));
    }

    if constexpr (P == DEC_FIRST) {
        // A tile without received rows is zero after the erasure multiply
        // and through the IFFT: DEC_MID / DEC_LAST read it as zero, skip it.
        // (pass_kernel has returned for such a tile already; the recheck
        // stays because removing it changes the kernels' machine code)
        if (a.zflags && tile_is_zero(a, tile)) {
            __builtin_amdgcn_s_waitcnt(vmcnt_wait(0));  // (see the end of this function)
            return;
        }
    }
    if constexpr (PT::LOAD == LD_GATHER_DEC) {
#pragma unroll
        for (int m = 0; m < NR; m++) {
            uint32_t tt[20];
            load_table_lds(tt, ert + kidx<T, START_B>(c, m) * 5);
            const uint32_t yl = L[m], yh = H[m];
            L[m] = H[m] = 0;
            mul_xor(L[m], H[m], yl, yh, tt);
        }
    }
    if constexpr (PT::LOAD == LD_DEC_LAST) {
        if (!d.ztile) tile_fd<T, NQR, START_B>(L, H, d.zl, d.zh, c, lds);
    }

    // SHARED: the second direction's layout-A tables are requested after the
    // first layout switch and written over the image after the second
    [[maybe_unused]] Stager<T, (SM::SHARED ? G::TSPLIT : 0)> s3s;
    // ---------------- IFFT ----------------
    bool in_b = START_B;
    if constexpr (PT::IFFT) {
        // DEC_MID: a wave whose rows all are zero skips its layout-A layers
        bool skip_a = false;
        if constexpr (ZERO_SKIP) skip_a = __all(d.zrow == (1u << NR) - 1);
        if constexpr (WaveStaged<P, T>::value) RS16_STAMP_ROWS(a, 6, L, H, 0, 1);
        if constexpr (!std::is_same<PRE, NoPre>::value)
            layers<P, T, NKI, false, 0, R, false, false, PR_NONE, NoFin, PRE, TWF>(L, H, c, a, tab1, tab2, 0, NoFin(),
                                                                                     pre);
        else if (!skip_a) layers<P, T, NKI, false, 0, R, false, false>(L, H, c, a, tab1, tab2);
        RS16_STAMP(a, 3);
        prio<1>();
        if constexpr (T > 4) {
            // the second direction's layout-A tables (Smem::RESTAGE)
            constexpr bool LS2 = SM::RESTAGE && !SM::SHARED;
            Stager<T, (LS2 ? G::TSPLIT : 0)> s3;
            if constexpr (LS2) s3.issue(a.skew_tab, TwiddleEntry<T>{a, c, 0, a.skew_fft});
            // (SHARED: the image overwrites the layout-A tables -- every wave
            // must be done with them first)
            if constexpr (SM::SHARED) __syncthreads();
            exchange<T, NQR, false>(
                L, H, c, lds,
                [&]() {
                    if constexpr (LS2) s3.commit((uint4*)(smem + SM::TAB1_OFF));
                },
                [&]() {
                    if constexpr (SPLIT_FD) {
                        if (fd_few) {
                            constexpr int QL = G::Q / NQR;
#pragma unroll
                            for (int i = 0; i < FD_ND; i++)
                                fd_image<T, QL>(dl[i], dh[i], c, lds, kidx<T, true>(c, fd_m0 + i));
                        }
                    }
                });
            RS16_STAMP(a, 4);
            if constexpr (SM::SHARED) s3s.issue(a.skew_tab, TwiddleEntry<T>{a, c, 0, a.skew_fft});
            if constexpr (EARLY_B) {
                Thr cs = c;
                asm volatile("" : "+v"(cs.offL));
                const EvenStore<P, T, PAIR_OUT> even{a, cs, FastStore<P, T, PAIR_OUT>(a, cs)};
                if constexpr (TOWER) ifft_b_halves<T>(L, H, tab1, even, TowerMul<WIDE3>());
                else ifft_b_halves<T>(L, H, tab1, even);
            } else {
                // (SHARED: the layout-B tables t >= TSPLIT sit beside the image)
                const uint4* tab1b = SM::SHARED ? (const uint4*)(smem + SM::TABB_OFF) - G::TSPLIT * 5 : tab1;
                layers<P, T, NKI, true, R, T, false, false, (ZERO_SKIP ? PR_ZERO : PR_NONE), NoFin, NoPre, TWF>(
                    L, H, c, a, tab1b, tab2, d.zmask);
            }
            in_b = true;
        }
        RS16_STAMP(a, 5);
        prio<2>();
    }
    // ---------------- formal derivative (tile bits) ----------------
    if constexpr (PT::FD) {
        if constexpr (SPLIT_FD) {
            if (fd_few) fd_regs<T>(L, H);
            else tile_fd<T, NQR, true>(L, H, L, H, c, lds);
        } else {
            if (in_b) tile_fd<T, NQR, true>(L, H, L, H, c, lds);
            else tile_fd<T, NQR, false>(L, H, L, H, c, lds);
        }
        RS16_STAMP(a, 6);
    }
    // ---------------- FFT ----------------
    if constexpr (PT::FFT) {
        if constexpr (T > 4) {
            if constexpr (WaveStaged<P, T>::value && !PT::IFFT) RS16_STAMP_ROWS(a, 6, L, H, 0, NR / 2);
            if constexpr (!std::is_same<PRE, NoPre>::value && !PT::IFFT)
                layers<P, T, NKF, true, R, T, true, TWO, PR_NONE, NoFin, PRE, TWF>(L, H, c, a, tab1, tab2, 0, NoFin(),
                                                                                     pre);
            else
                layers<P, T, NKF, true, R, T, true, TWO, (P == DEC_MID ? PR_OUT : PR_NONE), NoFin, NoPre, TWF>(
                    L, H, c, a, tab1, tab2);
            if constexpr (SPLIT_FD) {
                // the layout-A bits' derivative terms (fd_image) join the
                // register rows that feed consumed rows
                if (fd_few) {
#pragma unroll
                    for (int m = 0; m < NR; m++) {
#pragma unroll
                        for (int i = 0; i < FD_ND; i++)
                            if ((uint32_t)m == fd_m0 + i) L[m] ^= dl[i], H[m] ^= dh[i];
                    }
                }
            }
            RS16_STAMP(a, 7);
            prio<3>();
            // reveal multipliers: requested before the last layout switch,
            // written to LDS between its barriers (read after the layers)
            RevealStage<P, (LateReveal<P, T>::value ? T : 0)> rs;
            if constexpr (LateReveal<P, T>::value) {
                const uint32_t* el = nullptr;
                if (a.ework) {
                    const uint32_t base = a.row_base_out;
                    el = (const uint32_t*)(smem + SM::ELOG_OFF) + ((row_rel<T>(c, a, 0) + base) & 255u);
                }
                rs.issue(a, c, el);
            }
            if constexpr (SPLIT_FD) {
                if (fd_few) few_switch<T, FD_ND>(L, H, c, lds, fd_m0);
                else exchange<T, NQR, true>(L, H, c, lds);
            } else {
                exchange<T, NQR, true>(L, H, c, lds, [&]() {
                    if constexpr (LateReveal<P, T>::value) rs.commit(smem);
                });
            }
            if constexpr (SM::SHARED) {
                // (the image is dead once every wave's rows are back in
                // registers: exchange() ends with a barrier, few_switch()
                // does not)
                if constexpr (SPLIT_FD) {
                    if (fd_few) __syncthreads();
                }
                s3s.commit((uint4*)(smem + SM::TAB1_OFF));
                __syncthreads();
            }
            RS16_STAMP(a, 8);
            prio<4>();
            in_b = false;
        }
        bool need = true;
        if constexpr (P == DEC_MID) need = (c.s << R) < a.need_hi && ((c.s + 1) << R) > a.need_lo;
        if constexpr (st_restores(PT::STORE) && T > 4) {
            // a row set without a lost original stores nothing: its
            // layout-A FFT layers are skipped (a wave whose two row sets
            // both have none skips them -- most waves of a decode that lost
            // few, scattered originals; against running them always:
            // profiles/r06_restore_skip_ab.txt)
            uint32_t any = 0;
#pragma unroll
            for (int m = 0; m < NR; m++) any |= lostf[kidx<T, false>(c, m)];
            need = any != 0;
        }
        // second direction's layout-A tables: restaged into tab1 (T > 4), else in tab2
        if constexpr (EARLY && TOWER && P == ENC_LAST) {
            // (the last layer converts the rows it stores: B's pools ride in the functor)
            Thr cs = c;
            asm volatile("" : "+v"(cs.offL));
            layers<P, T, NKF, false, 0, R, true, false, PR_NONE, EarlyStoreTower<P, T, PAIR_OUT>, NoPre, TWF>(
                L, H, c, a, tab1, tab2, 0,
                EarlyStoreTower<P, T, PAIR_OUT>{{a, cs, rvt, lostf, FastStore<P, T, PAIR_OUT>(a, cs)}, pre.tb});
        } else if constexpr (EARLY) {
            Thr cs = c;
            asm volatile("" : "+v"(cs.offL));
            layers<P, T, NKF, false, 0, R, true, (TWO && !(SM::RESTAGE)), PR_NONE, EarlyStore<P, T, PAIR_OUT>, NoPre,
                   TWF>(L, H, c, a, tab1, tab2, 0,
                          EarlyStore<P, T, PAIR_OUT>{a, cs, rvt, lostf, FastStore<P, T, PAIR_OUT>(a, cs)});
        } else if (need) {
            layers<P, T, NKF, false, 0, R, true, (TWO && !(SM::RESTAGE))>(L, H, c, a, tab1, tab2);
        }
        RS16_STAMP(a, 9);
    }
    if constexpr (EARLY) {
        RS16_STAMP(a, 10);
        RS16_STAMP_END(a);
        return;
    }

    prio<5>();
    // ---------------- store ----------------
    // The next item's loads were issued before this item's butterflies and
    // have landed by now: retire them before the stores, so that the stores
    // stay in flight across the loop latch (with 2 NR loads + 2 NR stores
    // outstanding there, the compiler's own wait would be vmcnt(0)).
    __builtin_amdgcn_s_waitcnt(vmcnt_wait(0));
    // Row addresses are recomputed here from opaque copies of the item
    // coordinates: otherwise the compiler keeps the load-time addresses of
    // the same rows live through all the butterflies (32 VGPRs).
    Thr cs = c;
    cs.b_low = uni(cs.b_low);
    cs.b_high = uni(cs.b_high);
    asm volatile("" : "+s"(cs.b_low), "+s"(cs.b_high));
    asm volatile("" : "+v"(cs.offL));
    const FastStore<P, T, PAIR_OUT> fs(a, cs);
    if (PAIR_OUT || fs.on) {
        // (EARLY_B: the even rows went out inside the last block)
#pragma unroll
        for (int m = EARLY_B ? 1 : 0; m < NR; m += EARLY_B ? 2 : 1) fs.row(m, L[m], H[m]);
    } else if constexpr (EARLY_B) {
#pragma unroll
        for (int m = 1; m < NR; m += 2) {
            if (a.voff32) store_row<P, T, true>(a, cs, L[m], H[m], m, rvt, lostf);
            else store_row<P, T, false>(a, cs, L[m], H[m], m, rvt, lostf);
        }
    } else {
        if (a.voff32) store_rows<P, T, true>(a, cs, L, H, rvt, lostf);
        else store_rows<P, T, false>(a, cs, L, H, rvt, lostf);
    }
    RS16_STAMP(a, 10);
    RS16_STAMP_END(a);
}

// The four pass kernels below share their head, and the three late-rows ones
// their body, as text: two macros expanded inside each __global__ definition.
// Not as functions: with the late body in a __device__ __forceinline__
// function template that the flavours call, or with more template parameters
// on pass_kernel_late, 26 of the 86 kernels of the encoder's and the tower
// unit compile to other machine code (scripts/isa_compare.py).  The kernels'
// names and template parameters stay: scripts/kres.py and staging_waits.py
// match them.
// RS16_PASS_HEAD (`a`, `G` in scope; leaves c, tile, slab, rcn): the item of
// this workgroup (launch_pass: one per workgroup), its thread coordinates,
// with batched stripes the stripe's arrays and the tile within the stripe.
// (The scrub's arrays are displaced here, for its programs alone: stripe_displace,
// which the small kernels call too, stays as it is.)
template <int P> __device__ __forceinline__ void verify_displace(PassArgs& a, uint32_t st) {
    if constexpr (ProgTraits<P>::STORE == ST_VERIFY) {
        a.vfy_cmp += st * a.bs_vfy_cmp;
        a.vfy_rows += st * a.bs_vfy_rows;
        if (a.vfy_cols) a.vfy_cols += st * a.bs_vfy_cols;
        if (a.vfy_checked) a.vfy_checked += st * a.bs_vfy_checked;
    }
}
#define RS16_PASS_HEAD(P, T) \
    const uint32_t item = blockIdx.x; \
    Thr c; \
    c.lane = threadIdx.x & 63; \
    c.w = uni(threadIdx.x >> 6); \
    c.qt = c.lane % G::Q; \
    c.s = c.w * G::HWS + c.lane / G::Q; \
    c.ql = c.qt % Rnd<P, T>::QL; \
    c.round = c.qt / Rnd<P, T>::QL; \
    uint32_t tile, slab; \
    set_item(c, a, item, G::Q, tile, slab); \
    bool first_stripe = true; \
    if (a.stripe_tiles) { \
        const uint32_t st = uni(fast_div(tile, a.stripe_mul, a.stripe_one)); \
        first_stripe = st == 0; \
        tile -= st * a.stripe_tiles; \
        stripe_displace(a, st); \
        verify_displace<P>(a, st); \
    } \
    tile += a.tile_base; \
    c.b_low = tile & ((1u << a.lo) - 1); \
    c.b_high = tile >> a.lo; \
    RcvCount<P, T> rcn; \
    rcn.issue(a, c, slab == 0 && first_stripe);
// RS16_LATE_BODY: a late-rows kernel after its head -- load-issue order by
// workgroup slot (as pass_kernel), table staging, the first D row pairs through
// RQ (a LateRows type, named by a `using`: no commas), then process_item.
#define RS16_LATE_BODY(P, T, NV, RQ, PAIR_OUT, TOWER) \
    RS16_STAMP(a, 0); \
    const uint32_t slot = (__builtin_amdgcn_s_getreg((31 << 11) | 4) >> 16) & 15u; \
    if (slot == 0) __builtin_amdgcn_s_setprio(3); \
    else if (slot == 1) __builtin_amdgcn_s_setprio(2); \
    else if (slot == 2) __builtin_amdgcn_s_setprio(1); \
    TileStage<P, T> st; \
    st.issue(a, c); \
    ItemRegs<P, T> cur; \
    cur.zrow = cur.zmask = 0; \
    cur.ztile = false; \
    const RQ rq(a, c); \
    rq.prologue(cur.L, cur.H); \
    RS16_STAMP(a, 1); \
    prio<0>(); \
    st.template finish<false>(a, c, smem); \
    rcn.count(); \
    RS16_STAMP(a, 2); \
    process_item<P, T, NV, RQ, PAIR_OUT, TOWER>(a, c, tile, cur, smem, rq); \
    rcn.store(a, c);

// The pass: workgroup b processes item b of the launch (4 waves per SIMD,
// except the one-pass decoders, whose larger register sets take 1).
template <int P, int T, int NV = 0>
__global__ void __launch_bounds__(Geo<T>::THREADS, ((P == DEC_SINGLE || P == DEC_HALF_SINGLE) ? 1 : 4))
    pass_kernel(PassArgs a) {
    using G = Geo<T>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    RS16_PASS_HEAD(P, T)
    if constexpr (P == DEC_FIRST) {
        // a tile without received rows is skipped (process_item): return
        // before its table staging and row loads, so its slot frees at once
        if (a.zflags && tile_is_zero(a, tile)) return;
    }
    if constexpr (P == DEC_MID) {
        // mid_direct_kernel computed this stripe's consumed rows already
        uint32_t nlo, nhi;
        if (a.mid_direct && a.lostrange && mid_need(a, nlo, nhi)) return;
    }
    if constexpr (P == DEC_LAST) {
        // A tile without a lost original stores nothing: return before any
        // load (the decode's lost rows are [lostrange[0], lostrange[1])).
        if (a.lostrange) {
            // (lost_range written out: read through the helper, in any shape
            // tried, this test compiles to other machine code)
            const uint32_t r0 = ((cu32p)a.lostrange)[0], r1 = ((cu32p)a.lostrange)[1];
            if (!((tile << T) < r1 && ((tile + 1) << T) > r0)) return;
            // (tile_last_kernel took this stripe's few tiles)
            if (a.tl_max && tl_covers<T>(a)) return;
        }
    }
    // One item per workgroup, as straight-line code (a loop over items lets the compiler hoist per-row address terms out of it, which
    // costs more VGPRs than the 128 of four waves per SIMD).  The twiddle
    // tables are requested first, the tile's rows right behind them, so the
    // staging latency hides under the row loads.
    RS16_STAMP(a, 0);
    // Load-issue order: the workgroup in slot 0 of its CU (HW_ID.tg_id) issues
    // its rows first, slot 1 next, ...  Same-box A/B: kernel times equal,
    // step time -2 % (643-645 -> 654-659 GiB/s, 3 pairs).  The progress-based
    // schedule (prio<at>) takes over once the tables are staged.
    if constexpr (T >= 7) {
        const uint32_t slot = (__builtin_amdgcn_s_getreg((31 << 11) | 4) >> 16) & 15u;
        if (slot == 0) __builtin_amdgcn_s_setprio(3);
        else if (slot == 1) __builtin_amdgcn_s_setprio(2);
        else if (slot == 2) __builtin_amdgcn_s_setprio(1);
        // (a second-slot sleep before the loads, 2 or 4 us, measured neutral
        // to slower on the T = 7 passes: profiles/r06_t7_slot_sleep_rejected.txt)
    }
    TileStage<P, T> st;
    st.issue(a, c);  // twiddle tables first: they do not queue behind the tile
    // Decoder gather: the erasure tables are requested ahead of the rows (their
    // logs: the tile's eval_poly block + one FWHT, issued with the twiddles),
    // so they do not queue behind the tile in the memory pipeline (same-box
    // A/B: DEC_HALF_FIRST -0.9 us, 3 pairs)
    constexpr bool EARLY = ProgTraits<P>::LOAD == LD_GATHER_DEC;
    if constexpr (EARLY) st.gather(a, c, smem);
    ItemRegs<P, T> cur;
    if constexpr (WaveStaged<P, T>::value) {
        // The full-item loads on every path, the general ones on top of them
        // where the wave needs those.  The compiled form of "if (full) fast
        // loads else general loads" is two guarded blocks in a row, and with
        // them comes an edge around both (never taken) on which no row load
        // was issued at all: the wait for the staged tables, which counts the
        // loads behind them on the poorest path to it, was vmcnt(0) -- a wave
        // waited for its last row before it committed its tables.  With one
        // guarded block the poorest path is the full item's own: the wait
        // leaves its 2 NR row loads in flight, and each row is waited for at
        // its first use.  The price is on the GENERAL waves (wave_rows_mode:
        // a wave across the gather's row limit, 64-bit lane offsets, a row
        // mask): they request 2 NR dwords of the zero page first, and the
        // guarded block, which reuses those registers for its addresses,
        // waits for them to return before it requests the rows -- one more
        // round trip to the cache.  Partial slabs are not among them.
        static_assert(FastRows<P, T>::LOAD, "the encoder-family passes have the full-item loads");
        cur.zrow = cur.zmask = 0;
        cur.ztile = false;
        const uint32_t mode = uni(wave_rows_mode<P, T>(a, c));
        request_rows<P, T, true>(a, c, mode == ROWS_DIRECT, cur.L, cur.H);
        if (mode == ROWS_GENERAL) {
            if (a.voff32) load_rows<P, T, true>(a, c, tile, cur);
            else load_rows<P, T, false>(a, c, tile, cur);
            asm volatile("; general rows requested");
        }
    } else {
        load_item<P, T>(a, c, tile, cur);
    }
    if constexpr (P == DEC_MID) {
        // Only the last pass's tiles that hold a lost original are consumed:
        // tile row k = rows [k << lo, (k + 1) << lo) (read with the rows in flight)
        if (a.lostrange) {
            uint32_t r0, r1;
            lost_range(a, r0, r1);
            const bool any = r0 < r1;
            a.need_lo = max(a.need_lo, any ? r0 >> a.lo : 0u);
            a.need_hi = min(a.need_hi, any ? ((r1 - 1) >> a.lo) + 1 : 0u);
        }
    }
    RS16_STAMP(a, 1);
    prio<0>();
    st.template finish<EARLY>(a, c, smem);
    rcn.count();
    RS16_STAMP(a, 2);
    process_item<P, T, NV>(a, c, tile, cur, smem);
    rcn.store(a, c);
}

// The late-rows variant of a wave-staged pass (LateRows): pass_kernel for a
// launch without ROWS_GENERAL waves (PassConsts::late_rows).  Item mapping,
// table staging, layers and stores are pass_kernel's; the rows are requested
// in two parts, D pairs here and the rest from inside the first layer, all in
// straight-line code (no general block, so no edge without row loads in front
// of the table commit's wait).
template <int P, int T, int NV = 0>
__global__ void __launch_bounds__(Geo<T>::THREADS, 4) pass_kernel_late(PassArgs a) {
    using G = Geo<T>;
    static_assert(WaveStaged<P, T>::value, "late rows: the wave-staged passes");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    RS16_PASS_HEAD(P, T)
    using RQ = LateRows<P, T>;
    RS16_LATE_BODY(P, T, NV, RQ, false, false)
}
// The same kernel reading (PAIR_IN) and / or writing (PAIR_OUT) the work
// buffer's rows in the paired form (LateRows, FastStore) -- a compile-time
// choice, because a guarded block at the request sites is what the late-rows
// variant exists to avoid.  (A kernel of its own name: see RS16_PASS_HEAD.)
template <int P, int T, int NV, bool PAIR_IN, bool PAIR_OUT>
__global__ void __launch_bounds__(Geo<T>::THREADS, 4) pass_kernel_late_paired(PassArgs a) {
    static_assert(PAIR_IN || PAIR_OUT, "the unpaired kernel is pass_kernel_late");
    using G = Geo<T>;
    static_assert(WaveStaged<P, T>::value, "late rows: the wave-staged passes");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    RS16_PASS_HEAD(P, T)
    using RQ = LateRows<P, T, PAIR_IN>;
    RS16_LATE_BODY(P, T, NV, RQ, PAIR_OUT, false)
}

// The paired kernels of a sequence that keeps Z in tower form (DESIGN.md
// section 3.1; rs16_pass_tower.hip instantiates them).  ENC_FIRST and ENC_LAST
// carry B's pools (read from the padding of the twiddle table's entry 0,
// uniform) beside their row requests; ENC_MID needs none.  The twiddle table
// of all three is the tower one (PassArgs::skew_tab, the engine's choice per
// sequence).  NV is ENC_MID's narrow variant; ENC_FIRST and ENC_LAST have no
// narrow layer, and their NV names the wide multiply of every layer instead:
// 0 the 12 lookups, 1 the three byte maps (process_item's WIDE3; launch_pass
// finds that kernel through PassKernel::wide3, not as a narrow variant).
template <int P, int T, bool PAIR> struct LateRowsTower : LateRows<P, T, PAIR> {
    TowerB tb;
    __device__ __forceinline__ LateRowsTower(const PassArgs& a, const Thr& c) : LateRows<P, T, PAIR>(a, c) {
        const cu32p q = (cu32p)a.skew_tab + TOWER_B_DWORD;
#pragma unroll
        for (int i = 0; i < 5; i++) tb.p[i] = q[i];
    }
};
template <int P, int T, int NV> __global__ void __launch_bounds__(Geo<T>::THREADS, 4) pass_kernel_late_tower(PassArgs a) {
    static_assert(P == ENC_FIRST || P == ENC_MID || P == ENC_LAST, "tower rows: the encoder's three passes");
    constexpr bool PAIR_IN = P != ENC_FIRST, PAIR_OUT = P != ENC_LAST;
    using G = Geo<T>;
    using RQ = typename std::conditional<P == ENC_MID, LateRows<P, T, PAIR_IN>, LateRowsTower<P, T, PAIR_IN>>::type;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    RS16_PASS_HEAD(P, T)
    RS16_LATE_BODY(P, T, NV, RQ, PAIR_OUT, true)
}

// ---------------------------------------------------------------------------
// What an instantiation unit builds its PassKernel lookup from: taking a
// kernel's address here is what instantiates it in that unit.
// ---------------------------------------------------------------------------
template <int P, int T, int NV> PassFn late_entry() {
    if constexpr (WaveStaged<P, T>::value) return pass_kernel_late<P, T, NV>;
    else return nullptr;
}
// the paired flavour of program P's late-rows kernel (ENC_FIRST writes paired
// rows, ENC_MID reads and writes them, ENC_LAST reads them)
template <int P, int T, int NV = 0> PassFn paired_entry() {
    static_assert(P == ENC_FIRST || P == ENC_MID || P == ENC_LAST, "paired rows: the encoder's three passes");
    return pass_kernel_late_paired<P, T, NV, P != ENC_FIRST, P != ENC_LAST>;
}
template <int P, int T, int NV = 0> PassKernel pass_entry() {
    using PT = ProgTraits<P>;
    return {pass_kernel<P, T, NV>, Smem<P, T>::BYTES, Geo<T>::THREADS, Geo<T>::Q,
            !PT::IFFT ? Geo<T>::SHB : 0, (!PT::FFT && T > 4) ? Geo<T>::SHB : 0, Geo<T>::R,
            PT::LOAD == LD_GATHER_ENC ? 1 : 0, {late_entry<P, T, NV>(), nullptr, nullptr}, nullptr};
}
// the 12-lookup kernels of program P at T = 0 .. 8
template <int P> PassKernel pass_row(int T) {
    static const PassKernel row[9] = {pass_entry<P, 0>(), pass_entry<P, 1>(), pass_entry<P, 2>(),
                                      pass_entry<P, 3>(), pass_entry<P, 4>(), pass_entry<P, 5>(),
                                      pass_entry<P, 6>(), pass_entry<P, 7>(), pass_entry<P, 8>()};
    return row[T];
}
// narrow variant NV of program P at T = 5 .. 8 (no such kernel below)
template <int P, int NV> PassKernel narrow_row(int T) {
    static const PassKernel row[4] = {pass_entry<P, 5, NV>(), pass_entry<P, 6, NV>(), pass_entry<P, 7, NV>(),
                                      pass_entry<P, 8, NV>()};
    return T >= 5 ? row[T - 5] : PassKernel{};
}

}  // namespace rs16
