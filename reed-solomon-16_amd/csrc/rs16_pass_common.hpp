// rs16_pass_common.hpp -- what the pass kernels' translation units share: the
// device-side readers of the launch arguments' decode metadata, used by the
// pass template (rs16_pass.hpp) and by the two small kernels of the general
// decode (rs16_pass_small.hpp), and the host-side lookup through which
// launch_pass (rs16_pass_launch.hip) finds the kernels of the instantiation
// units.  Every kernel lives wholly in one unit (no relocatable device code).
#pragma once
#include "rs16_internal.hpp"

namespace rs16 {

// ---------------------------------------------------------------------------
// Host side: the kernel of (prog, T, narrow variant) and its launch shape.
// ---------------------------------------------------------------------------
typedef void (*PassFn)(PassArgs);
struct PassKernel {
    PassFn fn;     // nullptr: this unit has no such kernel
    int lds;       // dynamic LDS bytes (Smem<P, T>::BYTES)
    int threads;   // Geo<T>::THREADS
    int quads;     // Geo<T>::Q, quads per tile row
    // layout of the rows at the loads / at the stores: 0 = A (consecutive row
    // registers are 1 << lo rows apart), else B (1 << (lo + SHB)): SHB
    int load_shb, store_shb;
    int reg_bits;  // Geo<T>::R, row bits held in registers (2^R rows per thread)
    // Whether the pass gathers its rows below the row limit a_count (ENC_FIRST).
    int gather;
    // The late-rows variants of a wave-staged pass (rs16_pass.hpp) by ZForm
    // (nullptr: none).  Z_SHARD: pass_kernel_late.  Z_PAIRED:
    // pass_kernel_late_paired -- ENC_FIRST writes the work buffer's rows in
    // the paired form, ENC_MID reads and writes them, ENC_LAST reads them;
    // only the kernels a paired sequence can launch exist.  Z_TOWER:
    // pass_kernel_late_tower, the same in tower form.  The last two are
    // filled in by launch_pass's kernel table, each from its own lookup.
    PassFn late[3];
    // The tower flavour that multiplies by three byte maps in every layer
    // (ENC_FIRST / ENC_LAST; nullptr: none): what a
    // tower sequence launches instead of late[Z_TOWER], which keeps the 12
    // lookups (RS16_DIAG_WIDE_TWIDDLES).  Filled in like late[1 ..].
    PassFn wide3;
};
// The launch constants that decide a launch's address forms (the PassArgs
// fields of the same names), as launch_pass sets them from the kernel's
// geometry and the launch's strides, slice width, stride exponent, row
// alignment and diag flags.  Host arithmetic only: rs16_host_pass_consts
// (include/rs16.h) shows it to tests without a device.
// late_rows: the launch takes the kernel's late-rows variant -- no wave of it
// can be ROWS_GENERAL (rs16_pass.hpp wave_rows_mode).
struct PassConsts {
    uint32_t nslab, voff32, full_lanes;
    uint64_t rs_in, rs_seg, rs_out;
    uint32_t late_rows;
};
PassConsts pass_launch_consts(const PassKernel& k, int T, const PassArgs& a);
// The 12-lookup kernel of (prog, T) (fn nullptr: none), whose geometry every
// narrow variant of (prog, T) shares.
const PassKernel& pass_kernel_of(int prog, int T);
// Narrow-twiddle variants of the two-direction middle passes (NarrowVar,
// rs16_pass.hpp): nv = 0 is the 12-lookup kernel that every (prog, T) has.
constexpr int NARROW_VARIANTS = 4;
// One lookup per instantiation unit, each covering the programs named in its
// file; prog in [0, NUM_PROGS), T in [0, 8], nv in [0, NARROW_VARIANTS).
PassKernel pass_kernels_enc(int prog, int T, int nv);  // rs16_pass_enc.hip: GEN_*, ENC_*
PassFn pass_kernels_paired(int prog, int T, int nv);   // rs16_pass_enc.hip: the paired flavours (nullptr: none)
PassKernel pass_kernels_dec(int prog, int T, int nv);  // rs16_pass_dec.hip: DEC_*
PassFn pass_kernels_tower(int prog, int T, int nv);    // rs16_pass_tower.hip: the tower flavours (nullptr: none)
PassFn pass_kernel_tower_wide3(int prog, int T);       // rs16_pass_tower.hip: PassKernel::wide3 (nullptr: none)
PassKernel pass_kernels_repair(int prog, int T);       // rs16_pass_repair.hip: DEC_LAST_ALL, DEC_SINGLE_ALL (no narrow variants)
PassKernel pass_kernels_select(int prog, int T);       // rs16_pass_select.hip: DEC_LAST_SEL, DEC_SINGLE_SEL (no narrow variants)
PassKernel pass_kernels_verify(int prog, int T);       // rs16_pass_verify.hip: ENC_LAST_VFY, ENC_SINGLE_VFY (no narrow variants)

#if defined(__HIPCC__) || defined(__HIP__)
// ---------------------------------------------------------------------------
// Device side.
// ---------------------------------------------------------------------------
typedef const __attribute__((address_space(4))) uint32_t* cu32p;

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

// s_waitcnt immediate (gfx9 encoding) that waits for vmcnt <= n only
// (expcnt and lgkmcnt at their maxima, i.e. not waited for).
__host__ __device__ constexpr int vmcnt_wait(int n) { return (n & 15) | ((n >> 4) << 14) | (7 << 4) | (15 << 8); }

__device__ __forceinline__ void load_table_lds(uint32_t (&t)[20], const uint4* p) {
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const uint4 v = p[i];
        t[4 * i] = v.x;
        t[4 * i + 1] = v.y;
        t[4 * i + 2] = v.z;
        t[4 * i + 3] = v.w;
    }
}

// Batched stripes (PassArgs::stripe_tiles): stripe st reads and writes its
// own arrays, and -- stripes with losses of their own -- its own flags and
// decode metadata (all of those strides 0 when the stripes share one erasure
// pattern).  Every kernel displaces every field; the ones it never reads fold
// away.
__device__ __forceinline__ void stripe_displace(PassArgs& a, uint32_t st) {
    a.in += st * a.bs_in;
    a.in2 += st * a.bs_in2;
    a.out += st * a.bs_out;
    a.seg_a += st * a.bs_seg;
    a.seg_b += st * a.bs_seg_b;
    a.rest += st * a.bs_rest;
    a.rest_b += st * a.bs_rest_b;
    if (a.wanted) a.wanted += st * a.bs_wanted;
    if (a.flags_a) a.flags_a += st * a.bs_fa;
    if (a.flags_b) a.flags_b += st * a.bs_fb;
    if (a.elog) a.elog += st * a.bs_elog;
    if (a.ework) a.ework += st * a.bs_elog;
    if (a.rbits) a.rbits += st * a.bs_rbits;
    if (a.zflags) a.zflags += st * a.bs_zflags;
    if (a.lostrange) a.lostrange += st * a.bs_lost;
}

// Decode zero tiles: zflags[tile] = 1 when DEC_FIRST tile `tile` holds no
// received row (a.zflags not null; one scalar load of the flag's word).
__device__ __forceinline__ bool tile_is_zero(const PassArgs& a, uint32_t tile) {
    return (((cu32p)a.zflags)[tile >> 2] >> (8 * (tile & 3))) & 1u;
}
// The decode's lost originals are rows [r0, r1) (a.lostrange not null;
// r0 >= r1: none).
__device__ __forceinline__ void lost_range(const PassArgs& a, uint32_t& r0, uint32_t& r1) {
    r0 = ((cu32p)a.lostrange)[0];
    r1 = ((cu32p)a.lostrange)[1];
}

// The last pass's lost-original tiles (2^T rows each) span at most tl_max
// tiles: tile_last_kernel is the last pass of the stripe (else DEC_LAST).
template <int T> __device__ __forceinline__ bool tl_covers(const PassArgs& a) {
    uint32_t r0, r1;
    lost_range(a, r0, r1);
    return r0 < r1 && ((r1 - 1) >> T) - (r0 >> T) < a.tl_max;
}

// The consumed U rows [nlo, nhi) of the general decode's middle pass, when
// at most MID_DIRECT_MAX (mid_direct_kernel: the direct product).
__device__ __forceinline__ bool mid_need(const PassArgs& a, uint32_t& nlo, uint32_t& nhi) {
    uint32_t r0, r1;
    lost_range(a, r0, r1);
    if (r0 >= r1) return false;
    nlo = max(a.need_lo, r0 >> a.lo);
    nhi = min(a.need_hi, ((r1 - 1) >> a.lo) + 1);
    return nhi > nlo && nhi - nlo <= MID_DIRECT_MAX;
}

// Lost original?  (the rows the decoder reveals)
__device__ __forceinline__ bool row_lost_original(const PassArgs& a, uint32_t r) {
    const uint32_t base = a.rest_seg_b ? a.chunk : 0;
    const uint32_t cnt = a.rest_seg_b ? a.b_count : a.a_count;
    const uint8_t* fl = a.rest_seg_b ? a.flags_b : a.flags_a;
    return r >= base && r - base < cnt && fl && !fl[r - base];
}
// A row the pass reveals and stores, by the program's rule: a lost original
// (ROWS_LOST); a row of either segment without a received flag (ROWS_ALL, the
// repair's programs); a lost original whose byte of the read set is nonzero
// (ROWS_SEL, the selective decode's programs -- the byte is read only for a
// lost original, so never outside the read set's [0, original count)).
enum RowRule : int { ROWS_LOST = 0, ROWS_ALL, ROWS_SEL };
template <int RULE> __device__ __forceinline__ bool row_wanted(const PassArgs& a, uint32_t r) {
    if constexpr (RULE == ROWS_LOST) return row_lost_original(a, r);
    if constexpr (RULE == ROWS_SEL)
        return row_lost_original(a, r) && a.wanted[r - (a.rest_seg_b ? a.chunk : 0)] != 0;
    if (r < a.a_count) return a.flags_a && !a.flags_a[r];
    return r >= a.chunk && r - a.chunk < a.b_count && a.flags_b && !a.flags_b[r - a.chunk];
}
#endif

}  // namespace rs16
