// rs16_pass_repair.hip -- the pass kernels of the repair (rs16_repair_device):
// DEC_LAST_ALL at T = 4 .. 8 and DEC_SINGLE_ALL at T = 1 .. 8, the general
// decode's last pass and its one-pass form with the reveal and the stores
// extended to the lost rows of both segments (ST_RESTORE_ALL, rs16_pass.hpp).
// A unit of its own: the kernels of the other units compile as before.
#include "rs16_pass.hpp"

namespace rs16 {

// Rows [lo, hi) that lie in the 32-row word at `base`, as a bit mask.
__device__ __forceinline__ uint32_t rows_in_word(uint32_t base, uint32_t lo, uint32_t hi) {
    const uint32_t s = max(lo, base), e = min(hi, base + 32u);
    if (e <= s) return 0u;
    const uint32_t n = e - s;  // 1 .. 32
    return (n == 32u ? ~0u : (1u << n) - 1u) << (s - base);
}

// Does contiguous tile `tile` (rows [tile << T, (tile + 1) << T), lo = 0) hold
// a row the repair stores -- a row of segment A or B whose received bit is 0?
// From the received bitmap (at most 8 scalar dwords) and the segment bounds:
// the rows of neither segment have no bit either and are masked out.
template <int T> __device__ __forceinline__ bool tile_wanted(const PassArgs& a, uint32_t tile) {
    const uint32_t r0 = tile << T;
    const cu32p rb = (cu32p)a.rbits + (r0 >> 5);
    constexpr int NW = T > 5 ? 1 << (T - 5) : 1;
    uint32_t any = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
        const uint32_t base = (r0 & ~31u) + 32u * (uint32_t)w;
        uint32_t seg = rows_in_word(base, 0u, a.a_count) | rows_in_word(base, a.chunk, a.chunk + a.b_count);
        if constexpr (T < 5) seg &= rows_in_word(base, r0, r0 + (1u << T));
        any |= ~uni(rb[w]) & seg;
    }
    return any != 0;
}

// pass_kernel (rs16_pass.hpp) for the repair's two programs: the same head,
// staging, loads and item; the last pass returns before any load when its
// tile holds no row to store.  The interval of lost rows (PassArgs::lostrange)
// spans nearly every tile once rows of both segments are lost, so the test is
// per tile.
template <int P, int T>
__global__ void __launch_bounds__(Geo<T>::THREADS, (P == DEC_SINGLE_ALL ? 1 : 4)) pass_kernel_repair(PassArgs a) {
    using G = Geo<T>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    RS16_PASS_HEAD(P, T)
    if constexpr (P == DEC_LAST_ALL) {
        if (!tile_wanted<T>(a, tile)) return;
    }
    RS16_STAMP(a, 0);
    if constexpr (T >= 7) {
        // (load-issue order by workgroup slot, as pass_kernel)
        const uint32_t slot = (__builtin_amdgcn_s_getreg((31 << 11) | 4) >> 16) & 15u;
        if (slot == 0) __builtin_amdgcn_s_setprio(3);
        else if (slot == 1) __builtin_amdgcn_s_setprio(2);
        else if (slot == 2) __builtin_amdgcn_s_setprio(1);
    }
    TileStage<P, T> st;
    st.issue(a, c);
    constexpr bool EARLY = ProgTraits<P>::LOAD == LD_GATHER_DEC;
    if constexpr (EARLY) st.gather(a, c, smem);
    ItemRegs<P, T> cur;
    load_item<P, T>(a, c, tile, cur);
    RS16_STAMP(a, 1);
    prio<0>();
    st.template finish<EARLY>(a, c, smem);
    rcn.count();
    RS16_STAMP(a, 2);
    process_item<P, T, 0>(a, c, tile, cur, smem);
    rcn.store(a, c);
}

template <int P, int T> static PassKernel repair_entry() {
    using PT = ProgTraits<P>;
    return {pass_kernel_repair<P, T>, Smem<P, T>::BYTES, Geo<T>::THREADS, Geo<T>::Q,
            !PT::IFFT ? Geo<T>::SHB : 0, 0, Geo<T>::R, 0, {nullptr, nullptr, nullptr}, nullptr};
}

PassKernel pass_kernels_repair(int prog, int T) {
    if (prog == DEC_LAST_ALL) {
        switch (T) {
            case 4: return repair_entry<DEC_LAST_ALL, 4>();
            case 5: return repair_entry<DEC_LAST_ALL, 5>();
            case 6: return repair_entry<DEC_LAST_ALL, 6>();
            case 7: return repair_entry<DEC_LAST_ALL, 7>();
            case 8: return repair_entry<DEC_LAST_ALL, 8>();
            default: return {};
        }
    }
    if (prog == DEC_SINGLE_ALL) {
        switch (T) {
            case 1: return repair_entry<DEC_SINGLE_ALL, 1>();
            case 2: return repair_entry<DEC_SINGLE_ALL, 2>();
            case 3: return repair_entry<DEC_SINGLE_ALL, 3>();
            case 4: return repair_entry<DEC_SINGLE_ALL, 4>();
            case 5: return repair_entry<DEC_SINGLE_ALL, 5>();
            case 6: return repair_entry<DEC_SINGLE_ALL, 6>();
            case 7: return repair_entry<DEC_SINGLE_ALL, 7>();
            case 8: return repair_entry<DEC_SINGLE_ALL, 8>();
            default: return {};
        }
    }
    return {};
}

}  // namespace rs16
