// rs16_pass_select.hip -- the kernels of the selective decode
// (rs16_decode_device_select): DEC_LAST_SEL at T = 4 .. 8 and DEC_SINGLE_SEL at
// T = 1 .. 8, the general decode's last pass and its one-pass form, and
// tile_last_sel_kernel, tile_last_kernel's form -- each with the reveal and the
// stores narrowed to the lost originals whose byte of the read set is nonzero
// (ST_RESTORE_SEL, rs16_pass.hpp; row_wanted<ROWS_SEL>).  The row interval the
// kernels prune by (PassArgs::lostrange) is the eval kernels', taken over the
// same rows (ErasureSpec::wanted).  A unit of its own: the kernels of the other
// units compile as before.
#include "rs16_pass.hpp"
#include "rs16_colops.hpp"

namespace rs16 {

// pass_kernel (rs16_pass.hpp) for the selective decode's two programs: the
// same head, early returns, staging, loads and item.  The last pass keeps both
// of DEC_LAST's returns before any load -- a tile outside the wanted rows'
// interval, and a stripe whose few tiles tile_last_sel_kernel took.
template <int P, int T>
__global__ void __launch_bounds__(Geo<T>::THREADS, (P == DEC_SINGLE_SEL ? 1 : 4)) pass_kernel_select(PassArgs a) {
    using G = Geo<T>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    RS16_PASS_HEAD(P, T)
    if constexpr (P == DEC_LAST_SEL) {
        if (a.lostrange) {
            const uint32_t r0 = ((cu32p)a.lostrange)[0], r1 = ((cu32p)a.lostrange)[1];
            if (!((tile << T) < r1 && ((tile + 1) << T) > r0)) return;
            if (a.tl_max && tl_covers<T>(a)) return;
        }
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

template <int P, int T> static PassKernel select_entry() {
    using PT = ProgTraits<P>;
    return {pass_kernel_select<P, T>, Smem<P, T>::BYTES, Geo<T>::THREADS, Geo<T>::Q,
            !PT::IFFT ? Geo<T>::SHB : 0, 0, Geo<T>::R, 0, {nullptr, nullptr, nullptr}, nullptr};
}

PassKernel pass_kernels_select(int prog, int T) {
    if (prog == DEC_LAST_SEL) {
        switch (T) {
            case 4: return select_entry<DEC_LAST_SEL, 4>();
            case 5: return select_entry<DEC_LAST_SEL, 5>();
            case 6: return select_entry<DEC_LAST_SEL, 6>();
            case 7: return select_entry<DEC_LAST_SEL, 7>();
            case 8: return select_entry<DEC_LAST_SEL, 8>();
            default: return {};
        }
    }
    if (prog == DEC_SINGLE_SEL) {
        switch (T) {
            case 1: return select_entry<DEC_SINGLE_SEL, 1>();
            case 2: return select_entry<DEC_SINGLE_SEL, 2>();
            case 3: return select_entry<DEC_SINGLE_SEL, 3>();
            case 4: return select_entry<DEC_SINGLE_SEL, 4>();
            case 5: return select_entry<DEC_SINGLE_SEL, 5>();
            case 6: return select_entry<DEC_SINGLE_SEL, 6>();
            case 7: return select_entry<DEC_SINGLE_SEL, 7>();
            case 8: return select_entry<DEC_SINGLE_SEL, 8>();
            default: return {};
        }
    }
    return {};
}

// tile_last_kernel (rs16_pass_small.hpp) with the select rule: lost[], the
// reveal table choice and the stores follow "lost and wanted".
__global__ void __launch_bounds__(256) tile_last_sel_kernel(PassArgs a) {
    constexpr int RULE = ROWS_SEL;
#include "rs16_tile_last.inc"
}

// As launch_tile_last; the read set must be there.
hipError_t launch_tile_last_sel(const PassArgs& a, uint32_t num_tiles, hipStream_t s) {
    if (!a.wanted || (a.lostrange && a.tl_max == 0)) return hipErrorInvalidValue;
    if (num_tiles == 0 || a.qrow == 0) return hipSuccess;
    const uint32_t nwg = num_tiles * ((a.qrow + 3) / 4);
    hipLaunchKernelGGL(tile_last_sel_kernel, dim3(nwg), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace rs16
