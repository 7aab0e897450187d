// rs16_pass_verify.hip -- the pass kernels of the scrub (rs16_verify_device):
// ENC_LAST_VFY at T = 4 .. 8 and ENC_SINGLE_VFY at T = 1 .. 8, the encoder's
// last pass and its one-pass form with the recovery stores replaced by a
// compare against the stored recovery shards (ST_VERIFY, rs16_pass.hpp
// verify_rows): the stored row is loaded where the computed one would be
// stored, and only flag bytes are written, where the two differ.  The work
// rows they read are in the shards' own form (Z_SHARD): the general kernel
// only, no wave-staged, late-rows, paired or tower flavour.  A unit of its
// own: the kernels of the other units compile as before.
#include "rs16_pass.hpp"

namespace rs16 {

// pass_kernel (rs16_pass.hpp) for the scrub's two programs: the same head,
// staging, loads and item.
template <int P, int T> __global__ void __launch_bounds__(Geo<T>::THREADS, 4) pass_kernel_verify(PassArgs a) {
    using G = Geo<T>;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    RS16_PASS_HEAD(P, T)
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
    ItemRegs<P, T> cur;
    load_item<P, T>(a, c, tile, cur);
    RS16_STAMP(a, 1);
    prio<0>();
    st.template finish<false>(a, c, smem);
    rcn.count();
    RS16_STAMP(a, 2);
    process_item<P, T, 0>(a, c, tile, cur, smem);
    rcn.store(a, c);
}

template <int P, int T> static PassKernel verify_entry() {
    using PT = ProgTraits<P>;
    return {pass_kernel_verify<P, T>, Smem<P, T>::BYTES, Geo<T>::THREADS, Geo<T>::Q,
            !PT::IFFT ? Geo<T>::SHB : 0, 0, Geo<T>::R, PT::LOAD == LD_GATHER_ENC ? 1 : 0,
            {nullptr, nullptr, nullptr}, nullptr};
}

PassKernel pass_kernels_verify(int prog, int T) {
    if (prog == ENC_LAST_VFY) {
        switch (T) {
            case 4: return verify_entry<ENC_LAST_VFY, 4>();
            case 5: return verify_entry<ENC_LAST_VFY, 5>();
            case 6: return verify_entry<ENC_LAST_VFY, 6>();
            case 7: return verify_entry<ENC_LAST_VFY, 7>();
            case 8: return verify_entry<ENC_LAST_VFY, 8>();
            default: return {};
        }
    }
    if (prog == ENC_SINGLE_VFY) {
        switch (T) {
            case 1: return verify_entry<ENC_SINGLE_VFY, 1>();
            case 2: return verify_entry<ENC_SINGLE_VFY, 2>();
            case 3: return verify_entry<ENC_SINGLE_VFY, 3>();
            case 4: return verify_entry<ENC_SINGLE_VFY, 4>();
            case 5: return verify_entry<ENC_SINGLE_VFY, 5>();
            case 6: return verify_entry<ENC_SINGLE_VFY, 6>();
            case 7: return verify_entry<ENC_SINGLE_VFY, 7>();
            case 8: return verify_entry<ENC_SINGLE_VFY, 8>();
            default: return {};
        }
    }
    return {};
}

}  // namespace rs16
