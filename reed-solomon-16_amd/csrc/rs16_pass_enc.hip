// rs16_pass_enc.hip -- the pass kernels of the encoder and of the plain
// transforms: GEN_FFT, GEN_IFFT, ENC_FIRST, ENC_MID (with its narrow-twiddle
// variants), ENC_LAST and ENC_SINGLE at T = 0 .. 8, and the paired-rows
// flavours of the late-rows ENC_FIRST / ENC_MID / ENC_LAST kernels.  (Encoder
// and decoder programs in one unit each: see the Makefile on why not finer.)
#include "rs16_pass.hpp"

namespace rs16 {

// The paired-rows flavours (pass_kernel_late with PAIR_IN / PAIR_OUT), only
// for the kernels a paired sequence can launch: three late-rows passes exist
// for chunks of 2^14 rows (T = 7 / 7 / 7) and 2^15 rows (7 / 8 / 7).
PassFn pass_kernels_paired(int prog, int T, int nv) {
    if (prog == ENC_FIRST && T == 7 && nv == 0) return paired_entry<ENC_FIRST, 7>();
    if (prog == ENC_LAST && T == 7 && nv == 0) return paired_entry<ENC_LAST, 7>();
    if (prog == ENC_MID && T == 7) {
        if (nv == 0) return paired_entry<ENC_MID, 7, 0>();
        if (nv == 1) return paired_entry<ENC_MID, 7, 1>();
    }
    if (prog == ENC_MID && T == 8) {
        switch (nv) {
            case 0: return paired_entry<ENC_MID, 8, 0>();
            case 1: return paired_entry<ENC_MID, 8, 1>();
            case 2: return paired_entry<ENC_MID, 8, 2>();
            case 3: return paired_entry<ENC_MID, 8, 3>();
        }
    }
    return nullptr;
}

PassKernel pass_kernels_enc(int prog, int T, int nv) {
    if (prog == ENC_MID) {
        switch (nv) {
            case 0: return pass_row<ENC_MID>(T);
            case 1: return narrow_row<ENC_MID, 1>(T);
            // variants 2 / 3 are needed with 2^15-row stripes only (T = 8):
            // below, the launch takes a variant that assumes less
            case 2: return T == 8 ? pass_entry<ENC_MID, 8, 2>() : PassKernel{};
            case 3: return T == 8 ? pass_entry<ENC_MID, 8, 3>() : PassKernel{};
            default: return {};
        }
    }
    if (nv != 0) return {};
    switch (prog) {
        case GEN_FFT: return pass_row<GEN_FFT>(T);
        case GEN_IFFT: return pass_row<GEN_IFFT>(T);
        case ENC_FIRST: return pass_row<ENC_FIRST>(T);
        case ENC_LAST: return pass_row<ENC_LAST>(T);
        case ENC_SINGLE: return pass_row<ENC_SINGLE>(T);
        default: return {};
    }
}

}  // namespace rs16
