// rs16_pass_enc.hip -- the pass kernels of the encoder and of the plain
// transforms: GEN_FFT, GEN_IFFT, ENC_FIRST, ENC_MID (with its narrow-twiddle
// variants), ENC_LAST and ENC_SINGLE at T = 0 .. 8.  (Encoder and decoder
// programs in one unit each: see the Makefile on why not finer.)
#include "rs16_pass.hpp"

namespace rs16 {

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
