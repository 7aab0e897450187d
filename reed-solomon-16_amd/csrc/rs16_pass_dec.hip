// rs16_pass_dec.hip -- the pass kernels of the decoder: DEC_FIRST, DEC_MID
// (with its narrow-twiddle variant), DEC_LAST, DEC_SINGLE, DEC_HALF_LAST and
// DEC_HALF_SINGLE at T = 0 .. 8, and the general decode's two small kernels
// with their launchers (rs16_pass_small.hpp).
#include "rs16_pass.hpp"
#include "rs16_pass_small.hpp"

namespace rs16 {

PassKernel pass_kernels_dec(int prog, int T, int nv) {
    if (prog == DEC_MID) {
        // DEC_MID runs at skew 0 in both directions, so it is narrow
        // everywhere (variant 1) or not at all
        if (nv == 0) return pass_row<DEC_MID>(T);
        return nv == 1 ? narrow_row<DEC_MID, 1>(T) : PassKernel{};
    }
    if (nv != 0) return {};
    switch (prog) {
        case DEC_FIRST: return pass_row<DEC_FIRST>(T);
        case DEC_LAST: return pass_row<DEC_LAST>(T);
        case DEC_SINGLE: return pass_row<DEC_SINGLE>(T);
        case DEC_HALF_LAST: return pass_row<DEC_HALF_LAST>(T);
        case DEC_HALF_SINGLE: return pass_row<DEC_HALF_SINGLE>(T);
        default: return {};
    }
}

}  // namespace rs16
