// rs16_pass_tower.hip -- the tower flavours of the paired late-rows pass
// kernels (pass_kernel_late_tower, rs16_pass.hpp): the kernels of a sequence
// that keeps the work buffer's rows in tower form.
// One for every kernel a paired sequence can launch (rs16_pass_enc.hip,
// pass_kernels_paired).  A unit of its own: the kernels of the other units compile
// to the code they had without it (Makefile).
#include "rs16_pass.hpp"

namespace rs16 {

PassFn pass_kernels_tower(int prog, int T, int nv) {
    if (prog == ENC_FIRST && T == 7 && nv == 0) return pass_kernel_late_tower<ENC_FIRST, 7, 0>;
    if (prog == ENC_LAST && T == 7 && nv == 0) return pass_kernel_late_tower<ENC_LAST, 7, 0>;
    if (prog == ENC_MID && T == 7) {
        if (nv == 0) return pass_kernel_late_tower<ENC_MID, 7, 0>;
        if (nv == 1) return pass_kernel_late_tower<ENC_MID, 7, 1>;
    }
    if (prog == ENC_MID && T == 8) {
        switch (nv) {
            case 0: return pass_kernel_late_tower<ENC_MID, 8, 0>;
            case 1: return pass_kernel_late_tower<ENC_MID, 8, 1>;
            case 2: return pass_kernel_late_tower<ENC_MID, 8, 2>;
            case 3: return pass_kernel_late_tower<ENC_MID, 8, 3>;
        }
    }
    return nullptr;
}

// The first and last pass with the wide multiply by three byte maps (their
// third template argument is that choice, not a narrow variant: rs16_pass.hpp).
PassFn pass_kernel_tower_wide3(int prog, int T) {
    if (prog == ENC_FIRST && T == 7) return pass_kernel_late_tower<ENC_FIRST, 7, 1>;
    if (prog == ENC_LAST && T == 7) return pass_kernel_late_tower<ENC_LAST, 7, 1>;
    return nullptr;
}

}  // namespace rs16
