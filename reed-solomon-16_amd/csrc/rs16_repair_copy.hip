// rs16_repair_copy.hip -- the copy kernel of the repair's recovery-only path
// (rs16_repair_device with no original lost): the engine encodes the whole
// stripe into a buffer of its own and this kernel copies the rows whose
// received flag is 0 into the caller's recovery array.  A unit of its own, so
// the kernels of the other units compile as before.
#include "rs16_internal.hpp"

namespace rs16 {

// One wave per row, four rows per workgroup (grid x), stripes over grid y
// (strided when there are more stripes than grid rows).  A received row's
// wave returns on a scalar test of its flag byte -- any nonzero value means
// received; a lost row is copied in 16-byte accesses per lane (rows are
// multiples of 64 bytes and 64-byte aligned).
__global__ void __launch_bounds__(256) repair_copy_kernel(uint8_t* dst, const uint8_t* src, const uint8_t* flags,
                                                          uint32_t rows, uint64_t S, uint64_t bs_dst,
                                                          uint64_t bs_src, uint32_t nstripes) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t row = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (row >= rows || flags[row] != 0) return;
    const uint64_t nvec = S / 16;
    for (uint32_t st = blockIdx.y; st < nstripes; st += gridDim.y) {
        const uint4* s4 = (const uint4*)(src + st * bs_src + (uint64_t)row * S);
        uint4* d4 = (uint4*)(dst + st * bs_dst + (uint64_t)row * S);
        for (uint64_t v = lane; v < nvec; v += 64) d4[v] = s4[v];
    }
}

hipError_t launch_repair_copy(uint8_t* dst, const uint8_t* src, const uint8_t* flags, uint32_t rows, uint64_t S,
                              uint64_t bs_dst, uint64_t bs_src, uint32_t nstripes, hipStream_t s) {
    if (rows == 0 || nstripes == 0 || S == 0) return hipSuccess;
    if (S % 16) return hipErrorInvalidValue;
    dim3 grid((rows + 3) / 4, nstripes < 65535u ? nstripes : 65535u), block(256);
    hipLaunchKernelGGL(repair_copy_kernel, grid, block, 0, s, dst, src, flags, rows, S, bs_dst, bs_src, nstripes);
    return hipGetLastError();
}

}  // namespace rs16
