// rs16_verify_cmp.hip -- the compare kernel of the scrub's encode + compare
// path (rs16_verify_device where the engine's encode does not end in a pass
// with a comparing form): the engine encodes the stripe into a buffer of its
// own and this kernel compares it with the stored recovery shards, writing
// flag bytes only.  A unit of its own, so the kernels of the other units
// compile as before.
#include "rs16_internal.hpp"

namespace rs16 {

// One wave per row, four rows per workgroup (grid x), stripes over grid y
// (strided when there are more stripes than grid rows), as repair_copy_kernel.
// A row whose byte of the check set is 0 is not read: its wave returns on a
// scalar test of that byte.  16-byte accesses per lane (rows are multiples of
// 64 bytes and 64-byte aligned): vector v of a row lies in 64-byte block v >>
// 2.  Each lane ORs the XORs of its vectors and stores the row's flag once per
// stripe when the OR is nonzero, and the flag of each block it found a
// difference in; every store is the byte 1.
__global__ void __launch_bounds__(256) verify_cmp_kernel(const uint8_t* enc, const uint8_t* rec,
                                                         const uint8_t* checked, uint8_t* row_flags,
                                                         uint8_t* col_flags, uint32_t rows, uint64_t S,
                                                         uint64_t bs_enc, uint64_t bs_rec, uint64_t bs_rows,
                                                         uint64_t bs_cols, uint32_t nstripes) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t row = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    if (row >= rows || (checked && checked[row] == 0)) return;
    const uint64_t nvec = S / 16;
    for (uint32_t st = blockIdx.y; st < nstripes; st += gridDim.y) {
        const uint4* e4 = (const uint4*)(enc + st * bs_enc + (uint64_t)row * S);
        const uint4* r4 = (const uint4*)(rec + st * bs_rec + (uint64_t)row * S);
        uint32_t any = 0;
        for (uint64_t v = lane; v < nvec; v += 64) {
            const uint4 x = e4[v], y = r4[v];
            const uint32_t d = (x.x ^ y.x) | (x.y ^ y.y) | (x.z ^ y.z) | (x.w ^ y.w);
            any |= d;
            if (d && col_flags) col_flags[st * bs_cols + (v >> 2)] = 1;
        }
        if (any) row_flags[st * bs_rows + row] = 1;
    }
}

hipError_t launch_verify_cmp(const uint8_t* enc, const uint8_t* rec, const uint8_t* checked, uint8_t* row_flags,
                             uint8_t* col_flags, uint32_t rows, uint64_t S, uint64_t bs_enc, uint64_t bs_rec,
                             uint64_t bs_rows, uint64_t bs_cols, uint32_t nstripes, hipStream_t s) {
    if (rows == 0 || nstripes == 0 || S == 0) return hipSuccess;
    if (S % 16 || !enc || !rec || !row_flags) return hipErrorInvalidValue;
    dim3 grid((rows + 3) / 4, nstripes < 65535u ? nstripes : 65535u), block(256);
    hipLaunchKernelGGL(verify_cmp_kernel, grid, block, 0, s, enc, rec, checked, row_flags, col_flags, rows, S, bs_enc,
                       bs_rec, bs_rows, bs_cols, nstripes);
    return hipGetLastError();
}

}  // namespace rs16
