// rs16_elementwise.hip -- the elementwise engine ops of the MI355X GF(2^16)
// Reed-Solomon engine: mul, xor, the chunk XOR and copy of the multi-chunk
// encodes, the formal derivative.
#include <algorithm>

#include "rs16_internal.hpp"

namespace rs16 {

typedef const __attribute__((address_space(4))) uint32_t* cu32p;

// Engine::mul: x[] *= log_m (NoSimd::mul, src/engine/engine_nosimd.rs:65-79).
__global__ void __launch_bounds__(256) mul_kernel(uint8_t* x, size_t nquads, uint32_t entry, const uint32_t* mul_tab) {
    cu32p t = (cu32p)mul_tab + (size_t)entry * TAB_DWORDS;
    uint32_t tt[20];
#pragma unroll
    for (int i = 0; i < 20; i++) tt[i] = t[i];
    for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < nquads; q += (size_t)gridDim.x * blockDim.x) {
        const size_t off = (q >> 3) * 64 + (q & 7) * 4;
        uint32_t yl = *(uint32_t*)(x + off), yh = *(uint32_t*)(x + off + 32);
        uint32_t ol = 0, oh = 0;
        mul_xor(ol, oh, yl, yh, tt);
        *(uint32_t*)(x + off) = ol;
        *(uint32_t*)(x + off + 32) = oh;
    }
}
hipError_t launch_mul(uint8_t* x, size_t bytes, uint32_t entry, const uint32_t* mul_tab, hipStream_t s) {
    const size_t nq = bytes / 8;
    if (!nq) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((nq + 255) / 256, 4096);
    hipLaunchKernelGGL(mul_kernel, dim3(grid), dim3(256), 0, s, x, nq, entry, mul_tab);
    return hipGetLastError();
}

// Engine::xor: x[] ^= y[] (src/engine/engine_nosimd.rs:81-88), 16 B per lane.
__global__ void __launch_bounds__(256) xor_kernel(uint4* x, const uint4* y, size_t n16) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) {
        uint4 a = x[i], b = y[i];
        x[i] = make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w);
    }
}
hipError_t launch_xor(uint8_t* x, const uint8_t* y, size_t bytes, hipStream_t s) {
    const size_t n16 = bytes / 16;
    if (!n16) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((n16 + 255) / 256, 8192);
    hipLaunchKernelGGL(xor_kernel, dim3(grid), dim3(256), 0, s, (uint4*)x, (const uint4*)y, n16);
    return hipGetLastError();
}

// Multi-chunk encodes: w[0, cb) ^= XOR of the nch - 1 chunks behind it
// (HighRateEncoder's xor_within accumulation, src/rate/rate_high.rs:56-74),
// and chunk 0 copied into chunks 1 .. nch - 1 (LowRateEncoder's per-chunk
// copy of the transformed originals, src/rate/rate_low.rs:56-74); 16 B per lane.
__global__ void __launch_bounds__(256) xor_chunks_kernel(uint4* w, size_t c16, uint32_t nch) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < c16; i += (size_t)gridDim.x * blockDim.x) {
        uint4 a = w[i];
        for (uint32_t c = 1; c < nch; c++) {
            const uint4 b = w[c * c16 + i];
            a.x ^= b.x; a.y ^= b.y; a.z ^= b.z; a.w ^= b.w;
        }
        w[i] = a;
    }
}
__global__ void __launch_bounds__(256) copy_chunks_kernel(uint4* w, size_t c16, uint32_t nch) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < c16; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 a = w[i];
        for (uint32_t c = 1; c < nch; c++) w[c * c16 + i] = a;
    }
}
hipError_t launch_xor_chunks(uint8_t* w, size_t chunk_bytes, uint32_t nch, hipStream_t s) {
    const size_t c16 = chunk_bytes / 16;
    if (!c16 || nch < 2) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((c16 + 255) / 256, 8192);
    hipLaunchKernelGGL(xor_chunks_kernel, dim3(grid), dim3(256), 0, s, (uint4*)w, c16, nch);
    return hipGetLastError();
}
hipError_t launch_copy_chunks(uint8_t* w, size_t chunk_bytes, uint32_t nch, hipStream_t s) {
    const size_t c16 = chunk_bytes / 16;
    if (!c16 || nch < 2) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((c16 + 255) / 256, 8192);
    hipLaunchKernelGGL(copy_chunks_kernel, dim3(grid), dim3(256), 0, s, (uint4*)w, c16, nch);
    return hipGetLastError();
}

// Engine::formal_derivative (src/engine.rs:233-238), closed form, out of place:
// out[j] = in[j] ^ XOR_{b : j_b = 0, 2^b < n} in[j | 2^b]   (n a power of two).
__global__ void __launch_bounds__(256) fd_kernel(uint4* out, const uint4* in, uint32_t n, size_t row16) {
    const size_t total = (size_t)n * row16;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const uint32_t j = (uint32_t)(i / row16);
        const size_t col = i - (size_t)j * row16;
        uint4 acc = in[i];
        for (uint32_t b = 1; b < n; b <<= 1)
            if (!(j & b)) {
                uint4 v = in[(size_t)(j | b) * row16 + col];
                acc.x ^= v.x; acc.y ^= v.y; acc.z ^= v.z; acc.w ^= v.w;
            }
        out[i] = acc;
    }
}
hipError_t launch_formal_derivative(uint8_t* out, const uint8_t* in, size_t n, size_t S, hipStream_t s) {
    const size_t row16 = S / 16, total = n * row16;
    if (!total) return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(fd_kernel, dim3(grid), dim3(256), 0, s, (uint4*)out, (const uint4*)in, (uint32_t)n, row16);
    return hipGetLastError();
}

}  // namespace rs16
