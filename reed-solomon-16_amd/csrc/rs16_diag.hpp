// rs16_diag.hpp -- diagnostics hooks of the kernels (not product code).
//
// Phase timelines for scripts/stamps.py: a library built with
// -DRS16_STAMPS=1 (never the shipped one) makes thread 0 of every workgroup
// store s_memtime at phase i to stamps[block * 16 + i] of the launch
// arguments' `stamps` buffer (rs16_engine_set_stamps); slot 14 / 15 hold
// s_memrealtime at the start / end (for the clock), 12 / 13 the HW_ID and
// XCC_ID registers.  In every other build the hooks are empty macros, so the
// shipped kernels contain no trace of them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef RS16_STAMPS
#define RS16_STAMPS 0
#endif

// Prologue depth of the late-rows pass kernels (rs16_pass.hpp LateRows): a
// library built with -DRS16_LATE_DEPTH=n (n = 2, 4, 8; never the shipped one)
// requests n row pairs ahead of the table commit in every program, for the
// depth measurements.  0: each program's shipped depth (LateDepth).  Which
// launches take those kernels at all is a run-time switch of one build:
// RS16_DIAG_NO_LATE_ROWS (rs16_engine_set_diagnostics) forces pass_kernel.
#ifndef RS16_LATE_DEPTH
#define RS16_LATE_DEPTH 0
#endif

#if RS16_STAMPS
namespace rs16 {
template <class Args>
__device__ __forceinline__ void diag_stamp(const Args& a, int i) {
    if (a.stamps && threadIdx.x == 0) {
        uint64_t* p = a.stamps + blockIdx.x * 16;
        p[i] = __builtin_amdgcn_s_memtime();
        if (i == 0) {
            p[14] = __builtin_amdgcn_s_memrealtime();
            p[12] = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID
            p[13] = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // XCC_ID
        }
        if (i == 11) p[15] = __builtin_amdgcn_s_memrealtime();
    }
}
}  // namespace rs16
// phase i reached
#define RS16_STAMP(args, i) ::rs16::diag_stamp((args), (i))
// the workgroup's stores have completed (phase 11)
#define RS16_STAMP_END(args)                \
    do {                                    \
        __builtin_amdgcn_s_waitcnt(0);      \
        ::rs16::diag_stamp((args), 11);     \
    } while (0)
// phase i reached once the rows m and m2 of the wave's first butterfly are in
// its registers (the wave-staged passes: slot 6, which only the decoder's
// formal derivative uses otherwise)
#define RS16_STAMP_ROWS(args, i, L, H, m, m2)                                            \
    do {                                                                                 \
        asm volatile("" : "+v"((L)[m]), "+v"((H)[m]), "+v"((L)[m2]), "+v"((H)[m2]));      \
        ::rs16::diag_stamp((args), (i));                                                 \
    } while (0)
#else
#define RS16_STAMP(args, i) ((void)0)
#define RS16_STAMP_ROWS(args, i, L, H, m, m2) ((void)0)
#define RS16_STAMP_END(args) ((void)0)
#endif
