// rs16_update_batch.hip -- delta update of a column window of the recovery
// shards of a batch of stripes in one launch (rs16_update_device_batch,
// DESIGN.md 3.22).  The sum is rs16_update.hip's,
//   rec[i][j] ^= sum_e tab[idx[j][e]] . delta[i][e]   for stripe i,
// on (L, H) quads (rs16_gf.hpp); idx, the plan's m x n array of d_mul_tab
// entries, is the same for every stripe of a geometry.  Every 64-byte column
// block is a codeword of its own, so a window of `width` bytes of every row is
// updated by itself: the rows of the deltas and of the recovery shards each
// have their own pitch, and the stripes their own strides.
//
// A unit of its own: update_kernel (rs16_update.hip) shares no translation
// unit with it and keeps its machine code (scripts/isa_compare.py).
#include <algorithm>
#include <type_traits>

#include "rs16_internal.hpp"

namespace rs16 {

typedef const __attribute__((address_space(4))) uint32_t* cu32p;
// The table groups, the selectors kept in registers and the two quads per lane
// follow rs16_update.hip's numbers (measured there, profiles/r08_update.txt).
constexpr int UPDATE_BATCH_TABLE_GROUP = 4;
constexpr int UPDATE_BATCH_HOIST_QUADS = 16;
constexpr uint32_t UPDATE_BATCH_Q2_MIN_QROW = 128;
constexpr int UPDATE_BATCH_Q2_MAX_N = UPDATE_BATCH_HOIST_QUADS / 2;
// Windows of at most this many quads (128 bytes: four stripes a wave or more)
// of at least two stripes take the packed form.  With 32 (256 bytes, two
// stripes a wave) it lost to the unpacked form at n = 1 in every pair
// (profiles/r22_update_batch_pack256_rejected.txt).
// (-DRS16_UPDATE_BATCH_PACK_QROW=0 builds the library without the packed
// form: scripts/probe_update_batch.py measures one against the other.)
#ifndef RS16_UPDATE_BATCH_PACK_QROW
#define RS16_UPDATE_BATCH_PACK_QROW 16
#endif
constexpr uint32_t UPDATE_BATCH_PACK_QROW = RS16_UPDATE_BATCH_PACK_QROW;

// update_kernel's schedule (rs16_update.hip): a wave owns a slab of 64 Q quad
// columns of a run of rows_per_wave recovery rows, keeps the n delta quads (or
// their selectors) of its columns in registers, asks for every row one row
// ahead of its multiplies, gets the tables of (row, e) in groups of four over
// the scalar path and stores with plain stores.  What differs:
//
// - The wave's stripe (PACK: its group of stripes_per_wave stripes) is part
//   of its index: wave w is slab w mod nslab of stripe (w / nslab) mod ngroups
//   of run w / (nslab ngroups).  The four waves of a workgroup and the
//   workgroups next to it work on the same recovery rows of neighbouring
//   stripes, and so on the same table lines, which they find in their CU's
//   scalar cache.
// - Row bases are 64-bit scalars from the stripe's stride and the rows' pitch;
//   a lane's offset inside the window is 32 bits (width < 4 GiB).
// - PACK (qrow <= 16, Q = 1, one slab): lane l works on quad l mod qrow of
//   stripe l / qrow of the wave's group, the stripe's stride inside the lane's
//   64-bit offset; the table is still the whole wave's.  Lanes of a last,
//   partial group repeat the group's first stripe, lanes beyond
//   stripes_per_wave qrow repeat lane 0: the same loads and multiplies give
//   the same value, stored to the same place, and nothing is conditional.
template <int N, int Q, bool PACK>
__global__ void __launch_bounds__(256) update_batch_kernel(UpdateBatchArgs a) {
    static_assert(!PACK || Q == 1, "the packed form has one quad per lane");
    typedef std::conditional_t<PACK, uint64_t, uint32_t> Off;
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const uint32_t t = __builtin_amdgcn_readfirstlane(w / a.nslab);
    const uint32_t slab = w - t * a.nslab;
    const uint32_t run = __builtin_amdgcn_readfirstlane(t / a.ngroups);
    const uint32_t grp = t - run * a.ngroups;
    const uint32_t r0 = run * a.rows_per_wave;
    if (r0 >= a.rows) return;
    const uint32_t r1 = std::min(a.rows, r0 + a.rows_per_wave);
    const uint32_t lane = threadIdx.x & 63;
    // the wave's first stripe, and the lane's offsets from that stripe's rows
    const uint32_t s0 = grp * a.stripes_per_wave;
    Off offd[Q], offr[Q];
    if constexpr (PACK) {
        uint32_t sl = lane / a.qrow, q = lane - sl * a.qrow;
        if (sl >= a.stripes_per_wave) sl = 0, q = 0;
        if (s0 + sl >= a.nstripes) sl = 0;
        const uint32_t o = (q >> 3) * 64 + (q & 7) * 4;
        offd[0] = (uint64_t)sl * a.delta_stride + o;
        offr[0] = (uint64_t)sl * a.rec_stride + o;
    } else {
        const uint32_t q0 = slab * (64 * Q) + lane;
        if (q0 >= a.qrow) return;
        // (a column beyond the window works on the lane's first column once more)
#pragma unroll
        for (int c = 0; c < Q; c++) {
            const uint32_t q = q0 + 64 * c;
            const uint32_t qq = q < a.qrow ? q : q0;
            offd[c] = offr[c] = (qq >> 3) * 64 + (qq & 7) * 4;
        }
    }

    constexpr bool HOIST = N * Q <= UPDATE_BATCH_HOIST_QUADS;
    uint32_t dL[N][Q], dH[N][Q];
    MulSel sel[HOIST ? N : 1][Q];
    const uint8_t* dbase = a.delta + (uint64_t)s0 * a.delta_stride;
#pragma unroll
    for (int e = 0; e < N; e++)
#pragma unroll
        for (int c = 0; c < Q; c++) {
            const uint8_t* d = dbase + (uint64_t)e * a.delta_pitch + offd[c];
            dL[e][c] = *(const uint32_t*)d;
            dH[e][c] = *(const uint32_t*)(d + 32);
            if constexpr (HOIST) sel[e][c] = mul_selectors(dL[e][c], dH[e][c]);
        }

    constexpr int G = UPDATE_BATCH_TABLE_GROUP, NG = (N + G - 1) / G;
    uint8_t* p = a.rec + (uint64_t)s0 * a.rec_stride + (uint64_t)r0 * a.rec_pitch;
    cu32p ix = (cu32p)a.idx + (a.row0 + r0) * N;
    cu32p tab = (cu32p)a.mul_tab;
    uint32_t id[G];
#pragma unroll
    for (int j = 0; j < G && j < N; j++) id[j] = ix[j];
    uint32_t cl[Q], ch[Q];
#pragma unroll
    for (int c = 0; c < Q; c++) cl[c] = *(const uint32_t*)(p + offr[c]), ch[c] = *(const uint32_t*)(p + offr[c] + 32);
    for (uint32_t r = r0; r < r1; r++) {
        const bool more = r + 1 < r1;
        // (the last row asks for itself and its own indices again: in bounds, unused)
        uint8_t* pn = more ? p + a.rec_pitch : p;
        cu32p ixn = more ? ix + N : ix;
        uint32_t nl[Q], nh[Q];
#pragma unroll
        for (int c = 0; c < Q; c++)
            nl[c] = *(const uint32_t*)(pn + offr[c]), nh[c] = *(const uint32_t*)(pn + offr[c] + 32);
#pragma unroll
        for (int g = 0; g < NG; g++) {
            const int cnt = N - g * G < G ? N - g * G : G;
            uint32_t tt[G][20];
#pragma unroll
            for (int j = 0; j < cnt; j++) {
                cu32p tj = tab + (size_t)id[j] * TAB_DWORDS;
#pragma unroll
                for (int i = 0; i < 20; i++) tt[j][i] = tj[i];
            }
            cu32p nx = g + 1 < NG ? ix + (g + 1) * G : ixn;
            const int ncnt = g + 1 < NG ? (N - (g + 1) * G < G ? N - (g + 1) * G : G) : (N < G ? N : G);
#pragma unroll
            for (int j = 0; j < ncnt; j++) id[j] = nx[j];
            // (keeps the scheduler from sinking each table's request down to its multiply)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < cnt; j++) {
                if constexpr (Q > 1) {
                    // (the upper half of each pool to a VGPR once for the lane's Q quads, as in update_kernel)
#pragma unroll
                    for (int i = 1; i < 16; i += 2) asm("v_mov_b32 %0, %1" : "=v"(tt[j][i]) : "s"(tt[j][i]));
                }
#pragma unroll
                for (int c = 0; c < Q; c++) {
                    if constexpr (HOIST) {
                        mul_xor_sel<false>(cl[c], ch[c], sel[g * G + j][c], tt[j]);
                    } else {
                        // (the compiler must take the delta for changed, or it hoists the selectors after all)
                        asm volatile("" : "+v"(dL[g * G + j][c]), "+v"(dH[g * G + j][c]));
                        mul_xor(cl[c], ch[c], dL[g * G + j][c], dH[g * G + j][c], tt[j]);
                    }
                }
            }
        }
        // plain stores: the rows are read back by the next update or decode
#pragma unroll
        for (int c = 0; c < Q; c++) {
            *(uint32_t*)(p + offr[c]) = cl[c];
            *(uint32_t*)(p + offr[c] + 32) = ch[c];
        }
        p = pn;
        ix = ixn;
#pragma unroll
        for (int c = 0; c < Q; c++) cl[c] = nl[c], ch[c] = nh[c];
    }
}

template <int N> static void launch_n(const UpdateBatchArgs& a, dim3 blocks, hipStream_t s) {
    if constexpr (UPDATE_BATCH_PACK_QROW != 0) {
        if (a.stripes_per_wave > 1) {
            hipLaunchKernelGGL((update_batch_kernel<N, 1, true>), blocks, dim3(256), 0, s, a);
            return;
        }
    }
    if constexpr (N <= UPDATE_BATCH_Q2_MAX_N) {
        if (a.quads_per_lane == 2) {
            hipLaunchKernelGGL((update_batch_kernel<N, 2, false>), blocks, dim3(256), 0, s, a);
            return;
        }
    }
    hipLaunchKernelGGL((update_batch_kernel<N, 1, false>), blocks, dim3(256), 0, s, a);
}

// The launch's shape from rows, qrow, nstripes and n (rs16_internal.hpp):
// host arithmetic only, which rs16_host_update_batch_consts evaluates without
// a device.
bool update_batch_launch_consts(UpdateBatchArgs& a, uint32_t n, uint64_t* nblocks) {
    if (!a.rows || !a.qrow || !a.nstripes || n == 0 || n > UPDATE_MAX_SHARDS) return false;
    // (a packed wave holds four stripes or more: qrow <= 16)
    const bool pack = a.qrow <= UPDATE_BATCH_PACK_QROW && a.nstripes >= 2;
    a.quads_per_lane = a.qrow >= UPDATE_BATCH_Q2_MIN_QROW && n <= (uint32_t)UPDATE_BATCH_Q2_MAX_N ? 2 : 1;
    a.nslab = (a.qrow + 64 * a.quads_per_lane - 1) / (64 * a.quads_per_lane);
    a.stripes_per_wave = pack ? 64 / a.qrow : 1;
    a.ngroups = (a.nstripes + a.stripes_per_wave - 1) / a.stripes_per_wave;
    // Rows per wave by update_launch_consts' rule, over the waves of all
    // stripes: enough waves to fill the chip several times over, then longer
    // runs.
    const uint64_t per_run = (uint64_t)a.nslab * a.ngroups;
    const uint64_t wave_rows = (uint64_t)a.rows * per_run;
    a.rows_per_wave = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(wave_rows / 8192, 1), 32);
    // four waves a workgroup; a launch holds < 2^32 threads (longer runs before that)
    auto waves = [&] { return (uint64_t)((a.rows + a.rows_per_wave - 1) / a.rows_per_wave) * per_run; };
    while ((waves() + 3) / 4 * 256 > 0xFFFFFFFFull && a.rows_per_wave < a.rows) a.rows_per_wave *= 2;
    if ((waves() + 3) / 4 * 256 > 0xFFFFFFFFull) return false;
    a.waves = (uint32_t)waves();
    *nblocks = (waves() + 3) / 4;
    return true;
}

hipError_t launch_update_batch(UpdateBatchArgs a, uint32_t n, hipStream_t s) {
    if (!a.rows || !a.qrow || !a.nstripes) return hipSuccess;
    uint64_t blocks;
    if (!update_batch_launch_consts(a, n, &blocks)) return hipErrorInvalidValue;
    typedef void (*Launch)(const UpdateBatchArgs&, dim3, hipStream_t);
    static const Launch launch[UPDATE_MAX_SHARDS] = {
        launch_n<1>,  launch_n<2>,  launch_n<3>,  launch_n<4>,  launch_n<5>,  launch_n<6>,  launch_n<7>,  launch_n<8>,
        launch_n<9>,  launch_n<10>, launch_n<11>, launch_n<12>, launch_n<13>, launch_n<14>, launch_n<15>, launch_n<16>,
        launch_n<17>, launch_n<18>, launch_n<19>, launch_n<20>, launch_n<21>, launch_n<22>, launch_n<23>, launch_n<24>,
        launch_n<25>, launch_n<26>, launch_n<27>, launch_n<28>, launch_n<29>, launch_n<30>, launch_n<31>, launch_n<32>};
    launch[n - 1](a, dim3((unsigned)blocks), s);
    return hipGetLastError();
}

}  // namespace rs16
