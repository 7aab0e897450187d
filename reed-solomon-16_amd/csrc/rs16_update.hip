// rs16_update.hip -- delta update of recovery shards (rs16_update_device,
// DESIGN.md 3.15).  The encode is GF(2^16)-linear per element position,
// recovery_j = sum_i M[j][i] original_i, so overwriting the originals
// indices[0 .. n) changes recovery row j by sum_e M[j][indices[e]] delta_e
// with delta_e = old ^ new.  One read-modify-write sweep over the recovery
// rows: rec[j] ^= sum_e tab[idx[j][e]] . delta[e] on (L, H) quads (rs16_gf.hpp),
// idx = the plan's m x n array of d_mul_tab entries (rs16_update_plan_new).
//
// A unit of its own: no existing kernel shares a translation unit with it, so
// their machine code stays what it was (scripts/isa_compare.py).
#include <algorithm>

#include "rs16_internal.hpp"

namespace rs16 {

typedef const __attribute__((address_space(4))) uint32_t* cu32p;
#ifndef RS16_UPDATE_TABLE_GROUP
#define RS16_UPDATE_TABLE_GROUP 4
#endif
constexpr int UPDATE_TABLE_GROUP = RS16_UPDATE_TABLE_GROUP;
// selectors kept in registers up to this many quads (n x quads per lane) of a lane
#ifndef RS16_UPDATE_HOIST_QUADS
#define RS16_UPDATE_HOIST_QUADS 16
#endif
constexpr int UPDATE_HOIST_QUADS = RS16_UPDATE_HOIST_QUADS;
// Rows of at least this many quads (1 KiB) take two quads per lane, for up
// to UPDATE_Q2_MAX_N shards: those lanes keep their selectors (12 VGPRs a
// shard).  More shards at two quads per lane would have to extract the
// selectors per row, and the compiler then runs out of scalar registers for
// the table groups (it spills them to vector lanes and on to scratch).
#ifndef RS16_UPDATE_Q2_MIN_QROW
#define RS16_UPDATE_Q2_MIN_QROW 128
#endif
constexpr uint32_t UPDATE_Q2_MIN_QROW = RS16_UPDATE_Q2_MIN_QROW;
constexpr int UPDATE_Q2_MAX_N = UPDATE_HOIST_QUADS / 2;

// One wave owns a slab of 64 Q quad columns (512 Q bytes of a row; lane l
// holds quads l, 64 + l, ... of the slab) and a run of rows_per_wave recovery
// rows.  The n delta quads of each of its columns stay in registers for the
// whole run; every row is requested one row ahead of its multiplies.  The
// table of (row, e) is the same for the whole wave: the entry index and the
// 20 table dwords come over the scalar path (the index array is written by a
// host copy before any launch).  Every (row, e) is another 128-byte line of
// the 8 MiB d_mul_tab, so the scalar cache misses on each: a table fetched
// once serves the wave's Q quads per lane (Q = 2 from 1 KiB rows on).
// Rows narrower than a slab (64 .. 448 bytes at Q = 1) take one wave per row
// with the lanes beyond the row idle, as does the last slab of a row whose
// quad count is no multiple of the slab's.
template <int N, int Q>
__global__ void __launch_bounds__(256) update_kernel(UpdateArgs a) {
    // Wave w of the launch: slab w mod nslab of run w / nslab, so the waves
    // of a workgroup work on the slabs of the same rows where a row has
    // several and find each other's tables in their CU's scalar cache
    // (measured: a workgroup of four runs of one slab took 43 us where this
    // takes 35, 32768 x 1 KiB, n = 8).  32-bit and scalar throughout.
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    const uint32_t run = __builtin_amdgcn_readfirstlane(w / a.nslab);
    const uint32_t slab = w - run * a.nslab;
    const uint32_t r0 = run * a.rows_per_wave;
    if (r0 >= a.rows) return;
    const uint32_t r1 = std::min(a.rows, r0 + a.rows_per_wave);
    const uint32_t q0 = slab * (64 * Q) + (threadIdx.x & 63);
    if (q0 >= a.qrow) return;
    // A column beyond the row (the last slab's tail) works on the lane's first
    // column once more: the same loads and multiplies give the same value,
    // stored to the same place, and no load or store is conditional.
    size_t off[Q];
#pragma unroll
    for (int c = 0; c < Q; c++) {
        const uint32_t q = q0 + 64 * c;
        const uint32_t qq = q < a.qrow ? q : q0;
        off[c] = (size_t)(qq >> 3) * 64 + (qq & 7) * 4;
    }

    // The multiply's selectors depend on the delta alone: up to
    // UPDATE_HOIST_QUADS delta quads per lane they are extracted once per wave
    // and kept (6 VGPRs a quad), beyond that the deltas are kept (2 VGPRs)
    // and every row extracts them again, which costs VALU work but keeps more
    // waves on a SIMD (measured: profiles/r08_update.txt).
    constexpr bool HOIST = N * Q <= UPDATE_HOIST_QUADS;
    uint32_t dL[N][Q], dH[N][Q];
    MulSel sel[HOIST ? N : 1][Q];
#pragma unroll
    for (int e = 0; e < N; e++)
#pragma unroll
        for (int c = 0; c < Q; c++) {
            const uint8_t* d = a.delta + (size_t)e * a.S + off[c];
            dL[e][c] = *(const uint32_t*)d;
            dH[e][c] = *(const uint32_t*)(d + 32);
            if constexpr (HOIST) sel[e][c] = mul_selectors(dL[e][c], dH[e][c]);
        }

    // Tables in groups of G: the G x 20 dwords of a group are requested
    // together (80 SGPRs) with the entry indices of the group after it -- the
    // next row's first group behind a row's last -- so a group waits for one
    // scalar round trip, not for two dependent ones per table.
    constexpr int G = UPDATE_TABLE_GROUP, NG = (N + G - 1) / G;
    uint8_t* p = a.rec + r0 * a.S;
    cu32p ix = (cu32p)a.idx + (a.row0 + r0) * N;
    cu32p tab = (cu32p)a.mul_tab;
    uint32_t id[G];
#pragma unroll
    for (int j = 0; j < G && j < N; j++) id[j] = ix[j];
    uint32_t cl[Q], ch[Q];
#pragma unroll
    for (int c = 0; c < Q; c++) cl[c] = *(const uint32_t*)(p + off[c]), ch[c] = *(const uint32_t*)(p + off[c] + 32);
    for (uint32_t r = (uint32_t)r0; r < r1; r++) {
        const bool more = r + 1 < r1;
        // (the last row asks for itself and its own indices again: in bounds,
        // unused, and the loop body stays free of branches)
        uint8_t* pn = more ? p + a.S : p;
        cu32p ixn = more ? ix + N : ix;
        uint32_t nl[Q], nh[Q];
#pragma unroll
        for (int c = 0; c < Q; c++) nl[c] = *(const uint32_t*)(pn + off[c]), nh[c] = *(const uint32_t*)(pn + off[c] + 32);
#pragma unroll
        for (int g = 0; g < NG; g++) {
            const int cnt = N - g * G < G ? N - g * G : G;
            uint32_t tt[G][20];
#pragma unroll
            for (int j = 0; j < cnt; j++) {
                cu32p t = tab + (size_t)id[j] * TAB_DWORDS;
#pragma unroll
                for (int i = 0; i < 20; i++) tt[j][i] = t[i];
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
                    // v_perm takes one scalar operand: the upper half of each
                    // 8-entry pool goes to a VGPR once for the lane's Q quads
                    // (left to the compiler, every quad copies it again)
#pragma unroll
                    for (int i = 1; i < 16; i += 2) asm("v_mov_b32 %0, %1" : "=v"(tt[j][i]) : "s"(tt[j][i]));
                }
#pragma unroll
                for (int c = 0; c < Q; c++) {
                    if constexpr (HOIST) {
                        mul_xor_sel<false>(cl[c], ch[c], sel[g * G + j][c], tt[j]);
                    } else {
                        // (no code: the compiler must take the delta for changed, or it hoists
                        // the selectors out of the row loop after all and runs out of registers)
                        asm volatile("" : "+v"(dL[g * G + j][c]), "+v"(dH[g * G + j][c]));
                        mul_xor(cl[c], ch[c], dL[g * G + j][c], dH[g * G + j][c], tt[j]);
                    }
                }
            }
        }
        // plain stores: the rows are read back by the next update or decode
#pragma unroll
        for (int c = 0; c < Q; c++) {
            *(uint32_t*)(p + off[c]) = cl[c];
            *(uint32_t*)(p + off[c] + 32) = ch[c];
        }
        p = pn;
        ix = ixn;
#pragma unroll
        for (int c = 0; c < Q; c++) cl[c] = nl[c], ch[c] = nh[c];
    }
}

template <int N> static void launch_n(const UpdateArgs& a, dim3 blocks, hipStream_t s) {
    if constexpr (N <= UPDATE_Q2_MAX_N) {
        if (a.quads_per_lane == 2) {
            hipLaunchKernelGGL((update_kernel<N, 2>), blocks, dim3(256), 0, s, a);
            return;
        }
    }
    hipLaunchKernelGGL((update_kernel<N, 1>), blocks, dim3(256), 0, s, a);
}

// The launch's shape from rows, qrow and n (rs16_internal.hpp): host
// arithmetic only, which rs16_host_update_consts evaluates without a device.
bool update_launch_consts(UpdateArgs& a, uint32_t n, uint64_t* nblocks) {
    if (!a.rows || !a.qrow || n == 0 || n > UPDATE_MAX_SHARDS) return false;
    a.quads_per_lane = a.qrow >= UPDATE_Q2_MIN_QROW && n <= UPDATE_Q2_MAX_N ? 2 : 1;
    a.nslab = (a.qrow + 64 * a.quads_per_lane - 1) / (64 * a.quads_per_lane);
    // Rows per wave: enough waves to fill the chip several times over (1024
    // SIMDs), then longer runs, which spread the n delta loads of a wave over
    // more rows.
    const uint64_t wave_rows = (uint64_t)a.rows * a.nslab;
    a.rows_per_wave = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(wave_rows / 8192, 1), 32);
    // four waves a workgroup; a launch holds < 2^32 threads (very wide shards: longer runs)
    auto blocks = [&] { return ((uint64_t)((a.rows + a.rows_per_wave - 1) / a.rows_per_wave) * a.nslab + 3) / 4; };
    while (blocks() * 256 > 0xFFFFFFFFull && a.rows_per_wave < a.rows) a.rows_per_wave *= 2;
    if (blocks() * 256 > 0xFFFFFFFFull) return false;
    *nblocks = blocks();
    return true;
}

hipError_t launch_update(UpdateArgs a, uint32_t n, hipStream_t s) {
    if (!a.rows || !a.qrow) return hipSuccess;
    uint64_t blocks;
    if (!update_launch_consts(a, n, &blocks)) return hipErrorInvalidValue;
    typedef void (*Launch)(const UpdateArgs&, dim3, hipStream_t);
    static const Launch launch[UPDATE_MAX_SHARDS] = {
        launch_n<1>,  launch_n<2>,  launch_n<3>,  launch_n<4>,  launch_n<5>,  launch_n<6>,  launch_n<7>,  launch_n<8>,
        launch_n<9>,  launch_n<10>, launch_n<11>, launch_n<12>, launch_n<13>, launch_n<14>, launch_n<15>, launch_n<16>,
        launch_n<17>, launch_n<18>, launch_n<19>, launch_n<20>, launch_n<21>, launch_n<22>, launch_n<23>, launch_n<24>,
        launch_n<25>, launch_n<26>, launch_n<27>, launch_n<28>, launch_n<29>, launch_n<30>, launch_n<31>, launch_n<32>};
    launch[n - 1](a, dim3((unsigned)blocks), s);
    return hipGetLastError();
}

}  // namespace rs16
