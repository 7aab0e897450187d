// rs16_gf.hpp -- GF(2^16) arithmetic for the MI355X engine (host + device).
//
// Element layout (reference src/algorithm.md:6-32): every 64-byte block of a
// shard holds 32 elements as 32 low bytes followed by 32 high bytes.  The GPU
// works on *quads*: quad q of a block = the 4 elements whose low bytes are
// the dword at byte 4q ("L") and whose high bytes are the dword at byte 32+4q
// ("H").  All FFT/IFFT/mul work is done on (L, H) dword pairs.
//
// Multiplication by a constant (reference: NoSimd::mul / mul_add with
// 4-bit nibble tables, src/engine/engine_nosimd.rs:65-79,105-119) is done
// here with CDNA's byte-permute instruction instead of table loads:
// v_perm_b32 selects 4 bytes out of an 8-byte pool using 4 per-byte 3-bit
// selectors, i.e. it is 4 lookups into an 8-entry byte table in one VALU op.
// Since x -> x*c is GF(2)-linear, x*c = XOR over bit groups of T_g[bits_g(x)].
// The 16 bits of an element are split into six groups: L[0:2], L[3:5],
// L[6:7], H[0:2], H[3:5], H[6:7]; each group has one table per output byte
// (lo / hi), 12 lookups per quad.  A product costs 6 selector extractions per
// dword pair, 12 v_perm and 4 v_bitop3 (3-input XOR), with no LDS traffic and
// no bank conflicts.
//
// Table entry layout (TAB_DWORDS dwords per log_m, see rs16_tables.cpp):
//   dword (g*2 + ob)*2 + h   g in 0..3 = {L0-2, L3-5, H0-2, H3-5},
//                            ob = output byte (0 lo, 1 hi), h = entries 0-3 / 4-7
//   dword 16 + gg*2 + ob     gg in 0..1 = {L6-7, H6-7} (4 entries, one dword)
// Entry index: log_m in 0..65535 uses reference `mul` semantics
// (tables::mul, src/engine/tables.rs:70-76; 65535 == 0 == multiply by 1);
// entry ZERO_ENTRY (65536) is the all-zero table used for the FFT/IFFT
// "no multiply" sentinel (log_m == GF_MODULUS in engine_naive.rs:64,116).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define RS16_HD __host__ __device__ __forceinline__
#else
#define RS16_HD inline
#endif

namespace rs16 {

constexpr uint32_t GF_ORDER = 65536;
constexpr uint32_t GF_MODULUS = 65535;
constexpr uint32_t ZERO_ENTRY = 65536;
constexpr uint32_t TAB_ENTRIES = 65537;
constexpr uint32_t TAB_DWORDS = 32;  // 128-byte stride: one cache line per constant

// v_perm_b32 semantics for selectors 0..7: byte i of the result is byte
// sel_i of the 64-bit value {hi:lo} (0-3 from lo, 4-7 from hi).
RS16_HD uint32_t perm_sw(uint32_t hi, uint32_t lo, uint32_t sel) {
    uint64_t pool = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; i++) {
        uint32_t s = (sel >> (8 * i)) & 0xFF;
        r |= (uint32_t)((pool >> (8 * s)) & 0xFF) << (8 * i);
    }
    return r;
}

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) {
    return __builtin_amdgcn_perm(hi, lo, sel);
}
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}
#else
inline uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) { return perm_sw(hi, lo, sel); }
inline uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) { return a ^ b ^ c; }
#endif

// (xL, xH) ^= (yL, yH) * c  where t points at the table entry of c.
//
// NARROW: c lies in the GF(2^8) subfield.  The elements are Cantor-basis
// coordinates (rs16_tables.cpp) and span(v_0 .. v_7) is that subfield, so c is
// a subfield constant exactly when c < 256.  Multiplying by one maps the
// subfield to itself: an input's low byte never reaches the output's high
// byte, i.e. the hi-output pools of the groups L0-2, L3-5 and L6-7 -- dwords
// 2, 3, 6, 7 and 17 of the table -- are all zero.  Their three lookups and
// one of the six XORs are left out: 9 v_perm + 5 XOR against 12 + 6.  The
// same 20-dword table serves both forms (the narrow one ignores five dwords).
// Which twiddles are narrow: twiddle_narrow (rs16_internal.hpp).
//
// The two halves of a product are separate functions, so that a kernel which
// multiplies one y by many constants extracts y's six selectors once
// (mul_selectors) and pays only the lookups per constant (mul_xor_sel):
// rs16_update.hip.
struct MulSel {
    uint32_t s0, s1, s2, s3, s4, s5;
};
RS16_HD MulSel mul_selectors(uint32_t yL, uint32_t yH) {
#if defined(__HIP_DEVICE_COMPILE__)
    // The selectors of both dwords from two 64-bit shifts of the (L, H) pair
    // instead of four 32-bit ones (the host's form below): the bits H shifts
    // into L's top land where the byte masks clear them.  (As plain C the
    // compiler narrows the shifts back to 32 bits.)  tools/ubench_bfly: 117.7
    // -> 114.0 cycles per wave-butterfly at 4 waves per SIMD
    // (profiles/r06_ubench_bfly64.txt; whole passes: profiles/r06_shift64_ab.txt).
    const uint64_t y = ((uint64_t)yH << 32) | yL;
    uint64_t a, b;
    asm("v_lshrrev_b64 %0, 3, %1" : "=v"(a) : "v"(y));
    asm("v_lshrrev_b64 %0, 6, %1" : "=v"(b) : "v"(y));
    const uint32_t s0 = yL & 0x07070707u;
    const uint32_t s1 = (uint32_t)a & 0x07070707u;
    const uint32_t s2 = (uint32_t)b & 0x03030303u;
    const uint32_t s3 = yH & 0x07070707u;
    const uint32_t s4 = (uint32_t)(a >> 32) & 0x07070707u;
    const uint32_t s5 = (uint32_t)(b >> 32) & 0x03030303u;
#else
    const uint32_t s0 = yL & 0x07070707u;
    const uint32_t a = yL >> 3;
    const uint32_t s1 = a & 0x07070707u;
    const uint32_t s2 = (a >> 3) & 0x03030303u;
    const uint32_t s3 = yH & 0x07070707u;
    const uint32_t b = yH >> 3;
    const uint32_t s4 = b & 0x07070707u;
    const uint32_t s5 = (b >> 3) & 0x03030303u;
#endif
    return MulSel{s0, s1, s2, s3, s4, s5};
}
template <bool NARROW>
RS16_HD void mul_xor_sel(uint32_t& xL, uint32_t& xH, const MulSel& y, const uint32_t* t) {
    const uint32_t s0 = y.s0, s1 = y.s1, s2 = y.s2, s3 = y.s3, s4 = y.s4, s5 = y.s5;
    if constexpr (NARROW) {
        const uint32_t l0 = perm(t[1], t[0], s0);
        const uint32_t l1 = perm(t[5], t[4], s1);
        const uint32_t l3 = perm(t[9], t[8], s3), h3 = perm(t[11], t[10], s3);
        const uint32_t l4 = perm(t[13], t[12], s4), h4 = perm(t[15], t[14], s4);
        const uint32_t l2 = perm(t[16], t[16], s2);
        const uint32_t l5 = perm(t[18], t[18], s5), h5 = perm(t[19], t[19], s5);
        xL = xor3(xor3(xL, l0, l1), xor3(l2, l3, l4), l5);
        xH = xor3(xH, h3, h4) ^ h5;
    } else {
        const uint32_t l0 = perm(t[1], t[0], s0), h0 = perm(t[3], t[2], s0);
        const uint32_t l1 = perm(t[5], t[4], s1), h1 = perm(t[7], t[6], s1);
        const uint32_t l3 = perm(t[9], t[8], s3), h3 = perm(t[11], t[10], s3);
        const uint32_t l4 = perm(t[13], t[12], s4), h4 = perm(t[15], t[14], s4);
        const uint32_t l2 = perm(t[16], t[16], s2), h2 = perm(t[17], t[17], s2);
        const uint32_t l5 = perm(t[18], t[18], s5), h5 = perm(t[19], t[19], s5);
        xL = xor3(xor3(xL, l0, l1), xor3(l2, l3, l4), l5);
        xH = xor3(xor3(xH, h0, h1), xor3(h2, h3, h4), h5);
    }
}
template <bool NARROW>
RS16_HD void mul_xor_t(uint32_t& xL, uint32_t& xH, uint32_t yL, uint32_t yH, const uint32_t* t) {
    mul_xor_sel<NARROW>(xL, xH, mul_selectors(yL, yH), t);
}
RS16_HD void mul_xor(uint32_t& xL, uint32_t& xH, uint32_t yL, uint32_t yH, const uint32_t* t) {
    mul_xor_t<false>(xL, xH, yL, yH, t);
}
RS16_HD void mul_xor_narrow(uint32_t& xL, uint32_t& xH, uint32_t yL, uint32_t yH, const uint32_t* t) {
    mul_xor_t<true>(xL, xH, yL, yH, t);
}

// Tower form (tables: rs16_tables.cpp).  With beta =
// v_8 every element is a + b beta with a, b in the GF(2^8) subfield: b = the
// high byte, a = the low byte ^ B(high byte).  tower_conv switches a quad
// between the two forms (its own inverse, the high dword stays): three
// lookups of H's selectors in B's pools tb[0 .. 4] (groups H0-2, H3-5, H6-7).
// In tower form a subfield constant multiplies a and b by the same byte map
// and crosses nothing between them: mul_xor_tower_narrow, 6 lookups from
// dwords 0, 1, 4, 5 and 16 of the constant's tower table (its L -> lo pools).
constexpr uint32_t TOWER_B_DWORD = 20;  // B's pools: dwords 20 .. 24 of skew table entry 0
struct TowerB {
    uint32_t p[5];
};
// (s3, s4, s5 of y: the selectors of the high dword)
RS16_HD void tower_conv_sel(uint32_t& L, const MulSel& y, const TowerB& tb) {
    const uint32_t b0 = perm(tb.p[1], tb.p[0], y.s3);
    const uint32_t b1 = perm(tb.p[3], tb.p[2], y.s4);
    const uint32_t b2 = perm(tb.p[4], tb.p[4], y.s5);
    L = xor3(L, b0, b1) ^ b2;
}
RS16_HD MulSel high_selectors(uint32_t H) {
    const uint32_t a = H >> 3;
    return MulSel{0, 0, 0, H & 0x07070707u, a & 0x07070707u, (a >> 3) & 0x03030303u};
}
RS16_HD void tower_conv(uint32_t& L, uint32_t H, const TowerB& tb) { tower_conv_sel(L, high_selectors(H), tb); }
// the selectors of a row whose high dword's are known (y) and whose low dword changed since
RS16_HD MulSel low_selectors(uint32_t L, const MulSel& y) {
    const uint32_t a = L >> 3;
    return MulSel{L & 0x07070707u, a & 0x07070707u, (a >> 3) & 0x03030303u, y.s3, y.s4, y.s5};
}
RS16_HD void mul_xor_tower_narrow_sel(uint32_t& xL, uint32_t& xH, const MulSel& y, const uint32_t* t) {
    const uint32_t l0 = perm(t[1], t[0], y.s0), h0 = perm(t[1], t[0], y.s3);
    const uint32_t l1 = perm(t[5], t[4], y.s1), h1 = perm(t[5], t[4], y.s4);
    const uint32_t l2 = perm(t[16], t[16], y.s2), h2 = perm(t[16], t[16], y.s5);
    xL = xor3(xL, l0, l1) ^ l2;
    xH = xor3(xH, h0, h1) ^ h2;
}
RS16_HD void mul_xor_tower_narrow(uint32_t& xL, uint32_t& xH, uint32_t yL, uint32_t yH, const uint32_t* t) {
    mul_xor_tower_narrow_sel(xL, xH, mul_selectors(yL, yH), t);
}
// A wide constant c = c0 + c1 beta in tower form.  beta^2 = beta + v_7, so
//   (a + b beta) c = (a c0 + b c1 v_7) + (a c1 + b c0 + b c1) beta,
// and the constant's tower table holds four byte maps: L -> lo = M_{c0}
// (dwords 0, 1, 4, 5, 16), H -> lo = M_{c1 v_7} (8, 9, 12, 13, 18), L -> hi =
// M_{c1} (2, 3, 6, 7, 17), H -> hi = M_{c0 ^ c1} (10, 11, 14, 15, 19).  Three
// of them do (Karatsuba): with P1 = M_{c0}(a), Q = M_{c1 v_7}(b), P3 = M_{c0 ^
// c1}(a ^ b) the product is (P1 ^ Q, P3 ^ P1).  The selectors of a ^ b are
// sel(a) ^ sel(b) -- the maps are linear, no shift or mask -- and P1's partial
// XOR serves both bytes: 9 v_perm and 25 instructions per quad against 12 and
// 26.  rs16_tables.cpp checks the three-map product at table build.
RS16_HD void mul_xor_tower_wide_sel(uint32_t& xL, uint32_t& xH, const MulSel& y, const uint32_t* t) {
    const uint32_t u0 = y.s0 ^ y.s3, u1 = y.s1 ^ y.s4, u2 = y.s2 ^ y.s5;
    const uint32_t p0 = perm(t[1], t[0], y.s0), p1 = perm(t[5], t[4], y.s1), p2 = perm(t[16], t[16], y.s2);
    const uint32_t q0 = perm(t[9], t[8], y.s3), q1 = perm(t[13], t[12], y.s4), q2 = perm(t[18], t[18], y.s5);
    const uint32_t r0 = perm(t[11], t[10], u0), r1 = perm(t[15], t[14], u1), r2 = perm(t[19], t[19], u2);
    const uint32_t p = xor3(p0, p1, p2);
    xL = xor3(xor3(xL, p, q0), q1, q2);
    xH = xor3(xor3(xH, p, r0), r1, r2);
}
RS16_HD void mul_xor_tower_wide(uint32_t& xL, uint32_t& xH, uint32_t yL, uint32_t yH, const uint32_t* t) {
    mul_xor_tower_wide_sel(xL, xH, mul_selectors(yL, yH), t);
}
// The same with c1 = 1 (the one wide layer of a 2^15-row chunk's middle pass:
// its twiddles are s ^ v_8 with s in the subfield): M_{c1} is the identity and
// M_{c0 ^ c1}(b) = M_{c0}(b) ^ b, so the product is (M_{c0}(a) ^ M_{v_7}(b),
// M_{c0}(b) ^ a ^ b) -- the narrow multiply's six lookups, three of b's
// selectors in the H -> lo pools, and two plain XORs: 9 v_perm and 23
// instructions per quad.
RS16_HD void mul_xor_tower_beta_sel(uint32_t& xL, uint32_t& xH, uint32_t yL, uint32_t yH, const MulSel& y,
                                    const uint32_t* t) {
    const uint32_t l0 = perm(t[1], t[0], y.s0), h0 = perm(t[1], t[0], y.s3);
    const uint32_t l1 = perm(t[5], t[4], y.s1), h1 = perm(t[5], t[4], y.s4);
    const uint32_t l2 = perm(t[16], t[16], y.s2), h2 = perm(t[16], t[16], y.s5);
    const uint32_t q0 = perm(t[9], t[8], y.s3), q1 = perm(t[13], t[12], y.s4), q2 = perm(t[18], t[18], y.s5);
    xL = xor3(xor3(xL, l0, l1), xor3(l2, q0, q1), q2);
    xH = xor3(xor3(xH, h0, h1), h2, yL) ^ yH;
}
RS16_HD void mul_xor_tower_beta(uint32_t& xL, uint32_t& xH, uint32_t yL, uint32_t yH, const uint32_t* t) {
    mul_xor_tower_beta_sel(xL, xH, yL, yH, mul_selectors(yL, yH), t);
}

// Ones'-complement add/sub on logs (reference add_mod/sub_mod,
// src/engine.rs:90-100), in 32-bit arithmetic.
RS16_HD uint32_t add_mod(uint32_t x, uint32_t y) {
    uint32_t s = x + y;
    return (s + (s >> 16)) & 0xFFFFu;
}
RS16_HD uint32_t sub_mod(uint32_t x, uint32_t y) {
    uint32_t d = x - y;
    return (d + (d >> 16)) & 0xFFFFu;
}

}  // namespace rs16
