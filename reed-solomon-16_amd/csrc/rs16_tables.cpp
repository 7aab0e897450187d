// rs16_tables.cpp -- GF(2^16) constant tables, built once per process on the
// host and uploaded to HBM by each engine (rs16_engine.cpp).
//
// Field definition (must match the reference bit for bit):
//   GF_POLYNOMIAL 0x1002D, elements in the Cantor basis
//   (src/engine.rs:59-74; construction src/engine/tables.rs:83-124),
//   FFT twiddle logs "skew" (src/engine/tables.rs:164-205),
//   LogWalsh = FWHT(log) with log[0] = 0 (src/engine/tables.rs:127-139).
// The device-side multiply tables are a GPU-specific format (v_perm byte
// tables, rs16_gf.hpp), not the reference's Mul16 nibble tables.
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "rs16_internal.hpp"

namespace rs16 {

namespace {
const uint16_t kCantorBasis[16] = {0x0001, 0xACCA, 0x3C0E, 0x163E, 0xC582, 0xED2E, 0x914C, 0x4012,
                                   0x6C98, 0x10D8, 0x6A72, 0xB900, 0xFDB8, 0xFB34, 0xFF38, 0x991E};
HostTables g_tables;
std::once_flag g_once;

inline uint16_t gf_mul(const HostTables& t, uint16_t x, uint32_t log_m) {
    return x == 0 ? 0 : t.exp[add_mod(t.log[x], log_m)];
}

// (lo, hi) -> (lo ^ B(hi), hi): Cantor coordinates <-> tower form, its own inverse
inline uint16_t tower_conv(const HostTables& t, uint16_t x) {
    uint16_t r = x;
    for (int i = 0; i < 8; i++)
        if ((x >> (8 + i)) & 1) r ^= t.tower_a[i];
    return r;
}

void fwht_full(std::vector<uint16_t>& v) {
    for (uint32_t d = 1; d < GF_ORDER; d <<= 1)
        for (uint32_t r = 0; r < GF_ORDER; r += 2 * d)
            for (uint32_t i = r; i < r + d; i++) {
                uint32_t a = v[i], b = v[i + d];
                v[i] = (uint16_t)add_mod(a, b);
                v[i + d] = (uint16_t)sub_mod(a, b);
            }
}

void build(HostTables& t) {
    t.exp.assign(GF_ORDER, 0);
    t.log.assign(GF_ORDER, 0);
    // Exponent table of the LFSR over 0x1002D: position -> exponent.
    {
        uint32_t state = 1;
        for (uint32_t i = 0; i < GF_MODULUS; i++) {
            t.exp[state] = (uint16_t)i;
            state <<= 1;
            if (state >= GF_ORDER) state ^= 0x1002Du;
        }
        t.exp[0] = (uint16_t)GF_MODULUS;
    }
    // Cantor-basis element i (as XOR of basis vectors by the bits of i),
    // then log[i] = exponent of that element and exp = its inverse map.
    {
        std::vector<uint16_t> cb(GF_ORDER, 0);
        for (int b = 0; b < 16; b++) {
            uint32_t w = 1u << b;
            for (uint32_t j = 0; j < w; j++) cb[j + w] = cb[j] ^ kCantorBasis[b];
        }
        for (uint32_t i = 0; i < GF_ORDER; i++) t.log[i] = t.exp[cb[i]];
        for (uint32_t i = 0; i < GF_ORDER; i++) t.exp[t.log[i]] = (uint16_t)i;
        t.exp[GF_MODULUS] = t.exp[0];
    }
    // FFT twiddle logs.
    {
        std::vector<uint16_t> sk(GF_MODULUS, 0);
        uint16_t temp[15];
        for (int i = 1; i < 16; i++) temp[i - 1] = (uint16_t)(1u << i);
        for (int m = 0; m < 15; m++) {
            const uint32_t step = 1u << (m + 1);
            sk[(1u << m) - 1] = 0;
            for (int i = m; i < 15; i++) {
                const uint32_t s = 1u << (i + 1);
                for (uint32_t j = (1u << m) - 1; j < s; j += step) sk[j + s] = sk[j] ^ temp[i];
            }
            temp[m] = (uint16_t)(GF_MODULUS - t.log[gf_mul(t, temp[m], t.log[temp[m] ^ 1])]);
            for (int i = m + 1; i < 15; i++) temp[i] = gf_mul(t, temp[i], add_mod(t.log[temp[i] ^ 1], temp[m]));
        }
        t.skew.resize(GF_MODULUS);
        for (uint32_t i = 0; i < GF_MODULUS; i++) t.skew[i] = t.log[sk[i]];
    }
    // LogWalsh.
    t.log_walsh = t.log;
    t.log_walsh[0] = 0;
    fwht_full(t.log_walsh);

    // The pass kernels skip the multiply of uniform groups whose twiddle is
    // the sentinel and recognise those by index: the sentinel entries are
    // exactly the indices 2^i - 1 (rs16_pass.hpp, GroupLoop).  A table that
    // broke this would give wrong results, so it is checked here, once.
    for (uint32_t i = 0; i < GF_MODULUS; i++)
        if ((t.skew[i] == GF_MODULUS) != ((i & (i + 1)) == 0)) {
            fprintf(stderr, "rs16: skew table sentinel at unexpected index %u\n", i);
            abort();
        }
    // FFT/IFFT twiddle table *entries*: sentinel GF_MODULUS -> ZERO_ENTRY.
    t.skew_entry.assign(GF_ORDER, ZERO_ENTRY);
    for (uint32_t i = 0; i < GF_MODULUS; i++) t.skew_entry[i] = t.skew[i] == GF_MODULUS ? ZERO_ENTRY : t.skew[i];

    // v_perm multiply tables (layout in rs16_gf.hpp).
    t.mul_tab.assign((size_t)TAB_ENTRIES * TAB_DWORDS, 0);
    static const int kOff3[4] = {0, 3, 8, 11};
    static const int kOff2[2] = {6, 14};
    for (uint32_t lm = 0; lm < GF_ORDER; lm++) {
        uint32_t* e = &t.mul_tab[(size_t)lm * TAB_DWORDS];
        for (int g = 0; g < 4; g++)
            for (uint32_t v = 0; v < 8; v++) {
                uint16_t p = gf_mul(t, (uint16_t)(v << kOff3[g]), lm);
                for (int ob = 0; ob < 2; ob++) {
                    uint32_t byte = (p >> (8 * ob)) & 0xFF;
                    e[(g * 2 + ob) * 2 + (v >> 2)] |= byte << (8 * (v & 3));
                }
            }
        for (int gg = 0; gg < 2; gg++)
            for (uint32_t v = 0; v < 4; v++) {
                uint16_t p = gf_mul(t, (uint16_t)(v << kOff2[gg]), lm);
                for (int ob = 0; ob < 2; ob++) e[16 + gg * 2 + ob] |= ((p >> (8 * ob)) & 0xFFu) << (8 * v);
            }
    }
    // entry ZERO_ENTRY stays all zero.

    // The table of every twiddle index, so that a pass stages a twiddle's
    // table with one load instead of skew_entry -> mul_tab.
    t.skew_tab.resize((size_t)GF_ORDER * TAB_DWORDS);
    for (uint32_t i = 0; i < GF_ORDER; i++)
        std::copy_n(&t.mul_tab[(size_t)t.skew_entry[i] * TAB_DWORDS], TAB_DWORDS, &t.skew_tab[(size_t)i * TAB_DWORDS]);
    // The narrow pass variants leave out the lookups of the hi-output pools
    // of the low-byte groups (mul_xor_narrow, rs16_gf.hpp) in the layers
    // whose twiddle indices twiddle_narrow() accepts: those five dwords must
    // be zero for exactly these indices.  Checked here, once, like the sentinel.
    for (uint32_t i = 0; i < GF_MODULUS; i++) {
        const uint32_t* e = &t.skew_tab[(size_t)i * TAB_DWORDS];
        const bool zero = (e[2] | e[3] | e[6] | e[7] | e[17]) == 0;
        if (zero != twiddle_narrow(i)) {
            fprintf(stderr, "rs16: skew table entry %u is %s a subfield twiddle, against the index rule\n", i,
                    zero ? "" : "not");
            abort();
        }
    }

    // Tower form.  With beta = v_8 the high byte's
    // basis vectors are v_{8+i} = a_i + v_i beta with a_i in the subfield
    // span(v_0 .. v_7), so an element (lo, hi) is a + b beta with b = hi and a
    // = lo ^ B(hi), B the 8 x 8 bit matrix with columns a_i.  The a_i are
    // derived here; a basis without that form cannot take the tower form.
    for (uint32_t i = 0; i < 8; i++) {
        const uint16_t a = (uint16_t)((1u << (8 + i)) ^ gf_mul(t, (uint16_t)(1u << i), t.log[1u << 8]));
        if (a >= 256) {
            fprintf(stderr, "rs16: basis vector v_%u is not a_i + v_i v_8 with a_i in the subfield\n", 8 + i);
            abort();
        }
        t.tower_a[i] = (uint8_t)a;
    }
    // B's lookup pools, by the three selector groups of a high byte (bits
    // 0-2, 3-5, 6-7) as a multiply table holds them: 2 + 2 + 1 dwords.
    for (uint32_t v = 0; v < 8; v++) {
        t.tower_b[v >> 2] |= (tower_conv(t, (uint16_t)(v << 8)) & 0xFFu) << (8 * (v & 3));
        t.tower_b[2 + (v >> 2)] |= (tower_conv(t, (uint16_t)(v << 11)) & 0xFFu) << (8 * (v & 3));
        if (v < 4) t.tower_b[4] |= (tower_conv(t, (uint16_t)(v << 14)) & 0xFFu) << (8 * v);
    }
    // The twiddle tables in tower coordinates: conv . M_c . conv for every
    // skew index, in the layout of skew_tab.  The passes of a tower
    // sequence stage these; a subfield twiddle's table must then map both
    // bytes by one byte map and cross nothing between them -- checked here,
    // once, as the narrow rule above.
    t.skew_tab_tower.assign((size_t)GF_ORDER * TAB_DWORDS, 0);
    for (uint32_t i = 0; i < GF_MODULUS; i++) {
        const uint32_t lm = t.skew_entry[i];
        if (lm == ZERO_ENTRY) continue;
        uint32_t* e = &t.skew_tab_tower[(size_t)i * TAB_DWORDS];
        auto prod = [&](uint32_t x) { return tower_conv(t, gf_mul(t, tower_conv(t, (uint16_t)x), lm)); };
        for (int g = 0; g < 4; g++)
            for (uint32_t v = 0; v < 8; v++) {
                const uint16_t p = prod(v << kOff3[g]);
                for (int ob = 0; ob < 2; ob++) e[(g * 2 + ob) * 2 + (v >> 2)] |= ((p >> (8 * ob)) & 0xFFu) << (8 * (v & 3));
            }
        for (int gg = 0; gg < 2; gg++)
            for (uint32_t v = 0; v < 4; v++) {
                const uint16_t p = prod(v << kOff2[gg]);
                for (int ob = 0; ob < 2; ob++) e[16 + gg * 2 + ob] |= ((p >> (8 * ob)) & 0xFFu) << (8 * v);
            }
        if (!twiddle_narrow(i)) continue;
        const bool cross = (e[2] | e[3] | e[6] | e[7] | e[17] | e[8] | e[9] | e[12] | e[13] | e[18]) != 0;
        const bool same = e[10] == e[0] && e[11] == e[1] && e[14] == e[4] && e[15] == e[5] && e[19] == e[16];
        if (cross || !same) {
            fprintf(stderr, "rs16: tower table of subfield twiddle %u %s\n", i,
                    cross ? "crosses between the bytes" : "maps the two bytes differently");
            abort();
        }
    }
    // The wide multiply of the T = 7 passes (mul_xor_tower_wide, rs16_gf.hpp)
    // reads three of a tower table's four byte maps as M_{c0}, M_{c1 v_7} and
    // M_{c0 ^ c1}, (c0, c1) the constant's tower coordinates.  That rests on
    // beta^2 = beta + v_7 and shows in the table as L -> hi = (L -> lo) ^ (H ->
    // hi), pool by pool.  Checked here, once: the identity, the pools of every
    // twiddle, and the three-map product itself on 16 elements that take every
    // selector value in every bit group of a, b and a ^ b.
    {
        const uint16_t beta = 1u << 8, v7 = 1u << 7;
        if (gf_mul(t, beta, t.log[beta]) != (beta ^ v7)) {
            fprintf(stderr, "rs16: v_8^2 is not v_8 + v_7: no three-map wide multiply in tower form\n");
            abort();
        }
        for (uint32_t i = 0; i < GF_MODULUS; i++) {
            const uint32_t lm = t.skew_entry[i];
            if (lm == ZERO_ENTRY) continue;
            const uint32_t* e = &t.skew_tab_tower[(size_t)i * TAB_DWORDS];
            bool ok = (e[0] ^ e[10]) == e[2] && (e[1] ^ e[11]) == e[3] && (e[4] ^ e[14]) == e[6] &&
                      (e[5] ^ e[15]) == e[7] && (e[16] ^ e[19]) == e[17];
            for (uint32_t j = 0; j < 16 && ok; j++) {
                const uint32_t a = (j & 7) | (((j + 3) & 7) << 3) | ((j & 3) << 6);
                const uint32_t b = j < 8 ? ((j + 5) & 7) | (((j * 3) & 7) << 3) | (((j + 1) & 3) << 6) : 0;
                const uint16_t x = (uint16_t)(a | (b << 8));
                const uint16_t want = tower_conv(t, gf_mul(t, tower_conv(t, x), lm));
                uint32_t xl = 0, xh = 0;  // (a quad of four times x)
                mul_xor_tower_wide(xl, xh, a * 0x01010101u, b * 0x01010101u, e);
                ok = xl == (want & 0xFFu) * 0x01010101u && xh == (uint32_t)(want >> 8) * 0x01010101u;
            }
            if (!ok) {
                fprintf(stderr, "rs16: tower table of twiddle %u does not multiply by three byte maps\n", i);
                abort();
            }
            // c1 = 1 (L -> hi is the identity) for exactly the indices of twiddle_beta
            const bool one = e[2] == 0x03020100u && e[3] == 0x07060504u && e[6] == 0x18100800u &&
                             e[7] == 0x38302820u && e[17] == 0xC0804000u;
            if (one != twiddle_beta(i)) {
                fprintf(stderr, "rs16: twiddle %u is %s s + v_8 with s in the subfield, against the index rule\n", i,
                        one ? "" : "not");
                abort();
            }
        }
    }
    // The conversion's pools ride in the padding of entry 0 of both twiddle
    // tables (dwords TOWER_B_DWORD ..): the T = 7 passes of a tower sequence
    // read them from the table they stage their twiddles from.
    std::copy_n(t.tower_b, 5, &t.skew_tab[TOWER_B_DWORD]);
    std::copy_n(t.tower_b, 5, &t.skew_tab_tower[TOWER_B_DWORD]);

    // Column codec images: table g of layer kb (g = 2^L - 2^(L-kb) + j, group
    // j covering rows [j 2^(kb+1), (j+1) 2^(kb+1))) is the twiddle of skew
    // index j 2^(kb+1) + 2^kb + delta - 1 (engine_naive.rs:43-124).
    t.col_img.assign(COL_IMG_DWORDS, 0);
    for (uint32_t L = COL_LMIN; L <= COL_LGEN; L++)
        for (uint32_t d = 0; d < col_img_count(L); d++) {
            const uint32_t N = 1u << L, delta = d * N;
            uint32_t* img = &t.col_img[col_img_offset(L, d)];
            for (uint32_t g = 0; g + 1 < N; g++) {
                uint32_t kb = 0;
                while (g >= N - (N >> (kb + 1))) kb++;
                const uint32_t j = g - (N - (N >> kb));
                const uint32_t idx = (j << (kb + 1)) + (1u << kb) + delta - 1;
                std::copy_n(&t.skew_tab[(size_t)idx * TAB_DWORDS], 20, img + (size_t)g * 20);
            }
        }

    // eval_poly (src/engine.rs:207-218) = H(log_walsh . H(e)) over 65536
    // points; for e supported on [0, n) and outputs on [0, n) it is the XOR
    // convolution out[i] = sum_j e[j] W[i ^ j], W = H(log_walsh), i.e.
    // H_n(H_n(e) . V) with V = n^-1 H_n(W[0, n)) (n^-1 = 2^(16 - log2 n)
    // mod 65535).  Exact integers, reduced mod 65535.
    {
        std::vector<int64_t> w(GF_ORDER);
        for (uint32_t i = 0; i < GF_ORDER; i++) w[i] = t.log_walsh[i];
        auto fwht = [](int64_t* x, uint32_t n) {
            for (uint32_t d = 1; d < n; d <<= 1)
                for (uint32_t i = 0; i < n; i += 2 * d)
                    for (uint32_t j = i; j < i + d; j++) {
                        const int64_t a = x[j], b = x[j + d];
                        x[j] = a + b;
                        x[j + d] = a - b;
                    }
        };
        auto mod = [](int64_t v) { return (uint32_t)(((v % 65535) + 65535) % 65535); };
        fwht(w.data(), GF_ORDER);
        t.col_k.assign(COL_LGEN + 2, 0);
        {
            int64_t pre = 0;
            for (uint32_t n = 1, j = 0; n <= (2u << COL_LMAX); n <<= 1) {
                for (; j < n; j++) pre += mod(w[j]);
                uint32_t lg = 0;
                while ((1u << lg) < n) lg++;
                if (lg < t.col_k.size()) t.col_k[lg] = mod((int64_t)t.log_walsh[0] - pre);
            }
        }
        t.col_v.assign(COL_V_DWORDS, 0);
        for (uint32_t n = 1u << COL_LMIN; n <= (2u << COL_LMAX); n <<= 1) {
            std::vector<int64_t> v(n);
            for (uint32_t i = 0; i < n; i++) v[i] = mod(w[i]);
            fwht(v.data(), n);
            uint32_t lg = 0;
            while ((1u << lg) < n) lg++;
            const int64_t inv = (int64_t)1 << (16 - lg);  // n^-1 = 2^(16 - log2 n) mod 65535 (2^16 = 1)
            for (uint32_t k = 0; k < n; k++) t.col_v[col_v_offset(n) + k] = mod(mod(v[k]) * inv);
        }
    }
}
}  // namespace

// The general decode's middle pass as a matrix (rs16_engine::mid_matrix):
// DEC_MID maps the 2^hi rows t << lo | j of every tile column j (lo = L / 2,
// hi = L - lo, skew 0) by u = FFT_hi (I + H) IFFT_hi z -- the IFFT / FFT
// layers lo .. L-1 (src/engine/engine_nosimd.rs fft / ifft: twiddle
// skew[r + dist - 1] of the block at global row r, butterflies x ^= y m, y ^= x
// and y ^= x, x ^= y m) around the high-bit half of the formal derivative
// (src/engine.rs formal_derivative: row t takes row t | 2^c for every tile
// bit c clear in t).  The twiddle indices do not involve j, so one 2^hi x
// 2^hi matrix serves every column; entry [o][t] = the log of M[o][t]
// (ZERO_ENTRY for 0), column t computed as the image of the unit vector at t.
std::vector<uint32_t> mid_matrix_entries(const HostTables& t, int L) {
    const int lo = L / 2, hi = L - lo;
    const uint32_t N = 1u << hi;
    const uint16_t one = t.exp[0];  // the element whose log is 0
    std::vector<uint32_t> ent((size_t)N * N, ZERO_ENTRY);
    std::vector<uint16_t> v(N), w(N);
    auto tw = [&](uint32_t r_tile, int kb) {  // twiddle log of the block at tile row r_tile, layer kb
        const uint32_t m = (uint32_t)(lo + kb);
        return (uint32_t)t.skew[((size_t)r_tile << lo) + (1u << m) - 1];
    };
    for (uint32_t c = 0; c < N; c++) {
        std::fill(v.begin(), v.end(), 0);
        v[c] = one;
        for (int kb = 0; kb < hi; kb++) {  // IFFT, low layers first
            const uint32_t d = 1u << kb;
            for (uint32_t r = 0; r < N; r += 2 * d) {
                const uint32_t lm = tw(r, kb);
                for (uint32_t i = r; i < r + d; i++) {
                    v[i + d] ^= v[i];
                    if (lm != GF_MODULUS) v[i] ^= gf_mul(t, v[i + d], lm);
                }
            }
        }
        for (uint32_t i = 0; i < N; i++) {  // (I + H): the formal derivative's tile bits
            uint16_t x = v[i];
            for (uint32_t b = 1; b < N; b <<= 1)
                if (!(i & b)) x ^= v[i | b];
            w[i] = x;
        }
        for (int kb = hi - 1; kb >= 0; kb--) {  // FFT, high layers first
            const uint32_t d = 1u << kb;
            for (uint32_t r = 0; r < N; r += 2 * d) {
                const uint32_t lm = tw(r, kb);
                for (uint32_t i = r; i < r + d; i++) {
                    if (lm != GF_MODULUS) w[i] ^= gf_mul(t, w[i + d], lm);
                    w[i + d] ^= w[i];
                }
            }
        }
        for (uint32_t o = 0; o < N; o++) ent[(size_t)o * N + c] = w[o] ? t.log[w[o]] : ZERO_ENTRY;
    }
    return ent;
}

const HostTables& host_tables() {
    std::call_once(g_once, [] { build(g_tables); });
    return g_tables;
}

}  // namespace rs16
