// Stand-alone check of the host tables: builds them (rs16_tables.cpp runs its
// consistency checks while it does, and aborts on a failure -- sentinel and
// narrow index rules, the tower basis, the tower tables of subfield twiddles,
// beta^2 = beta + v_7, the three-map wide multiply and the c1 = 1 rule), then
// runs the two wide tower multiplies on the table of every index the passes stage.  Meant for a sanitizer
// build on the host, no device involved:
//   hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -I reed-solomon-16_amd/csrc \
//       tools/tables_check.cpp reed-solomon-16_amd/csrc/rs16_tables.cpp -o tools/tables_check && tools/tables_check
#include <cstdio>

#include "rs16_internal.hpp"

int main() {
    using namespace rs16;
    const HostTables& t = host_tables();
    if (t.skew_tab.size() != (size_t)GF_ORDER * TAB_DWORDS || t.skew_tab_tower.size() != t.skew_tab.size()) {
        fprintf(stderr, "tables_check: twiddle table sizes\n");
        return 1;
    }
    // every index a first or last pass of a 2^15-row chunk stages, and the middle pass's wide layer
    uint32_t acc = 0, n = 0;
    for (uint32_t x = 1; x < GF_ORDER; x++) {
        if (x % 128 == 0 && !twiddle_beta(x - 1)) continue;
        const uint32_t* e = &t.skew_tab_tower[(size_t)(x - 1) * TAB_DWORDS];
        uint32_t l = 0, h = 0;
        mul_xor_tower_wide(l, h, x * 0x9E3779B9u, x * 0x85EBCA6Bu, e);
        if (twiddle_beta(x - 1)) {
            uint32_t l2 = 0, h2 = 0;
            mul_xor_tower_beta(l2, h2, x * 0x9E3779B9u, x * 0x85EBCA6Bu, e);
            if (l2 != l || h2 != h) {
                fprintf(stderr, "tables_check: the c1 = 1 multiply differs from the three-map one at index %u\n", x - 1);
                return 1;
            }
        }
        acc ^= l ^ h, n++;
    }
    printf("tables_check ok: %u twiddles, checksum %08x\n", n, acc);
    return 0;
}
