// Stand-alone check of csrc/als_deep_plan.hpp (built with -fsanitize=address,undefined by tests/test_als_deep_cpu.py): for every
// served block count the blocks' numbering is a bijection, every element of the symmetric matrix maps into the packed triangle (LDS
// and global layouts), (i, j) and (j, i) of different blocks map to the same place, distinct elements of the block triangle to distinct places, and the
// gather ring fits inside M's region of the LDS budget.
#include <cstdio>
#include <vector>

#include "als_deep_plan.hpp"

using namespace gorse;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("%s:%d: %s (nb %d)\n", __FILE__, __LINE__, #c, nb); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

int main() {
    for (int d = kDeepMinD; d <= kDeepMaxD; d++) {
        const int nb = deep_nb(d), nt = deep_nt(nb);
        CHECK(deep_serves(d) && nb >= 5 && nb <= 8 && 32 * nb >= d && 32 * (nb - 1) < d);
        for (int t = 0; t < nt; t++) {
            const int bi = deep_tile_bi(nb, t), bj = deep_tile_bj(nb, t);
            CHECK(bi >= 0 && bi <= bj && bj < nb && deep_tile(nb, bi, bj) == t);
        }
        std::vector<int> lds((size_t)nt * kDeepTileLds, 0), mem((size_t)deep_packed(nb), 0);
        for (int i = 0; i < 32 * nb; i++)
            for (int j = 0; j < 32 * nb; j++) {
                const int l = deep_lds_index(nb, i, j), m = deep_mem_index(nb, i, j);
                if (i / 32 != j / 32) CHECK(l == deep_lds_index(nb, j, i) && m == deep_mem_index(nb, j, i));  // (a diagonal block is stored whole)
                if (i / 32 <= j / 32) {
                    CHECK(lds.at(l)++ == 0);
                    CHECK(mem.at(m)++ == 0);
                }
            }
        CHECK(deep_ring_bytes(nb) <= (size_t)nt * kDeepTileLds * sizeof(float));
        CHECK(deep_lds_bytes(nb) <= 160 * 1024);
        CHECK(deep_partial_stride(nb) == deep_packed(nb) + 32 * nb && (size_t)deep_packed(nb) <= (size_t)d * d);
    }
    const int nb = 0;
    CHECK(!deep_serves(128) && !deep_serves(257));
    std::printf("als_deep_plan ok\n");
    return 0;
}
