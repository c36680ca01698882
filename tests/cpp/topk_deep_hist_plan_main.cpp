// Stand-alone check of gorse_amd/csrc/topk_deep_hist_plan.hpp (the host rules of a deep handle's tie path), built by
// tests/test_topk_deep_ties_cpu.py with AddressSanitizer and UBSan.  Walks every width the deep form serves and just outside, prints
// "dtype d groups sort_lds" per width at an edge of the groups rule and "topk_deep_hist_plan ok".
#include <cstdio>
#include <cstdlib>

#include "../../gorse_amd/csrc/topk_deep_hist_plan.hpp"

using namespace gorse::topk_deep_hist_plan;
using gorse::topk_plan::tie_sort_lds_bytes;

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                               \
        }                                                          \
    } while (0)

int main() {
    const size_t cu_lds = (size_t)160 * 1024;
    // the shape: 128 queries per workgroup, a 32 KB slice image, 4 + 4 DMA instructions per wave and slice, vmcnt(8) inside 6 bits
    CHECK(kHistQueries == 128 && kHistQueriesPerWave * kWaves == kHistQueries && kHistQueries == 64 * gorse::topk_plan::kNcbMain);
    CHECK(kHistSliceBytes == (size_t)(kRows + kHistQueries) * kSliceRowBytes && kHistSliceBytes == 32768);
    CHECK(kDmaA * kWaves * 1024 == kRows * kSliceRowBytes && kHistDmaB * kWaves * 1024 == kHistQueries * kSliceRowBytes);
    CHECK(kDmaA == 4 && kHistDmaB == 4 && kHistDmaPerSlice == 8 && 2 * kHistDmaPerSlice + 1 < 63);
    CHECK(hist_lds_bytes() == kBufs * kHistSliceBytes + 2 * kRows * 4 + 5 * kHistQueries * 4 && hist_lds_bytes() == 101888);
    CHECK(hist_lds_bytes() <= cu_lds && kDeepHistTileRows == kRows);
    for (int bf = 0; bf < 2; bf++) {
        const int top = bf ? kMaxBf16D : kMaxF32D;
        for (int d = 1, last = 0; d <= top + 64; d++) {
            const int g = tie_sort_groups(d);
            CHECK(g == 16 || g == 8 || g == 4 || g == 2 || g == 1);
            CHECK(g == 16 || tie_sort_lds_bytes(d, 2 * g) > cu_lds);            // no larger power of two fits ...
            if (d <= top) CHECK(g >= 2 && tie_sort_lds_bytes(d, g) <= cu_lds);  // ... and at every served width one of the kernel's forms does
            if (serves(bf, d)) {  // whole K-slices, at least two per tile; a lane's 32-bit source offsets
                const size_t pad = padded_depth(bf, d);
                CHECK(pad % kSlice == 0 && pad >= 2 * kSlice && (size_t)(kHistQueries - 1) * pad * 2 + kSliceRowBytes <= 0xffffffffu);
            }
            if (g != last || d == top) printf("%s %d %d %zu\n", bf ? "bf16" : "f32", d, g, tie_sort_lds_bytes(d, g));
            last = g;
        }
    }
    CHECK(tie_sort_groups(1445) == 16 && tie_sort_groups(1446) == 8 && tie_sort_groups(4096) == 4 && tie_sort_lds_bytes(4096, 4) == 147472);
    printf("topk_deep_hist_plan ok\n");
    return 0;
}
