// Stand-alone check of gorse_amd/csrc/topk_deep_plan.hpp (the host-side rules of the deep sweep form of the exact top-k), built by
// tests/test_topk_deep_cpu.py with AddressSanitizer and UBSan.  Walks every width in the served ranges and just outside them, prints
// one line "dtype d serves padded slices groups" per width at an edge of a rule and "topk_deep_plan ok".
#include <cstdio>
#include <cstdlib>

#include "../../gorse_amd/csrc/topk_deep_plan.hpp"

using namespace gorse::topk_deep_plan;
using gorse::topk_plan::operand_depth;
using gorse::topk_plan::rescore_lds_bytes;

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                               \
        }                                                          \
    } while (0)

int main() {
    CHECK(kDmaPerSlice == 12 && kSliceBytes == 49152 && lds_bytes() == 152576 && kQueries == 256 && kThreads == 256);
    CHECK(kMinDeepQueries == gorse::topk_plan::kMinSweepQueries);
    for (int bf = 0; bf < 2; bf++) {
        const int top = bf ? kMaxBf16D : kMaxF32D;
        int last_groups = 0;
        for (int d = 1; d <= top + 64; d++) {
            const bool s = serves(bf, d);
            const int pad = padded_depth(bf, d);
            CHECK(s == (operand_depth(bf, d) == 0 && d <= top));  // exactly the widths the register-resident form leaves, up to the limit
            CHECK((pad != 0) == s && slices(bf, d) * kSlice == pad);
            const int g = rescore_groups(d);
            CHECK(g == 16 || g == 8 || g == 4 || g == 2 || g == 1);
            CHECK(rescore_lds_bytes(d, g) <= (size_t)144 * 1024);                            // the staging fits ...
            CHECK(g == 16 || rescore_lds_bytes(d, 2 * g) > (size_t)144 * 1024);              // ... and no larger power of two does
            if (s) {
                CHECK(pad % kSlice == 0 && pad >= operand_values(bf, d) && pad - operand_values(bf, d) < kSlice);
                CHECK(slices(bf, d) >= 2 && pad % 16 == 0 && pad / 16 > 24);                 // deeper than every register-resident depth
                CHECK((size_t)(kQueries - 1) * pad * 2 + kSliceRowBytes <= 0xffffffffu);     // a lane's 32-bit source offset
            }
            if (s != serves(bf, d - 1) || s != serves(bf, d + 1) || g != last_groups || (s && pad != padded_depth(bf, d + 1)))
                printf("%s %d %d %d %d %d\n", bf ? "bf16" : "f32", d, (int)s, pad, slices(bf, d), g);
            last_groups = g;
        }
    }
    CHECK(!serves(true, 384) && serves(true, 385) && serves(true, 4096) && !serves(true, 4097));
    CHECK(!serves(false, 128) && serves(false, 129) && serves(false, 1536) && !serves(false, 1537));
    CHECK(padded_depth(true, 385) == 448 && padded_depth(true, 400) == 448 && padded_depth(true, 1024) == 1024 && padded_depth(true, 4096) == 4096);
    CHECK(padded_depth(false, 129) == 448 && padded_depth(false, 340) == 1024 && padded_depth(false, 1536) == 4608);
    CHECK(rescore_groups(1024) == 16 && rescore_groups(1536) == 8 && rescore_groups(4096) == 2);
    printf("topk_deep_plan ok\n");
    return 0;
}
