// Stand-alone check of gorse_amd/csrc/rec_sweep_plan.hpp (the pilot schedule's sample stride, the sample's bound inside LDS, the
// survivor capacity, the slices of the two matrix launches, the launch round, the score keys), built by tests/test_rec_sweep_cpu.py
// with AddressSanitizer and UBSan.  Prints "rec_sweep_plan ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../gorse_amd/csrc/rec_sweep_plan.hpp"

using namespace gorse::recsweep;

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                               \
        }                                                          \
    } while (0)

static uint32_t bits(float x) {
    uint32_t b;
    memcpy(&b, &x, 4);
    return b;
}

static void check_plan(int64_t I, int32_t k, int64_t n_users, int32_t hint) {
    const Plan p = make_plan(I, k, n_users, hint);
    CHECK(p.kk == k + 1 && p.stride >= 1);
    CHECK(p.n_sample == ceil_div64(I, p.stride) && (int64_t)(p.n_sample - 1) * p.stride < I);  // the last sampled item exists
    CHECK(p.n_sample <= kMaxSample && p.samp_ld % kTile == 0 && p.samp_ld >= p.n_sample && p.samp_ld < p.n_sample + kTile);
    CHECK(p.select_lds == ((size_t)p.n_sample + 256) * 4 && p.select_lds <= (size_t)kLdsBytes);
    CHECK(p.cap >= 1 && p.cap <= kMaxCap && p.finish_lds <= (size_t)kLdsBytes);
    CHECK(p.cap == kMaxCap || p.cap >= 2 * p.kk * p.stride);
    CHECK(p.stride == 1 || p.n_sample >= 4 * p.kk || p.stride == ceil_div64(I, kMaxSample));
    CHECK(p.chunk >= 1 && p.chunk <= n_users && (p.chunk == n_users || p.chunk % kQueries == 0));
    CHECK(p.chunk == n_users || p.chunk == kQueries || (size_t)p.chunk * p.per_query_bytes <= kScratchBytes);
    CHECK(p.per_query_bytes >= (size_t)p.samp_ld * 4 + (size_t)p.cap * 8);
    // the slices cover their items exactly once, each starts on a tile edge and none is empty
    const int64_t n[2] = {p.n_sample, I};
    const int32_t sl[2] = {p.pilot_slices, p.sweep_slices}, len[2] = {p.pilot_slice_len, p.sweep_slice_len};
    for (int x = 0; x < 2; x++) {
        CHECK(sl[x] >= 1 && sl[x] <= kMaxSlices && len[x] % kTile == 0);
        CHECK((int64_t)sl[x] * len[x] >= n[x] && (int64_t)(sl[x] - 1) * len[x] < n[x]);
    }
}

int main() {
    const int64_t items[] = {1, 2, 31, 32, 33, 257, 1000, 4099, 32768, 32769, 200000, 524288, 524289, 1000000, 2147483647};
    const int32_t ks[] = {1, 2, 10, 100, 255, 256};
    const int64_t users[] = {1, 127, 128, 129, 6040, 65536, 10000000};
    const int32_t hints[] = {0, 1, 8, 32, 1000};
    for (int64_t I : items)
        for (int32_t k : ks)
            for (int64_t u : users)
                for (int32_t h : hints) check_plan(I, k, u, h);
    // the shapes the README measures, and the rules' corners
    Plan p = make_plan(200000, 100, 65536, 0);
    CHECK(p.stride == kBaseStride && p.n_sample == 12500 && p.cap == 2 * 101 * 16 + 128);
    p = make_plan(33, 100, 7, 0);
    CHECK(p.stride == 1 && p.n_sample == 33 && p.chunk == 7 && p.pilot_slices == 1 && p.sweep_slices == 1);
    p = make_plan(4099, 1, 3, 0);
    CHECK(p.stride == 16 && p.n_sample == 257 && p.cap == 192);
    p = make_plan(1000000, 100, 1000, 0);
    CHECK(p.stride == 31 && p.n_sample <= kMaxSample);
    CHECK(serves(16, 1) && serves(256, 256) && !serves(48 + 8, 10) && !serves(272, 10) && !serves(0, 10) && !serves(64, 257) && !serves(64, 0));
    // keys ascend with the score, round-trip, and keep 0 and kKeyNaN free for every number
    const std::vector<float> asc = {-INFINITY, -3.0f, -1e-45f, -0.0f, 0.0f, 1e-45f, 2.5f, INFINITY};
    for (size_t a = 0; a < asc.size(); a++) {
        const uint32_t key = score_key(bits(asc[a]));
        CHECK(key != 0 && key != kKeyNaN && key_score_bits(key) == bits(asc[a]));
        if (a) CHECK(score_key(bits(asc[a - 1])) < key);
    }
    printf("rec_sweep_plan ok\n");
    return 0;
}
