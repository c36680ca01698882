// Stand-alone check of gorse_amd/csrc/nbr_plan.hpp (validation of gorse_nbr_set_table / gorse_nbr_recommend, the bounds and the
// launch planner), built by tests/test_nbr_cpu.py with AddressSanitizer and UBSan.  Prints "nbr_plan ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>

#include "../../gorse_amd/csrc/nbr_plan.hpp"

using namespace gorse::nbr;

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                               \
        }                                                          \
    } while (0)

static int32_t table(int32_t which, const std::vector<int64_t> &ptr, const std::vector<int32_t> &idx, const std::vector<float> *w,
                     int32_t transform, double scale, int64_t n_items, int64_t *mx = nullptr) {
    std::string msg;
    const int32_t rc = validate_table(which, (int64_t)ptr.size() - 1, ptr.data(), idx.empty() ? nullptr : idx.data(), w ? w->data() : nullptr,
                                      transform, scale, n_items, mx, &msg);
    CHECK((rc == GORSE_OK) == msg.empty());
    return rc;
}

static void check_tables() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> w{0.5f, 0.25f, 1.0f, 2.0f};
    int64_t mx = -2;
    CHECK(table(GORSE_NBR_HOP2, {0, 2, 2, 4}, {1, 9, 0, 3}, &w, GORSE_NBR_RECIP, 1.0, 10, &mx) == GORSE_OK && mx == 9);
    CHECK(table(GORSE_NBR_HOP2, {0}, {}, nullptr, 0, 1.0, 10, &mx) == GORSE_OK && mx == -1);  // no rows
    CHECK(table(GORSE_NBR_HOP2, {0, 0, 0}, {}, &w, 0, 1.0, 10, &mx) == GORSE_OK && mx == -1);  // empty rows
    // ranges: a hop-2 index outside [0, n_items), any negative index; hop 1 is held against hop 2's rows only at the call
    CHECK(table(GORSE_NBR_HOP2, {0, 2, 2, 4}, {1, 10, 0, 3}, &w, 0, 1.0, 10) == GORSE_ERR_RANGE);
    CHECK(table(GORSE_NBR_HOP2, {0, 2, 2, 4}, {1, -1, 0, 3}, nullptr, 0, 1.0, 10) == GORSE_ERR_RANGE);
    CHECK(table(GORSE_NBR_HOP1, {0, 2, 2, 4}, {1, -1, 0, 3}, nullptr, 0, 1.0, 10) == GORSE_ERR_RANGE);
    CHECK(table(GORSE_NBR_HOP1, {0, 2, 2, 4}, {1, 1000, 0, 3}, nullptr, 0, 1.0, 10, &mx) == GORSE_OK && mx == 1000);
    // repeats: refused in a weighted hop-2 row only
    CHECK(table(GORSE_NBR_HOP2, {0, 1, 4}, {3, 3, 5, 3}, &w, 0, 1.0, 10) == GORSE_ERR_INVALID);
    CHECK(table(GORSE_NBR_HOP2, {0, 2, 4}, {3, 5, 5, 3}, &w, 0, 1.0, 10) == GORSE_OK);  // across rows
    CHECK(table(GORSE_NBR_HOP2, {0, 1, 4}, {3, 3, 5, 3}, nullptr, 0, 1.0, 10) == GORSE_OK);
    CHECK(table(GORSE_NBR_HOP1, {0, 1, 4}, {3, 3, 5, 3}, &w, 0, 1.0, 10) == GORSE_OK);
    // weights, transform, scale, shape
    for (float bad : {inf, -inf, nan}) {
        std::vector<float> wb{0.5f, 0.25f, bad, 2.0f};
        CHECK(table(GORSE_NBR_HOP1, {0, 2, 2, 4}, {1, 2, 0, 3}, &wb, 0, 1.0, 10) == GORSE_ERR_INVALID);
        CHECK(table(GORSE_NBR_HOP2, {0, 2, 2, 4}, {1, 2, 0, 3}, &wb, 1, 1.0, 10) == GORSE_ERR_INVALID);
        CHECK(table(GORSE_NBR_HOP2, {0, 2, 2, 4}, {1, 2, 0, 3}, &w, 0, (double)bad, 10) == GORSE_ERR_INVALID);
    }
    CHECK(table(GORSE_NBR_HOP2, {0, 2, 2, 4}, {1, 2, 0, 3}, &w, 2, 1.0, 10) == GORSE_ERR_INVALID);
    CHECK(table(GORSE_NBR_HOP2, {0, 2, 2, 4}, {1, 2, 0, 3}, nullptr, 2, std::nan(""), 10) == GORSE_OK);  // ignored without weights
    CHECK(table(2, {0, 2, 2, 4}, {1, 2, 0, 3}, &w, 0, 1.0, 10) == GORSE_ERR_INVALID);
    CHECK(table(-1, {0, 2, 2, 4}, {1, 2, 0, 3}, &w, 0, 1.0, 10) == GORSE_ERR_INVALID);
    CHECK(table(GORSE_NBR_HOP2, {0, 2, 1, 4}, {1, 2, 0, 3}, &w, 0, 1.0, 10) == GORSE_ERR_INVALID);
    CHECK(table(GORSE_NBR_HOP2, {1, 2, 2, 4}, {1, 2, 0, 3}, &w, 0, 1.0, 10) == GORSE_ERR_INVALID);
    CHECK(table(GORSE_NBR_HOP2, {0, 2}, {}, nullptr, 0, 1.0, 10) == GORSE_ERR_INVALID);  // entries without indices
    std::string msg;
    CHECK(validate_table(GORSE_NBR_HOP2, 1, nullptr, nullptr, nullptr, 0, 1.0, 10, nullptr, &msg) == GORSE_ERR_INVALID);
    CHECK(validate_table(GORSE_NBR_HOP2, -1, nullptr, nullptr, nullptr, 0, 1.0, 10, nullptr, &msg) == GORSE_ERR_INVALID);
}

static int32_t call(int64_t n, const std::vector<int32_t> *rows, int32_t k, const std::vector<int64_t> *sp, const std::vector<int32_t> *si,
                    int64_t n_rows1, int64_t n_items) {
    std::string msg;
    const int32_t rc = validate_call(n, rows ? rows->data() : nullptr, k, sp ? sp->data() : nullptr, si ? si->data() : nullptr, n_rows1,
                                     n_items, &msg);
    CHECK((rc == GORSE_OK) == msg.empty());
    return rc;
}

static void check_calls() {
    const std::vector<int32_t> rows{0, 4, -1, 4}, beyond{0, 5}, seen{3, 3, 9, 0}, seen_hi{3, 10}, seen_lo{-1, 3};
    const std::vector<int64_t> sp{0, 1, 1, 3, 4}, sp_off{2, 2, 3, 4, 4}, sp_bad{0, 2, 1, 3, 4}, sp2{0, 1, 2};
    CHECK(call(4, &rows, 1, &sp, &seen, 5, 10) == GORSE_OK);
    CHECK(call(4, &rows, GORSE_NBR_MAX_K, &sp_off, &seen, 5, 10) == GORSE_OK);
    CHECK(call(4, &rows, 10, nullptr, nullptr, 5, 10) == GORSE_OK);
    CHECK(call(5, nullptr, 10, nullptr, nullptr, 5, 10) == GORSE_OK);
    CHECK(call(0, nullptr, 10, nullptr, nullptr, 5, 10) == GORSE_OK);
    for (int32_t k : {0, -1, GORSE_NBR_MAX_K + 1}) CHECK(call(4, &rows, k, &sp, &seen, 5, 10) == GORSE_ERR_INVALID);
    CHECK(call(-1, nullptr, 10, nullptr, nullptr, 5, 10) == GORSE_ERR_INVALID);
    CHECK(call(2, &beyond, 10, nullptr, nullptr, 5, 10) == GORSE_ERR_RANGE);
    CHECK(call(6, nullptr, 10, nullptr, nullptr, 5, 10) == GORSE_ERR_RANGE);
    CHECK(call(2, &rows, 10, &sp2, &seen_hi, 5, 10) == GORSE_ERR_RANGE);
    CHECK(call(2, &rows, 10, &sp2, &seen_lo, 5, 10) == GORSE_ERR_RANGE);
    CHECK(call(4, &rows, 10, &sp_bad, &seen, 5, 10) == GORSE_ERR_INVALID);
    CHECK(call(2, &rows, 10, &sp2, nullptr, 5, 10) == GORSE_ERR_INVALID);
}

static void check_bounds() {
    // hop 2: rows of 3, 0, 5 and 2 entries; hop 1 repeats a source
    const std::vector<int64_t> ptr2{0, 3, 3, 8, 10}, ptr1{0, 0, 1, 4, 6};
    const std::vector<int32_t> idx1{1, 0, 2, 0, 3, 2};
    std::vector<int64_t> sum;
    row_bounds(4, ptr1.data(), idx1.data(), ptr2.data(), &sum);
    CHECK((sum == std::vector<int64_t>{0, 0, 11, 7}));
    CHECK(query_bound(100, 11, 4) == 15 && query_bound(8, 11, 4) == 12 && query_bound(8, 0, 0) == 0);
    row_bounds(0, ptr1.data(), idx1.data(), ptr2.data(), &sum);
    CHECK(sum.empty());
}

// every property a plan must have, written without looking at how make_plan walks
static void check_plan(const std::vector<int64_t> &bound, int32_t lds_slots, int64_t chunk, int64_t scratch) {
    Plan P;
    CHECK(make_plan((int64_t)bound.size(), bound.data(), lds_slots, chunk, scratch, &P));
    const int64_t n = (int64_t)bound.size();
    const int32_t lds = std::max(2, std::min(lds_slots, kMaxLdsSlots));
    CHECK((int64_t)P.order.size() == n && (int64_t)P.cap.size() == n && (int64_t)P.off.size() == n && P.n_lds + P.n_global == n);
    std::vector<int> hit((size_t)n, 0);
    int64_t at = 0, n_lds = 0;
    for (const Launch &L : P.launches) {
        CHECK(L.q0 == at && L.q1 > L.q0 && L.q1 <= n);
        CHECK(chunk <= 0 || L.q1 - L.q0 <= chunk);
        CHECK(L.threads == (L.slots > 0 && L.slots <= kWaveSlots ? 64 : 256));
        int64_t used = 0;
        for (int64_t p = L.q0; p < L.q1; p++) {
            const int32_t t = P.order[(size_t)p];
            CHECK(t >= 0 && t < n && hit[(size_t)t]++ == 0);
            CHECK(P.cap[(size_t)p] >= bound[(size_t)t] + 1);  // a free slot always remains: the probe ends
            if (L.slots > 0) {
                CHECK(P.cap[(size_t)p] == L.slots && L.slots <= lds && P.off[(size_t)p] == 0);
                CHECK(bound[(size_t)t] + 1 <= lds);
                n_lds++;
            } else {
                CHECK(bound[(size_t)t] + 1 > lds);  // only what no LDS table holds
                CHECK(P.off[(size_t)p] == used);    // the launch's tables lie side by side
                used += P.cap[(size_t)p];
            }
            if (p > L.q0) CHECK(P.order[(size_t)p - 1] < t);
        }
        CHECK(L.slots > 0 || used <= scratch || L.q1 - L.q0 == 1);
        at = L.q1;
    }
    CHECK(at == n && n_lds == P.n_lds);
}

static void check_plans() {
    check_plan({}, 0, 0, kScratchSlots);
    const std::vector<int64_t> edges{0, 1, 2, 510, 511, 512, 4094, 4095, 4096, 13054, 13055, 13056, 100000, 0, 511, 13055};
    for (int32_t lds : {kMaxLdsSlots, 1, 2, 3, 64, 512, 513, 4096, 5000, 1 << 20})
        for (int64_t chunk : {(int64_t)0, (int64_t)1, (int64_t)3, (int64_t)100})
            for (int64_t scratch : {(int64_t)1, (int64_t)20000, kScratchSlots}) check_plan(edges, lds, chunk, scratch);
    std::mt19937_64 rng(5);
    for (int rep = 0; rep < 50; rep++) {
        std::vector<int64_t> b((size_t)(rng() % 200));
        for (auto &x : b) x = (int64_t)(rng() % (rep % 2 ? 40000 : 700));
        check_plan(b, (int32_t)(rng() % 20000), (int64_t)(rng() % 50), (int64_t)(1 + rng() % 100000));
    }
    Plan P;
    const std::vector<int64_t> huge{(int64_t)1 << 31};
    CHECK(!make_plan(1, huge.data(), kMaxLdsSlots, 0, kScratchSlots, &P));
}

int main() {
    check_tables();
    check_calls();
    check_bounds();
    check_plans();
    printf("nbr_plan ok\n");
    return 0;
}
