// Stand-alone check of gorse_amd/csrc/fm_eval_plan.hpp (the partition and the slice descriptors of gorse_fm_set_test /
// gorse_fm_evaluate), built by tests/test_fm_evaluate_cpu.py with AddressSanitizer and UBSan.  Prints "fm_eval_plan ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../gorse_amd/csrc/fm_eval_plan.hpp"

using namespace gorse::fm;

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                               \
        }                                                          \
    } while (0)

// every property a plan must have, written without looking at how eval_slices walks
static void check_plan(int64_t n_pos, int64_t n_neg, int32_t bs, int64_t R) {
    EvalSlices sl;
    eval_slices(n_pos, n_neg, bs, R, sl);
    const int64_t n = n_pos + n_neg, cap = std::max<int64_t>(R, bs);
    CHECK((int64_t)sl.desc.size() == 3 * n);
    CHECK(sl.round_begin.front() == 0);
    if (n == 0) {
        CHECK(sl.rounds() == 0 && sl.n_slices == 0 && sl.max_round == 0);
        return;
    }
    CHECK(sl.round_begin.back() == n);
    const int32_t *row = sl.desc.data(), *row0 = row + n, *len = row0 + n;
    int64_t slices = 0, widest = 0;
    for (int64_t k = 0; k < sl.rounds(); k++) {
        const int64_t r0 = sl.round_begin[(size_t)k], r1 = sl.round_begin[(size_t)k + 1];
        CHECK(r1 > r0 && (r1 - r0 <= cap));
        widest = std::max(widest, r1 - r0);
        for (int64_t r = r0; r < r1;) {
            // a slice starts here: it lies inside one side and inside the round, and is full unless it ends its side
            const int64_t side_end = r < n_pos ? n_pos : n, side_begin = r < n_pos ? 0 : n_pos;
            const int64_t want = std::min<int64_t>(bs, side_end - r);
            CHECK((r - side_begin) % bs == 0);
            CHECK(r + want <= r1);
            for (int64_t q = r; q < r + want; q++) {
                CHECK(row[q] == q);
                CHECK(row0[q] == r - r0);
                CHECK(len[q] == want);
            }
            r += want;
            slices++;
        }
    }
    CHECK(slices == sl.n_slices);
    CHECK(widest == sl.max_round);
    CHECK(sl.n_slices == (n_pos + bs - 1) / bs + (n_neg + bs - 1) / bs);
}

int main() {
    // the partition: positives first, then the others, both in dataset order; 0 and NaN are negatives
    {
        const float t[] = {1.0f, -1.0f, 0.0f, 2.0f, -0.0f, NAN, 1e-45f, -1.0f};
        std::vector<int32_t> order;
        CHECK(eval_partition(t, 8, order) == 3);
        const int32_t want[] = {0, 3, 6, 1, 2, 4, 5, 7};
        for (int i = 0; i < 8; i++) CHECK(order[(size_t)i] == want[i]);
        CHECK(eval_partition(t, 0, order) == 0 && order.empty());
        const float allp[] = {1, 1, 1}, alln[] = {-1, 0, -1};
        CHECK(eval_partition(allp, 3, order) == 3 && order[0] == 0 && order[2] == 2);
        CHECK(eval_partition(alln, 3, order) == 0 && order[0] == 0 && order[2] == 2);
    }
    // slices: the empty split, one side empty, n one below, at and one above the batch size, rounds of every width
    const int32_t bss[] = {1, 7, 64};
    for (int32_t bs : bss)
        for (int64_t R : {(int64_t)0, (int64_t)bs, (int64_t)2 * bs, (int64_t)2 * bs + 3, (int64_t)1 << 20})
            for (int64_t np : {(int64_t)0, (int64_t)1, (int64_t)bs - 1, (int64_t)bs, (int64_t)bs + 1, (int64_t)3 * bs + 2})
                for (int64_t nn : {(int64_t)0, (int64_t)1, (int64_t)bs - 1, (int64_t)bs, (int64_t)bs + 1, (int64_t)2 * bs + 5})
                    check_plan(np, nn, bs, R);
    // a slice boundary never runs on through the first negative
    {
        EvalSlices sl;
        eval_slices(10, 10, 7, 1000, sl);
        const int32_t *len = sl.desc.data() + 40;
        CHECK(len[0] == 7 && len[7] == 3 && len[9] == 3 && len[10] == 7 && len[17] == 3);
        CHECK(sl.rounds() == 1 && sl.n_slices == 4);
    }
    // embedding offsets are 64-bit: the last row of the largest table lies far beyond 2^31 elements
    CHECK(eval_emb_offset((int64_t)INT32_MAX - 1, 4096) == ((int64_t)INT32_MAX - 1) * 4096);
    CHECK(eval_emb_offset(1 << 20, 4096) == (int64_t)1 << 32);
    printf("fm_eval_plan ok\n");
    return 0;
}
