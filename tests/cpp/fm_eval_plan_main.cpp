// Stand-alone check of gorse_amd/csrc/fm_eval_plan.hpp (the partition of gorse_fm_set_test and the slice and round planner of
// gorse_fm_evaluate and gorse_fm_rank_users), built by tests/test_fm_evaluate_cpu.py with AddressSanitizer and UBSan.  Prints
// "fm_eval_plan ok".
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

// every property a plan must have, written without looking at how plan_slices walks.  item = NULL: a row's item is the row.
static void check_plan(const std::vector<int64_t> &ptr, const int32_t *item, int32_t bs, int64_t R) {
    const int64_t n_segs = (int64_t)ptr.size() - 1, n = ptr.back(), cap = std::max<int64_t>(R, bs);
    SlicePlan sl;
    plan_slices(ptr.data(), n_segs, item, bs, R, sl);
    CHECK((int64_t)sl.desc.size() == 4 * n);
    CHECK(sl.round_begin.front() == 0);
    int64_t want_slices = 0;
    for (int64_t s = 0; s < n_segs; s++) want_slices += (ptr[(size_t)s + 1] - ptr[(size_t)s] + bs - 1) / bs;
    CHECK(sl.n_slices == want_slices);
    if (n == 0) {
        CHECK(sl.rounds() == 0 && sl.n_slices == 0 && sl.max_round == 0);
        return;
    }
    CHECK(sl.round_begin.back() == n);
    const int32_t *seg = sl.desc.data(), *it = seg + n, *row0 = it + n, *len = row0 + n;
    int64_t slices = 0, widest = 0, s = 0;
    for (int64_t k = 0; k < sl.rounds(); k++) {
        const int64_t r0 = sl.round_begin[(size_t)k], r1 = sl.round_begin[(size_t)k + 1];
        CHECK(r1 > r0 && (r1 - r0 <= cap));
        widest = std::max(widest, r1 - r0);
        for (int64_t r = r0; r < r1;) {
            // a slice starts here: it lies inside one segment and inside the round, and is full unless it ends its segment
            while (ptr[(size_t)s + 1] <= r) s++;  // the segment that holds r (empty ones are passed over)
            const int64_t seg_begin = ptr[(size_t)s], seg_end = ptr[(size_t)s + 1];
            const int64_t want = std::min<int64_t>(bs, seg_end - r);
            CHECK((r - seg_begin) % bs == 0);
            CHECK(r + want <= r1);
            for (int64_t q = r; q < r + want; q++) {
                CHECK(seg[q] == s);
                CHECK(it[q] == (item ? item[q] : q));
                CHECK(row0[q] == r - r0);
                CHECK(len[q] == want);
            }
            r += want;
            slices++;
        }
    }
    CHECK(slices == sl.n_slices);
    CHECK(widest == sl.max_round);
}

// a test split: the positives, then the negatives
static void check_split(int64_t n_pos, int64_t n_neg, int32_t bs, int64_t R) { check_plan({0, n_pos, n_pos + n_neg}, nullptr, bs, R); }

// users' candidate lists of the given lengths; the candidates are numbers that are not the rows'
static void check_users(const std::vector<int64_t> &lens, int32_t bs, int64_t R) {
    std::vector<int64_t> ptr{0};
    for (int64_t l : lens) ptr.push_back(ptr.back() + l);
    std::vector<int32_t> cand((size_t)ptr.back());
    for (size_t r = 0; r < cand.size(); r++) cand[r] = (int32_t)((r * 7919 + 13) % 1000);
    check_plan(ptr, cand.data(), bs, R);
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
        for (int64_t R : {(int64_t)0, (int64_t)bs, (int64_t)2 * bs, (int64_t)2 * bs + 3, (int64_t)1 << 20}) {
            for (int64_t np : {(int64_t)0, (int64_t)1, (int64_t)bs - 1, (int64_t)bs, (int64_t)bs + 1, (int64_t)3 * bs + 2})
                for (int64_t nn : {(int64_t)0, (int64_t)1, (int64_t)bs - 1, (int64_t)bs, (int64_t)bs + 1, (int64_t)2 * bs + 5})
                    check_split(np, nn, bs, R);
            // ranking: R = 0 and R = bs lie below or at bs (a round is then one slice), 2 bs + 3 is exceeded by the long lists
            const int64_t b = bs, big = 5 * b + 3;
            check_users({}, bs, R);                              // no user
            check_users({0}, bs, R);                             // a total of 0
            check_users({0, 0, 0}, bs, R);
            for (int64_t l : {b - 1, b, b + 1, big}) check_users({l}, bs, R);  // 1 user: one below, at, one above bs; beyond R
            check_users({0, b + 1, 2, big}, bs, R);              // no candidates at the front
            check_users({b + 1, 0, 0, 2, big, b}, bs, R);        // in the middle
            check_users({3, b - 1, big, b, 0}, bs, R);           // at the end
            check_users({0, b, 0, b + 1, 0}, bs, R);             // all three
            std::vector<int64_t> many;
            for (int64_t t = 0; t < 50; t++) many.push_back((t * 5 + 3) % (2 * b + 2));
            check_users(many, bs, R);                            // many users, every length from 0 to 2 bs + 1
        }
    // R below bs is raised to bs: no slice is split, every round is one slice
    {
        SlicePlan sl;
        const int64_t ptr[] = {0, 20, 20, 33};
        plan_slices(ptr, 3, nullptr, 7, 3, sl);
        CHECK(sl.n_slices == 5 && sl.rounds() == 5 && sl.max_round == 7);
        CHECK(round_rows_for(0, 16, 7, 3) == 7 && round_rows_for(0, 16, 7, 14) == 14);
        CHECK(round_rows_for(766, 16, 1024, 0) == kRoundBytes / (800 * 4));
        CHECK(round_rows_for(4096, 128, 1 << 20, 0) == 1 << 20);
    }
    // a slice boundary never runs on through the first negative
    {
        SlicePlan sl;
        const int64_t sides[] = {0, 10, 20};
        plan_slices(sides, 2, nullptr, 7, 1000, sl);
        const int32_t *seg = sl.desc.data(), *len = seg + 60;
        CHECK(len[0] == 7 && len[7] == 3 && len[9] == 3 && len[10] == 7 && len[17] == 3);
        CHECK(seg[9] == 0 && seg[10] == 1);
        CHECK(sl.rounds() == 1 && sl.n_slices == 4);
    }
    // embedding offsets are 64-bit: the last row of the largest table lies far beyond 2^31 elements
    CHECK(eval_emb_offset((int64_t)INT32_MAX - 1, 4096) == ((int64_t)INT32_MAX - 1) * 4096);
    CHECK(eval_emb_offset(1 << 20, 4096) == (int64_t)1 << 32);
    printf("fm_eval_plan ok\n");
    return 0;
}
