// Stand-alone check of gorse_amd/csrc/cand_plan.hpp (the validation every gorse_cand_* call runs before it launches or replaces
// anything), built by tests/test_cand_cpu.py with AddressSanitizer and UBSan.  Prints "cand_plan ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gorse_amd/csrc/cand_plan.hpp"

using namespace gorse::cand;

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                               \
        }                                                          \
    } while (0)

// exactly sized heap copies: a read past the end is the sanitizer's to find
static int32_t begin(int64_t nq, const std::vector<int64_t> *ptr, const std::vector<int32_t> &items, int32_t capacity, int64_t n_items) {
    std::string msg;
    const int32_t rc = validate_begin(nq, ptr ? ptr->data() : nullptr, items.empty() ? nullptr : items.data(), capacity, n_items, &msg);
    CHECK((rc == GORSE_OK) == msg.empty());
    return rc;
}

static int32_t stage(const Pass &P, int32_t k) {
    std::string msg;
    const int32_t rc = validate_stage(P, k, &msg);
    CHECK((rc == GORSE_OK) == msg.empty());
    return rc;
}

static int32_t shared(int64_t n, const std::vector<int32_t> &items, int64_t n_items, bool scores = true) {
    std::string msg;
    std::vector<double> sc(items.size(), 1.0);
    const int32_t rc = validate_shared(n, items.empty() ? nullptr : items.data(), scores && !sc.empty() ? sc.data() : nullptr, n_items, &msg);
    CHECK((rc == GORSE_OK) == msg.empty());
    return rc;
}

static int32_t lists(int64_t nq, const std::vector<int64_t> *ptr, const std::vector<int32_t> &items, int64_t n_items) {
    std::string msg;
    std::vector<double> sc(items.size(), 1.0);
    const int32_t rc = validate_lists(nq, ptr ? ptr->data() : nullptr, items.empty() ? nullptr : items.data(), sc.empty() ? nullptr : sc.data(),
                                      n_items, &msg);
    CHECK((rc == GORSE_OK) == msg.empty());
    return rc;
}

int main() {
    const int64_t top = 2147483646;  // the largest item of a chain with n_items = 2^31 - 1
    // ---- begin
    std::vector<int64_t> p{0, 2, 2, 5};
    CHECK(begin(3, &p, {4, 4, 0, 9, 1}, 1, 10) == GORSE_OK);  // unsorted, a repeat, an empty row
    CHECK(begin(3, nullptr, {}, 7, 10) == GORSE_OK);          // no base rows
    CHECK(begin(0, nullptr, {}, 7, 10) == GORSE_OK);
    std::vector<int64_t> p0{0};
    CHECK(begin(0, &p0, {}, 7, 10) == GORSE_OK);
    CHECK(begin(3, &p, {4, 4, 0, (int32_t)top, 1}, 1, top + 1) == GORSE_OK);
    CHECK(begin(3, &p, {4, 4, 0, 10, 1}, 1, 10) == GORSE_ERR_RANGE);
    CHECK(begin(3, &p, {4, 4, 0, -1, 1}, 1, 10) == GORSE_ERR_RANGE);
    CHECK(begin(3, &p, {}, 1, 10) == GORSE_ERR_INVALID);  // items NULL
    CHECK(begin(-1, nullptr, {}, 1, 10) == GORSE_ERR_INVALID);
    CHECK(begin((int64_t)1 << 31, nullptr, {}, 1, 10) == GORSE_ERR_INVALID);
    CHECK(begin(3, nullptr, {}, 0, 10) == GORSE_ERR_INVALID);
    CHECK(begin(3, nullptr, {}, -5, 10) == GORSE_ERR_INVALID);
    CHECK(begin(INT32_MAX, nullptr, {}, INT32_MAX, 10) == GORSE_ERR_INVALID);  // n_queries * capacity
    std::vector<int64_t> p1{1, 2, 2, 5}, p2{0, 3, 2, 5};
    CHECK(begin(3, &p1, {4, 4, 0, 9, 1}, 1, 10) == GORSE_ERR_INVALID);
    CHECK(begin(3, &p2, {4, 4, 0, 9, 1}, 1, 10) == GORSE_ERR_INVALID);  // found before any item is read
    std::vector<int64_t> p3{0, (int64_t)1 << 31, (int64_t)1 << 31, (int64_t)1 << 31};
    CHECK(begin(3, &p3, {1}, 1, 10) == GORSE_ERR_INVALID);  // a row too long, found before any item is read

    // ---- a stage against the pass
    Pass P;
    CHECK(stage(P, 5) == GORSE_ERR_INVALID);  // no pass
    P.begun = true, P.n_queries = 3, P.capacity = 300;
    CHECK(stage(P, 1) == GORSE_OK && stage(P, GORSE_CAND_MAX_K) == GORSE_OK);
    CHECK(stage(P, 0) == GORSE_ERR_INVALID && stage(P, -1) == GORSE_ERR_INVALID && stage(P, GORSE_CAND_MAX_K + 1) == GORSE_ERR_INVALID);
    P.sum_k = 290;
    CHECK(stage(P, 10) == GORSE_OK);            // the capacity reached exactly
    CHECK(stage(P, 11) == GORSE_ERR_INVALID);   // passed by one
    P.sum_k = 0, P.n_stages = GORSE_CAND_MAX_STAGES - 1;
    CHECK(stage(P, 1) == GORSE_OK);
    P.n_stages = GORSE_CAND_MAX_STAGES;
    CHECK(stage(P, 1) == GORSE_ERR_INVALID);
    P.n_stages = 2, P.finished = true;
    CHECK(stage(P, 1) == GORSE_ERR_INVALID);
    P.capacity = INT32_MAX, P.sum_k = INT32_MAX - 1, P.finished = false;
    CHECK(stage(P, 1) == GORSE_OK && stage(P, 2) == GORSE_ERR_INVALID);  // no overflow of the sum

    // ---- the list stages
    CHECK(shared(3, {1, 9, 1}, 10) == GORSE_OK && shared(0, {}, 10) == GORSE_OK);
    CHECK(shared(3, {1, 10, 1}, 10) == GORSE_ERR_RANGE && shared(3, {1, -2, 1}, 10) == GORSE_ERR_RANGE);
    CHECK(shared(2, {(int32_t)top, 0}, top + 1) == GORSE_OK && shared(2, {(int32_t)top, 0}, top) == GORSE_ERR_RANGE);
    CHECK(shared(-1, {}, 10) == GORSE_ERR_INVALID && shared(3, {}, 10) == GORSE_ERR_INVALID && shared(3, {1, 2, 3}, 10, false) == GORSE_ERR_INVALID);
    std::vector<int32_t> big((size_t)kMaxSharedList + 1, 3);
    CHECK(shared(kMaxSharedList + 1, big, 10) == GORSE_ERR_INVALID);
    big.pop_back();
    CHECK(shared(kMaxSharedList, big, 10) == GORSE_OK);
    CHECK(lists(3, &p, {4, 4, 0, 9, 1}, 10) == GORSE_OK && lists(0, &p0, {}, 10) == GORSE_OK);
    CHECK(lists(3, nullptr, {}, 10) == GORSE_ERR_INVALID);
    CHECK(lists(3, &p1, {4, 4, 0, 9, 1}, 10) == GORSE_ERR_INVALID && lists(3, &p2, {4, 4, 0, 9, 1}, 10) == GORSE_ERR_INVALID);
    CHECK(lists(3, &p, {}, 10) == GORSE_ERR_INVALID);
    CHECK(lists(3, &p, {4, 4, 0, 9, 10}, 10) == GORSE_ERR_RANGE && lists(3, &p, {-1, 4, 0, 9, 1}, 10) == GORSE_ERR_RANGE);
    printf("cand_plan ok\n");
    return 0;
}
