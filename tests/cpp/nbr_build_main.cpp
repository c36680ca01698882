// Stand-alone check of the host-side argument validation of gorse_nbr_set_table_from_topk / _from_sparse
// (gorse_amd/csrc/nbr_plan.hpp, validate_from_search), built by tests/test_nbr_build_cpu.py with AddressSanitizer and UBSan.
// Prints "nbr_build ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "../../gorse_amd/csrc/nbr_plan.hpp"

using namespace gorse::nbr;

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                               \
        }                                                          \
    } while (0)

static std::vector<int64_t> g_rows, g_src;

static int32_t call(int32_t which, int64_t n_rows, const std::vector<int64_t> *sources, int32_t n, int32_t transform, double scale,
                    int64_t index_n, int64_t n_items) {
    std::string msg;
    g_rows.assign(3, 77), g_src.assign(3, 77);
    const int32_t rc = validate_from_search(which, n_rows, sources ? sources->data() : nullptr, n, transform, scale, index_n, n_items, &g_rows,
                                            &g_src, &msg);
    CHECK((rc == GORSE_OK) == msg.empty());
    return rc;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // sources == NULL: row r is stored row r
    CHECK(call(GORSE_NBR_HOP2, 4, nullptr, 5, GORSE_NBR_RAW, 1.0, 4, 4) == GORSE_OK);
    CHECK((g_rows == std::vector<int64_t>{0, 1, 2, 3}) && g_src == g_rows);
    CHECK(call(GORSE_NBR_HOP1, 0, nullptr, 1, GORSE_NBR_RECIP, 0.5, 4, 1) == GORSE_OK && g_rows.empty() && g_src.empty());
    // a subset with empty rows and repeats: the valid ones in row order
    const std::vector<int64_t> some{3, -1, 0, 3, -7, 2};
    CHECK(call(GORSE_NBR_HOP1, 6, &some, GORSE_NBR_MAX_LIST, GORSE_NBR_RAW, -2.0, 4, 1) == GORSE_OK);
    CHECK((g_rows == std::vector<int64_t>{0, 2, 3, 5}) && (g_src == std::vector<int64_t>{3, 0, 3, 2}));
    const std::vector<int64_t> none{-1, -1};
    CHECK(call(GORSE_NBR_HOP2, 2, &none, 5, GORSE_NBR_RAW, 1.0, 4, 9) == GORSE_OK && g_rows.empty());
    // GORSE_ERR_INVALID
    CHECK(call(2, 4, nullptr, 5, GORSE_NBR_RAW, 1.0, 4, 4) == GORSE_ERR_INVALID);
    CHECK(call(-1, 4, nullptr, 5, GORSE_NBR_RAW, 1.0, 4, 4) == GORSE_ERR_INVALID);
    CHECK(call(GORSE_NBR_HOP2, -1, nullptr, 5, GORSE_NBR_RAW, 1.0, 4, 4) == GORSE_ERR_INVALID);
    CHECK(call(GORSE_NBR_HOP2, (int64_t)INT32_MAX + 1, nullptr, 5, GORSE_NBR_RAW, 1.0, 4, 4) == GORSE_ERR_INVALID);
    CHECK(call(GORSE_NBR_HOP2, 4, nullptr, 0, GORSE_NBR_RAW, 1.0, 4, 4) == GORSE_ERR_INVALID);
    CHECK(call(GORSE_NBR_HOP2, 4, nullptr, -3, GORSE_NBR_RAW, 1.0, 4, 4) == GORSE_ERR_INVALID);
    CHECK(call(GORSE_NBR_HOP2, 4, nullptr, GORSE_NBR_MAX_LIST + 1, GORSE_NBR_RAW, 1.0, 4, 4) == GORSE_ERR_INVALID);
    for (double bad : {inf, -inf, nan}) CHECK(call(GORSE_NBR_HOP2, 4, nullptr, 5, GORSE_NBR_RAW, bad, 4, 4) == GORSE_ERR_INVALID);
    CHECK(call(GORSE_NBR_HOP2, 4, nullptr, 5, 2, 1.0, 4, 4) == GORSE_ERR_INVALID);
    CHECK(call(GORSE_NBR_HOP2, 4, nullptr, 5, -1, 1.0, 4, 4) == GORSE_ERR_INVALID);
    // GORSE_ERR_RANGE: a source beyond the index; more rows than the index without a source list; hop 2 names items
    const std::vector<int64_t> far{0, 4, 1};
    CHECK(call(GORSE_NBR_HOP1, 3, &far, 5, GORSE_NBR_RAW, 1.0, 4, 4) == GORSE_ERR_RANGE);
    CHECK(call(GORSE_NBR_HOP1, 5, nullptr, 5, GORSE_NBR_RAW, 1.0, 4, 9) == GORSE_ERR_RANGE);
    CHECK(call(GORSE_NBR_HOP2, 4, nullptr, 5, GORSE_NBR_RAW, 1.0, 4, 3) == GORSE_ERR_RANGE);
    CHECK(call(GORSE_NBR_HOP1, 4, nullptr, 5, GORSE_NBR_RAW, 1.0, 4, 3) == GORSE_OK);  // hop 1 names hop-2 rows: held at the call
    // an invalid argument is reported before a range
    CHECK(call(GORSE_NBR_HOP2, 3, &far, 0, GORSE_NBR_RAW, 1.0, 4, 3) == GORSE_ERR_INVALID);
    printf("nbr_build ok\n");
    return 0;
}
