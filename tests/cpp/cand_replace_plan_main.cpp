// Stand-alone check of gorse_amd/csrc/cand_replace_plan.hpp (what gorse_cand_add_replacement and gorse_fm_rank_cand_decayed validate
// before they launch or replace anything, the history word, the decayed doubles' sort key and the host's decayed order), built by
// tests/test_cand_replace_cpu.py with AddressSanitizer and UBSan.  Prints "cand_replace_plan ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../gorse_amd/csrc/cand_replace_plan.hpp"

using namespace gorse::cand;

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                               \
        }                                                          \
    } while (0)

// exactly sized heap copies: a read past the end is the sanitizer's to find
static int32_t history(int64_t nq, const std::vector<int64_t> *ptr, const std::vector<int32_t> &items, const std::vector<uint8_t> &kind,
                       int64_t n_items) {
    std::string msg;
    const int32_t rc = validate_history(nq, ptr ? ptr->data() : nullptr, items.empty() ? nullptr : items.data(),
                                        kind.empty() ? nullptr : kind.data(), n_items, &msg);
    CHECK((rc == GORSE_OK) == msg.empty());
    return rc;
}

static int32_t pass(const Pass &P) {
    std::string msg;
    const int32_t rc = validate_replacement_pass(P, &msg);
    CHECK((rc == GORSE_OK) == msg.empty());
    return rc;
}

static int32_t decays(double p, double r) {
    std::string msg;
    const int32_t rc = validate_decays(p, r, &msg);
    CHECK((rc == GORSE_OK) == msg.empty());
    return rc;
}

int main() {
    const int64_t top = 2147483646;  // the largest item of a chain with n_items = 2^31 - 1
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");

    // ---- the pass
    Pass P;
    CHECK(pass(P) == GORSE_ERR_INVALID);
    P.begun = true;
    CHECK(pass(P) == GORSE_ERR_INVALID);  // not finished
    P.finished = true;
    CHECK(pass(P) == GORSE_OK);
    P.replaced = true;
    CHECK(pass(P) == GORSE_ERR_INVALID);  // a second time
    CHECK(!Pass().replaced);              // what gorse_cand_begin starts from

    // ---- the history rows
    std::vector<int64_t> p{0, 2, 2, 5}, p0{0}, p1{1, 2, 2, 5}, p2{0, 3, 2, 5};
    CHECK(history(3, &p, {4, 4, 0, 9, 1}, {1, 2, 2, 1, 1}, 10) == GORSE_OK);  // unsorted, an item with both kinds, an empty row
    CHECK(history(0, &p0, {}, {}, 10) == GORSE_OK);
    CHECK(history(3, &p, {4, 4, 0, (int32_t)top, 1}, {1, 2, 2, 1, 1}, top + 1) == GORSE_OK);
    CHECK(history(3, nullptr, {}, {}, 10) == GORSE_ERR_INVALID);
    CHECK(history(3, &p1, {4, 4, 0, 9, 1}, {1, 2, 2, 1, 1}, 10) == GORSE_ERR_INVALID);
    CHECK(history(3, &p2, {4, 4, 0, 9, 1}, {1, 2, 2, 1, 1}, 10) == GORSE_ERR_INVALID);  // found before any entry is read
    std::vector<int64_t> p3{0, (int64_t)1 << 31, (int64_t)1 << 31, (int64_t)1 << 31};
    CHECK(history(3, &p3, {1}, {1}, 10) == GORSE_ERR_INVALID);  // a row too long, found before any entry is read
    CHECK(history(3, &p, {}, {1, 2, 2, 1, 1}, 10) == GORSE_ERR_INVALID && history(3, &p, {4, 4, 0, 9, 1}, {}, 10) == GORSE_ERR_INVALID);
    CHECK(history(3, &p, {4, 4, 0, 9, 1}, {1, 2, 0, 1, 1}, 10) == GORSE_ERR_INVALID);
    CHECK(history(3, &p, {4, 4, 0, 9, 1}, {1, 2, 2, 1, 3}, 10) == GORSE_ERR_INVALID);
    CHECK(history(3, &p, {4, 4, 0, 10, 1}, {1, 2, 2, 1, 1}, 10) == GORSE_ERR_RANGE);
    CHECK(history(3, &p, {-1, 4, 0, 9, 1}, {1, 2, 2, 1, 1}, 10) == GORSE_ERR_RANGE);
    CHECK(history(3, &p, {4, 4, 0, 10, 1}, {1, 2, 9, 1, 1}, 10) == GORSE_ERR_INVALID);  // the first offence decides

    // ---- the decays: validate:"gt=0"
    CHECK(decays(0.8, 0.7) == GORSE_OK && decays(1.0, 1.0) == GORSE_OK && decays(1.5, 5e-324) == GORSE_OK && decays(inf, 2.0) == GORSE_OK);
    CHECK(decays(0.0, 0.7) == GORSE_ERR_INVALID && decays(0.8, 0.0) == GORSE_ERR_INVALID && decays(-0.0, 0.7) == GORSE_ERR_INVALID);
    CHECK(decays(-1.0, 0.7) == GORSE_ERR_INVALID && decays(0.8, -1.0) == GORSE_ERR_INVALID);
    CHECK(decays(nan, 0.7) == GORSE_ERR_INVALID && decays(0.8, nan) == GORSE_ERR_INVALID);

    // ---- the history word: ascending words = ascending items, an item's positive entry in front
    CHECK(history_word(0, 1) == 0 && history_word(0, 2) == 1 && history_word(7, 1) == 14 && history_word(7, 2) == 15);
    CHECK(history_word((int32_t)top, 1) == 0xfffffffcu && history_word((int32_t)top, 2) == 0xfffffffdu);
    CHECK(history_word((int32_t)top - 1, 2) < history_word((int32_t)top, 1) && (history_word((int32_t)top, 2) >> 1) == (uint32_t)top);

    // ---- the key: descending doubles ascend, -0 folded onto +0, every NaN on top
    const std::vector<double> down{inf, 1.7e308, 8.0, 6.3, 1.0, 5e-324, 0.0, -5e-324, -1.0, -1.7e308, -inf};
    for (size_t i = 0; i + 1 < down.size(); i++) CHECK(decay_key(double_bits(down[i])) < decay_key(double_bits(down[i + 1])));
    CHECK(decay_key(double_bits(-0.0)) == decay_key(double_bits(0.0)));
    CHECK(decay_key(double_bits(nan)) == ~(uint64_t)0 && decay_key(double_bits(-nan)) == ~(uint64_t)0);
    CHECK(decay_key(0xfff0000000000001ull) == ~(uint64_t)0 && decay_key(double_bits(-inf)) < ~(uint64_t)0);
    CHECK(9.0 * 0.7 == 6.3 && 10.0 * 0.8 == 8.0);  // the reference's known answers are exact products

    // ---- the host's decayed order.  Scores 10 8 8 nan 9 7 -0, the first, the NaN and the 9 decayed (0.8, 0.8, 0.7):
    //      8 8 8 nan 6.3 7 -0: the tie of three keeps the ranker's order (10 first, then the 8s by position), NaN last
    const std::vector<float> s{10.0f, 8.0f, 8.0f, std::nanf(""), 9.0f, 7.0f, -0.0f, 0.0f};
    const std::vector<double> f{10.0 * 0.8, 8.0, 8.0, nan, 9.0 * 0.7, 7.0, -0.0, 0.0};
    std::vector<int32_t> order(s.size());
    decayed_positions(s.data(), f.data(), (int64_t)s.size(), order.data());
    CHECK((order == std::vector<int32_t>{0, 1, 2, 5, 4, 6, 7, 3}));
    // a decay above 1 lifts an entry over the ranker's leader; equal finals then follow the ranker, not the position
    const std::vector<float> s2{4.0f, 8.0f, 2.0f};
    const std::vector<double> f2{8.0, 8.0, 8.0};
    decayed_positions(s2.data(), f2.data(), 3, order.data());
    CHECK(order[0] == 1 && order[1] == 0 && order[2] == 2);
    decayed_positions(s.data(), f.data(), 0, order.data());
    printf("cand_replace_plan ok\n");
    return 0;
}
