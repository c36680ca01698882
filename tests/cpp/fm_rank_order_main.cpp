// Stand-alone check of the host side of gorse_fm_rank_users' ordering (gorse_amd/csrc/fm_rank_order.hpp): the comparator is a
// strict weak order that realises "descending score, -0 == +0, NaN last", std::stable_sort with it keeps ties by position, and
// the device's sort key orders exactly as the comparator does.  Built with -fsanitize=address,undefined by
// tests/test_fm_rank_order_cpu.py; exits 0 when everything holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "../../gorse_amd/csrc/fm_rank_order.hpp"

using gorse::fm::rank_before;
using gorse::fm::rank_key;
using gorse::fm::rank_positions;

static int failures = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                              \
        }                                                            \
    } while (0)

static float from_bits(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
static uint32_t bits_of(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// the rule, restated without the comparator: insertion into a list kept in ranked order
static std::vector<int32_t> by_insertion(const std::vector<float> &s) {
    std::vector<int32_t> out;
    for (int32_t i = 0; i < (int32_t)s.size(); i++) {
        size_t at = out.size();
        if (!std::isnan(s[i]))
            for (size_t q = 0; q < out.size(); q++)
                if (std::isnan(s[out[q]]) || s[out[q]] < s[i]) {  // the first entry that ranks strictly behind
                    at = q;
                    break;
                }
        out.insert(out.begin() + at, i);
    }
    return out;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity();
    const std::vector<float> special = {0.0f, -0.0f, 1.0f, -1.0f, inf, -inf, 1e-45f, -1e-45f, 3.4e38f, -3.4e38f, 2.5f, 2.5f,
                                        from_bits(0x7fc00000u), from_bits(0xffc00000u), from_bits(0x7f800001u),
                                        from_bits(0xffffffffu), from_bits(0x7fffffffu)};
    // comparator: irreflexive, asymmetric, transitive, and its equivalence is transitive
    for (float a : special) {
        CHECK(!rank_before(a, a));
        for (float b : special) {
            CHECK(!(rank_before(a, b) && rank_before(b, a)));
            // the key orders as the comparator does
            CHECK(rank_before(a, b) == (rank_key(bits_of(a)) < rank_key(bits_of(b))));
            for (float c : special) {
                if (rank_before(a, b) && rank_before(b, c)) CHECK(rank_before(a, c));
                const bool ab = !rank_before(a, b) && !rank_before(b, a), bc = !rank_before(b, c) && !rank_before(c, b);
                if (ab && bc) CHECK(!rank_before(a, c) && !rank_before(c, a));
            }
        }
    }
    CHECK(rank_key(bits_of(0.0f)) == rank_key(bits_of(-0.0f)));
    CHECK(rank_key(0x7fc00000u) == 0xffffffffu && rank_key(0xffc00001u) == 0xffffffffu);
    CHECK(rank_key(bits_of(-inf)) < 0xffffffffu);
    // hand-written lists
    {
        const std::vector<float> s = {1.0f, from_bits(0xffc00000u), 3.0f, -0.0f, 3.0f, 0.0f, from_bits(0x7fc00000u), -2.0f};
        const std::vector<int32_t> want = {2, 4, 0, 3, 5, 7, 1, 6};
        std::vector<int32_t> got(s.size());
        rank_positions(s.data(), (int64_t)s.size(), got.data());
        CHECK(got == want);
        CHECK(by_insertion(s) == want);
    }
    {
        std::vector<int32_t> got(1, -1);
        const float one = 5.0f;
        rank_positions(&one, 1, got.data());
        CHECK(got[0] == 0);
        rank_positions(&one, 0, got.data());  // an empty list touches nothing
        CHECK(got[0] == 0);
    }
    // random lists with many ties, NaNs and zeros of both signs
    uint64_t state = 88172645463325252ull;
    auto next = [&]() {
        state ^= state << 13;
        state ^= state >> 7;
        state ^= state << 17;
        return state;
    };
    for (int rep = 0; rep < 200; rep++) {
        const size_t n = 1 + next() % 300;
        std::vector<float> s(n);
        for (auto &x : s) {
            const uint64_t r = next() % 16;
            x = r == 0 ? from_bits(0x7fc00000u | (uint32_t)(next() & 0xffff)) : r == 1 ? from_bits(0xffc00000u) : r == 2 ? -0.0f
              : r == 3 ? 0.0f : (float)((int)(next() % 9) - 4) * 0.5f;
        }
        std::vector<int32_t> got(n);
        rank_positions(s.data(), (int64_t)n, got.data());
        CHECK(got == by_insertion(s));
    }
    if (failures == 0) std::printf("fm_rank_order ok\n");
    return failures == 0 ? 0 : 1;
}
