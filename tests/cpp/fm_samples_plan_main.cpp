// Stand-alone check of gorse_amd/csrc/fm_samples_plan.hpp (the composed row of a sample and the per-batch accumulation plan of
// gorse_fm_set_train_samples), built by tests/test_fm_samples_cpu.py with AddressSanitizer and UBSan.  Every argument is a
// world file the test wrote: the two sides, the samples, and per batch the (feature, row, value) sequence a numpy restatement of
// fm.hip's build_plan gives on the materialised rows.  Values travel as their bit patterns.  Prints "fm_samples_plan ok".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "../../gorse_amd/csrc/fm_samples_plan.hpp"

using namespace gorse::fm;

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                               \
        }                                                          \
    } while (0)

static int64_t num(FILE *f) {
    long long v = 0;
    CHECK(fscanf(f, "%lld", &v) == 1);
    return (int64_t)v;
}

static float bits(FILE *f) {
    const uint32_t u = (uint32_t)num(f);
    float x;
    memcpy(&x, &u, 4);
    return x;
}

struct Side {
    std::vector<int64_t> ptr;
    std::vector<int32_t> idx, lead;
    std::vector<float> val;
    bool has_lead = true;
    void read(FILE *f) {
        const int64_t n = num(f);
        has_lead = num(f) != 0;
        ptr.resize((size_t)n + 1);
        for (auto &p : ptr) p = num(f);
        idx.resize((size_t)ptr.back()), val.resize((size_t)ptr.back()), lead.resize((size_t)n);
        for (auto &i : idx) i = (int32_t)num(f);
        for (auto &v : val) v = bits(f);
        for (auto &l : lead) l = (int32_t)num(f);
    }
    SideRows rows() const { return SideRows{ptr.data(), idx.data(), val.data(), has_lead ? lead.data() : nullptr}; }
};

// the batches of a run on two threads: the result must not depend on how the batches are split
struct TwoThreads {
    template <class F>
    void operator()(int64_t nb, F fn) const {
        std::thread a([&] { fn((int64_t)0, nb / 2); }), b([&] { fn(nb / 2, nb); });
        a.join();
        b.join();
    }
};

static void same_bits(float a, float b) { CHECK(memcmp(&a, &b, 4) == 0); }

static void check_world(const char *path) {
    FILE *f = fopen(path, "r");
    CHECK(f != nullptr);
    Side U, I;
    U.read(f);
    I.read(f);
    const int64_t n = num(f);
    const int32_t bs = (int32_t)num(f);
    const int64_t width = num(f);
    std::vector<int32_t> user((size_t)n), item((size_t)n);
    for (auto &u : user) u = (int32_t)num(f);
    for (auto &c : item) c = (int32_t)num(f);
    CHECK(composed_width(U.rows(), I.rows(), user.data(), item.data(), n) == width);
    SamplePlan p, q;
    CHECK(plan_samples(U.rows(), I.rows(), user.data(), item.data(), n, bs, p));
    CHECK(plan_samples(U.rows(), I.rows(), user.data(), item.data(), n, bs, q, TwoThreads{}));
    CHECK(p.uniq == q.uniq && p.seg == q.seg && p.row == q.row && p.uoff == q.uoff && p.eoff == q.eoff && p.max_slots == q.max_slots);
    CHECK(p.val.size() == q.val.size() && (p.val.empty() || memcmp(p.val.data(), q.val.data(), p.val.size() * 4) == 0));
    const int64_t nb = num(f);
    CHECK(nb == (n + bs - 1) / bs && (int64_t)p.uoff.size() == nb + 1 && (int64_t)p.eoff.size() == nb + 1);
    CHECK(p.uoff[0] == 0 && p.eoff[0] == 0 && (int64_t)p.seg.size() == p.uoff.back() + nb);
    CHECK((int64_t)p.uniq.size() == p.uoff.back() && (int64_t)p.row.size() == p.eoff.back() && p.val.size() == p.row.size());
    int64_t widest = 0;
    for (int64_t k = 0; k < nb; k++) {
        const int64_t entries = num(f);
        const int64_t u0 = p.uoff[(size_t)k], nslots = p.uoff[(size_t)k + 1] - u0, e0 = p.eoff[(size_t)k];
        CHECK(p.eoff[(size_t)k + 1] - e0 == entries);
        const int32_t *seg = p.seg.data() + u0 + k;
        CHECK(seg[0] == 0 && seg[nslots] == entries);
        widest = std::max(widest, nslots);
        const int64_t rows = std::min<int64_t>(bs, n - k * bs);
        int64_t s = 0;
        for (int64_t e = 0; e < entries; e++) {
            const int32_t feat = (int32_t)num(f), row = (int32_t)num(f);
            const float x = bits(f);
            while (s < nslots && seg[s + 1] <= e) s++;
            CHECK(s < nslots && seg[s] <= e && seg[s] < seg[s + 1]);  // no empty slot
            CHECK(p.uniq[(size_t)(u0 + s)] == feat && (s == 0 || p.uniq[(size_t)(u0 + s - 1)] < feat));
            CHECK(p.row[(size_t)(e0 + e)] == row && row >= 0 && row < rows);
            same_bits(p.val[(size_t)(e0 + e)], x);
            CHECK(x != 0.0f);
        }
        CHECK(entries > 0 ? s == nslots - 1 : nslots == 0);
    }
    CHECK(p.max_slots == widest);
    fclose(f);
}

int main(int argc, char **argv) {
    CHECK(argc > 1);
    for (int a = 1; a < argc; a++) check_world(argv[a]);
    // no samples at all: an empty plan
    SamplePlan p;
    const int64_t zero = 0;
    const SideRows none{&zero, nullptr, nullptr, nullptr};
    CHECK(plan_samples(none, none, nullptr, nullptr, 0, 64, p));
    CHECK(p.uoff.size() == 1 && p.eoff.size() == 1 && p.uniq.empty() && p.seg.empty() && p.max_slots == 0);
    printf("fm_samples_plan ok\n");
    return 0;
}
