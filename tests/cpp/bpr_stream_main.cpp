// Stand-alone check of gorse_amd/csrc/bpr_stream.hpp (the BPR sample stream: model/cf/model.go:449-468), built by
// tests/test_bpr_stream_cpu.py with AddressSanitizer and UBSan.  usage: bpr_stream WORLD OUT
// WORLD: "U I" | U + 1 row pointers | the rows in stored order | the rows sorted | the number of runs | per run "seed epoch base n".
// Every sample of every run is drawn the three ways the kernels of csrc/bpr_prepare.hip compose the header's functions:
//   1. the whole triplet in one go                                   (bpr_sample_kernel)
//   2. the user first, the items later by replay                     (bpr_sample_user_kernel, bpr_sample_items_kernel, the bins' finish)
//   3. the first user draw and the first negative candidate inline, the rest by a restart from the start of the stream
//                                                                    (bpr_bin_count_kernel, bpr_sample_items_batch_kernel)
// and the three must give the same triplet -- (-1, -1, -1) for a sample given up on -- and give up on the same samples.  OUT receives
// route 1's triplets, one "u i j" per line, for the test to compare with the oracle.  Prints "bpr_stream ok".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gorse_amd/csrc/bpr_stream.hpp"

using namespace gorse;

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                               \
        }                                                          \
    } while (0)

struct World {
    int32_t U = 0, I = 0;
    std::vector<int64_t> uptr;
    std::vector<int32_t> uidx, usorted;
};
struct Triplet {
    int32_t u, i, j;
    bool operator==(const Triplet &o) const { return u == o.u && i == o.i && j == o.j; }
};
constexpr Triplet kGivenUp{-1, -1, -1};

static int64_t num(FILE *f) {
    long long v = 0;
    CHECK(fscanf(f, "%lld", &v) == 1);
    return (int64_t)v;
}
static uint64_t unum(FILE *f) {
    unsigned long long v = 0;
    CHECK(fscanf(f, "%llu", &v) == 1);
    return (uint64_t)v;
}

// 1. bpr_sample_kernel
static Triplet whole(const World &w, uint64_t seed, uint64_t epoch, uint64_t sample) {
    Philox g;
    g.init(seed, epoch, sample);
    const int32_t u = draw_user(g, w.U, w.uptr.data());
    if (u < 0) return kGivenUp;
    const int64_t beg = w.uptr[(size_t)u], cnt = w.uptr[(size_t)u + 1] - beg;
    const int32_t pi = w.uidx[(size_t)(beg + g.int31n((int32_t)cnt))];
    const int32_t nj = draw_negative(g, w.I, w.usorted.data() + beg, cnt);
    return nj < 0 ? kGivenUp : Triplet{u, pi, nj};
}

// 2. bpr_sample_user_kernel, then bpr_sample_items_kernel (and step 3 of bpr_bin_finish_kernel) for the user it left
static Triplet by_replay(const World &w, uint64_t seed, uint64_t epoch, uint64_t sample) {
    const int32_t u = redraw_user(seed, epoch, sample, w.U, w.uptr.data());
    if (u < 0) return kGivenUp;
    const int64_t rbeg = w.uptr[(size_t)u], cnt = w.uptr[(size_t)u + 1] - rbeg;
    Philox g;
    g.init(seed, epoch, sample);
    replay_user(g, w.U, u);
    const int32_t pi = w.uidx[(size_t)(rbeg + g.int31n((int32_t)cnt))];
    const int32_t nj = draw_negative(g, w.I, w.usorted.data() + rbeg, cnt);
    return nj < 0 ? kGivenUp : Triplet{u, pi, nj};
}

// 3. bpr_bin_count_kernel, then bpr_sample_items_batch_kernel: the first draws are the kernels' own lines, the fallbacks the header's
static Triplet batched(const World &w, uint64_t seed, uint64_t epoch, uint64_t sample) {
    Philox g;
    g.init(seed, epoch, sample);
    const int32_t cu = g.int31n(w.U);
    int32_t u = w.uptr[(size_t)cu + 1] > w.uptr[(size_t)cu] ? cu : -1;
    if (u < 0) u = redraw_user(seed, epoch, sample, w.U, w.uptr.data());
    if (u < 0) return kGivenUp;
    const int64_t rbeg = w.uptr[(size_t)u];
    const int32_t cnt = (int32_t)(w.uptr[(size_t)u + 1] - rbeg);
    g.init(seed, epoch, sample);
    for (int k = 0; k < kMaxDraws; k++)
        if (cnt == 0 || g.int31n(w.U) == u) break;
    const int32_t r = g.int31n(cnt > 0 ? cnt : 1);
    const int32_t c = g.int31n(w.I);
    const int32_t pi = w.uidx[(size_t)(rbeg + r)];
    int32_t nj = c;
    if (row_contains(w.usorted.data() + rbeg, cnt, c))
        nj = redraw_negative(seed, epoch, sample, w.U, w.I, u, w.usorted.data() + rbeg, cnt);
    return nj < 0 ? kGivenUp : Triplet{u, pi, nj};
}

int main(int argc, char **argv) {
    CHECK(argc == 3);
    FILE *f = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    CHECK(f != nullptr && out != nullptr);
    World w;
    w.U = (int32_t)num(f), w.I = (int32_t)num(f);
    CHECK(w.U > 0 && w.I > 0);
    w.uptr.resize((size_t)w.U + 1);
    for (auto &p : w.uptr) p = num(f);
    CHECK(w.uptr[0] == 0);
    // (exact-size vectors: a draw past a row's end is a heap overflow the sanitizer sees)
    w.uidx.resize((size_t)w.uptr.back()), w.usorted.resize((size_t)w.uptr.back());
    for (auto &x : w.uidx) x = (int32_t)num(f);
    for (auto &x : w.usorted) x = (int32_t)num(f);
    const int64_t runs = num(f);
    for (int64_t r = 0; r < runs; r++) {
        const uint64_t seed = unum(f), epoch = unum(f);
        const int64_t base = num(f), n = num(f);
        int64_t given_up[3] = {0, 0, 0};
        for (int64_t s = 0; s < n; s++) {
            const uint64_t sample = (uint64_t)(base + s);
            const Triplet a = whole(w, seed, epoch, sample), b = by_replay(w, seed, epoch, sample), c = batched(w, seed, epoch, sample);
            CHECK(a == b && a == c);
            given_up[0] += a == kGivenUp, given_up[1] += b == kGivenUp, given_up[2] += c == kGivenUp;
            if (!(a == kGivenUp)) {
                const int64_t beg = w.uptr[(size_t)a.u], cnt = w.uptr[(size_t)a.u + 1] - beg;
                CHECK(cnt > 0 && a.j >= 0 && a.j < w.I);
                CHECK(row_contains(w.usorted.data() + beg, cnt, a.i) && !row_contains(w.usorted.data() + beg, cnt, a.j));
            }
            fprintf(out, "%d %d %d\n", a.u, a.i, a.j);
        }
        CHECK(given_up[0] == given_up[1] && given_up[0] == given_up[2]);
        printf("run %" PRId64 ": %" PRId64 " samples, %" PRId64 " given up\n", r, n, given_up[0]);
    }
    fclose(f);
    CHECK(fclose(out) == 0);
    printf("bpr_stream ok\n");
    return 0;
}
