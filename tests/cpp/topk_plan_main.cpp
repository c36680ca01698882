// Stand-alone check of gorse_amd/csrc/topk_plan.hpp (the host-side rules of path B of the exact top-k), built by
// tests/test_topk_depth_table_cpu.py with AddressSanitizer and UBSan.  Prints "topk_plan ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gorse_amd/csrc/topk_plan.hpp"

using namespace gorse::topk_plan;

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                               \
        }                                                          \
    } while (0)

// The sweep's launch geometry for every instantiated (depth, main / history sweep, rows per tile, square / symmetric form), as the
// functions gave it before they moved into the header: depth, history, 32-row blocks per tile, symmetric, column blocks per wave |
// waves, LDS-DMA, tile buffers, LDS bytes.
struct Geom {
    int kp, hist, rb, sym, ncb, waves, dma, bufs;
    size_t lds;
};
static const Geom kGeometry[] = {
    {1, 0, 2, 0, 2, 8, 0, 3, 20384},   {1, 0, 4, 0, 2, 8, 0, 3, 30368},   {1, 1, 2, 0, 2, 2, 0, 2, 9344},
    {2, 0, 2, 0, 2, 8, 0, 3, 26528},   {2, 0, 4, 0, 2, 8, 1, 4, 45120},   {2, 0, 4, 1, 2, 8, 1, 4, 57472},
    {2, 1, 2, 0, 2, 8, 0, 2, 21120},   {3, 0, 2, 0, 2, 8, 0, 3, 32672},   {3, 0, 4, 0, 2, 8, 0, 3, 54944},
    {3, 1, 2, 0, 2, 2, 0, 2, 17536},   {4, 0, 2, 0, 2, 8, 1, 4, 44096},   {4, 0, 4, 0, 2, 8, 1, 4, 77888},
    {4, 0, 4, 1, 2, 8, 1, 4, 90240},   {4, 1, 2, 0, 2, 8, 1, 4, 44096},   {6, 0, 2, 0, 2, 8, 0, 3, 51104},
    {6, 0, 4, 0, 2, 8, 0, 3, 91808},   {6, 1, 2, 0, 2, 2, 0, 2, 29824},   {8, 0, 2, 0, 2, 8, 1, 4, 76864},
    {8, 0, 4, 0, 2, 8, 1, 4, 143424},  {8, 0, 4, 1, 2, 8, 1, 4, 155776},  {8, 1, 2, 0, 2, 8, 1, 4, 76864},
    {12, 0, 2, 0, 1, 8, 0, 3, 82848},  {12, 1, 2, 0, 1, 4, 0, 2, 54400},  {16, 0, 2, 0, 1, 8, 1, 4, 137280},
    {16, 1, 2, 0, 1, 8, 0, 2, 73344},  {24, 0, 2, 0, 1, 8, 0, 2, 106112}, {24, 1, 2, 0, 1, 8, 0, 2, 106112},
};

static void geometry() {
    size_t row = 0;
    for (int kp : kSupportedKP)
        for (int hist = 0; hist < 2; hist++)
            for (int rb = 2; rb <= 4; rb += 2)
                for (int sym = 0; sym < 2; sym++) {
                    // what dispatch_sweep instantiates: 128-row tiles for the main sweep up to depth 8, the symmetric form of those at
                    // the depths that have one; two column blocks per wave up to depth 8
                    if (rb == 4 && (hist || kp > 8)) continue;
                    if (sym && !(sweep_sym_kp(kp) && !hist && rb == 4)) continue;
                    const int ncb = kp <= 8 ? kNcbMain : 1;
                    const int wv = sweep_waves(hist, kp), bq = 32 * ncb * wv;
                    CHECK(row < sizeof(kGeometry) / sizeof(kGeometry[0]));
                    const Geom &g = kGeometry[row++];
                    CHECK(g.kp == kp && g.hist == hist && g.rb == rb && g.sym == sym && g.ncb == ncb);
                    CHECK(g.waves == wv);
                    CHECK(g.dma == (int)sweep_dma(kp, hist, rb, wv));
                    CHECK(g.bufs == sweep_bufs(kp, rb, bq, wv, hist, sym));
                    CHECK(g.lds == sweep_lds_bytes(kp, rb, bq, wv, hist, sym));
                    CHECK(g.lds <= (size_t)160 * 1024);  // the LDS of a CU
                    if (sym) CHECK(g.dma && bq == kSymBQ);
                    // the history sweeps' forms: the main sweep's eight-wave DMA form exactly at the depths sweep_hist_dma names
                    if (hist) CHECK(sweep_hist_dma(kp) == (wv == kWavesMain && kp <= 8));
                }
    CHECK(row == sizeof(kGeometry) / sizeof(kGeometry[0]));
    CHECK(!sweep_hist_dma(1) && sweep_hist_dma(2) && !sweep_hist_dma(3) && sweep_hist_dma(4) && !sweep_hist_dma(6) && sweep_hist_dma(8) &&
          !sweep_hist_dma(12) && !sweep_hist_dma(16) && !sweep_hist_dma(24));
    // the LDS of the other kernels at d = 128 and k = 100
    CHECK(rescore_lds_bytes(128, 16) == 25120 && tie_sort_lds_bytes(128, 16) == 74256 && lane_lds_bytes(101, 64) == 89856);
    CHECK(tie_sort_lds_bytes(1024, 16) <= (size_t)160 * 1024);
}

static void depth_and_warm_start() {
    const int bf[] = {1, 16, 17, 80, 81, 384, 385}, bf_kp[] = {1, 1, 2, 6, 6, 24, 0};
    const int f32[] = {1, 5, 6, 42, 43, 128, 129}, f32_kp[] = {1, 1, 2, 8, 12, 24, 0};
    for (int i = 0; i < 7; i++) CHECK(operand_depth(true, bf[i]) == bf_kp[i] && operand_depth(false, f32[i]) == f32_kp[i]);
    for (int kp : kSupportedKP) CHECK(operand_depth(true, 16 * kp) == kp && (kp == 24 || operand_depth(true, 16 * kp + 1) > kp));
    CHECK(operand_depth(false, 1 << 30) == 0);  // 3 d does not overflow

    const int64_t n17 = (int64_t)1 << 17, n18 = (int64_t)1 << 18;
    CHECK(warm_start(0, 8, n17) && !warm_start(0, 7, n17) && !warm_start(0, 8, n17 - 1));
    CHECK(warm_start(GORSE_TEST_TOPK_WARM_ALWAYS, 8, 1000) && !warm_start(GORSE_TEST_TOPK_WARM_ALWAYS, 7, n17));
    CHECK(!warm_start(GORSE_TEST_TOPK_WARM_OFF, 8, n17) && !warm_start(GORSE_TEST_TOPK_WARM_OFF | GORSE_TEST_TOPK_WARM_ALWAYS, 8, n17));
    CHECK(two_pilots(0, n18) && !two_pilots(0, n18 - 1) && two_pilots(GORSE_TEST_TOPK_WARM_ALWAYS, 1000));
    CHECK(pilot_kth(5, 16) == 4 && pilot_kth(11, 16) == 5 && pilot_kth(257, 16) == 31);  // lambda + 3.3 sqrt(lambda) + 1.5, rounded up
    for (int of = 2; of < kMaxKth; of++) CHECK(pilot_kth(of, 16) >= 2 && pilot_kth(of, 16) <= pilot_kth(of + 1, 16));
}

static void symmetric_form() {
    const int64_t N = (int64_t)1 << 17;
    CHECK(sym_eligible(0, 8, 11, N, 0, 2 * kSymBQ));
    // the operand depth
    for (int kp : kSupportedKP) CHECK(sym_eligible(0, kp, 11, N, 0, 2 * kSymBQ) == (kp == 2 || kp == 4 || kp == 8));
    // the warm start: kth, N and their switches
    CHECK(sym_eligible(0, 8, 8, N, 0, 2 * kSymBQ) && !sym_eligible(0, 8, 7, N, 0, 2 * kSymBQ));
    CHECK(!sym_eligible(0, 8, 11, N - 1, 0, 2 * kSymBQ) && sym_eligible(GORSE_TEST_TOPK_WARM_ALWAYS, 8, 11, N - 1, 0, 2 * kSymBQ));
    CHECK(!sym_eligible(GORSE_TEST_TOPK_WARM_OFF, 8, 11, N, 0, 2 * kSymBQ));
    // the form's own switches, and the tile height
    CHECK(!sym_eligible(GORSE_TEST_TOPK_SYM_OFF, 8, 11, N, 0, 2 * kSymBQ) && !sym_eligible(GORSE_TEST_TOPK_REPLAY_COUNTERS, 8, 11, N, 0, 2 * kSymBQ));
    CHECK(!sym_eligible(GORSE_TEST_TOPK_TILE64, 8, 11, N, 0, 2 * kSymBQ));
    CHECK(sym_eligible(GORSE_TEST_TOPK_SLICES8 | GORSE_TEST_TOPK_COLD_SLICES | GORSE_TEST_TOPK_TRI_SLICES(3), 8, 11, N, 0, 2 * kSymBQ));
    // a start on a 128-row boundary
    CHECK(sym_eligible(0, 8, 11, N, 128, 2 * kSymBQ) && sym_eligible(0, 8, 11, N, 128 * 1000, 2 * kSymBQ));
    CHECK(!sym_eligible(0, 8, 11, N, 64, 2 * kSymBQ) && !sym_eligible(0, 8, 11, N, 127, 2 * kSymBQ) && !sym_eligible(0, 8, 11, N, 129, 2 * kSymBQ));
    // two query blocks
    CHECK(kSymBQ == 512 && !sym_eligible(0, 8, 11, N, 0, 2 * kSymBQ - 1) && sym_eligible(0, 8, 11, N, 0, kChunkQ));
    CHECK(rows_per_tile(0) == 128 && rows_per_tile(GORSE_TEST_TOPK_TILE64) == 64 && kHistTileRows == 64);
}

static void triangle() {
    const int64_t nqs[] = {1024, 5000, 512 * 7 + 1, 1536, 513, 512 * 9};
    const int worlds[] = {1, 2, 3, 4, 8};
    for (int64_t nq : nqs)
        for (int world : worlds) {
            const TriGeom g(nq, world);
            CHECK(g.nblk == (nq + kSymBQ - 1) / kSymBQ);
            std::vector<int64_t> blocks((size_t)world, 0), owned((size_t)world, 0);
            for (int64_t c = 0; c < g.nblk; c++) blocks[(size_t)(c % world)]++;
            for (int64_t t = 0; t < nq; t++) owned[(size_t)((t / kSymBQ) % world)]++;
            int64_t sum = 0, at = 0;
            for (int r = 0; r < world; r++) {
                CHECK(g.blocks_of(r) == blocks[(size_t)r] && g.owned(r) == owned[(size_t)r]);
                sum += g.owned(r);
                int64_t lo = -1, hi = -1;
                g.slice(r, &lo, &hi);
                CHECK(lo == at && hi >= lo && hi <= nq && (hi == nq || hi % kSymBQ == 0));  // the pilot slices tile [0, nq) by whole blocks
                at = hi;
            }
            CHECK(sum == nq && at == nq);
        }
    const TriGeom few(1536, 8);  // more ranks than blocks: the ranks past the last block own nothing
    CHECK(few.blocks_of(2) == 1 && few.blocks_of(3) == 0 && few.owned(3) == 0 && few.owned(7) == 0);
    // own slices: the fewest of 1, 2, 4 that give a rank's launch ~768 workgroups; one rank alone is never sliced
    CHECK(tri_own_slices(0, 244, 8) == 4 && tri_own_slices(0, 768, 2) == 1 && tri_own_slices(0, 767, 2) == 2);
    CHECK(tri_own_slices(0, 384, 2) == 2 && tri_own_slices(0, 383, 2) == 4 && tri_own_slices(0, 1, 2) == 4 && tri_own_slices(0, 244, 1) == 1);
    CHECK(tri_own_slices(GORSE_TEST_TOPK_TRI_SLICES(1), 244, 8) == 1 && tri_own_slices(GORSE_TEST_TOPK_TRI_SLICES(2), 2000, 8) == 2);
    CHECK(tri_own_slices(GORSE_TEST_TOPK_TRI_SLICES(3), 2000, 1) == 4 && tri_own_slices(GORSE_TEST_TOPK_TRI_SLICES(2), 244, 1) == 2);
    CHECK(kMaxOwnSlices == 4);
}

static void tie_path() {
    const int64_t M = 1000000;
    // the sizes the rules' comments quote: a full C4 pass keeps eight slices, one rank of eight takes more, shorter ones
    CHECK(hist_slices(0, M, 10136) == 8 && hist_slices(0, M, 1250) == 32);
    CHECK(hist_slices(0, 20000, 5) == 1 && hist_slices(0, 3 * 32768, 100) == 3 && hist_slices(0, 8 * 32768 - 1, 100) == 7);
    CHECK(hist_slices(0, 8 * 32768, 100) == 16);                              // slices of at least 16384 rows
    CHECK(hist_slices(0, M, 64 * 128) == 8 && hist_slices(0, M, 63 * 128) == 16);  // ~512 workgroups of 128 queries
    CHECK(hist_slices(0, (int64_t)1 << 30, 1) == kMaxSlicesFew);
    CHECK(hist_slices(GORSE_TEST_TOPK_SLICES8, 20000, 5) == 8 && hist_slices(GORSE_TEST_TOPK_SLICES8, M, 1250) == 8);
    CHECK(hist_slices(GORSE_TEST_TOPK_SLICE1, M, 1250) == 1 && hist_slices(GORSE_TEST_TOPK_SLICE1 | GORSE_TEST_TOPK_SLICES8, M, 10136) == 1);
    CHECK(hist_slices(0, 0, 1) == 1);
    // the lane replay: fewer queries per wave while the launch has fewer than 256 waves, never fewer than 16
    CHECK(replay_queries_per_wave(0, 101, 10136) == 32 && replay_queries_per_wave(0, 101, 1250) == 16 && replay_queries_per_wave(0, 101, 1) == 16);
    CHECK(replay_queries_per_wave(0, 101, 255 * 64 + 1) == 64 && replay_queries_per_wave(0, 101, 255 * 64) == 32);
    CHECK(replay_queries_per_wave(GORSE_TEST_TOPK_REPLAY_WAVE64, 101, 1250) == 64 && replay_queries_per_wave(GORSE_TEST_TOPK_REPLAY_WAVE64, 101, 1) == 64);
    // ... and no more than fit in 144 KB with their heaps, whatever the switch
    CHECK(replay_queries_per_wave(0, kMaxKth, M) == 32 && replay_queries_per_wave(GORSE_TEST_TOPK_REPLAY_WAVE64, kMaxKth, M) == 32);
    for (int slots = 2; slots <= kMaxKth; slots++)
        CHECK(lane_lds_bytes(slots, replay_queries_per_wave(GORSE_TEST_TOPK_REPLAY_WAVE64, slots, M)) <= (size_t)144 * 1024);
}

int main() {
    geometry();
    depth_and_warm_start();
    symmetric_form();
    triangle();
    tie_path();
    printf("topk_plan ok\n");
    return 0;
}
