// Stand-alone check of gorse_amd/csrc/bpr_plan.hpp (the host-side rules of the BPR step), built by tests/test_bpr_plan_cpu.py with
// AddressSanitizer and UBSan.  Prints "bpr_plan ok".
// The expected values below were printed once from the expressions the launch code held before they moved into the header (the
// schedule predicate of epoch_impl with user_runs_supported, chunk_capacity, ensure_trip, launch_prepare_users, the grids of
// launch_update_users / launch_update_mode / launch_user_sort, exclusive_scan_i32), not from the header.
#include <cstdio>
#include <cstdlib>

#include "../../gorse_amd/csrc/bpr_plan.hpp"

using namespace gorse;

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            exit(1);                                               \
        }                                                          \
    } while (0)

template <class T, size_t N>
constexpr size_t count(const T (&)[N]) {
    return N;
}

// ---- the schedule: for mode 0..3, nFactors {8, 12, 16, 32, 64, 128, 256}, users {4095, 4096}, user runs enabled {0, 1}, the test
// bit {0, 1}, in that nesting: two digits per case, the schedule (0 sequential, 1 per-sample, 2 user runs) and the kernel mode
static const char *const kSchedule[4] = {
    "1010102010102020101010101010101010101020101020201010102010102020101010201010202010101020101020201010101010101010",
    "0101010101010101010101010101010101010101010101010101010101010101010101010101010101010101010101010101010101010101",
    "1212121212121212121212121212121212121212121212121212121212121212121212121212121212121212121212121212121212121212",
    "1010102310102323101010101010101010101023101023231010102310102323101010231010232310101023101023231010101010101010",
};
static void schedule() {
    CHECK(MODE_ATOMIC == 0 && MODE_EXACT == 1 && MODE_RACY == 2 && MODE_STORES == 3);
    CHECK(kBprSequential == 0 && kBprPerSample == 1 && kBprUserRuns == 2);
    const int widths[] = {8, 12, 16, 32, 64, 128, 256};
    for (int mode = 0; mode < 4; mode++) {
        const char *p = kSchedule[mode];
        for (int d : widths)
            for (int64_t U : {(int64_t)4095, (int64_t)4096})
                for (int en = 0; en < 2; en++)
                    for (int forced = 0; forced < 2; forced++) {
                        const BprSchedulePlan s = bpr_schedule(mode, d, U, en != 0, forced != 0);
                        CHECK(p[0] && p[1]);
                        CHECK((int)s.schedule == p[0] - '0' && s.kernel_mode == p[1] - '0');
                        p += 2;
                    }
        CHECK(*p == 0);
    }
    // the named edges once more, readably: 4095 / 4096 users without and with the test bit; a width outside the list; the store mode
    CHECK(bpr_schedule(MODE_ATOMIC, 64, 4095, true, false).schedule == kBprPerSample);
    CHECK(bpr_schedule(MODE_ATOMIC, 64, 4096, true, false).schedule == kBprUserRuns);
    CHECK(bpr_schedule(MODE_ATOMIC, 64, 4095, true, true).schedule == kBprUserRuns);
    CHECK(bpr_schedule(MODE_ATOMIC, 12, 1 << 20, true, true).schedule == kBprPerSample);
    CHECK(bpr_schedule(MODE_STORES, 64, 4096, true, false).kernel_mode == MODE_STORES);
    CHECK(bpr_schedule(MODE_STORES, 64, 4095, true, false).kernel_mode == MODE_ATOMIC);
    CHECK(bpr_schedule(MODE_RACY, 64, 1 << 20, true, true).schedule == kBprPerSample);
    CHECK(bpr_schedule(MODE_EXACT, 64, 1 << 20, true, true).schedule == kBprSequential);
    // variant bits, the library's default | enabled
    const int en[][3] = {{0, 0, 0}, {0, 1, 1}, {128, 0, 1}, {128, 1, 1}, {268435456, 0, 0}, {268435456, 1, 0}, {268435584, 0, 1}, {268435584, 1, 1}};
    CHECK(GORSE_TEST_BPR_USER_RUNS == 128 && GORSE_TEST_BPR_PER_SAMPLE == 268435456);
    for (const auto &r : en) CHECK((int)bpr_user_runs_enabled(r[0], r[1] != 0) == r[2]);
    // The coupling of the accumulated tier (gorse_mf_create: hot_rows.hpp acc_rows_eligible) to the schedule: a handle that gets the
    // tier runs user runs natively -- the tier's rows are only folded in the sole-writer form by a user-run launch.
    int eligible = 0;
    for (int64_t U : {(int64_t)0, (int64_t)943, kUserRunUsers - 1, kUserRunUsers, kUserRunUsers + 1, (int64_t)6040, (int64_t)1 << 20, (int64_t)10000000})
        for (int64_t I : {(int64_t)1, (int64_t)1682, (int64_t)3706, (int64_t)8192, (int64_t)131072, (int64_t)131073, (int64_t)1 << 20})
            for (int d = 1; d <= 260; d++)
                if (acc_rows_eligible(U, I, d, 0)) {
                    eligible++;
                    CHECK(bpr_schedule(MODE_ATOMIC, d, U, true, false).schedule == kBprUserRuns);
                    CHECK(bpr_schedule(MODE_STORES, d, U, true, false).schedule == kBprUserRuns);
                }
    CHECK(eligible > 0 && acc_rows_eligible(6040, 3706, 64, 0) && !acc_rows_eligible(4095, 3706, 64, 0) && !acc_rows_eligible(6040, 3706, 12, 0));
}

static void chunk() {
    // users, override | capacity
    const int64_t cap[][3] = {{0, 0, 4194304},          {131072, 0, 4194304},        {131073, 0, 4194336}, {4194304, 0, 134217728},
                              {10000000, 0, 134217728}, {1000, 12345, 12345},        {10000000, 7, 7}};
    for (const auto &r : cap) CHECK(bpr_chunk_capacity(r[0], r[1]) == r[2]);
    // want, chunk | samples per triplet buffer
    const int64_t trip[][3] = {{0, 4194304, 2}, {1, 4194304, 2}, {5, 4194304, 6}, {5000000, 4194304, 4194304},
                               {0, 7, 2},       {1, 7, 2},       {5, 7, 6},       {5000000, 7, 8}};
    for (const auto &r : trip) CHECK(bpr_trip_capacity(r[0], r[1]) == (size_t)r[2]);
}

static void preparation() {
    // users, samples, feedbacks, variant | shift, bins, binned, finish, batched item draws
    struct Route {
        int64_t U, n;
        size_t uidx_n;
        int variant, shift, nbins, binned, finish, batch;
    };
    const Route routes[] = {
        {6040, 1000000, 1000000, 0, 4, 378, 1, 1, 0},         // S-ml1m: the finish kernel
        {6040, 1000000, 1000000, 524288, 4, 378, 1, 0, 0},    // GORSE_TEST_BPR_THREE_KERNELS
        {6040, 1000000, 1000000, 2097152, 4, 378, 0, 0, 0},   // GORSE_TEST_BPR_NO_BINS
        {500000, 4194304, 1000000, 0, 9, 977, 1, 1, 0},       // shift = kFinShift
        {600000, 4194304, 1000000, 0, 10, 586, 1, 0, 0},      // shift = kFinShift + 1
        {6040, 1741824, 1000000, 0, 4, 378, 1, 1, 0},         // n / nbins = 4608 = 3/4 kFinCap
        {6040, 1742202, 1000000, 0, 4, 378, 1, 0, 0},         // n / nbins = 4609
        {6040, 1000000, 8388608, 0, 4, 378, 1, 1, 0},         // feedbacks = kItemsBatchFrom
        {6040, 1000000, 8388609, 0, 4, 378, 1, 0, 1},         // one more: three kernels, batched item draws
        {20000000, 1000, 1000000, 0, 16, 306, 0, 0, 0},       // more user ids per bin than the sort kernel's LDS holds: no bins
        {20000000, 1000, 8388609, 0, 16, 306, 0, 0, 1},
        {10000000, 134217728, 1000000, 0, 11, 4883, 1, 0, 0}, // the 10M-user set
        {943, 100000, 100000, 0, 1, 472, 1, 1, 0},
        {6040, 1, 1000000, 0, 4, 378, 1, 1, 0},
    };
    CHECK(GORSE_TEST_BPR_THREE_KERNELS == 524288 && GORSE_TEST_BPR_NO_BINS == 2097152);
    CHECK(kFinShift == 9 && kFinCap / 4 * 3 == 4608 && kFinStage == 6144 && kItemsBatchFrom == 8388608);
    for (const Route &r : routes) {
        const BprPrepRoute p = bpr_prep_route(r.U, r.n, r.uidx_n, r.variant);
        CHECK(p.pb.shift == r.shift && p.pb.nbins == r.nbins);
        CHECK((int)p.binned == r.binned && (int)p.finish == r.finish && (int)p.batch_items == r.batch);
    }
    // samples | workgroups of a flat kernel
    const int64_t flat[][2] = {{1, 1}, {256, 1}, {257, 2}, {524288, 2048}, {524289, 2048}, {1000000000, 2048}};
    for (const auto &r : flat) CHECK(bpr_flat_grid(r[0]) == r[1]);
    CHECK(kFlatThreads == 256);
    // counters | tiles, one workgroup
    const int64_t scan[][3] = {{1, 1, 1}, {2048, 1, 1}, {2049, 2, 1}, {32768, 16, 1}, {32769, 17, 0}, {10000002, 4883, 0}};
    for (const auto &r : scan) CHECK(bpr_scan_tiles(r[0]) == r[1] && (int)bpr_scan_one_workgroup(r[0]) == r[2]);
    CHECK(kScanTile == 2048 && kScanSmallTiles * kScanTile == 32768);
}

static void user_run_launch() {
    // users, nFactors, GORSE_BPR_D8_PAIRS | worker workgroups
    const int64_t workers[][4] = {{1, 16, 1, 1},     {16, 16, 1, 1},      {17, 16, 1, 2},      {65536, 16, 1, 4096}, {65537, 16, 1, 4096},
                                  {65536, 128, 1, 4096}, {32, 8, 1, 1},   {33, 8, 1, 2},       {131072, 8, 1, 4096}, {131073, 8, 1, 4096},
                                  {32, 8, 0, 2},     {33, 8, 0, 3},       {65537, 8, 0, 4096}};
    for (const auto &r : workers) CHECK(bpr_user_run_workers(r[0], (int)r[1], r[2] != 0) == r[3]);
    // hot slots, accumulated slots | folder workgroups
    const int folders[][3] = {{0, 0, 0}, {0, 7, 64}, {5, 0, 32}, {5, 7, 64}};
    for (const auto &r : folders) CHECK(bpr_folders(r[0], r[1]) == r[2]);
    CHECK(kFolderBlocks == 32 && kFolderBlocksAcc == 32);
    // hot slots, accumulated slots, items | the negative's class is looked up (either side of n_hot * 64 = I)
    const int64_t neg_rep[][4] = {{10, 0, 640, 1}, {10, 0, 641, 0}, {0, 0, 640, 0}, {0, 3, 640, 1}, {10, 3, 641, 1}, {1024, 0, 65536, 1},
                                  {1024, 0, 65537, 0}};
    for (const auto &r : neg_rep) CHECK((int)bpr_neg_replicas((int)r[0], (int)r[1], r[2]) == r[3]);
    // stores, cold items, store mode | the store route
    const int neg_store[][4] = {{0, 0, 0, 0}, {0, 0, 1, 0}, {0, 5, 0, 0}, {0, 5, 1, 0}, {1, 0, 0, 0}, {1, 0, 1, 0}, {1, 5, 0, 0}, {1, 5, 1, 1}};
    for (const auto &r : neg_store) CHECK((int)bpr_neg_store(r[0] != 0, r[1], r[2]) == r[3]);
    // GORSE_BPR_FOLD_SOLE_WRITER, accumulated slots, store route, base table | the sole-writer fold
    const int sole[][5] = {{0, 0, 0, 0, 0}, {0, 0, 0, 1, 0}, {0, 0, 1, 0, 0}, {0, 0, 1, 1, 0}, {0, 7, 0, 0, 0}, {0, 7, 0, 1, 0},
                           {0, 7, 1, 0, 0}, {0, 7, 1, 1, 0}, {1, 0, 0, 0, 0}, {1, 0, 0, 1, 0}, {1, 0, 1, 0, 0}, {1, 0, 1, 1, 0},
                           {1, 7, 0, 0, 0}, {1, 7, 0, 1, 1}, {1, 7, 1, 0, 0}, {1, 7, 1, 1, 0}};
    CHECK(count(sole) == 16);
    for (const auto &r : sole) CHECK((int)bpr_fold_sole(r[0] != 0, r[1], r[2] != 0, r[3] != 0) == r[4]);
}

static void per_sample_launch() {
    // samples | worker workgroups
    const int64_t workers[][2] = {{1, 1}, {16, 1}, {17, 2}, {65536, 4096}, {65537, 4096}, {1000000000, 4096}};
    for (const auto &r : workers) CHECK(bpr_sample_workers(r[0]) == r[1]);
    CHECK(kRunsPerBlock == 16 && kUpdateBlocks == 4096);
    // mode, hot slots, accumulated slots | folder workgroups
    const int folders[][4] = {{0, 0, 0, 0}, {0, 5, 0, 32}, {0, 5, 7, 64}, {1, 0, 0, 0}, {1, 5, 0, 0}, {1, 5, 7, 0},
                              {2, 0, 0, 0}, {2, 5, 0, 0},  {2, 5, 7, 0},  {3, 0, 0, 0}, {3, 5, 0, 0}, {3, 5, 7, 0}};
    for (const auto &r : folders) CHECK(bpr_sample_folders(r[0], r[1], r[2]) == r[3]);
    // nFactors | register chunks of the kernel, dynamic LDS bytes
    const int lds[][3] = {{8, 0, 1536}, {12, 0, 2304}, {16, 1, 0}, {32, 2, 0}, {64, 4, 0}, {128, 8, 0}, {256, 0, 49152}};
    for (const auto &r : lds) CHECK(bpr_sample_chunks(r[0]) == r[1] && bpr_sample_lds_bytes(r[0]) == (size_t)r[2]);
    // hot slots, accumulated slots, nFactors | workgroups of the fold kernel (either side of 130,816 and of 131,072 elements)
    const int64_t fold[][4] = {{1, 0, 1, 1},         {130816, 0, 1, 511}, {130816, 1, 1, 512},  {131072, 0, 1, 512},
                               {131072, 1, 1, 512},  {1024, 0, 128, 512}, {1024, 0, 129, 512},  {926, 2780, 64, 512}};
    for (const auto &r : fold) CHECK(bpr_fold_grid((int)r[0], (int)r[1], (int)r[2]) == r[3]);
    CHECK(kFoldThreads == 256);
}

int main() {
    schedule();
    chunk();
    preparation();
    user_run_launch();
    per_sample_launch();
    printf("bpr_plan ok\n");
    return 0;
}
