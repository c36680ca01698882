// bpr_stream.hpp -- the BPR sample stream, stated once.  Reference: model/cf/model.go:449-468.
//
// Sample s of an epoch is the counter-based stream Philox(seed, epoch, sample_base + s).  In the order of its draws:
//   the USER     : Int31n(users) until one has feedback              (model.go:452-458)
//   the POSITIVE : Int31n(feedbacks of the user), in stored order    (model.go:459-461)
//   the NEGATIVE : Int31n(items) until one is not in the user's row  (model.go:462-468)
// The reference spins on both loops; here each gives up after kMaxDraws draws and the sample is skipped.  Every sampling and
// preparation kernel of bpr_prepare.hip composes the functions below (whole triplet; user first, items later by replay; batched first draws
// with a restart from the start of the stream), and so does the host (host/gorse_cf.hpp takes the generator from here):
// tests/cpp/bpr_stream_main.cpp composes them the same three ways and requires the same triplets.
// A pure header for hipcc and for a plain host compiler: nothing of HIP is included.
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define GORSE_HD __host__ __device__
#define GORSE_STREAM_FN __host__ __device__ inline __attribute__((always_inline))
#define GORSE_UNROLL _Pragma("unroll")
#else
#define GORSE_HD
#define GORSE_STREAM_FN inline
#define GORSE_UNROLL
#endif

namespace gorse {

// ---- Philox4x32-10 (Salmon et al., SC'11) + Go math/rand Int31n -------------------------
struct Philox {
    uint32_t c0, c1, c2, c3, k0, k1;
    uint32_t buf[4];
    int pos;
    GORSE_HD inline void init(uint64_t seed, uint64_t epoch, uint64_t sample) {
        c0 = (uint32_t)sample;
        c1 = (uint32_t)(sample >> 32);
        c2 = 0;  // block counter
        c3 = (uint32_t)epoch;
        k0 = (uint32_t)seed;
        k1 = (uint32_t)(seed >> 32);
        pos = 4;
    }
    GORSE_HD inline void block() {
        uint32_t a0 = c0, a1 = c1, a2 = c2, a3 = c3, x0 = k0, x1 = k1;
        GORSE_UNROLL
        for (int r = 0; r < 10; r++) {
            uint64_t p0 = (uint64_t)0xD2511F53u * a0;
            uint64_t p1 = (uint64_t)0xCD9E8D57u * a2;
            uint32_t n0 = (uint32_t)(p1 >> 32) ^ a1 ^ x0;
            uint32_t n1 = (uint32_t)p1;
            uint32_t n2 = (uint32_t)(p0 >> 32) ^ a3 ^ x1;
            uint32_t n3 = (uint32_t)p0;
            a0 = n0;
            a1 = n1;
            a2 = n2;
            a3 = n3;
            x0 += 0x9E3779B9u;
            x1 += 0xBB67AE85u;
        }
        buf[0] = a0;
        buf[1] = a1;
        buf[2] = a2;
        buf[3] = a3;
        c2++;
        pos = 0;
    }
    GORSE_HD inline uint32_t int31() {
        if (pos == 4) block();
        // static indexing keeps buf in registers on the device
        uint32_t v = pos == 0 ? buf[0] : pos == 1 ? buf[1] : pos == 2 ? buf[2] : buf[3];
        pos++;
        return v >> 1;
    }
    // Go math/rand (*Rand).Int31n
    GORSE_HD inline int32_t int31n(int32_t n) {
        if ((n & (n - 1)) == 0) return (int32_t)(int31() & (uint32_t)(n - 1));
        uint32_t mx = (uint32_t)((1u << 31) - 1 - (1u << 31) % (uint32_t)n);
        uint32_t v = int31();
        while (v > mx) v = int31();
        return (int32_t)(v % (uint32_t)n);
    }
};

constexpr int kMaxDraws = 4096;  // per-sample retry cap (the reference spins forever)

// x in the ascending row[0 .. n); ROW: a pointer to the row, in LDS or in global memory
template <typename ROW>
GORSE_STREAM_FN bool row_contains(ROW row, int64_t n, int32_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        int64_t mid = (lo + hi) >> 1;
        if (row[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < n && row[lo] == x;
}

// ---- the draws ---------------------------------------------------------------------------------
// Two kinds.  draw_user / replay_user / draw_negative work on a generator the caller goes on using.  redraw_user / redraw_negative
// take a sample's stream from its START with a generator of their own: the whole user draw of a kernel that keeps nothing else of
// the stream, and the restarts of the kernels that carry four samples' first draws per thread.  The second kind spells its loops out
// instead of calling the first: a generator handed on by reference compiles differently from one the function owns, and inside the
// four-chain kernels, which sit at the scalar register limit, that costs spilled scalar registers (bpr_sample_items_batch_kernel:
// 24 instead of 12) or a wave per SIMD (bpr_bin_count_kernel: 104 scalar registers instead of 92).  scripts/isa_census.py shows it;
// tests/cpp/bpr_stream_main.cpp requires that both kinds draw the same.

// model.go:452-458: the user -- the first drawn row that holds feedback, -1 when kMaxDraws draws met none.  g: at the start of the
// sample's stream; uptr: the CSR row pointers of the users.
GORSE_STREAM_FN int32_t draw_user(Philox &g, int32_t U, const int64_t *uptr) {
    for (int t = 0; t < kMaxDraws; t++) {
        const int32_t cu = g.int31n(U);
        if (uptr[cu + 1] > uptr[cu]) return cu;
    }
    return -1;
}
// ... of sample `sample`, from the start of its stream
GORSE_STREAM_FN int32_t redraw_user(uint64_t seed, uint64_t epoch, uint64_t sample, int32_t U, const int64_t *uptr) {
    Philox g;
    g.init(seed, epoch, sample);
    for (int t = 0; t < kMaxDraws; t++) {
        const int32_t cu = g.int31n(U);
        if (uptr[cu + 1] > uptr[cu]) return cu;
    }
    return -1;
}

// the user draws again for a sample whose user is known to be u: the rows drawn before u were empty (u is the first non-empty
// one), so no look-up is needed.  g: at the start of the sample's stream; left in front of the positive's draw.
GORSE_STREAM_FN void replay_user(Philox &g, int32_t U, int32_t u) {
    for (int k = 0; k < kMaxDraws; k++)
        if (g.int31n(U) == u) break;
}

// model.go:462-468: the negative -- the first drawn item outside the user's sorted row[0 .. cnt), -1 when kMaxDraws draws met
// none.  g: behind the positive's draw.
template <typename ROW>
GORSE_STREAM_FN int32_t draw_negative(Philox &g, int32_t I, ROW row, int64_t cnt) {
    for (int k = 0; k < kMaxDraws; k++) {
        const int32_t c = g.int31n(I);
        if (!row_contains(row, cnt, c)) return c;
    }
    return -1;
}
// ... of sample `sample`, from the start of its stream, given its user u: replay_user, the positive's draw passed over, draw_negative
template <typename ROW>
GORSE_STREAM_FN int32_t redraw_negative(uint64_t seed, uint64_t epoch, uint64_t sample, int32_t U, int32_t I, int32_t u, ROW row,
                                        int64_t cnt) {
    Philox g;
    g.init(seed, epoch, sample);
    for (int k = 0; k < kMaxDraws; k++)
        if (g.int31n(U) == u) break;
    (void)g.int31n((int32_t)cnt);  // the positive's draw
    for (int k = 0; k < kMaxDraws; k++) {
        const int32_t c = g.int31n(I);
        if (!row_contains(row, cnt, c)) return c;
    }
    return -1;
}

}  // namespace gorse
