// common.hpp -- shared plumbing of libgorse_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/gorse_hip.h"
#include "../../include/gorse_hip_test.h"
#include "bpr_stream.hpp"  // Philox, kMaxDraws and the BPR sample stream

namespace gorse {

// ---- error reporting ---------------------------------------------------------------
inline std::string &last_error() {
    static thread_local std::string e;
    return e;
}
inline int32_t fail(int32_t code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    last_error() = buf;
    return code;
}
#define GORSE_HIP_CHECK(expr)                                                                          \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return gorse::fail(GORSE_ERR_HIP, "%s:%d %s -> %s", __FILE__, __LINE__, #expr,            \
                               hipGetErrorString(_e));                                                 \
    } while (0)
#define GORSE_TRY(expr)              \
    do {                             \
        int32_t _r = (expr);         \
        if (_r != GORSE_OK) return _r; \
    } while (0)

// ---- device buffer -----------------------------------------------------------------
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    int32_t alloc(size_t count) {
        release();
        if (count == 0) count = 1;
        hipError_t e = hipMalloc((void **)&p, count * sizeof(T));
        if (e != hipSuccess) {
            (void)hipGetLastError();  // reported here: the next launch's hipGetLastError must not find it
            p = nullptr;
            return fail(GORSE_ERR_NOMEM, "hipMalloc(%zu bytes): %s", count * sizeof(T), hipGetErrorString(e));
        }
        n = count;
        return GORSE_OK;
    }
    int32_t ensure(size_t count) { return count <= n ? GORSE_OK : alloc(count); }
};

// ---- staging layout -----------------------------------------------------------------
// Consecutive pieces of one staging buffer, each 256-byte aligned: take() returns a piece's offset, off is what to ensure() at the end.
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    }
};

// ---- per-kernel-class event profiling --------------------------------------------------
// Each profiled launch is bracketed by an event pair recorded on the stream the kernel
// runs on; pairs are resolved lazily (hipEventElapsedTime) when the profile is read.
struct KernelProfile {
    struct Pair {
        hipEvent_t a, b;
        int cls;
    };
    bool on = false;
    std::vector<Pair> pending;
    std::vector<hipEvent_t> pool;
    std::vector<int64_t> launches;
    std::vector<double> ms;
    explicit KernelProfile(int nclasses) : launches(nclasses, 0), ms(nclasses, 0.0) {}
    ~KernelProfile() {
        for (auto &p : pending) {
            (void)hipEventDestroy(p.a);
            (void)hipEventDestroy(p.b);
        }
        for (auto e : pool) (void)hipEventDestroy(e);
    }
    hipEvent_t get() {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e;
        (void)hipEventCreate(&e);
        return e;
    }
    // usage: auto t = prof.begin(cls, stream); launch; prof.end(t, stream);
    int begin(int cls, hipStream_t s) {
        if (!on) return -1;
        Pair p{get(), get(), cls};
        (void)hipEventRecord(p.a, s);
        pending.push_back(p);
        return (int)pending.size() - 1;
    }
    void end(int tok, hipStream_t s) {
        if (tok >= 0) (void)hipEventRecord(pending[tok].b, s);
    }
    // A span bound to its launches instead of recorded around them: the pair goes to hipExtLaunchKernelGGL (hip/hip_ext.h) as the
    // startEvent of the span's first kernel and the stopEvent of its last (the same launch when the span is one kernel), so no marker
    // packet of the profile's stands between two kernels of the stream.  Two nulls while profiling is off.  The events stay the
    // profile's until resolve(): a caller that hands the stop event on (as a chunk's "consumed" event) drops it before that.
    void events(int cls, hipEvent_t *start, hipEvent_t *stop) {
        *start = *stop = nullptr;
        if (!on) return;
        Pair p{get(), get(), cls};
        pending.push_back(p);
        *start = p.a;
        *stop = p.b;
    }
    void resolve() {  // caller has synchronised the streams
        for (auto &p : pending) {
            float t = 0;
            if (hipEventElapsedTime(&t, p.a, p.b) == hipSuccess) {
                ms[p.cls] += t;
                launches[p.cls] += 1;
            }
            pool.push_back(p.a);
            pool.push_back(p.b);
        }
        pending.clear();
    }
    void reset() {
        resolve();
        for (auto &x : launches) x = 0;
        for (auto &x : ms) x = 0;
    }
};

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Host-side one-off passes over a dataset (row sorts, validation, counting) split over the host's cores: a Fit of the
// 10M x 1M set hands over 1e9 feedback entries, and a single thread spends most of a minute on them.  fn(t, begin, end)
// works on rows [begin, end); `weight` (may be null) is the CSR row pointer the cut points are balanced by.
template <typename F>
inline void parallel_rows(int64_t rows, const int64_t *weight, F fn) {
    const int64_t work = weight ? weight[rows] - weight[0] : rows;
    int nt = (int)std::min<int64_t>(std::max(1u, std::thread::hardware_concurrency()), 64);
    // a thread per 64K entries at least (starting one costs ~0.1 ms): S-ml1m's million entries took 20 ms of a 45 ms Fit on one thread
    nt = (int)std::min<int64_t>(nt, work >> 16);
    if (nt < 2 || rows < 2 * nt) nt = 1;
    if (nt == 1) {
        fn(0, (int64_t)0, rows);
        return;
    }
    std::vector<int64_t> cut((size_t)nt + 1, rows);
    cut[0] = 0;
    for (int t = 1; t < nt; t++) {
        if (weight)
            cut[t] = std::lower_bound(weight, weight + rows + 1, weight[0] + work * t / nt) - weight;
        else
            cut[t] = rows * t / nt;
        cut[t] = std::min(std::max(cut[t], cut[t - 1]), rows);
    }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++) th.emplace_back([&, t] { fn(t, cut[t], cut[t + 1]); });
    for (auto &x : th) x.join();
}

}  // namespace gorse
