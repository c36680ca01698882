// csr_scan.hpp -- the 64-bit exclusive scan that turns per-row counts into a CSR row pointer, shared by nbr_build.hip (the rows of a
// neighbour table) and cand.hip (the exclusion rows and the finished candidate rows of a chain).  Three kernels, 2048 counts per
// workgroup; each translation unit that includes this gets its own copy of them.
#pragma once
#include "common.hpp"

namespace {

constexpr int kScanThreads = 256, kScanPer = 8;  // the scan: 2048 counts per workgroup

// exclusive scan of v over the workgroup's 256 threads; *total = the workgroup's sum.  Ends behind a barrier: sh may be used again.
__device__ __forceinline__ long long block_exclusive(long long v, long long *sh, long long *total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
        const long long t = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    const long long incl = sh[tid];
    *total = sh[kScanThreads - 1];
    __syncthreads();
    return incl - v;
}

// The row pointer: x[0 .. n) exclusive-scanned in place, 64 bits wide (a million rows of a hundred entries pass 2^31 at twenty
// times that).  sums[b] = the sum of workgroup b's 2048 entries; one workgroup scans the sums; every workgroup scans its own.
__global__ __launch_bounds__(kScanThreads) void nbr_scan_sums_kernel(const long long *__restrict__ x, int64_t n, long long *__restrict__ sums) {
    __shared__ long long sh[kScanThreads];
    const int64_t first = ((int64_t)blockIdx.x * kScanThreads + threadIdx.x) * kScanPer;
    long long v = 0;
    for (int e = 0; e < kScanPer; e++)
        if (first + e < n) v += x[first + e];
    long long total;
    (void)block_exclusive(v, sh, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}
__global__ __launch_bounds__(kScanThreads) void nbr_scan_top_kernel(long long *sums, int64_t nb) {
    __shared__ long long sh[kScanThreads];
    long long carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += kScanThreads) {
        const int64_t b = b0 + threadIdx.x;
        const long long v = b < nb ? sums[b] : 0;
        long long total;
        const long long ex = block_exclusive(v, sh, &total);
        if (b < nb) sums[b] = carry + ex;
        carry += total;
    }
}
__global__ __launch_bounds__(kScanThreads) void nbr_scan_apply_kernel(long long *x, int64_t n, const long long *__restrict__ sums) {
    __shared__ long long sh[kScanThreads];
    const int64_t first = ((int64_t)blockIdx.x * kScanThreads + threadIdx.x) * kScanPer;
    long long own[kScanPer], v = 0;
#pragma unroll
    for (int e = 0; e < kScanPer; e++) {
        own[e] = first + e < n ? x[first + e] : 0;
        v += own[e];
    }
    long long total;
    long long run = sums[blockIdx.x] + block_exclusive(v, sh, &total);
#pragma unroll
    for (int e = 0; e < kScanPer; e++) {
        if (first + e < n) x[first + e] = run;
        run += own[e];
    }
}

// x[0 .. n) exclusive-scanned in place on `st`; `sums` is the scan's own scratch (grown as needed)
inline int32_t csr_exclusive_scan(long long *x, int64_t n, gorse::DevBuf<long long> &sums, hipStream_t st) {
    const int64_t per = (int64_t)kScanThreads * kScanPer, nb = gorse::ceil_div(n, per);
    GORSE_TRY(sums.ensure((size_t)nb));
    nbr_scan_sums_kernel<<<dim3((unsigned)nb), dim3(kScanThreads), 0, st>>>(x, n, sums.p);
    nbr_scan_top_kernel<<<dim3(1), dim3(kScanThreads), 0, st>>>(sums.p, nb);
    nbr_scan_apply_kernel<<<dim3((unsigned)nb), dim3(kScanThreads), 0, st>>>(x, n, sums.p);
    GORSE_HIP_CHECK(hipGetLastError());
    return GORSE_OK;
}

}  // namespace
