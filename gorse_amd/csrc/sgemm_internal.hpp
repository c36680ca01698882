// sgemm_internal.hpp -- what sgemm.hip (dispatch) and sgemm_nt.hip (the NT case on the matrix cores) share.
#pragma once
#include <algorithm>

#include "common.hpp"

namespace gorse {

// Which NT calls sgemm_nt_mfma_kernel can serve: a body of at least one full 16-chunk, and a tile count that fits one grid dimension.
inline bool sgemm_nt_mfma_serves(int m, int n, int k) {
    return k >= 16 && m >= 1 && n >= 1 && ceil_div(m, 64) * ceil_div(n, 64) < ((int64_t)1 << 31);
}
// Which of them take it unasked: both edges at least one wave tile, and enough elements that tiles outnumber what the per-element
// kernels do with the same rows (profiles/mm_nt_bench.json holds the threshold shape on both sides).
constexpr int64_t kNtMfmaMinElems = (int64_t)1 << 18;
inline bool sgemm_nt_mfma_auto(int m, int n, int k) {
    return sgemm_nt_mfma_serves(m, n, k) && std::min(m, n) >= 32 && (int64_t)m * n >= kNtMfmaMinElems;
}

// C = A B^T in floats.Dot's bits, operands in device memory, enqueued on st
int32_t sgemm_nt_mfma_launch(hipStream_t st, int m, int n, int k, const float *a, int lda, const float *b, int ldb, float *c, int ldc);

}  // namespace gorse
