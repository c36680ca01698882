// als_deep_plan.hpp -- the packed block triangle of the Deep ALS form (csrc/als_deep.hip), shared with the CPU test of its index
// arithmetic (tests/cpp/als_deep_plan_check.cpp).  Pure C++: constexpr functions, usable on the host and in the kernels.
//
// A row's system matrix M (d x d, symmetric, 128 < d <= 256) is kept as the upper triangle of its NB x NB grid of 32 x 32 blocks,
// NB = ceil(d / 32): NT = NB (NB + 1) / 2 whole blocks (bi <= bj), block rows one after the other.  Element (i, j) with i's block
// above or on j's lives in block (i / 32, j / 32) at (i % 32, j % 32); an element below the block diagonal is read as (j, i).
#pragma once
#include <cstddef>
#include <cstdint>

namespace gorse {

constexpr int kDeepMinD = 129, kDeepMaxD = 256;  // the widths the form serves
constexpr int kDeepTileLd = 33;                  // LDS row stride of a block: a block's column is read without bank conflicts
constexpr int kDeepTileLds = 32 * kDeepTileLd;   // floats per block in LDS
constexpr int kDeepTileMem = 32 * 32;            // floats per block in global memory (partials, S)
constexpr int kDeepBatch = 32;                   // gathered rows per LDS ring buffer
constexpr int kDeepVec = 256 * 3 + 32;           // the sweep's vectors behind M: column sums, p, y, one block's steps

constexpr bool deep_serves(int d) { return d >= kDeepMinD && d <= kDeepMaxD; }
constexpr int deep_nb(int d) { return (d + 31) / 32; }
constexpr int deep_nt(int nb) { return nb * (nb + 1) / 2; }
// block (bi, bj), bi <= bj < nb -> its number in block-row order, and back
constexpr int deep_tile(int nb, int bi, int bj) { return bi * nb - bi * (bi - 1) / 2 + (bj - bi); }
constexpr int deep_tile_bi(int nb, int t) {
    int bi = 0;
    while (t >= nb - bi) t -= nb - bi, bi++;
    return bi;
}
constexpr int deep_tile_bj(int nb, int t) {
    int bi = 0;
    while (t >= nb - bi) t -= nb - bi, bi++;
    return bi + t;
}
// where element (i, j) of the symmetric matrix is stored: LDS (padded blocks) / global memory (dense blocks)
constexpr int deep_lds_index(int nb, int i, int j) {
    return i / 32 <= j / 32 ? deep_tile(nb, i / 32, j / 32) * kDeepTileLds + (i % 32) * kDeepTileLd + j % 32
                            : deep_tile(nb, j / 32, i / 32) * kDeepTileLds + (j % 32) * kDeepTileLd + i % 32;
}
constexpr int deep_mem_index(int nb, int i, int j) {
    return i / 32 <= j / 32 ? deep_tile(nb, i / 32, j / 32) * kDeepTileMem + (i % 32) * 32 + j % 32
                            : deep_tile(nb, j / 32, i / 32) * kDeepTileMem + (j % 32) * 32 + i % 32;
}
// floats of one partial (a chunk's blocks, then its 32 nb column sums) and of the packed S
constexpr int64_t deep_packed(int nb) { return (int64_t)deep_nt(nb) * kDeepTileMem; }
constexpr int64_t deep_partial_stride(int nb) { return deep_packed(nb) + 32 * nb; }
// dynamic LDS of the kernels: M's blocks (the gather ring of 2 x kDeepBatch rows lives inside them while G is accumulated) + vectors
constexpr size_t deep_lds_bytes(int nb) { return ((size_t)deep_nt(nb) * kDeepTileLds + kDeepVec) * sizeof(float); }
constexpr size_t deep_ring_bytes(int nb) { return (size_t)2 * kDeepBatch * 32 * nb * sizeof(float); }

}  // namespace gorse
