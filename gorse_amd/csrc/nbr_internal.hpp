// nbr_internal.hpp -- the gorse_nbr handle shared by nbr_recommend.hip (the walk) and nbr_build.hip (tables built on the device
// from a similarity search's results).
#pragma once
#include "common.hpp"

namespace gorse {

struct NbrTable {
    bool set = false, weighted = false;
    bool on_device_only = false;  // built by nbr_build.hip: the indices never crossed to the host (idx stays empty)
    int64_t n_rows = 0, nnz = 0, max_index = -1;
    int32_t transform = GORSE_NBR_RAW;
    double scale = 1.0;
    std::vector<int64_t> ptr;  // host copy of the row pointer: the planner's bounds and gorse_nbr_get_table read it
    std::vector<int32_t> idx;  // host-built hop 1 only: the bounds are one pass over its indices and hop 2's row pointer
    DevBuf<int64_t> d_ptr;
    DevBuf<int32_t> d_idx;
    DevBuf<float> d_w;
};

}  // namespace gorse

struct gorse_nbr {
    int device = 0;
    int64_t n_items = 0;
    hipStream_t stream = nullptr;
    gorse::NbrTable tab[2];
    std::vector<int64_t> src_sum;  // per hop-1 row, valid while bounds_valid
    bool bounds_valid = false;
    gorse::DevBuf<char> in, out, scratch;
    gorse::DevBuf<char> seen_in;  // gorse_nbr_recommend's seen rows (row pointer | items); the candidate chain brings its own
    int64_t n_lds = 0, n_global = 0;
    double ms = 0.0;
    int32_t use() {
        GORSE_HIP_CHECK(hipSetDevice(device));
        return GORSE_OK;
    }
};

namespace gorse {
// nbr_build.hip: src_sum[r] of a hop-1 table whose indices lie on the device only -- nbr::row_bounds computed there, n_rows values back
int32_t nbr_device_row_bounds(gorse_nbr *h, std::vector<int64_t> *src_sum);

// nbr_recommend.hip, in two halves so that the candidate chain (cand.hip) walks from its own device-resident exclusion rows.
// check: everything gorse_nbr_recommend validates (seen_indptr == NULL: no seen rows to look at).
// core: plans and walks.  The seen rows are a CSR on the device (d_sptr from 0, d_seen) whose row pointer the host holds too
// (sptr_host: the planner's bounds need the row lengths); sptr_host == NULL: no seen rows.  The result rows stay in h->out:
// n_queries * k items padded with -1, the sums' bits padded with 0, and the counts, valid until the handle's next call.  Returns
// behind the walk (the handle's stream is idle).
struct NbrDeviceRows {
    const int32_t *items = nullptr;
    const unsigned long long *sums = nullptr;
    const int32_t *cnt = nullptr;
};
int32_t nbr_recommend_check(gorse_nbr *h, const char *who, int64_t n_queries, const int32_t *rows, int32_t k, const int64_t *seen_indptr,
                            const int32_t *seen_items);
int32_t nbr_recommend_core(gorse_nbr *h, int64_t n_queries, const int32_t *rows, int32_t k, const int64_t *sptr_host,
                           const int64_t *d_sptr, const int32_t *d_seen, NbrDeviceRows *res);
}  // namespace gorse
