// topk_tri.hip -- the triangle-sharded all-pairs search of path B of the exact top-k (top-k row):
// gorse_topk_tri_*, over the stages of a chunk that topk_mfma.hip defines.
// Query-row sharding gives a rank the saving of the symmetric sweep on its own diagonal square only (1 / world^2 of the matrix).
// Here the TRIANGLE is sharded: rank r sweeps the query blocks C with C % world == r -- each block's own lists, and what it finds
// for the rows of every earlier block as queries, whoever owns them -- so the union over the ranks is exactly the single-rank
// symmetric sweep, every score still serving both of its queries.  The pilots are sharded by contiguous slices of the queries
// (their thresholds are all-gathered: 4 bytes per query); after the sweep a rank holds partial foreign lists of queries the
// OTHER ranks own, which travel to the owners (pack -> all-to-all -> unpack: ~130 entries of 8 bytes per query in all); rescoring
// and tie path then run on the owner.  The exchange itself is the caller's (gorse_amd/dist.py: torch.distributed, or host memory when
// the ranks are emulated on one device); every buffer that crosses the boundary may be host or device memory.
#include "topk_mfma_internal.hpp"

using namespace gorse;

namespace {

__device__ __forceinline__ int64_t tri_query_of(int64_t i, int rank, int world) {  // the i-th query a rank owns
    return ((i / kSymBQ) * world + rank) * (int64_t)kSymBQ + i % kSymBQ;
}
__global__ void tri_pack_counts_kernel(const int32_t *__restrict__ fcnt, const uint8_t *__restrict__ cflag, int64_t n_owned, int dest,
                                       int world, int32_t *__restrict__ counts) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_owned; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = tri_query_of(i, dest, world);
        const int32_t c = fcnt[t];
        // -1 = "this part of the list is useless": a staging overflow here (flag 1; flag 2 = no pilot threshold is known to every
        // rank) or more entries than a list holds -- the owner then sends the query down the tie path
        counts[i] = (cflag[t] == 1 || c > kCapF) ? -1 : c;
    }
}
// exclusive prefix of max(counts, 0) by ONE workgroup (n <= a million words: two passes over a few megabytes)
__global__ __launch_bounds__(1024) void tri_scan_kernel(const int32_t *__restrict__ counts, int64_t n, int64_t *__restrict__ offsets) {
    __shared__ long long part[1024];
    const int tid = threadIdx.x;
    const int64_t per = (n + 1023) / 1024, a = tid * per, b = a + per < n ? a + per : n;
    long long s = 0;
    for (int64_t i = a; i < b; i++) s += counts[i] > 0 ? counts[i] : 0;
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        long long run = 0;
        for (int i = 0; i < 1024; i++) {
            const long long v = part[i];
            part[i] = run;
            run += v;
        }
        offsets[n] = run;
    }
    __syncthreads();
    long long run = part[tid];
    for (int64_t i = a; i < b; i++) {
        offsets[i] = run;
        run += counts[i] > 0 ? counts[i] : 0;
    }
}
__global__ void tri_pack_entries_kernel(const uint2 *__restrict__ fbuf, const int32_t *__restrict__ counts, const int64_t *__restrict__ offsets,
                                        int64_t n_owned, int dest, int world, uint2 *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n_owned; i += (int64_t)gridDim.x * (blockDim.x >> 6)) {
        const int c = counts[i];
        const uint2 *src = fbuf + tri_query_of(i, dest, world) * kCapF;
        uint2 *dst = out + offsets[i];
        for (int e = lane; e < c; e += 64) dst[e] = src[e];
    }
}
__global__ void tri_unpack_kernel(uint2 *__restrict__ fbuf, int32_t *__restrict__ fcnt, const int32_t *__restrict__ counts,
                                  const int64_t *__restrict__ offsets, const uint2 *__restrict__ entries, int64_t n_owned, int rank, int world) {
    const int lane = threadIdx.x & 63;
    for (int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < n_owned; i += (int64_t)gridDim.x * (blockDim.x >> 6)) {
        const int64_t t = tri_query_of(i, rank, world);
        const int c = counts[i];
        const int base = fcnt[t];  // (every lane reads it before lane 0 writes: a wave runs in step)
        if (c < 0) {
            if (lane == 0) fcnt[t] = kCapF + 1;  // overflowed on the sender's side: topk_rescore_kernel flags the query
            continue;
        }
        const uint2 *src = entries + offsets[i];
        uint2 *dst = fbuf + t * kCapF;
        for (int e = lane; e < c; e += 64)
            if (base + e < kCapF) dst[base + e] = src[e];
        if (lane == 0) fcnt[t] = base + c;  // may pass kCapF: the list overflowed at its owner
    }
}

TriGeom tri_geom(const ChunkState &cs) { return TriGeom(cs.m, cs.tri_world); }

int32_t tri_state(gorse_topk *h, int stage_min, ChunkState **out) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    ChunkState *cs = h->cstate;
    if (!cs || cs->tri_stage < stage_min) return fail(GORSE_ERR_INVALID, "gorse_topk_tri_*: called out of order (stage %d, needs %d)", cs ? cs->tri_stage : 0, stage_min);
    GORSE_TRY(h->use());
    *out = cs;
    return GORSE_OK;
}

}  // namespace

extern "C" int32_t gorse_topk_tri_begin(gorse_topk *h, int64_t q_begin, int64_t q_end, int32_t k, int32_t rank, int32_t world) {
    if (!h) return fail(GORSE_ERR_INVALID, "handle is NULL");
    if (q_begin < 0 || q_end > h->N || q_begin >= q_end || k <= 0) return fail(GORSE_ERR_RANGE, "bad query range");
    if (world < 1 || rank < 0 || rank >= world) return fail(GORSE_ERR_INVALID, "rank %d of %d", rank, world);
    const int64_t nq = q_end - q_begin;
    GORSE_TRY(h->use());
    // what the symmetric sweep needs (sym_eligible, as chunk_main asks it), of an MFMA search over one chunk
    const bool ok = topk_mfma_usable(h, nq, k) && nq <= kChunkQ && sym_eligible(g_topk_variant, h->kp, k + 1, h->N, q_begin, nq);
    if (!ok)
        return fail(GORSE_ERR_INVALID, "this search has no symmetric form (operand depth, a range that does not start on a 128-row boundary, fewer than "
                                       "%d queries or more than %lld, an index of fewer than 2^17 rows): shard its query rows instead", 2 * kSymBQ, (long long)kChunkQ);
    ChunkState &cs = *h->chunk_state();
    GORSE_TRY(search_setup(h, cs, nullptr, q_begin, nullptr, nq, k, 0));
    cs.c0 = 0, cs.m = nq, cs.tri_rank = rank, cs.tri_world = world;
    // few, long workgroups are cut by rows, every slice with own lists of its own (tri_own_slices, topk_plan.hpp)
    cs.sym_slices = tri_own_slices(g_topk_variant, tri_geom(cs).blocks_of(rank), world);
    if (cs.sym_slices > 1) {
        GORSE_TRY(h->cbuf.ensure((size_t)cs.sym_slices * cs.mb * kCap));
        GORSE_TRY(h->ccnt.ensure((size_t)cs.sym_slices * cs.mb));
        GORSE_TRY(h->cflag.ensure((size_t)cs.sym_slices * cs.mb));
    }
    GORSE_TRY(chunk_prepare(h, cs));
    if (!cs.warm) return fail(GORSE_ERR_INVALID, "the sweep of this search is not warm-started");
    GORSE_TRY(h->f0.ensure((size_t)cs.mb));
    GORSE_TRY(h->f1.ensure((size_t)cs.sym_slices * cs.mb));
    tri_geom(cs).slice(rank, &cs.tri_lo, &cs.tri_hi);
    const int tok = h->prof.begin(GORSE_PROF_TOPK_SWEEP, h->stream);
    GORSE_TRY(chunk_pilots(h, cs, cs.tri_lo, cs.tri_hi));
    h->prof.end(tok, h->stream);
    cs.tri_stage = 1;
    return GORSE_OK;
}

extern "C" int32_t gorse_topk_tri_slice(gorse_topk *h, int32_t rank, int64_t *lo, int64_t *hi, int64_t *owned) {
    ChunkState *cs;
    GORSE_TRY(tri_state(h, 1, &cs));
    if (rank < 0 || rank >= cs->tri_world) return fail(GORSE_ERR_INVALID, "rank %d of %d", rank, cs->tri_world);
    int64_t a, b;
    tri_geom(*cs).slice(rank, &a, &b);
    if (lo) *lo = a;
    if (hi) *hi = b;
    if (owned) *owned = tri_geom(*cs).owned(rank);
    return GORSE_OK;
}

extern "C" int32_t gorse_topk_tri_thresholds_get(gorse_topk *h, int64_t lo, int64_t hi, float *dst) {
    ChunkState *cs;
    GORSE_TRY(tri_state(h, 1, &cs));
    if (lo < 0 || hi > cs->m || lo > hi || !dst) return fail(GORSE_ERR_RANGE, "bad slice");
    GORSE_HIP_CHECK(hipMemcpyAsync(dst, h->f0.p + lo, (size_t)(hi - lo) * 4, hipMemcpyDefault, h->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    return GORSE_OK;
}
extern "C" int32_t gorse_topk_tri_thresholds_put(gorse_topk *h, int64_t lo, int64_t hi, const float *src) {
    ChunkState *cs;
    GORSE_TRY(tri_state(h, 1, &cs));
    if (lo < 0 || hi > cs->m || lo > hi || !src) return fail(GORSE_ERR_RANGE, "bad slice");
    GORSE_HIP_CHECK(hipMemcpyAsync(h->f0.p + lo, src, (size_t)(hi - lo) * 4, hipMemcpyDefault, h->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));  // the source may be reused
    return GORSE_OK;
}

extern "C" int32_t gorse_topk_tri_sweep(gorse_topk *h) {
    ChunkState *cs;
    GORSE_TRY(tri_state(h, 1, &cs));
    const int tok = h->prof.begin(GORSE_PROF_TOPK_SWEEP, h->stream);
    GORSE_TRY(chunk_main(h, *cs));
    h->prof.end(tok, h->stream);
    if (!cs->sym) return fail(GORSE_ERR_INVALID, "the main sweep did not take the symmetric form");
    cs->tri_stage = 2;
    return GORSE_OK;
}

extern "C" int32_t gorse_topk_tri_pack(gorse_topk *h, int32_t dest, int64_t *n_counts, int64_t *n_entries) {
    ChunkState *cs;
    GORSE_TRY(tri_state(h, 2, &cs));
    if (dest < 0 || dest >= cs->tri_world || dest == cs->tri_rank) return fail(GORSE_ERR_INVALID, "bad destination rank %d", dest);
    const int64_t n = tri_geom(*cs).owned(dest);
    GORSE_TRY(h->tri_counts.ensure((size_t)std::max<int64_t>(n, 1)));
    GORSE_TRY(h->tri_offsets.ensure((size_t)n + 1));
    long long total = 0;
    if (n > 0) {
        tri_pack_counts_kernel<<<dim3((unsigned)std::min<int64_t>(ceil_div(n, 256), 2048)), dim3(256), 0, h->stream>>>(
            h->fcnt.p, h->cflag.p, n, dest, cs->tri_world, h->tri_counts.p);
        tri_scan_kernel<<<dim3(1), dim3(1024), 0, h->stream>>>(h->tri_counts.p, n, reinterpret_cast<int64_t *>(h->tri_offsets.p));
        GORSE_HIP_CHECK(hipGetLastError());
        GORSE_HIP_CHECK(hipMemcpyAsync(&total, h->tri_offsets.p + n, 8, hipMemcpyDeviceToHost, h->stream));
        GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
        GORSE_TRY(h->tri_entries.ensure((size_t)std::max<long long>(total, 1)));
        if (total > 0) {
            tri_pack_entries_kernel<<<dim3((unsigned)std::min<int64_t>(ceil_div(n, 4), 8192)), dim3(256), 0, h->stream>>>(
                h->fbuf.p, h->tri_counts.p, reinterpret_cast<const int64_t *>(h->tri_offsets.p), n, dest, cs->tri_world, h->tri_entries.p);
            GORSE_HIP_CHECK(hipGetLastError());
            GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));  // the message is complete when this returns: another handle's stream may read it
        }
    }
    h->tri_packed_counts = n, h->tri_packed_entries = total;
    if (n_counts) *n_counts = n;
    if (n_entries) *n_entries = total;
    return GORSE_OK;
}

extern "C" int32_t gorse_topk_tri_pack_read(gorse_topk *h, int32_t *counts, uint64_t *entries) {
    ChunkState *cs;
    GORSE_TRY(tri_state(h, 2, &cs));
    if (counts && h->tri_packed_counts > 0)
        GORSE_HIP_CHECK(hipMemcpyAsync(counts, h->tri_counts.p, (size_t)h->tri_packed_counts * 4, hipMemcpyDefault, h->stream));
    if (entries && h->tri_packed_entries > 0)
        GORSE_HIP_CHECK(hipMemcpyAsync(entries, h->tri_entries.p, (size_t)h->tri_packed_entries * 8, hipMemcpyDefault, h->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    return GORSE_OK;
}

extern "C" int32_t gorse_topk_tri_unpack(gorse_topk *h, int32_t src, const int32_t *counts, int64_t n_counts, const uint64_t *entries,
                                         int64_t n_entries) {
    ChunkState *cs;
    GORSE_TRY(tri_state(h, 2, &cs));
    if (src < 0 || src >= cs->tri_world || src == cs->tri_rank) return fail(GORSE_ERR_INVALID, "bad source rank %d", src);
    const int64_t n = tri_geom(*cs).owned(cs->tri_rank);
    if (n_counts != n) return fail(GORSE_ERR_INVALID, "rank %d owns %lld queries, the message holds %lld", cs->tri_rank, (long long)n, (long long)n_counts);
    if (n == 0) return GORSE_OK;
    if (!counts || (n_entries > 0 && !entries) || n_entries < 0) return fail(GORSE_ERR_INVALID, "NULL message");
    GORSE_TRY(h->tri_in_counts.ensure((size_t)n));
    GORSE_TRY(h->tri_offsets.ensure((size_t)n + 1));
    GORSE_TRY(h->tri_in_entries.ensure((size_t)std::max<int64_t>(n_entries, 1)));
    GORSE_HIP_CHECK(hipMemcpyAsync(h->tri_in_counts.p, counts, (size_t)n * 4, hipMemcpyDefault, h->stream));
    if (n_entries > 0) GORSE_HIP_CHECK(hipMemcpyAsync(h->tri_in_entries.p, entries, (size_t)n_entries * 8, hipMemcpyDefault, h->stream));
    tri_scan_kernel<<<dim3(1), dim3(1024), 0, h->stream>>>(h->tri_in_counts.p, n, reinterpret_cast<int64_t *>(h->tri_offsets.p));
    long long total = 0;
    GORSE_HIP_CHECK(hipMemcpyAsync(&total, h->tri_offsets.p + n, 8, hipMemcpyDeviceToHost, h->stream));
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    if (total != n_entries) return fail(GORSE_ERR_INVALID, "the message's counts add up to %lld entries, it holds %lld", total, (long long)n_entries);
    tri_unpack_kernel<<<dim3((unsigned)std::min<int64_t>(ceil_div(n, 4), 8192)), dim3(256), 0, h->stream>>>(
        h->fbuf.p, h->fcnt.p, h->tri_in_counts.p, reinterpret_cast<const int64_t *>(h->tri_offsets.p), h->tri_in_entries.p, n, cs->tri_rank, cs->tri_world);
    GORSE_HIP_CHECK(hipGetLastError());
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));  // the caller's buffers may be reused
    return GORSE_OK;
}

extern "C" int32_t gorse_topk_tri_finish(gorse_topk *h, int32_t *idx_out, float *dist_out) {
    ChunkState *cs;
    GORSE_TRY(tri_state(h, 2, &cs));
    GORSE_TRY(chunk_finish(h, *cs));
    // the rows of the queries this rank owns into the caller's nq x k arrays (the others are left alone): one strided copy for
    // the whole blocks, one for a partial last block
    const TriGeom g = tri_geom(*cs);
    const int k = cs->k, W = cs->tri_world, r = cs->tri_rank;
    const int64_t nb = g.blocks_of(r);
    if (nb > 0 && (idx_out || dist_out)) {
        const int64_t last = r + (nb - 1) * W;
        const bool partial = (last + 1) * kSymBQ > g.nq;
        const int64_t full = partial ? nb - 1 : nb;
        const size_t width = (size_t)kSymBQ * k * 4, pitch = width * W, first = (size_t)r * kSymBQ * k;
        if (full > 0) {
            if (idx_out) GORSE_HIP_CHECK(hipMemcpy2DAsync(idx_out + first, pitch, h->res_idx.p + first, pitch, width, (size_t)full, hipMemcpyDeviceToHost, h->stream));
            if (dist_out) GORSE_HIP_CHECK(hipMemcpy2DAsync(dist_out + first, pitch, h->res_dist.p + first, pitch, width, (size_t)full, hipMemcpyDeviceToHost, h->stream));
        }
        if (partial) {
            const size_t at = (size_t)last * kSymBQ * k, bytes = (size_t)(g.nq - last * kSymBQ) * k * 4;
            if (idx_out) GORSE_HIP_CHECK(hipMemcpyAsync(idx_out + at, h->res_idx.p + at, bytes, hipMemcpyDeviceToHost, h->stream));
            if (dist_out) GORSE_HIP_CHECK(hipMemcpyAsync(dist_out + at, h->res_dist.p + at, bytes, hipMemcpyDeviceToHost, h->stream));
        }
    }
    GORSE_HIP_CHECK(hipStreamSynchronize(h->stream));
    cs->tri_stage = 3;
    return GORSE_OK;
}

// One process, N handles (one per GPU -- or N on one device: the emulation the tests run): the whole triangle-sharded search in one
// call, the two exchanges as device-to-device copies between the handles (hipMemcpyDefault: peer-to-peer over xGMI where the devices
// can reach each other, staged otherwise).  What a Go master that owns all GPUs of a node calls (integration/go/common/ann/
// bruteforce_hip.go SearchAllSharded); one process per GPU drives gorse_topk_tri_* itself and moves the messages over its own transport.
extern "C" int32_t gorse_topk_tri_all_pairs_local(gorse_topk **hs, int32_t n, int64_t q_begin, int64_t q_end, int32_t k, int32_t *idx_out,
                                                  float *dist_out) {
    if (!hs || n < 1) return fail(GORSE_ERR_INVALID, "no handles");
    for (int r = 0; r < n; r++)
        if (!hs[r]) return fail(GORSE_ERR_INVALID, "handle %d is NULL", r);
    for (int r = 0; r < n; r++) GORSE_TRY(gorse_topk_tri_begin(hs[r], q_begin, q_end, k, r, n));  // every rank's pilots are enqueued ...
    for (int r = 0; r < n; r++) {                                                                // ... before anybody waits for them
        GORSE_TRY(hs[r]->use());
        GORSE_HIP_CHECK(hipStreamSynchronize(hs[r]->stream));
    }
    for (int r = 0; r < n; r++)  // all-gather of the thresholds: every rank fetches the other ranks' slices from where they lie
        for (int s = 0; s < n; s++) {
            if (s == r) continue;
            int64_t lo = 0, hi = 0;
            GORSE_TRY(gorse_topk_tri_slice(hs[s], s, &lo, &hi, nullptr));
            if (hi > lo) GORSE_TRY(gorse_topk_tri_thresholds_put(hs[r], lo, hi, hs[s]->f0.p + lo));
        }
    for (int r = 0; r < n; r++) GORSE_TRY(gorse_topk_tri_sweep(hs[r]));  // enqueued on every device, then awaited
    for (int r = 0; r < n; r++) {
        GORSE_TRY(hs[r]->use());
        GORSE_HIP_CHECK(hipStreamSynchronize(hs[r]->stream));
    }
    for (int src = 0; src < n; src++)  // all-to-all of the foreign lists
        for (int dst = 0; dst < n; dst++) {
            if (dst == src) continue;
            int64_t nc = 0, ne = 0;
            GORSE_TRY(gorse_topk_tri_pack(hs[src], dst, &nc, &ne));
            if (nc > 0) GORSE_TRY(gorse_topk_tri_unpack(hs[dst], src, hs[src]->tri_counts.p, nc, reinterpret_cast<const uint64_t *>(hs[src]->tri_entries.p), ne));
        }
    for (int r = 0; r < n; r++) GORSE_TRY(gorse_topk_tri_finish(hs[r], idx_out, dist_out));  // every rank writes the rows it owns
    return GORSE_OK;
}
