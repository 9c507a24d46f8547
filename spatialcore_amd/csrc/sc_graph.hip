// The active CSR graph: setters, processing order, transpose, squidpy's graph moments, weight sum, neighbourhood
// composition.  The neighbour searches that produce graphs are in sc_search.hip.  gfx950 only.
#include <float.h>
#include <math.h>

#include <vector>

#include "sc_sortscan.h"

// ------------------------------------------------------------------------------------------------
// A3: CSR graph
// ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_check_csr(const long long *__restrict__ indptr,
                                                   const int32_t *__restrict__ indices, int64_t n,
                                                   int *__restrict__ flag)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int bad = 0;
    for (long long e = indptr[i]; e < indptr[i + 1]; ++e) {
        int32_t j = indices[e];
        if (j < 0 || j >= n) bad |= 1;
        if (e > indptr[i] && indices[e - 1] >= j) bad |= 2;
    }
    if (bad) atomicOr(flag, bad);
}

// ---- processing order with spatial locality (see sc_ctx.h) ----
__global__ __launch_bounds__(256) void k_iota32(int32_t *__restrict__ a, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = (int32_t)i;
}

__global__ __launch_bounds__(256) void k_rank_of(const int32_t *__restrict__ order, int64_t n, int32_t *__restrict__ rank)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) rank[order[r]] = (int32_t)r;
}

__global__ __launch_bounds__(256) void k_relabel_edges(const int32_t *__restrict__ indices, const double *__restrict__ w,
                                                       const int32_t *__restrict__ rank, int64_t nnz,
                                                       int32_t *__restrict__ indices_r, float *__restrict__ w32)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    indices_r[e] = rank[indices[e]];
    w32[e] = (float)w[e];
}

__global__ __launch_bounds__(256) void k_edge_rows(const long long *__restrict__ indptr, const int32_t *__restrict__ rank,
                                                   int64_t n, int32_t *__restrict__ erow_r)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t r = rank[i];
    for (long long e = indptr[i]; e < indptr[i + 1]; ++e) erow_r[e] = r;
}

// The graph setters call this: if the points of the last neighbour search are the graph's cells (same count), a
// spatially compact processing order is kept with the graph (the bin-sorted order of the neighbour search), otherwise
// the identity.  A wrong guess costs speed, never correctness: it is only the order in which
// kernels that gather neighbours' rows (k_lag, k_lag_u8, local Moran, enrichment) walk the cells.
int sc_graph_capture_order(sc_ctx *c, int64_t n)
{
    c->g_order_ready = false;
    SC_TRY(c->g_order.ensure(sizeof(int32_t) * (size_t)n, &c->mem));
    // The row-major bin order of the neighbour search (it is there already).  A Morton (Z) curve over the bin grid's extent
    // instead (one more radix sort, 1.5 ms at 1M cells) was measured in r03 on k_lag, the local Moran count kernels and the
    // enrichment: it cuts their L2 misses (k_lag: a third of the fetched bytes) but not their time (all of them are bound
    // by the rows through the CUs' texture path, not by where they come from).
    if (c->pts_n == n && c->sid.p)
        SC_HIP(hipMemcpyAsync(c->g_order.p, c->sid.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    else
        hipLaunchKernelGGL(k_iota32, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, c->stream, c->g_order.as<int32_t>(), n);
    SC_HIP(hipGetLastError());
    c->g_order_captured = true;
    return SC_OK;
}

int sc_graph_ensure_order(sc_ctx *c)
{
    if (c->g_order_ready) return SC_OK;
    const int64_t n = c->g_n, nnz = c->g_nnz;
    SC_REQUIRE(n > 0 && c->g_order_captured, SC_ERR_STATE, "no graph set");
    SC_TRY(c->g_rank.ensure(sizeof(int32_t) * (size_t)n, &c->mem));
    SC_TRY(c->g_indices_r.ensure(sizeof(int32_t) * (size_t)(nnz > 0 ? nnz : 1), &c->mem));
    SC_TRY(c->g_w32.ensure(sizeof(float) * (size_t)(nnz > 0 ? nnz : 1), &c->mem));
    SC_TRY(c->g_erow_r.ensure(sizeof(int32_t) * (size_t)(nnz > 0 ? nnz : 1), &c->mem));
    hipLaunchKernelGGL(k_rank_of, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, c->stream, c->g_order.as<int32_t>(), n,
                       c->g_rank.as<int32_t>());
    if (nnz > 0)
        hipLaunchKernelGGL(k_relabel_edges, dim3((unsigned)ceil_div64(nnz, 256)), dim3(256), 0, c->stream,
                           c->g_indices.as<int32_t>(), c->g_data.as<double>(), c->g_rank.as<int32_t>(), nnz,
                           c->g_indices_r.as<int32_t>(), c->g_w32.as<float>());
    hipLaunchKernelGGL(k_edge_rows, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, c->stream, c->g_indptr.as<long long>(),
                       c->g_rank.as<int32_t>(), n, c->g_erow_r.as<int32_t>());
    SC_HIP(hipGetLastError());
    c->g_order_ready = true;
    return SC_OK;
}

// The active graph is gone: its arrays are about to be replaced (the setters) or used as scratch (sc_radius_fill_2d).
// Waits for a moments computation on the side stream, which still reads them, and forgets everything derived from them.
void sc_graph_drop(sc_ctx *c)
{
    sc_graph_moments_drain(c);
    c->g_n = 0;
    c->g_nnz = 0;
    c->gt_valid = false;
    c->s0_valid = false;
    c->s0_only_valid = false;
    c->prep_early = false;
}

extern "C" int sc_graph_set_csr(sc_ctx *c, const int64_t *indptr, const int32_t *indices, const double *data,
                                int64_t n, int64_t nnz)
{
    SC_REQUIRE(c && indptr, SC_ERR_INVALID, "sc_graph_set_csr: null pointer");
    SC_REQUIRE(n >= 1 && n <= 0x7fffffffLL && nnz >= 0, SC_ERR_INVALID, "sc_graph_set_csr: bad shape");
    SC_REQUIRE(nnz == 0 || (indices && data), SC_ERR_INVALID, "sc_graph_set_csr: null indices/data");
    SC_REQUIRE(indptr[0] == 0 && indptr[n] == nnz, SC_ERR_INVALID, "sc_graph_set_csr: indptr does not span nnz");
    int64_t deg_max = 0, deg_min = INT64_MAX;
    for (int64_t i = 0; i < n; ++i) {
        SC_REQUIRE(indptr[i + 1] >= indptr[i], SC_ERR_INVALID, "sc_graph_set_csr: indptr not monotone");
        const int64_t deg = indptr[i + 1] - indptr[i];
        if (deg > deg_max) deg_max = deg;
        if (deg < deg_min) deg_min = deg;
    }
    // all weights equal (a kNN graph after row normalisation: 1 / k)?  Integer-count genes then sit on an integer
    // lattice and their permutation counts are decided exactly (sc_moran.hip, "lattice genes")
    double uniform_w = nnz > 0 ? data[0] : 0.0;
    for (int64_t e = 1; e < nnz && uniform_w != 0.0; ++e)
        if (data[e] != uniform_w) uniform_w = 0.0;
    if (!(uniform_w > 0.0) || uniform_w > 1e300) uniform_w = 0.0;
    SC_HIP(hipSetDevice(c->device));
    sc_graph_drop(c);
    SC_TRY(c->g_indptr.ensure(sizeof(int64_t) * (size_t)(n + 1), &c->mem));
    SC_TRY(c->g_indices.ensure(sizeof(int32_t) * (size_t)(nnz > 0 ? nnz : 1), &c->mem));
    SC_TRY(c->g_data.ensure(sizeof(double) * (size_t)(nnz > 0 ? nnz : 1), &c->mem));
    SC_TRY(c->perm_flag.ensure(sizeof(int), &c->mem));
    SC_HIP(hipMemcpyAsync(c->g_indptr.p, indptr, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, c->stream));
    if (nnz > 0) {
        SC_HIP(hipMemcpyAsync(c->g_indices.p, indices, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice,
                              c->stream));
        SC_HIP(hipMemcpyAsync(c->g_data.p, data, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, c->stream));
    }
    SC_HIP(hipMemsetAsync(c->perm_flag.p, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(k_check_csr, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, c->stream,
                       c->g_indptr.as<long long>(), c->g_indices.as<int32_t>(), n, c->perm_flag.as<int>());
    int flag = 0;
    SC_HIP(hipMemcpyAsync(&flag, c->perm_flag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    SC_REQUIRE(!(flag & 1), SC_ERR_INVALID, "sc_graph_set_csr: column index out of range");
    SC_REQUIRE(!(flag & 2), SC_ERR_INVALID,
               "sc_graph_set_csr: rows must have strictly ascending column indices (sort_indices/sum_duplicates)");
    SC_TRY(sc_graph_capture_order(c, n));
    c->g_n = n;
    c->g_nnz = nnz;
    c->g_uniform_w = uniform_w;
    c->g_deg_max = deg_max;
    c->g_regular = deg_min == deg_max;   // (the lattice form of the Moran statistic needs equal weights AND equal degrees)
    return SC_OK;
}

// rows of the kNN result, re-ordered ascending by column index (as scipy's COO->CSR gives, AC:404)
__global__ __launch_bounds__(256) void k_knn_to_csr(const int32_t *__restrict__ knn, int64_t n, int k, double w,
                                                    long long *__restrict__ indptr, int32_t *__restrict__ indices,
                                                    double *__restrict__ data)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    indptr[i] = i * k;
    if (i == n) return;
    int32_t *row = indices + i * k;
    for (int j = 0; j < k; ++j) {
        int32_t v = knn[i * k + j];
        int m = j;
        while (m > 0 && row[m - 1] > v) { row[m] = row[m - 1]; --m; }
        row[m] = v;
        data[i * k + j] = w;
    }
}

extern "C" int sc_graph_from_knn(sc_ctx *c, double weight)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "null context");
    SC_HIP(hipSetDevice(c->device));
    SC_REQUIRE(c->knn_n > 0, SC_ERR_STATE, "sc_graph_from_knn: no kNN result (call sc_knn_2d first)");
    int64_t n = c->knn_n, nnz = n * c->knn_k;
    sc_graph_drop(c);
    SC_TRY(c->g_indptr.ensure(sizeof(int64_t) * (size_t)(n + 1), &c->mem));
    SC_TRY(c->g_indices.ensure(sizeof(int32_t) * (size_t)nnz, &c->mem));
    SC_TRY(c->g_data.ensure(sizeof(double) * (size_t)nnz, &c->mem));
    hipLaunchKernelGGL(k_knn_to_csr, dim3((unsigned)ceil_div64(n + 1, 256)), dim3(256), 0, c->stream,
                       c->knn_idx.as<int32_t>(), n, c->knn_k, weight, c->g_indptr.as<long long>(),
                       c->g_indices.as<int32_t>(), c->g_data.as<double>());
    SC_HIP(hipGetLastError());
    SC_TRY(sc_graph_capture_order(c, n));
    c->g_n = n;     // (no host wait: consumers are ordered behind these launches on the context's stream)
    c->g_nnz = nnz;
    c->g_uniform_w = (weight > 0.0 && weight < 1e300) ? weight : 0.0;
    c->g_deg_max = c->knn_k;
    c->g_regular = true;
    return SC_OK;
}

extern "C" int sc_graph_shape(sc_ctx *c, int64_t *n, int64_t *nnz)
{
    SC_REQUIRE(c && n && nnz, SC_ERR_INVALID, "null pointer");
    *n = c->g_n;
    *nnz = c->g_nnz;
    return SC_OK;
}

extern "C" int sc_graph_get(sc_ctx *c, int64_t *indptr_out, int32_t *indices_out, double *data_out)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "null context");
    SC_HIP(hipSetDevice(c->device));
    SC_REQUIRE(c->g_n > 0, SC_ERR_STATE, "sc_graph_get: no graph set");
    if (indptr_out)
        SC_HIP(hipMemcpyAsync(indptr_out, c->g_indptr.p, sizeof(int64_t) * (size_t)(c->g_n + 1), hipMemcpyDeviceToHost,
                              c->stream));
    if (indices_out && c->g_nnz)
        SC_HIP(hipMemcpyAsync(indices_out, c->g_indices.p, sizeof(int32_t) * (size_t)c->g_nnz, hipMemcpyDeviceToHost,
                              c->stream));
    if (data_out && c->g_nnz)
        SC_HIP(hipMemcpyAsync(data_out, c->g_data.p, sizeof(double) * (size_t)c->g_nnz, hipMemcpyDeviceToHost,
                              c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}

// ---- transpose (deterministic: counting sort by column, rows then sorted by source row) ----------

__global__ __launch_bounds__(256) void k_col_count(const int32_t *__restrict__ indices, int64_t nnz,
                                                   unsigned long long *__restrict__ cnt)
{
    int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nnz) atomicAdd(&cnt[indices[e]], 1ull);
}

// one thread per source row i (ascending e): slot claimed with an atomic cursor; rows of the
// transpose are sorted afterwards so that the final layout does not depend on the claim order
__global__ __launch_bounds__(256) void k_transpose_fill(const long long *__restrict__ indptr,
                                                        const int32_t *__restrict__ indices,
                                                        const double *__restrict__ data, int64_t n,
                                                        unsigned long long *__restrict__ cursor,
                                                        int32_t *__restrict__ t_indices, double *__restrict__ t_data)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (long long e = indptr[i]; e < indptr[i + 1]; ++e) {
        unsigned long long pos = atomicAdd(&cursor[indices[e]], 1ull);
        t_indices[pos] = (int32_t)i;
        t_data[pos] = data[e];
    }
}

__global__ __launch_bounds__(256) void k_sort_rows(const long long *__restrict__ indptr, int32_t *__restrict__ indices,
                                                   double *__restrict__ data, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long e0 = indptr[i], e1 = indptr[i + 1];
    for (long long a = e0 + 1; a < e1; ++a) {
        int32_t v = indices[a];
        double w = data[a];
        long long b = a;
        while (b > e0 && indices[b - 1] > v) { indices[b] = indices[b - 1]; data[b] = data[b - 1]; --b; }
        indices[b] = v;
        data[b] = w;
    }
}

static int graph_build_transpose(sc_ctx *c, bool wait);

int sc_graph_ensure_transpose(sc_ctx *c)
{
    if (c->gt_valid) {
        // built on the side stream by a moments computation that may still be running: order this stream behind it
        if (c->mom_pending && c->mom_done) SC_HIP(hipStreamWaitEvent(c->stream, c->mom_done, 0));
        return SC_OK;
    }
    return graph_build_transpose(c, true);
}

// the transposed graph, built on c->stream (which the caller may have pointed at the side stream)
static int graph_build_transpose(sc_ctx *c, bool wait)
{
    SC_REQUIRE(c->g_n > 0, SC_ERR_STATE, "no graph set");
    int64_t n = c->g_n, nnz = c->g_nnz;
    SC_TRY(c->gt_indptr.ensure(sizeof(long long) * (size_t)(n + 1), &c->mem));
    SC_TRY(c->gt_cursor.ensure(sizeof(long long) * (size_t)(n + 1), &c->mem));
    SC_TRY(c->gt_indices.ensure(sizeof(int32_t) * (size_t)(nnz > 0 ? nnz : 1), &c->mem));
    SC_TRY(c->gt_data.ensure(sizeof(double) * (size_t)(nnz > 0 ? nnz : 1), &c->mem));
    unsigned long long *cur = c->gt_cursor.as<unsigned long long>();
    SC_HIP(hipMemsetAsync(cur, 0, sizeof(long long) * (size_t)(n + 1), c->stream));
    if (nnz > 0)
        hipLaunchKernelGGL(k_col_count, dim3((unsigned)ceil_div64(nnz, 256)), dim3(256), 0, c->stream,
                           c->g_indices.as<int32_t>(), nnz, cur);
    SC_TRY(sc_exclusive_sum(c, c->gt_tmp, c->stream, (long long *)cur, c->gt_indptr.as<long long>(), n + 1));
    SC_HIP(hipMemcpyAsync(cur, c->gt_indptr.p, sizeof(long long) * (size_t)(n + 1), hipMemcpyDeviceToDevice,
                          c->stream));
    hipLaunchKernelGGL(k_transpose_fill, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, c->stream,
                       c->g_indptr.as<long long>(), c->g_indices.as<int32_t>(), c->g_data.as<double>(), n, cur,
                       c->gt_indices.as<int32_t>(), c->gt_data.as<double>());
    hipLaunchKernelGGL(k_sort_rows, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, c->stream,
                       c->gt_indptr.as<long long>(), c->gt_indices.as<int32_t>(), c->gt_data.as<double>(), n);
    SC_HIP(hipGetLastError());
    if (wait) SC_HIP(hipStreamSynchronize(c->stream));
    c->gt_valid = true;
    return SC_OK;
}

// ---- moments ---------------------------------------------------------------------------------------

#define MOM_ROWS_PER_BLOCK 1024

// per block partials of: s0 (sum w), t2 (sum over W-edges of the (w_ij + w_ji)^2 contributions), s2
__global__ __launch_bounds__(256) void k_moments(const long long *__restrict__ indptr,
                                                 const int32_t *__restrict__ indices,
                                                 const double *__restrict__ data,
                                                 const long long *__restrict__ t_indptr,
                                                 const double *__restrict__ t_data, int64_t n,
                                                 double *__restrict__ partial)
{
    __shared__ double sh[3][256];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    int64_t r0 = (int64_t)blockIdx.x * MOM_ROWS_PER_BLOCK;
    int64_t r1 = r0 + MOM_ROWS_PER_BLOCK < n ? r0 + MOM_ROWS_PER_BLOCK : n;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += 256) {
        double rs = 0.0, cs = 0.0;
        for (long long e = indptr[i]; e < indptr[i + 1]; ++e) {
            int32_t j = indices[e];
            double w = data[e];
            rs += w;
            // look for the reverse edge (j -> i) in row j (ascending columns)
            long long lo = indptr[j], hi = indptr[j + 1];
            double wr = 0.0;
            bool found = false;
            while (lo < hi) {
                long long mid = (lo + hi) >> 1;
                int32_t v = indices[mid];
                if (v < i) lo = mid + 1;
                else if (v > i) hi = mid;
                else { wr = data[mid]; found = true; break; }
            }
            // (i,j) and (j,i) both stored: this edge contributes (w_ij + w_ji)^2 once (the mirror edge
            // contributes the same again when its own row is visited); one-directional: both (i,j)
            // and (j,i) of W + W^T equal w_ij
            a1 += found ? (w + wr) * (w + wr) : 2.0 * w * w;
        }
        for (long long e = t_indptr[i]; e < t_indptr[i + 1]; ++e) cs += t_data[e];
        a0 += rs;
        a2 += (rs + cs) * (rs + cs);
    }
    sh[0][threadIdx.x] = a0; sh[1][threadIdx.x] = a1; sh[2][threadIdx.x] = a2;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int m = 0; m < 3; ++m) sh[m][threadIdx.x] += sh[m][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 3) partial[(int64_t)blockIdx.x * 3 + threadIdx.x] = sh[threadIdx.x][0];
}

// Start the full moments (s0, s1, s2) of the active graph on the SIDE stream, behind everything enqueued on the context
// stream so far, and return without waiting: transpose, reverse-edge search and per-block partials into pinned host
// memory.  The scoring's set-up calls this so that the 6 ms (1M cells x 15) leave its serial prelude; sc_graph_moments
// collects.  Nothing else may replace the graph's arrays before sc_graph_moments_drain.
int sc_graph_moments_begin(sc_ctx *c)
{
    if (c->s0_valid || c->mom_pending) return SC_OK;
    SC_REQUIRE(c->g_n > 0, SC_ERR_STATE, "no graph set");
    const int64_t n = c->g_n;
    const int blocks = (int)ceil_div64(n, MOM_ROWS_PER_BLOCK);
    SC_TRY(c->streams.ensure(SR_MOMENTS));
    if (!c->mom_ready) SC_HIP(hipEventCreateWithFlags(&c->mom_ready, hipEventDisableTiming));
    if (!c->mom_done) SC_HIP(hipEventCreateWithFlags(&c->mom_done, hipEventDisableTiming));
    if (blocks > c->mom_blocks) {
        if (c->mom_host) (void)hipHostFree(c->mom_host);
        c->mom_host = nullptr;
        SC_HIP(hipHostMalloc(reinterpret_cast<void **>(&c->mom_host), sizeof(double) * 3 * (size_t)blocks, hipHostMallocDefault));
        c->mom_blocks = blocks;
    }
    // every allocation the side stream's work needs happens here, on the host, before anything is enqueued
    SC_TRY(c->gt_indptr.ensure(sizeof(long long) * (size_t)(n + 1), &c->mem));
    SC_TRY(c->mom_dev.ensure(sizeof(double) * 3 * (size_t)blocks, &c->mem));
    SC_HIP(hipEventRecord(c->mom_ready, c->stream));
    SC_HIP(hipStreamWaitEvent(c->stream_m, c->mom_ready, 0));
    hipStream_t main_stream = c->stream;
    c->stream = c->stream_m;
    int rc = c->gt_valid ? SC_OK : graph_build_transpose(c, false);
    if (rc == SC_OK) {
        hipLaunchKernelGGL(k_moments, dim3(blocks), dim3(256), 0, c->stream, c->g_indptr.as<long long>(),
                           c->g_indices.as<int32_t>(), c->g_data.as<double>(), c->gt_indptr.as<long long>(),
                           c->gt_data.as<double>(), n, c->mom_dev.as<double>());
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(c->mom_host, c->mom_dev.p, sizeof(double) * 3 * (size_t)blocks, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipEventRecord(c->mom_done, c->stream) != hipSuccess) {
            sc_set_error("graph moments: launch on the side stream failed");
            rc = SC_ERR_HIP;
        }
    }
    c->stream = main_stream;
    if (rc != SC_OK) { (void)hipStreamSynchronize(c->stream_m); return rc; }
    c->mom_pending = true;
    return SC_OK;
}

void sc_graph_moments_drain(sc_ctx *c)
{
    if (!c->mom_pending) return;
    (void)hipEventSynchronize(c->mom_done);
    c->mom_pending = false;
}

static int graph_moments(sc_ctx *c, double *s0, double *s1, double *s2)
{
    SC_REQUIRE(c->g_n > 0, SC_ERR_STATE, "no graph set");
    if (c->s0_valid) {  // a function of the graph alone: computed once per graph (the Moran path asks twice)
        *s0 = c->s0; *s1 = c->s1; *s2 = c->s2;
        return SC_OK;
    }
    SC_TRY(sc_graph_moments_begin(c));
    SC_HIP(hipEventSynchronize(c->mom_done));
    c->mom_pending = false;
    const int blocks = (int)ceil_div64(c->g_n, MOM_ROWS_PER_BLOCK);
    const double *h = c->mom_host;
    double a0 = 0, a1 = 0, a2 = 0;
    for (int b = 0; b < blocks; ++b) { a0 += h[3 * b]; a1 += h[3 * b + 1]; a2 += h[3 * b + 2]; }
    *s0 = a0; *s1 = a1 / 2.0; *s2 = a2;
    c->s0 = a0; c->s1 = a1 / 2.0; c->s2 = a2;
    c->s0_valid = true;
    return SC_OK;
}

extern "C" int sc_graph_moments(sc_ctx *c, double *s0, double *s1, double *s2)
{
    SC_REQUIRE(c && s0 && s1 && s2, SC_ERR_INVALID, "null pointer");
    SC_HIP(hipSetDevice(c->device));
    return graph_moments(c, s0, s1, s2);
}

// s0 alone -- all the scoring needs -- without the transpose and the reverse-edge search of the full moments (4.7 ms of the
// step's serial prelude at bench size): the same per-row sums and the same reduction tree as k_moments' first partial,
// so the value is bit-identical to graph_moments' s0.
__global__ __launch_bounds__(256) void k_weight_sum(const long long *__restrict__ indptr, const double *__restrict__ data,
                                                    int64_t n, double *__restrict__ partial)
{
    __shared__ double sh[256];
    double a0 = 0.0;
    const int64_t r0 = (int64_t)blockIdx.x * MOM_ROWS_PER_BLOCK;
    const int64_t r1 = r0 + MOM_ROWS_PER_BLOCK < n ? r0 + MOM_ROWS_PER_BLOCK : n;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += 256) {
        double rs = 0.0;
        for (long long e = indptr[i]; e < indptr[i + 1]; ++e) rs += data[e];
        a0 += rs;
    }
    sh[threadIdx.x] = a0;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0];
}

int sc_graph_ensure_s0(sc_ctx *c)
{
    if (c->s0_valid || c->s0_only_valid) return SC_OK;
    SC_REQUIRE(c->g_n > 0, SC_ERR_STATE, "no graph set");
    const int64_t n = c->g_n;
    const int blocks = (int)ceil_div64(n, MOM_ROWS_PER_BLOCK);
    SC_TRY(c->red_tmp.ensure(sizeof(double) * 3 * (size_t)blocks, &c->mem));
    hipLaunchKernelGGL(k_weight_sum, dim3(blocks), dim3(256), 0, c->stream, c->g_indptr.as<long long>(), c->g_data.as<double>(), n,
                       c->red_tmp.as<double>());
    SC_HIP(hipGetLastError());
    std::vector<double> h((size_t)blocks);
    SC_HIP(hipMemcpyAsync(h.data(), c->red_tmp.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    double a0 = 0;
    for (int b = 0; b < blocks; ++b) a0 += h[(size_t)b];
    c->s0 = a0;
    c->s0_only_valid = true;
    return SC_OK;
}

// The same sum in two halves for a caller that must not wait (moran_prepare_early): launch + copy of the per-block
// sums into the caller's pinned host array, and the host-side addition once the caller has synchronised.
int sc_graph_weight_sum_blocks(const sc_ctx *c) { return (int)ceil_div64(c->g_n, MOM_ROWS_PER_BLOCK); }

int sc_graph_weight_sum_launch(sc_ctx *c, double *pinned_out)
{
    SC_REQUIRE(c->g_n > 0, SC_ERR_STATE, "no graph set");
    const int64_t n = c->g_n;
    const int blocks = sc_graph_weight_sum_blocks(c);
    SC_TRY(c->s0_tmp.ensure(sizeof(double) * (size_t)blocks, &c->mem));
    hipLaunchKernelGGL(k_weight_sum, dim3(blocks), dim3(256), 0, c->stream, c->g_indptr.as<long long>(), c->g_data.as<double>(), n,
                       c->s0_tmp.as<double>());
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(pinned_out, c->s0_tmp.p, sizeof(double) * (size_t)blocks, hipMemcpyDeviceToHost, c->stream));
    return SC_OK;
}

void sc_graph_weight_sum_collect(sc_ctx *c, const double *partial, int blocks)
{
    double a0 = 0;
    for (int b = 0; b < blocks; ++b) a0 += partial[b];   // (the order of sc_graph_ensure_s0)
    c->s0 = a0;
    c->s0_only_valid = true;
}

// y[i] = sum_e w[e] * x[col[e]]  for one contiguous vector
__global__ __launch_bounds__(256) void k_spmv_vec(const long long *__restrict__ indptr,
                                                  const int32_t *__restrict__ indices, const double *__restrict__ w,
                                                  const double *__restrict__ x, double *__restrict__ y, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (long long e = indptr[i]; e < indptr[i + 1]; ++e) s = __dadd_rn(s, __dmul_rn(w[e], x[indices[e]]));
    y[i] = s;
}

void sc_launch_spmv_vec(sc_ctx *c, const int64_t *indptr, const int32_t *indices, const double *w, const double *x,
                        double *y, int64_t n)
{
    hipLaunchKernelGGL(k_spmv_vec, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, c->stream,
                       (const long long *)indptr, indices, w, x, y, n);
}

// ------------------------------------------------------------------------------------------------
// A9: neighbourhood composition on the active graph's pattern
// ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_profile(const long long *__restrict__ indptr,
                                                 const int32_t *__restrict__ indices,
                                                 const int32_t *__restrict__ labels, int64_t n, int n_types,
                                                 float *__restrict__ counts, unsigned long long *__restrict__ n_empty)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float *row = counts + i * n_types;
    long long e0 = indptr[i], e1 = indptr[i + 1];
    for (long long e = e0; e < e1; ++e) row[labels[indices[e]]] += 1.0f;
    if (e1 == e0) atomicAdd(n_empty, 1ull);
}

extern "C" int sc_profile_counts(sc_ctx *c, const int32_t *labels, int64_t n, int32_t n_types, float *counts_out,
                                 int64_t *n_empty_out)
{
    SC_REQUIRE(c && labels && counts_out, SC_ERR_INVALID, "sc_profile_counts: null pointer");
    SC_HIP(hipSetDevice(c->device));
    SC_REQUIRE(c->g_n > 0, SC_ERR_STATE, "sc_profile_counts: no graph set");
    SC_REQUIRE(n == c->g_n, SC_ERR_INVALID, "sc_profile_counts: %lld labels for a graph of %lld cells", (long long)n,
               (long long)c->g_n);
    SC_REQUIRE(n_types >= 1 && n_types <= 65536, SC_ERR_INVALID, "n_types out of range");
    for (int64_t i = 0; i < n; ++i)
        SC_REQUIRE(labels[i] >= 0 && labels[i] < n_types, SC_ERR_INVALID, "label %d of cell %lld out of range",
                   labels[i], (long long)i);
    size_t cbytes = sizeof(float) * (size_t)n * (size_t)n_types;
    SC_TRY(c->scratch_a.ensure(cbytes, &c->mem));
    SC_TRY(c->scratch_idx.ensure(sizeof(int32_t) * (size_t)n + 16, &c->mem));
    SC_TRY(c->perm_flag.ensure(sizeof(unsigned long long), &c->mem));
    SC_HIP(hipMemcpyAsync(c->scratch_idx.p, labels, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemsetAsync(c->scratch_a.p, 0, cbytes, c->stream));
    SC_HIP(hipMemsetAsync(c->perm_flag.p, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_profile, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, c->stream,
                       c->g_indptr.as<long long>(), c->g_indices.as<int32_t>(), c->scratch_idx.as<int32_t>(), n,
                       (int)n_types, c->scratch_a.as<float>(), c->perm_flag.as<unsigned long long>());
    SC_HIP(hipGetLastError());
    unsigned long long empty = 0;
    SC_HIP(hipMemcpyAsync(counts_out, c->scratch_a.p, cbytes, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipMemcpyAsync(&empty, c->perm_flag.p, sizeof(empty), hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    if (n_empty_out) *n_empty_out = (int64_t)empty;
    if (empty) {
        sc_set_error("%llu cells have empty neighborhood profiles", empty);
        return SC_ERR_EMPTY;
    }
    return SC_OK;
}
