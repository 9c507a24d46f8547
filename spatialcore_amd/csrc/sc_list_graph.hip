// sc_list_graph.hip -- sc_list_graph.h: the resident weighted graph of diffusion maps, UMAP and Louvain.  The symmetric
// union of the neighbour lists as a CSR pattern, a caller's CSR, the finish (row sums, density, the density-normalised
// symmetric transition matrix of Haghverdi et al. 2016, connected components), the copy-out, and the validity rule.
// DESIGN.md 4.6u; restated by tests/diffusion_restated.py.  gfx950 only.
//
// fp64, -ffp-contract=off, no floating-point atomics: a row's sum takes the stored entries in column order, a running sum
// from 0.  None of this depends on the grid.
#include <cmath>

#include "sc_csr_input.h"
#include "sc_list_graph.h"
#include "sc_sortscan.h"
#include "sc_unionfind.h"

namespace {

typedef unsigned long long u64;

// both directions of every list entry as (row << 32 | column)
__global__ __launch_bounds__(256) void k_df_keys(const int32_t *__restrict__ idx, int64_t nk, int k, u64 *__restrict__ keys,
                                                 uint32_t *__restrict__ pay)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nk) return;
    const u64 i = (u64)(p / k), j = (u64)(uint32_t)idx[p];
    keys[2 * p] = (i << 32) | j;
    keys[2 * p + 1] = (j << 32) | i;
    pay[2 * p] = 0u;
    pay[2 * p + 1] = 0u;
}
__global__ __launch_bounds__(256) void k_df_compact(const u64 *__restrict__ keys, const long long *__restrict__ cnt,
                                                    const long long *__restrict__ off, int64_t total, int32_t *__restrict__ indices)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total || !cnt[p]) return;
    indices[off[p]] = (int32_t)(uint32_t)(keys[p] & 0xffffffffull);
}
// indptr[i] = entries before the first sorted key of row >= i, i = 0 .. n
__global__ __launch_bounds__(256) void k_df_indptr(const u64 *__restrict__ keys, const long long *__restrict__ off, int64_t total,
                                                   int64_t n, int64_t *__restrict__ indptr)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    const u64 want = (u64)i << 32;
    int64_t lo = 0, hi = total;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < want) lo = mid + 1; else hi = mid;
    }
    indptr[i] = off[lo];
}
// q_i = sum_j w_ij
__global__ __launch_bounds__(256) void k_df_rowsum(const int64_t *__restrict__ indptr, const double *__restrict__ w, int64_t n,
                                                   double *__restrict__ q)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) s = s + w[e];
    q[i] = s;
}
// D_i = sum_j w_ij / (q_i q_j)
__global__ __launch_bounds__(256) void k_df_density(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                    const double *__restrict__ w, const double *__restrict__ q, int64_t n,
                                                    double *__restrict__ D)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double qi = q[i];
    double s = 0.0;
    for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) s = s + w[e] / (qi * q[indices[e]]);
    D[i] = s;
}
// T_e = (w_e / (q_i q_j)) / (sqrt(D_i) sqrt(D_j)); the same launch hooks the edge's ends together
__global__ __launch_bounds__(256) void k_df_transition(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                       const double *__restrict__ w, const double *__restrict__ q,
                                                       const double *__restrict__ D, int64_t n, int64_t nnz,
                                                       double *__restrict__ T, int32_t *__restrict__ parent)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const int64_t i = df_row_of(indptr, n, e), j = indices[e];
    T[e] = (w[e] / (q[i] * q[j])) / (sqrt(D[i]) * sqrt(D[j]));
    if (j < i) uf_union(parent, (int32_t)i, (int32_t)j);
}
__global__ __launch_bounds__(256) void k_df_parent_init(int32_t *__restrict__ parent, int64_t n, int32_t *__restrict__ roots)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) *roots = 0;
    if (i < n) parent[i] = (int32_t)i;
}
__global__ __launch_bounds__(256) void k_df_count_roots(const int32_t *__restrict__ parent, int64_t n, int32_t *__restrict__ roots)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && parent[i] == (int32_t)i) atomicAdd(roots, 1);   // an integer count: the same whatever the order
}

}  // namespace

void lg_invalidate(sc_ctx *c, bool lists_too)
{
    c->lg.valid = c->lz.valid = false;
    if (lists_too) c->knn.valid = false;
}
void lg_mark_finished(sc_ctx *c)
{
    c->lg.valid = true;
    c->lz.valid = false;
}
void lz_open(sc_ctx *c) { c->lz.valid = true; }
void lz_close(sc_ctx *c) { c->lz.valid = false; }

int lg_resident(const sc_ctx *c, const char *who, const char *hint, const sc_ctx::ListGraph **g)
{
    SC_REQUIRE(c->lg.valid, SC_ERR_STATE, "%s: no graph is resident%s", who, hint);
    *g = &c->lg;
    return SC_OK;
}

int lg_build_union(sc_ctx *c, long long *nnz_out)
{
    sc_ctx::ListGraph &f = c->lg;
    const sc_ctx::DenseKnn &kn = c->knn;
    hipStream_t s = c->stream;
    const int64_t n = f.n = kn.n, nk = n * kn.k, total = 2 * nk;
    SC_TRY(f.keys.ensure(sizeof(u64) * (size_t)total, &c->mem));
    SC_TRY(f.keys2.ensure(sizeof(u64) * (size_t)total, &c->mem));
    SC_TRY(f.pay.ensure(sizeof(uint32_t) * (size_t)total, &c->mem));
    SC_TRY(f.pay2.ensure(sizeof(uint32_t) * (size_t)total, &c->mem));
    SC_TRY(f.cnt.ensure(sizeof(long long) * (size_t)(total + 1), &c->mem));
    SC_TRY(f.off.ensure(sizeof(long long) * (size_t)(total + 1), &c->mem));
    SC_TRY(f.indptr.ensure(sizeof(int64_t) * (size_t)(n + 1), &c->mem));
    SC_TRY(f.indices.ensure(sizeof(int32_t) * (size_t)total, &c->mem));
    const dim3 tpb(256);
    hipLaunchKernelGGL(k_df_keys, dim3((unsigned)ceil_div64(nk, 256)), tpb, 0, s, kn.idx.as<int32_t>(), nk, kn.k, f.keys.as<u64>(),
                       f.pay.as<uint32_t>());
    SC_TRY(sc_sort_pairs(c, c->rs_tmp, s, f.keys.as<u64>(), f.keys2.as<u64>(), f.pay.as<uint32_t>(), f.pay2.as<uint32_t>(), total,
                         32 + sc_bits_for(n)));
    sc_run_heads(s, f.keys2.as<u64>(), total, f.cnt.as<long long>());
    SC_TRY(sc_counts_to_offsets(c, f.cnt.as<long long>(), f.off.as<long long>(), total, nnz_out));
    hipLaunchKernelGGL(k_df_compact, dim3((unsigned)ceil_div64(total, 256)), tpb, 0, s, f.keys2.as<u64>(), f.cnt.as<long long>(),
                       f.off.as<long long>(), total, f.indices.as<int32_t>());
    hipLaunchKernelGGL(k_df_indptr, dim3((unsigned)ceil_div64(n + 1, 256)), tpb, 0, s, f.keys2.as<u64>(), f.off.as<long long>(), total, n,
                       f.indptr.as<int64_t>());
    return SC_OK;
}

int lg_finish(sc_ctx *c, int64_t *n_components_out)
{
    sc_ctx::ListGraph &f = c->lg;
    const int64_t n = f.n, nnz = f.nnz;
    hipStream_t s = c->stream;
    SC_TRY(f.q.ensure(sizeof(double) * 2 * (size_t)n, &c->mem));
    SC_TRY(f.T.ensure(sizeof(double) * (size_t)nnz, &c->mem));
    SC_TRY(f.parent.ensure(sizeof(int32_t) * (size_t)n, &c->mem));
    SC_TRY(f.flag.ensure(sizeof(int32_t), &c->mem));
    const dim3 rows((unsigned)ceil_div64(n, 256)), entries((unsigned)ceil_div64(nnz, 256)), tpb(256);
    double *q = f.q.as<double>(), *D = q + n;
    const int64_t *indptr = f.indptr.as<int64_t>();
    const int32_t *indices = f.indices.as<int32_t>();
    hipLaunchKernelGGL(k_df_parent_init, rows, tpb, 0, s, f.parent.as<int32_t>(), n, f.flag.as<int32_t>());
    hipLaunchKernelGGL(k_df_rowsum, rows, tpb, 0, s, indptr, f.w.as<double>(), n, q);
    hipLaunchKernelGGL(k_df_density, rows, tpb, 0, s, indptr, indices, f.w.as<double>(), q, n, D);
    hipLaunchKernelGGL(k_df_transition, entries, tpb, 0, s, indptr, indices, f.w.as<double>(), q, D, n, nnz, f.T.as<double>(),
                       f.parent.as<int32_t>());
    hipLaunchKernelGGL(k_df_count_roots, rows, tpb, 0, s, f.parent.as<int32_t>(), n, f.flag.as<int32_t>());
    SC_HIP(hipGetLastError());
    int32_t roots = 0;
    SC_HIP(hipMemcpyAsync(&roots, f.flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    *n_components_out = roots;
    lg_mark_finished(c);
    return SC_OK;
}

extern "C" int sc_diffmap_graph_csr(sc_ctx *c, const int64_t *indptr, const int32_t *indices, const double *w, int64_t n,
                                    int64_t *n_components_out)
{
    SC_REQUIRE(c && indptr && indices && w && n_components_out, SC_ERR_INVALID, "sc_diffmap_graph_csr: null pointer");
    SC_REQUIRE(n >= 2 && n <= INT32_MAX, SC_ERR_INVALID, "sc_diffmap_graph_csr: need 2 <= n <= 2^31 - 1, got %lld", (long long)n);
    SC_REQUIRE(indptr[0] == 0, SC_ERR_INVALID, "sc_diffmap_graph_csr: indptr[0] must be 0");
    for (int64_t i = 0; i < n; ++i)
        SC_REQUIRE(indptr[i + 1] > indptr[i], SC_ERR_INVALID, "sc_diffmap_graph_csr: row %lld is empty (every cell needs a neighbour)",
                   (long long)i);
    const int64_t nnz = indptr[n];
    SC_REQUIRE(nnz <= ((int64_t)1 << 32), SC_ERR_INVALID, "sc_diffmap_graph_csr: at most 2^32 stored entries, got %lld", (long long)nnz);
    SC_TRY(csr_check_columns("sc_diffmap_graph_csr", indptr, indices, n, n, "n", [&](int64_t, int64_t p) -> int {
        SC_REQUIRE(std::isfinite(w[p]) && w[p] > 0.0, SC_ERR_INVALID, "sc_diffmap_graph_csr: stored value %lld must be finite and > 0",
                   (long long)p);
        return SC_OK;
    }));
    SC_HIP(hipSetDevice(c->device));
    sc_ctx::ListGraph &f = c->lg;
    hipStream_t s = c->stream;
    lg_invalidate(c, true);
    f.n = n;
    f.nnz = nnz;
    SC_TRY(f.indptr.ensure(sizeof(int64_t) * (size_t)(n + 1), &c->mem));
    SC_TRY(f.indices.ensure(sizeof(int32_t) * (size_t)nnz, &c->mem));
    SC_TRY(f.w.ensure(sizeof(double) * (size_t)nnz, &c->mem));
    SC_HIP(hipMemcpyAsync(f.indptr.p, indptr, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(f.indices.p, indices, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(f.w.p, w, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, s));
    KernelTimerScope ts(c, SC_K_DIFF_GRAPH);
    return lg_finish(c, n_components_out);
}

extern "C" int sc_diffmap_graph_get(sc_ctx *c, int64_t *indptr, int32_t *indices, double *w, double *T)
{
    SC_REQUIRE(c && indptr && indices && w, SC_ERR_INVALID, "sc_diffmap_graph_get: null pointer");
    const sc_ctx::ListGraph *f = nullptr;
    SC_TRY(lg_resident(c, "sc_diffmap_graph_get", "", &f));
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    SC_HIP(hipMemcpyAsync(indptr, f->indptr.p, sizeof(int64_t) * (size_t)(f->n + 1), hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(indices, f->indices.p, sizeof(int32_t) * (size_t)f->nnz, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(w, f->w.p, sizeof(double) * (size_t)f->nnz, hipMemcpyDeviceToHost, s));
    if (T) SC_HIP(hipMemcpyAsync(T, f->T.p, sizeof(double) * (size_t)f->nnz, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}
