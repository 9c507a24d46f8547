// sc_diffusion.hip -- diffusion maps (Haghverdi et al. 2016) on the neighbour lists the dense search leaves on the device
// (sc_neighbors.hip): the locally scaled Gaussian kernel on the symmetric union of the lists, the density-normalised
// symmetric transition matrix, its connected components, and Lanczos with full reorthogonalisation on it.  DESIGN.md
// 4.6m; restated in the same orders by tests/diffusion_restated.py.  gfx950 only.
//
// fp64 throughout, -ffp-contract=off, no floating-point atomics.  ONE order per sum:
//  - a row of the kernel matrix, of K' and of T x: the stored entries in column order, a running sum from 0;
//  - a dot product over the cells (v . w, w . w): chunks of DF_CHUNK = 1024 cells; inside a chunk element e = r * 64 + lane,
//    a lane adds its 16 products for r ascending starting from the first, the 64 lane sums meet in the adjacent-pair
//    tree (lane l takes lane l ^ 1, then l ^ 2, ...), a short last chunk is padded with zero products; the chunk sums
//    are added in chunk order, a running sum from 0;
//  - w_i - sum_l v_li c_l: one subtraction per l, l ascending;
//  - a Ritz vector sum_j v_ji s_j: j ascending, starting from the j = 0 product.
// None of this depends on the grid.  (A weight's squared distance is the search's: sc_dense_knn.h, df_d2.)
#include <cmath>
#include <vector>

#include "sc_csr_input.h"
#include "sc_dense_knn.h"
#include "sc_unionfind.h"

namespace {

typedef unsigned long long u64;

constexpr int DF_CHUNK = 1024;    // cells per partial of a dot product
constexpr int DF_RITZ_MAX = 64;

static int bits_for(int64_t count)   // bits that hold 0 .. count - 1 (at least 1)
{
    int b = 1;
    while (((int64_t)1 << b) < count) ++b;
    return b;
}

// ---- graph -------------------------------------------------------------------------------------------------------
// s2_i = median of row i's k squared distances (ascending): the middle one, or (a + b) / 2 of the two middle ones
__global__ __launch_bounds__(256) void k_df_scale2(const double *__restrict__ d2, int64_t n, int k, double *__restrict__ s2)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *r = d2 + i * k;
    s2[i] = (k & 1) ? r[k / 2] : (r[k / 2 - 1] + r[k / 2]) / 2.0;
}
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
// cnt[p] = 1 where a sorted key differs from the one before it (cnt[total] = 0 for the scan)
__global__ __launch_bounds__(256) void k_df_first(const u64 *__restrict__ keys, int64_t total, long long *__restrict__ cnt)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > total) return;
    cnt[p] = (p < total && (p == 0 || keys[p] != keys[p - 1])) ? 1 : 0;
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
// w_e = sqrt(2 sqrt(s2_i) sqrt(s2_j) / (s2_i + s2_j)) exp(-d2(i, j) / (s2_i + s2_j)), d2 as the search adds it
__global__ __launch_bounds__(256) void k_df_weights(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                    int64_t n, int64_t nnz, const double *__restrict__ X, int dp,
                                                    const double *__restrict__ s2, double *__restrict__ w)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const int64_t i = df_row_of(indptr, n, e), j = indices[e];
    const double *a = X + i * dp, *b = X + j * dp;
    // df_d2<0>'s terms written out: through the helper one compare-and-branch comes out inverted, and this code is kept as it was
    const double f0 = a[0] - b[0];
    double acc = f0 * f0;
    for (int c = 1; c < dp; ++c) {
        const double f = a[c] - b[c];
        acc = acc + f * f;
    }
    const double si = s2[i], sj = s2[j], den = si + sj;
    const double num = (2.0 * sqrt(si)) * sqrt(sj);
    w[e] = sqrt(num / den) * exp(-acc / den);
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

// ---- Lanczos -----------------------------------------------------------------------------------------------------
// y = T x, a row's entries in column order
__global__ __launch_bounds__(256) void k_df_spmv(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                 const double *__restrict__ T, const double *__restrict__ x, int64_t n,
                                                 double *__restrict__ y)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) s = s + T[e] * x[indices[e]];
    y[i] = s;
}
// part[chunk][l] = the chunk's share of V_l . w for l = 0 .. nvec - 1 (V_l = V + l * n).  One workgroup per chunk keeps its
// 1024 entries of w in registers; wavefront v takes the vectors l = v, v + 4, ...: no LDS, no barrier.
__global__ __launch_bounds__(256) void k_df_dots(const double *__restrict__ V, int64_t nvec, const double *__restrict__ w, int64_t n,
                                                 double *__restrict__ part)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t e0 = (int64_t)blockIdx.x * DF_CHUNK + lane;
    double wr[DF_CHUNK / 64];
#pragma unroll
    for (int r = 0; r < DF_CHUNK / 64; ++r) {
        const int64_t e = e0 + r * 64;
        wr[r] = e < n ? w[e] : 0.0;
    }
    for (int64_t l = wave; l < nvec; l += 4) {
        const double *v = V + l * n;
        double s = (e0 < n ? v[e0] : 0.0) * wr[0];
#pragma unroll
        for (int r = 1; r < DF_CHUNK / 64; ++r) {
            const int64_t e = e0 + r * 64;
            s = s + (e < n ? v[e] : 0.0) * wr[r];
        }
        for (int h = 1; h < 64; h <<= 1) s = s + __shfl_xor(s, h, 64);
        if (lane == 0) part[(int64_t)blockIdx.x * nvec + l] = s;
    }
}
// coef[l] = part[chunk][l] added in chunk order
__global__ __launch_bounds__(256) void k_df_chunk_add(const double *__restrict__ part, int64_t chunks, int64_t nvec,
                                                      double *__restrict__ coef)
{
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= nvec) return;
    double s = 0.0;
    for (int64_t ch = 0; ch < chunks; ++ch) s = s + part[ch * nvec + l];
    coef[l] = s;
}
// w_i <- w_i - V_li coef_l, l ascending
__global__ __launch_bounds__(256) void k_df_update(const double *__restrict__ V, int64_t nvec, const double *__restrict__ coef,
                                                   int64_t n, double *__restrict__ w)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = w[i];
    for (int64_t l = 0; l < nvec; ++l) s = s - V[l * n + i] * coef[l];
    w[i] = s;
}
// out = w / sqrt(*norm2); thread 0 records beta = sqrt(*norm2) and, with both coefficient passes given, alpha = c1 + c2
__global__ __launch_bounds__(256) void k_df_normalise(const double *__restrict__ w, const double *__restrict__ norm2, int64_t n,
                                                      double *__restrict__ out, double *__restrict__ beta_out,
                                                      const double *__restrict__ c1, const double *__restrict__ c2,
                                                      double *__restrict__ alpha_out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const double beta = sqrt(*norm2);
    if (i == 0) {
        if (beta_out) *beta_out = beta;
        if (alpha_out) *alpha_out = *c1 + *c2;
    }
    if (i < n) out[i] = w[i] / beta;
}
// y_i = sum_j V_ji S[j][l], j ascending from the j = 0 product (S is m x c row-major)
__global__ __launch_bounds__(256) void k_df_combine(const double *__restrict__ V, int64_t m, const double *__restrict__ S, int c,
                                                    int l, int64_t n, double *__restrict__ y)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = V[i] * S[l];
    for (int64_t j = 1; j < m; ++j) s = s + V[j * n + i] * S[j * c + l];
    y[i] = s;
}
// r_i <- r_i - lambda y_i
__global__ __launch_bounds__(256) void k_df_residual(const double *__restrict__ y, double lambda, int64_t n, double *__restrict__ r)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) r[i] = r[i] - lambda * y[i];
}

// V_l . w for l < nvec into coef (both on the device): the partials, then their sum
int df_dots(sc_ctx *c, const double *V, int64_t nvec, const double *w, double *coef)
{
    sc_ctx::Diffusion &f = c->df;
    const int64_t chunks = ceil_div64(f.n, DF_CHUNK);
    SC_TRY(f.part.ensure(sizeof(double) * (size_t)(chunks * nvec), &c->mem));
    hipLaunchKernelGGL(k_df_dots, dim3((unsigned)chunks), dim3(256), 0, c->stream, V, nvec, w, f.n, f.part.as<double>());
    hipLaunchKernelGGL(k_df_chunk_add, dim3((unsigned)ceil_div64(nvec, 256)), dim3(256), 0, c->stream, f.part.as<double>(), chunks, nvec,
                       coef);
    return SC_OK;
}

}  // namespace

// the symmetric union of the resident lists as a CSR pattern (rows sorted by column): both directions of every entry as
// keys, one device-wide sort, the first of every run kept.  Leaves indptr / indices on the device; *nnz_out = stored entries.
int df_build_union(sc_ctx *c, long long *nnz_out)
{
    sc_ctx::Diffusion &f = c->df;
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
    SC_TRY((rs_sort<u64, uint32_t>(c, f.keys.as<u64>(), f.keys2.as<u64>(), f.pay.as<uint32_t>(), f.pay2.as<uint32_t>(), total,
                                    32 + bits_for(n))));
    hipLaunchKernelGGL(k_df_first, dim3((unsigned)ceil_div64(total + 1, 256)), tpb, 0, s, f.keys2.as<u64>(), total, f.cnt.as<long long>());
    SC_TRY(sc_counts_to_offsets(c, f.cnt.as<long long>(), f.off.as<long long>(), total, nnz_out));
    hipLaunchKernelGGL(k_df_compact, dim3((unsigned)ceil_div64(total, 256)), tpb, 0, s, f.keys2.as<u64>(), f.cnt.as<long long>(),
                       f.off.as<long long>(), total, f.indices.as<int32_t>());
    hipLaunchKernelGGL(k_df_indptr, dim3((unsigned)ceil_div64(n + 1, 256)), tpb, 0, s, f.keys2.as<u64>(), f.off.as<long long>(), total, n,
                       f.indptr.as<int64_t>());
    return SC_OK;
}

// steps 4 and 6 on the resident CSR (indptr, indices, w): q, D, T and the number of connected components
int df_finish_graph(sc_ctx *c, int64_t *n_components_out)
{
    sc_ctx::Diffusion &f = c->df;
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
    f.graph_valid = true;
    f.lanczos_valid = false;
    return SC_OK;
}

extern "C" int sc_diffmap_graph(sc_ctx *c, double *s2_out, int64_t *n_edges_out, int64_t *n_components_out)
{
    SC_REQUIRE(c && n_edges_out && n_components_out, SC_ERR_INVALID, "sc_diffmap_graph: null pointer");
    sc_ctx::Diffusion &f = c->df;
    const sc_ctx::DenseKnn &kn = c->knn;
    SC_REQUIRE(kn.valid, SC_ERR_STATE, "sc_diffmap_graph: no neighbour lists are resident (call sc_knn_dense first)");
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t n = kn.n, nk = n * kn.k, total = 2 * nk;
    f.graph_valid = f.lanczos_valid = false;
    SC_TRY(f.s2.ensure(sizeof(double) * (size_t)n, &c->mem));
    std::vector<double> s2_host((size_t)n);
    long long nnz = 0;
    const dim3 rows((unsigned)ceil_div64(n, 256)), tpb(256);
    {
        KernelTimerScope ts(c, SC_K_DIFF_GRAPH);
        hipLaunchKernelGGL(k_df_scale2, rows, tpb, 0, s, kn.d2.as<double>(), n, kn.k, f.s2.as<double>());
        SC_TRY(df_build_union(c, &nnz));
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(s2_host.data(), f.s2.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    SC_REQUIRE(nnz >= nk && nnz <= total, SC_ERR_HIP, "sc_diffmap_graph: edge count %lld out of range", nnz);
    for (int64_t i = 0; i < n; ++i)
        SC_REQUIRE(s2_host[(size_t)i] > 0.0, SC_ERR_INVALID,
                   "sc_diffmap_graph: the local scale of cell %lld is zero: more than half of its %d nearest neighbours are exact "
                   "duplicates of it, and the kernel is undefined there (remove the duplicates or use a larger n_neighbors)",
                   (long long)i, kn.k);
    if (s2_out)
        for (int64_t i = 0; i < n; ++i) s2_out[i] = s2_host[(size_t)i];
    f.nnz = nnz;
    SC_TRY(f.w.ensure(sizeof(double) * (size_t)nnz, &c->mem));
    {
        KernelTimerScope ts(c, SC_K_DIFF_GRAPH);
        hipLaunchKernelGGL(k_df_weights, dim3((unsigned)ceil_div64(nnz, 256)), tpb, 0, s, f.indptr.as<int64_t>(), f.indices.as<int32_t>(), n,
                           (int64_t)nnz, kn.X.as<double>(), kn.d, f.s2.as<double>(), f.w.as<double>());
        SC_TRY(df_finish_graph(c, n_components_out));
    }
    *n_edges_out = nnz;
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
    sc_ctx::Diffusion &f = c->df;
    hipStream_t s = c->stream;
    c->knn.valid = f.graph_valid = f.lanczos_valid = false;
    f.n = n;
    f.nnz = nnz;
    SC_TRY(f.indptr.ensure(sizeof(int64_t) * (size_t)(n + 1), &c->mem));
    SC_TRY(f.indices.ensure(sizeof(int32_t) * (size_t)nnz, &c->mem));
    SC_TRY(f.w.ensure(sizeof(double) * (size_t)nnz, &c->mem));
    SC_HIP(hipMemcpyAsync(f.indptr.p, indptr, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(f.indices.p, indices, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(f.w.p, w, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, s));
    KernelTimerScope ts(c, SC_K_DIFF_GRAPH);
    return df_finish_graph(c, n_components_out);
}

extern "C" int sc_diffmap_graph_get(sc_ctx *c, int64_t *indptr, int32_t *indices, double *w, double *T)
{
    SC_REQUIRE(c && indptr && indices && w, SC_ERR_INVALID, "sc_diffmap_graph_get: null pointer");
    sc_ctx::Diffusion &f = c->df;
    SC_REQUIRE(f.graph_valid, SC_ERR_STATE, "sc_diffmap_graph_get: no graph is resident");
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    SC_HIP(hipMemcpyAsync(indptr, f.indptr.p, sizeof(int64_t) * (size_t)(f.n + 1), hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(indices, f.indices.p, sizeof(int32_t) * (size_t)f.nnz, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(w, f.w.p, sizeof(double) * (size_t)f.nnz, hipMemcpyDeviceToHost, s));
    if (T) SC_HIP(hipMemcpyAsync(T, f.T.p, sizeof(double) * (size_t)f.nnz, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}

extern "C" int sc_lanczos_begin(sc_ctx *c, const double *start, int64_t max_basis)
{
    SC_REQUIRE(c && start, SC_ERR_INVALID, "sc_lanczos_begin: null pointer");
    sc_ctx::Diffusion &f = c->df;
    SC_REQUIRE(f.graph_valid, SC_ERR_STATE, "sc_lanczos_begin: no transition matrix is resident (call sc_diffmap_graph first)");
    const int64_t n = f.n;
    SC_REQUIRE(max_basis >= 1 && max_basis <= n, SC_ERR_INVALID, "sc_lanczos_begin: need 1 <= max_basis <= n = %lld, got %lld",
               (long long)n, (long long)max_basis);
    bool nonzero = false;
    for (int64_t i = 0; i < n; ++i) {
        SC_REQUIRE(std::isfinite(start[i]), SC_ERR_INVALID, "sc_lanczos_begin: start value %lld is not finite", (long long)i);
        nonzero |= start[i] != 0.0;
    }
    SC_REQUIRE(nonzero, SC_ERR_INVALID, "sc_lanczos_begin: the start vector is all zero");
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    f.lanczos_valid = false;
    SC_TRY(f.V.ensure(sizeof(double) * (size_t)(max_basis + 1) * (size_t)n, &c->mem));
    SC_TRY(f.wv.ensure(sizeof(double) * (size_t)n, &c->mem));
    SC_TRY(f.coef.ensure(sizeof(double) * (size_t)(2 * (max_basis + 1) + 1), &c->mem));
    SC_TRY(f.ab.ensure(sizeof(double) * (size_t)(2 * max_basis + 1), &c->mem));
    // every later dot product fits: growing a buffer frees it, which would wait for the device in the middle of a run
    SC_TRY(f.part.ensure(sizeof(double) * (size_t)(ceil_div64(n, DF_CHUNK) * (max_basis + 1)), &c->mem));
    SC_HIP(hipMemcpyAsync(f.wv.p, start, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s));
    double *norm2 = f.coef.as<double>() + 2 * (max_basis + 1);
    double *beta = f.ab.as<double>() + max_basis;
    SC_TRY(df_dots(c, f.wv.as<double>(), 1, f.wv.as<double>(), norm2));
    hipLaunchKernelGGL(k_df_normalise, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, s, f.wv.as<double>(), norm2, n, f.V.as<double>(), beta,
                       (const double *)nullptr, (const double *)nullptr, (double *)nullptr);
    SC_HIP(hipGetLastError());
    SC_HIP(hipStreamSynchronize(s));
    f.m = 0;
    f.max_basis = max_basis;
    f.lanczos_valid = true;
    return SC_OK;
}

extern "C" int sc_lanczos_run(sc_ctx *c, int32_t steps, double *alpha_out, double *beta_out, int64_t *m_out)
{
    SC_REQUIRE(c && alpha_out && beta_out && m_out, SC_ERR_INVALID, "sc_lanczos_run: null pointer");
    sc_ctx::Diffusion &f = c->df;
    SC_REQUIRE(f.lanczos_valid, SC_ERR_STATE, "sc_lanczos_run: no Lanczos run is open (call sc_lanczos_begin first)");
    SC_REQUIRE(steps >= 0 && f.m + steps <= f.max_basis, SC_ERR_INVALID,
               "sc_lanczos_run: %d more steps after %lld exceed the basis of %lld", steps, (long long)f.m, (long long)f.max_basis);
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t n = f.n, mb = f.max_basis;
    const dim3 rows((unsigned)ceil_div64(n, 256)), tpb(256);
    double *V = f.V.as<double>(), *w = f.wv.as<double>();
    double *c1 = f.coef.as<double>(), *c2 = c1 + (mb + 1), *norm2 = c1 + 2 * (mb + 1);
    double *alpha = f.ab.as<double>(), *beta = alpha + mb;
    const int64_t m0 = f.m;
    for (int64_t j = m0; j < m0 + steps; ++j) {
        {
            KernelTimerScope ts(c, SC_K_DIFF_SPMV);
            hipLaunchKernelGGL(k_df_spmv, rows, tpb, 0, s, f.indptr.as<int64_t>(), f.indices.as<int32_t>(), f.T.as<double>(), V + j * n, n, w);
        }
        KernelTimerScope ts(c, SC_K_DIFF_ORTH);
        SC_TRY(df_dots(c, V, j + 1, w, c1));
        hipLaunchKernelGGL(k_df_update, rows, tpb, 0, s, V, j + 1, c1, n, w);
        SC_TRY(df_dots(c, V, j + 1, w, c2));
        hipLaunchKernelGGL(k_df_update, rows, tpb, 0, s, V, j + 1, c2, n, w);
        SC_TRY(df_dots(c, w, 1, w, norm2));
        hipLaunchKernelGGL(k_df_normalise, rows, tpb, 0, s, w, norm2, n, V + (j + 1) * n, beta + j + 1, c1 + j, c2 + j, alpha + j);
    }
    SC_HIP(hipGetLastError());
    f.m = m0 + steps;
    SC_HIP(hipMemcpyAsync(alpha_out, alpha, sizeof(double) * (size_t)f.m, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(beta_out, beta, sizeof(double) * (size_t)(f.m + 1), hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    *m_out = f.m;
    // a vanishing norm ends the Krylov sequence; after step n - 1 it must vanish (the basis is complete), which is no error
    const double tiny = (double)n * 2.220446049250313e-16;
    for (int64_t j = m0 + 1; j <= f.m; ++j)
        if (j < n && !(beta_out[j] >= tiny)) {
            f.lanczos_valid = false;
            sc_set_error("sc_lanczos_run: Krylov breakdown at step %lld (beta = %.3e < n 2^-52): the start vector lies in an invariant "
                         "subspace", (long long)j, beta_out[j]);
            return SC_ERR_STATE;
        }
    return SC_OK;
}

extern "C" int sc_lanczos_ritz(sc_ctx *c, const double *S, int64_t m, int32_t cols, const double *lambda, double *vecs_out,
                               double *resid_out)
{
    SC_REQUIRE(c && S && lambda && vecs_out && resid_out, SC_ERR_INVALID, "sc_lanczos_ritz: null pointer");
    sc_ctx::Diffusion &f = c->df;
    SC_REQUIRE(f.lanczos_valid, SC_ERR_STATE, "sc_lanczos_ritz: no Lanczos run is open (call sc_lanczos_begin first)");
    SC_REQUIRE(m >= 1 && m <= f.m, SC_ERR_INVALID, "sc_lanczos_ritz: need 1 <= m <= %lld steps taken, got %lld", (long long)f.m,
               (long long)m);
    SC_REQUIRE(cols >= 1 && cols <= DF_RITZ_MAX, SC_ERR_INVALID, "sc_lanczos_ritz: need 1 <= columns <= %d, got %d", DF_RITZ_MAX, cols);
    for (int64_t p = 0; p < m * cols; ++p)
        SC_REQUIRE(std::isfinite(S[p]), SC_ERR_INVALID, "sc_lanczos_ritz: coefficient %lld is not finite", (long long)p);
    for (int l = 0; l < cols; ++l) SC_REQUIRE(std::isfinite(lambda[l]), SC_ERR_INVALID, "sc_lanczos_ritz: lambda[%d] is not finite", l);
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t n = f.n;
    SC_TRY(f.S.ensure(sizeof(double) * (size_t)(m * cols), &c->mem));
    SC_TRY(f.Y.ensure(sizeof(double) * (size_t)cols * (size_t)n, &c->mem));
    SC_TRY(f.res.ensure(sizeof(double) * (size_t)(cols + 1), &c->mem));
    SC_HIP(hipMemcpyAsync(f.S.p, S, sizeof(double) * (size_t)(m * cols), hipMemcpyHostToDevice, s));
    const dim3 rows((unsigned)ceil_div64(n, 256)), tpb(256);
    double *w = f.wv.as<double>(), *res = f.res.as<double>(), *norm2 = res + cols;
    for (int l = 0; l < cols; ++l) {
        double *y = f.Y.as<double>() + (int64_t)l * n;
        hipLaunchKernelGGL(k_df_combine, rows, tpb, 0, s, f.V.as<double>(), m, f.S.as<double>(), (int)cols, l, n, w);
        SC_TRY(df_dots(c, w, 1, w, norm2));
        hipLaunchKernelGGL(k_df_normalise, rows, tpb, 0, s, w, norm2, n, y, (double *)nullptr, (const double *)nullptr,
                           (const double *)nullptr, (double *)nullptr);
        hipLaunchKernelGGL(k_df_spmv, rows, tpb, 0, s, f.indptr.as<int64_t>(), f.indices.as<int32_t>(), f.T.as<double>(), y, n, w);
        hipLaunchKernelGGL(k_df_residual, rows, tpb, 0, s, y, lambda[l], n, w);
        SC_TRY(df_dots(c, w, 1, w, res + l));
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(vecs_out, f.Y.p, sizeof(double) * (size_t)cols * (size_t)n, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(resid_out, res, sizeof(double) * (size_t)cols, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    for (int l = 0; l < cols; ++l) resid_out[l] = std::sqrt(resid_out[l]);
    return SC_OK;
}

extern "C" int sc_lanczos_end(sc_ctx *c)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "sc_lanczos_end: null context");
    SC_HIP(hipSetDevice(c->device));
    SC_HIP(hipStreamSynchronize(c->stream));
    sc_ctx::Diffusion &f = c->df;
    // the end of a diffusion map gives back its large transients: the basis, and the search's partial lists (knn.pidx / pd2),
    // which nothing reads after the search that filled them and which the next search sizes again
    for (DBuf *b : {&f.V, &f.Y, &f.part, &c->knn.pidx, &c->knn.pd2}) b->release();
    f.lanczos_valid = false;
    return SC_OK;
}
