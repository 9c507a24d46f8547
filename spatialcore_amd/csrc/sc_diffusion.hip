// sc_diffusion.hip -- diffusion maps (Haghverdi et al. 2016) on the neighbour lists the dense search leaves on the device
// (sc_neighbors.hip): the locally scaled Gaussian kernel on the symmetric union of the lists, and Lanczos with full
// reorthogonalisation on the transition matrix of the resident graph (sc_list_graph.h: the union, the density-normalised
// symmetric transition matrix, its connected components).  DESIGN.md 4.6m; restated in the same orders by
// tests/diffusion_restated.py.  gfx950 only.
//
// fp64 throughout, -ffp-contract=off, no floating-point atomics.  ONE order per sum:
//  - a row of the kernel matrix, of K' and of T x: the stored entries in column order, a running sum from 0;
//  - a dot product over the cells (v . w, w . w): the chunked order of sc_chunk_sum.h, the chunk sums added in chunk order;
//  - w_i - sum_l v_li c_l: one subtraction per l, l ascending;
//  - a Ritz vector sum_j v_ji s_j: j ascending, starting from the j = 0 product.
// None of this depends on the grid.  (A weight's squared distance is the search's: sc_dense_knn.h, df_d2.)
#include <cmath>
#include <vector>

#include "sc_chunk_sum.h"
#include "sc_dense_knn.h"
#include "sc_list_graph.h"

namespace {

typedef unsigned long long u64;

constexpr int DF_RITZ_MAX = 64;

// ---- graph -------------------------------------------------------------------------------------------------------
// s2_i = median of row i's k squared distances (ascending): the middle one, or (a + b) / 2 of the two middle ones
__global__ __launch_bounds__(256) void k_df_scale2(const double *__restrict__ d2, int64_t n, int k, double *__restrict__ s2)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *r = d2 + i * k;
    s2[i] = (k & 1) ? r[k / 2] : (r[k / 2 - 1] + r[k / 2]) / 2.0;
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
    const int64_t e0 = (int64_t)blockIdx.x * SUM_CHUNK + lane;
    double wr[SUM_CHUNK / 64];
#pragma unroll
    for (int r = 0; r < SUM_CHUNK / 64; ++r) {
        const int64_t e = e0 + r * 64;
        wr[r] = e < n ? w[e] : 0.0;
    }
    for (int64_t l = wave; l < nvec; l += 4) {
        const double *v = V + l * n;
        double s = (e0 < n ? v[e0] : 0.0) * wr[0];
#pragma unroll
        for (int r = 1; r < SUM_CHUNK / 64; ++r) {
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
    sc_ctx::Lanczos &f = c->lz;
    const int64_t n = c->lg.n;
    const int64_t chunks = ceil_div64(n, SUM_CHUNK);
    SC_TRY(f.part.ensure(sizeof(double) * (size_t)(chunks * nvec), &c->mem));
    hipLaunchKernelGGL(k_df_dots, dim3((unsigned)chunks), dim3(256), 0, c->stream, V, nvec, w, n, f.part.as<double>());
    hipLaunchKernelGGL(k_df_chunk_add, dim3((unsigned)ceil_div64(nvec, 256)), dim3(256), 0, c->stream, f.part.as<double>(), chunks, nvec,
                       coef);
    return SC_OK;
}

}  // namespace

extern "C" int sc_diffmap_graph(sc_ctx *c, double *s2_out, int64_t *n_edges_out, int64_t *n_components_out)
{
    SC_REQUIRE(c && n_edges_out && n_components_out, SC_ERR_INVALID, "sc_diffmap_graph: null pointer");
    sc_ctx::Lanczos &f = c->lz;
    sc_ctx::ListGraph &g = c->lg;
    const sc_ctx::DenseKnn &kn = c->knn;
    SC_REQUIRE(kn.valid, SC_ERR_STATE, "sc_diffmap_graph: no neighbour lists are resident (call sc_knn_dense first)");
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t n = kn.n, nk = n * kn.k, total = 2 * nk;
    lg_invalidate(c, false);
    SC_TRY(f.s2.ensure(sizeof(double) * (size_t)n, &c->mem));
    std::vector<double> s2_host((size_t)n);
    long long nnz = 0;
    const dim3 rows((unsigned)ceil_div64(n, 256)), tpb(256);
    {
        KernelTimerScope ts(c, SC_K_DIFF_GRAPH);
        hipLaunchKernelGGL(k_df_scale2, rows, tpb, 0, s, kn.d2.as<double>(), n, kn.k, f.s2.as<double>());
        SC_TRY(lg_build_union(c, &nnz));
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
    g.nnz = nnz;
    SC_TRY(g.w.ensure(sizeof(double) * (size_t)nnz, &c->mem));
    {
        KernelTimerScope ts(c, SC_K_DIFF_GRAPH);
        hipLaunchKernelGGL(k_df_weights, dim3((unsigned)ceil_div64(nnz, 256)), tpb, 0, s, g.indptr.as<int64_t>(), g.indices.as<int32_t>(), n,
                           (int64_t)nnz, kn.X.as<double>(), kn.d, f.s2.as<double>(), g.w.as<double>());
        SC_TRY(lg_finish(c, n_components_out));
    }
    *n_edges_out = nnz;
    return SC_OK;
}

extern "C" int sc_lanczos_begin(sc_ctx *c, const double *start, int64_t max_basis)
{
    SC_REQUIRE(c && start, SC_ERR_INVALID, "sc_lanczos_begin: null pointer");
    sc_ctx::Lanczos &f = c->lz;
    SC_REQUIRE(c->lg.valid, SC_ERR_STATE, "sc_lanczos_begin: no transition matrix is resident (call sc_diffmap_graph first)");
    const int64_t n = c->lg.n;
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
    lz_close(c);
    SC_TRY(f.V.ensure(sizeof(double) * (size_t)(max_basis + 1) * (size_t)n, &c->mem));
    SC_TRY(f.wv.ensure(sizeof(double) * (size_t)n, &c->mem));
    SC_TRY(f.coef.ensure(sizeof(double) * (size_t)(2 * (max_basis + 1) + 1), &c->mem));
    SC_TRY(f.ab.ensure(sizeof(double) * (size_t)(2 * max_basis + 1), &c->mem));
    // every later dot product fits: growing a buffer frees it, which would wait for the device in the middle of a run
    SC_TRY(f.part.ensure(sizeof(double) * (size_t)(ceil_div64(n, SUM_CHUNK) * (max_basis + 1)), &c->mem));
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
    lz_open(c);
    return SC_OK;
}

extern "C" int sc_lanczos_run(sc_ctx *c, int32_t steps, double *alpha_out, double *beta_out, int64_t *m_out)
{
    SC_REQUIRE(c && alpha_out && beta_out && m_out, SC_ERR_INVALID, "sc_lanczos_run: null pointer");
    sc_ctx::Lanczos &f = c->lz;
    const sc_ctx::ListGraph &g = c->lg;
    SC_REQUIRE(f.valid, SC_ERR_STATE, "sc_lanczos_run: no Lanczos run is open (call sc_lanczos_begin first)");
    SC_REQUIRE(steps >= 0 && f.m + steps <= f.max_basis, SC_ERR_INVALID,
               "sc_lanczos_run: %d more steps after %lld exceed the basis of %lld", steps, (long long)f.m, (long long)f.max_basis);
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t n = g.n, mb = f.max_basis;
    const dim3 rows((unsigned)ceil_div64(n, 256)), tpb(256);
    double *V = f.V.as<double>(), *w = f.wv.as<double>();
    double *c1 = f.coef.as<double>(), *c2 = c1 + (mb + 1), *norm2 = c1 + 2 * (mb + 1);
    double *alpha = f.ab.as<double>(), *beta = alpha + mb;
    const int64_t m0 = f.m;
    for (int64_t j = m0; j < m0 + steps; ++j) {
        {
            KernelTimerScope ts(c, SC_K_DIFF_SPMV);
            hipLaunchKernelGGL(k_df_spmv, rows, tpb, 0, s, g.indptr.as<int64_t>(), g.indices.as<int32_t>(), g.T.as<double>(), V + j * n, n, w);
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
            lz_close(c);
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
    sc_ctx::Lanczos &f = c->lz;
    const sc_ctx::ListGraph &g = c->lg;
    SC_REQUIRE(f.valid, SC_ERR_STATE, "sc_lanczos_ritz: no Lanczos run is open (call sc_lanczos_begin first)");
    SC_REQUIRE(m >= 1 && m <= f.m, SC_ERR_INVALID, "sc_lanczos_ritz: need 1 <= m <= %lld steps taken, got %lld", (long long)f.m,
               (long long)m);
    SC_REQUIRE(cols >= 1 && cols <= DF_RITZ_MAX, SC_ERR_INVALID, "sc_lanczos_ritz: need 1 <= columns <= %d, got %d", DF_RITZ_MAX, cols);
    for (int64_t p = 0; p < m * cols; ++p)
        SC_REQUIRE(std::isfinite(S[p]), SC_ERR_INVALID, "sc_lanczos_ritz: coefficient %lld is not finite", (long long)p);
    for (int l = 0; l < cols; ++l) SC_REQUIRE(std::isfinite(lambda[l]), SC_ERR_INVALID, "sc_lanczos_ritz: lambda[%d] is not finite", l);
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t n = g.n;
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
        hipLaunchKernelGGL(k_df_spmv, rows, tpb, 0, s, g.indptr.as<int64_t>(), g.indices.as<int32_t>(), g.T.as<double>(), y, n, w);
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
    sc_ctx::Lanczos &f = c->lz;
    // the end of a diffusion map gives back its large transients: the basis, and the search's partial lists (knn.pidx / pd2),
    // which nothing reads after the search that filled them and which the next search sizes again
    for (DBuf *b : {&f.V, &f.Y, &f.part, &c->knn.pidx, &c->knn.pd2}) b->release();
    lz_close(c);
    return SC_OK;
}
