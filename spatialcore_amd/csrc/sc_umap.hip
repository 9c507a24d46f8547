// sc_umap.hip -- UMAP's fuzzy simplicial set (McInnes, Healy, Melville 2018: smooth_knn_dist, compute_membership_strengths
// and the probabilistic union, restated from the published algorithm) on the neighbour lists sc_knn_dense* leave on the
// device, and a deterministic layout of any symmetric weighted graph in 2 or 3 dimensions.  DESIGN.md 4.6r; the exact
// definitions are in include/spatialcore_hip.h and are restated in the same orders by tests/umap_restated.py.  gfx950 only.
//
// fp64 throughout, -ffp-contract=off, no floating-point atomics.  ONE order per sum:
//  - a row's distance sum and a row's membership sum: the k list entries in list order, a running sum from 0;
//  - the sum of all distances: the n row sums in the chunked order of sc_chunk_sum.h, the chunk sums added in chunk order;
//  - a squared distance of the layout: the C coordinates in order, from the first product;
//  - a vertex's position: its stored entries in CSR order, per firing entry the attraction, then the negatives q ascending.
// The layout reads the positions of the previous epoch only, so no result depends on the grid or on the hardware queues.
#include <cmath>
#include <vector>

#include "sc_chunk_sum.h"
#include "sc_csr_input.h"
#include "sc_list_graph.h"
#include "sc_philox.h"
#include "sc_umap.h"

namespace {

typedef unsigned long long u64;

constexpr int UM_ITERS = 64;       // umap's bisection limit
constexpr int UM_NEG_MAX = 16;

// ---- fuzzy simplicial set ------------------------------------------------------------------------------------------
// rho_i = the smallest non-zero distance of row i (0 if there is none); dsum_i = sum_j d_ij, list order, from 0
__global__ __launch_bounds__(256) void k_um_rho(const double *__restrict__ d2, int64_t n, int k, double *__restrict__ rho,
                                                double *__restrict__ dsum)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *r = d2 + i * k;
    double lo = 0.0, s = 0.0;
    for (int j = 0; j < k; ++j) {
        const double d = sqrt(r[j]);
        s = s + d;
        if (d > 0.0 && (lo == 0.0 || d < lo)) lo = d;
    }
    rho[i] = lo;
    dsum[i] = s;
}
// part[chunk] = the chunk's share of sum_i v_i: one wavefront per chunk, in the order of sc_chunk_sum.h
__global__ __launch_bounds__(64) void k_um_chunk_sum(const double *__restrict__ v, int64_t n, double *__restrict__ part)
{
    const int lane = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * SUM_CHUNK + lane;
    double s = e0 < n ? v[e0] : 0.0;
    for (int r = 1; r < SUM_CHUNK / 64; ++r) {
        const int64_t e = e0 + r * 64;
        s = s + (e < n ? v[e] : 0.0);
    }
    for (int h = 1; h < 64; h <<= 1) s = s + __shfl_xor(s, h, 64);
    if (lane == 0) part[blockIdx.x] = s;
}
// *mean = (the chunk sums added in chunk order from 0) / count
__global__ void k_um_mean(const double *__restrict__ part, int64_t chunks, double count, double *__restrict__ mean)
{
    double s = 0.0;
    for (int64_t ch = 0; ch < chunks; ++ch) s = s + part[ch];
    *mean = s / count;
}
// p(d2) of one list entry under (rho, sigma): the ONE function both directions of an edge go through
__device__ __forceinline__ double um_member(double d2, double rho, double sigma)
{
    const double t = sqrt(d2) - rho;
    return t > 0.0 ? exp(-(t / sigma)) : 1.0;
}
// sigma_i by umap's bisection, then umap's floor.  One thread per row, its K >= k distances in registers.
template <int K>
__global__ __launch_bounds__(256) void k_um_sigma(const double *__restrict__ d2, int64_t n, int k, double target,
                                                  const double *__restrict__ rho, const double *__restrict__ dsum,
                                                  const double *__restrict__ mean_all, double *__restrict__ sigma)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double t[K];
    const double rh = rho[i];
#pragma unroll
    for (int j = 0; j < K; ++j) t[j] = j < k ? sqrt(d2[i * k + j]) - rh : 0.0;
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    for (int it = 0; it < UM_ITERS; ++it) {
        double psum = 0.0;
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (j < k) psum = psum + (t[j] > 0.0 ? exp(-(t[j] / mid)) : 1.0);
        if (fabs(psum - target) < 1e-5) break;
        if (psum > target) {
            hi = mid;
            mid = (lo + hi) / 2.0;
        } else {
            lo = mid;
            if (hi == INFINITY) mid = mid * 2.0;
            else mid = (lo + hi) / 2.0;
        }
    }
    const double mean = rh > 0.0 ? dsum[i] / (double)(k + 1) : *mean_all;
    const double floor_ = 1e-3 * mean;
    sigma[i] = mid < floor_ ? floor_ : mid;
}
// p of j in row i's list (0 if j is not in it)
__device__ __forceinline__ double um_directed(const int32_t *__restrict__ idx, const double *__restrict__ d2, int k, int64_t i,
                                              int32_t j, const double *__restrict__ rho, const double *__restrict__ sigma)
{
    const int32_t *li = idx + i * k;
    for (int p = 0; p < k; ++p)
        if (li[p] == j) return um_member(d2[i * k + p], rho[i], sigma[i]);
    return 0.0;
}
// w_e = (p_ij + p_ji) - p_ij p_ji
__global__ __launch_bounds__(256) void k_um_weights(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                    int64_t n, int64_t nnz, const int32_t *__restrict__ idx,
                                                    const double *__restrict__ d2, int k, const double *__restrict__ rho,
                                                    const double *__restrict__ sigma, double *__restrict__ w)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const int64_t i = df_row_of(indptr, n, e);
    const int32_t j = indices[e];
    const double pij = um_directed(idx, d2, k, i, j, rho, sigma);
    const double pji = um_directed(idx, d2, k, (int64_t)j, (int32_t)i, rho, sigma);
    w[e] = (pij + pji) - pij * pji;
}

// ---- layout ----------------------------------------------------------------------------------------------------------
// the bits of max_t w_t: positive doubles order as their bit patterns, so the integer maximum is the exact one
__global__ __launch_bounds__(256) void k_um_wmax(const double *__restrict__ w, int64_t nnz, u64 *__restrict__ bits)
{
    u64 m = 0;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nnz; t += (int64_t)gridDim.x * blockDim.x) {
        const u64 b = (u64)__double_as_longlong(w[t]);
        m = b > m ? b : m;
    }
    for (int h = 1; h < 64; h <<= 1) {
        const u64 o = (u64)__shfl_xor((long long)m, h, 64);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(bits, m);
}

struct UmCoef {
    double a, b, m2ab, g2b, alpha;   // m2ab = (-2 a) b, g2b = (2 gamma) b
};

// one interaction of `cur` with the old position y
template <int C, bool ATTRACT>
__device__ __forceinline__ void um_step(double (&cur)[C], const double (&y)[C], const UmCoef &k)
{
    double dlt[C];
#pragma unroll
    for (int c = 0; c < C; ++c) dlt[c] = cur[c] - y[c];
    double dd = dlt[0] * dlt[0];
#pragma unroll
    for (int c = 1; c < C; ++c) dd = dd + dlt[c] * dlt[c];
    if (dd > 0.0) {
        const double pb = pow(dd, k.b);
        const double den = k.a * pb + 1.0;
        const double coef = ATTRACT ? (k.m2ab * (pb / dd)) / den : k.g2b / ((0.001 + dd) * den);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            double g = coef * dlt[c];
            g = g > 4.0 ? 4.0 : (g < -4.0 ? -4.0 : g);
            cur[c] = cur[c] + k.alpha * g;
        }
    }
}

// Epoch e: one thread per vertex walks its row in stored order, reading the old positions only.  Rows are taken in index
// order: launching them by descending length was measured and bought nothing.  Per firing entry the
// gather addresses (the neighbour and the negatives, four per Philox call) do not depend on `cur`: the loads of a block
// of four negatives are issued before the arithmetic that precedes their use.
template <int C>
__global__ __launch_bounds__(256) void k_um_epoch(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                  const double *__restrict__ w, int64_t n, const double *__restrict__ Yold,
                                                  double *__restrict__ Ynew, const u64 *__restrict__ wmax_bits, UmCoef k, int neg,
                                                  uint32_t k0, uint32_t k1, uint32_t e)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double wmax = __longlong_as_double((long long)*wmax_bits);
    double cur[C];
#pragma unroll
    for (int c = 0; c < C; ++c) cur[c] = Yold[i * C + c];
    const int64_t t1 = indptr[i + 1];
    for (int64_t t = indptr[i]; t < t1; ++t) {
        if (!um_fires(w[t], wmax, e)) continue;
        double yj[C];
        const int64_t j = indices[t];
#pragma unroll
        for (int c = 0; c < C; ++c) yj[c] = Yold[j * C + c];
        for (int q0 = 0;; q0 += 4) {
            uint32_t s[4] = {0u, 0u, 0u, 0u};
            double ys[4][C];
            if (q0 < neg) {
                uint32_t o[4] = {(uint32_t)t, (uint32_t)((u64)t >> 32), e, (uint32_t)(q0 >> 2)};
                philox4x32_10(o, k0, k1);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    s[u] = (uint32_t)(((uint64_t)o[u] * (uint64_t)n) >> 32);   // < n
#pragma unroll
                    for (int c = 0; c < C; ++c) ys[u][c] = Yold[(int64_t)s[u] * C + c];
                }
            }
            if (q0 == 0) um_step<C, true>(cur, yj, k);
            if (q0 < neg) {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (q0 + u < neg && (int64_t)s[u] != i) um_step<C, false>(cur, ys[u], k);
            }
            if (q0 + 4 >= neg) break;
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) Ynew[i * C + c] = cur[c];
}

}  // namespace

extern "C" int sc_fuzzy_graph(sc_ctx *c, double *rho_out, double *sigma_out, int64_t *n_edges_out, int64_t *n_components_out)
{
    SC_REQUIRE(c && n_edges_out && n_components_out, SC_ERR_INVALID, "sc_fuzzy_graph: null pointer");
    sc_ctx::UmapWork &f = c->um;
    sc_ctx::ListGraph &g = c->lg;
    const sc_ctx::DenseKnn &kn = c->knn;
    SC_REQUIRE(kn.valid, SC_ERR_STATE, "sc_fuzzy_graph: no neighbour lists are resident (call sc_knn_dense first)");
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t n = kn.n, nk = n * kn.k, chunks = ceil_div64(n, SUM_CHUNK);
    const int k = kn.k;
    lg_invalidate(c, false);
    SC_TRY(f.rho.ensure(sizeof(double) * (size_t)n, &c->mem));
    SC_TRY(f.sigma.ensure(sizeof(double) * (size_t)n, &c->mem));
    SC_TRY(f.dsum.ensure(sizeof(double) * (size_t)(n + chunks + 1), &c->mem));
    double *dsum = f.dsum.as<double>(), *part = dsum + n, *mean = part + chunks;
    long long nnz = 0;
    const dim3 rows((unsigned)ceil_div64(n, 256)), tpb(256);
    const double target = std::log2((double)(k + 1));
    {
        KernelTimerScope ts(c, SC_K_UMAP_GRAPH);
        hipLaunchKernelGGL(k_um_rho, rows, tpb, 0, s, kn.d2.as<double>(), n, k, f.rho.as<double>(), dsum);
        hipLaunchKernelGGL(k_um_chunk_sum, dim3((unsigned)chunks), dim3(64), 0, s, dsum, n, part);
        hipLaunchKernelGGL(k_um_mean, dim3(1), dim3(1), 0, s, part, chunks, (double)(n * (k + 1)), mean);
        if (k <= 8)
            hipLaunchKernelGGL(k_um_sigma<8>, rows, tpb, 0, s, kn.d2.as<double>(), n, k, target, f.rho.as<double>(), dsum, mean,
                               f.sigma.as<double>());
        else if (k <= 16)
            hipLaunchKernelGGL(k_um_sigma<16>, rows, tpb, 0, s, kn.d2.as<double>(), n, k, target, f.rho.as<double>(), dsum, mean,
                               f.sigma.as<double>());
        else
            hipLaunchKernelGGL(k_um_sigma<32>, rows, tpb, 0, s, kn.d2.as<double>(), n, k, target, f.rho.as<double>(), dsum, mean,
                               f.sigma.as<double>());
        SC_TRY(lg_build_union(c, &nnz));
    }
    SC_HIP(hipGetLastError());
    SC_REQUIRE(nnz >= nk && nnz <= 2 * nk, SC_ERR_HIP, "sc_fuzzy_graph: edge count %lld out of range", nnz);
    g.nnz = nnz;
    SC_TRY(g.w.ensure(sizeof(double) * (size_t)nnz, &c->mem));
    {
        KernelTimerScope ts(c, SC_K_UMAP_GRAPH);
        hipLaunchKernelGGL(k_um_weights, dim3((unsigned)ceil_div64(nnz, 256)), tpb, 0, s, g.indptr.as<int64_t>(), g.indices.as<int32_t>(), n,
                           (int64_t)nnz, kn.idx.as<int32_t>(), kn.d2.as<double>(), k, f.rho.as<double>(), f.sigma.as<double>(),
                           g.w.as<double>());
        SC_TRY(lg_finish(c, n_components_out));
    }
    if (rho_out) SC_HIP(hipMemcpyAsync(rho_out, f.rho.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    if (sigma_out) SC_HIP(hipMemcpyAsync(sigma_out, f.sigma.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    *n_edges_out = nnz;
    return SC_OK;
}

extern "C" int sc_umap_layout(sc_ctx *c, const int64_t *indptr, const int32_t *indices, const double *w, int64_t n, double *Y,
                              int32_t C, double a, double b, double gamma, double alpha0, int32_t neg, int32_t n_epochs,
                              uint64_t seed, int32_t e0, int32_t e1)
{
    SC_REQUIRE(c && Y, SC_ERR_INVALID, "sc_umap_layout: null pointer");
    SC_REQUIRE((indptr && indices && w) || (!indptr && !indices && !w), SC_ERR_INVALID,
               "sc_umap_layout: indptr, indices and w must all be given or all be NULL (the resident graph)");
    SC_REQUIRE(n >= 1 && n <= INT32_MAX, SC_ERR_INVALID, "sc_umap_layout: need 1 <= n <= 2^31 - 1, got %lld", (long long)n);
    SC_REQUIRE(C == 2 || C == 3, SC_ERR_INVALID, "sc_umap_layout: need 2 or 3 components, got %d", C);
    SC_REQUIRE(std::isfinite(a) && a > 0.0 && std::isfinite(b) && b > 0.0, SC_ERR_INVALID,
               "sc_umap_layout: a and b must be finite and > 0, got a=%g, b=%g", a, b);
    SC_REQUIRE(std::isfinite(gamma) && gamma >= 0.0, SC_ERR_INVALID, "sc_umap_layout: gamma must be finite and >= 0, got %g", gamma);
    SC_REQUIRE(std::isfinite(alpha0) && alpha0 > 0.0, SC_ERR_INVALID, "sc_umap_layout: alpha0 must be finite and > 0, got %g", alpha0);
    SC_REQUIRE(neg >= 0 && neg <= UM_NEG_MAX, SC_ERR_INVALID, "sc_umap_layout: need 0 <= neg <= %d, got %d", UM_NEG_MAX, neg);
    SC_REQUIRE(n_epochs >= 1, SC_ERR_INVALID, "sc_umap_layout: need n_epochs >= 1, got %d", n_epochs);
    SC_REQUIRE(0 <= e0 && e0 <= e1 && e1 <= n_epochs, SC_ERR_INVALID,
               "sc_umap_layout: the epoch range [%d, %d) must lie inside [0, %d)", e0, e1, n_epochs);
    for (int64_t p = 0; p < n * C; ++p)
        SC_REQUIRE(std::isfinite(Y[p]), SC_ERR_INVALID, "sc_umap_layout: position value %lld is not finite", (long long)p);
    sc_ctx::UmapWork &f = c->um;
    const sc_ctx::ListGraph *g = nullptr;
    int64_t nnz = 0;
    if (indptr) {
        SC_REQUIRE(indptr[0] == 0, SC_ERR_INVALID, "sc_umap_layout: indptr[0] must be 0");
        for (int64_t i = 0; i < n; ++i)   // (its own wording, which tests/umap_host_checks.cpp pins)
            SC_REQUIRE(indptr[i + 1] >= indptr[i], SC_ERR_INVALID, "sc_umap_layout: indptr descends at row %lld", (long long)i);
        nnz = indptr[n];
        SC_TRY(csr_check_columns("sc_umap_layout", indptr, indices, n, n, "n", [&](int64_t, int64_t p) -> int {
            SC_REQUIRE(std::isfinite(w[p]) && w[p] > 0.0, SC_ERR_INVALID, "sc_umap_layout: stored value %lld must be finite and > 0", (long long)p);
            return SC_OK;
        }));
    } else {
        SC_TRY(lg_resident(c, "sc_umap_layout", " (call sc_fuzzy_graph or sc_diffmap_graph first)", &g));
        SC_REQUIRE(n == g->n, SC_ERR_INVALID, "sc_umap_layout: the resident graph has %lld vertices, got n=%lld", (long long)g->n,
                   (long long)n);
        nnz = g->nnz;
    }
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t ybytes = sizeof(double) * (size_t)(n * C);
    SC_TRY(f.ly0.ensure(ybytes, &c->mem));
    SC_TRY(f.ly1.ensure(ybytes, &c->mem));
    SC_TRY(f.lmax.ensure(sizeof(u64), &c->mem));
    const int64_t *d_indptr = nullptr;
    const int32_t *d_indices = nullptr;
    const double *d_w = nullptr;
    if (indptr) {
        SC_TRY(f.lip.ensure(sizeof(int64_t) * (size_t)(n + 1), &c->mem));
        SC_TRY(f.lix.ensure(sizeof(int32_t) * (size_t)(nnz > 0 ? nnz : 1), &c->mem));
        SC_TRY(f.lw.ensure(sizeof(double) * (size_t)(nnz > 0 ? nnz : 1), &c->mem));
        SC_HIP(hipMemcpyAsync(f.lip.p, indptr, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, s));
        if (nnz > 0) {
            SC_HIP(hipMemcpyAsync(f.lix.p, indices, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, s));
            SC_HIP(hipMemcpyAsync(f.lw.p, w, sizeof(double) * (size_t)nnz, hipMemcpyHostToDevice, s));
        }
        d_indptr = f.lip.as<int64_t>();
        d_indices = f.lix.as<int32_t>();
        d_w = f.lw.as<double>();
    } else {
        d_indptr = g->indptr.as<int64_t>();
        d_indices = g->indices.as<int32_t>();
        d_w = g->w.as<double>();
    }
    SC_HIP(hipMemcpyAsync(f.ly0.p, Y, ybytes, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemsetAsync(f.lmax.p, 0, sizeof(u64), s));
    double *cur = f.ly0.as<double>(), *nxt = f.ly1.as<double>();
    {
        KernelTimerScope ts(c, SC_K_UMAP_LAYOUT);
        if (nnz > 0) {
            const int64_t want = ceil_div64(nnz, 256);
            hipLaunchKernelGGL(k_um_wmax, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, s, d_w, nnz, f.lmax.as<u64>());
        }
        UmCoef k;
        k.a = a;
        k.b = b;
        k.m2ab = (-2.0 * a) * b;
        k.g2b = (2.0 * gamma) * b;
        const dim3 rows((unsigned)ceil_div64(n, 256)), tpb(256);
        for (int32_t e = e0; e < e1 && nnz > 0; ++e) {
            k.alpha = alpha0 * (1.0 - (double)e / (double)n_epochs);
            if (C == 2)
                hipLaunchKernelGGL(k_um_epoch<2>, rows, tpb, 0, s, d_indptr, d_indices, d_w, n, cur, nxt, f.lmax.as<u64>(), k, (int)neg,
                                   (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)e);
            else
                hipLaunchKernelGGL(k_um_epoch<3>, rows, tpb, 0, s, d_indptr, d_indices, d_w, n, cur, nxt, f.lmax.as<u64>(), k, (int)neg,
                                   (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)e);
            double *tmp = cur;
            cur = nxt;
            nxt = tmp;
        }
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(Y, cur, ybytes, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}
