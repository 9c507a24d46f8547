// Lee's L, the float32-faithful observed value (sc_lee_observed_f32).  gfx950 only.
//
// For a float32 matrix the reference computes everything in float32 with numpy's
// summation order (AC:1118-1146, 307-315): mean = S(x) / n, std = sqrt(S(d * d) / n) with d = x - mean, z = d / std,
// lag = W32 @ z_y (scipy csr_matvec: row-sequential, multiply and add rounded separately), L = float(S(z_x * lag)),
// where S is numpy's sum of a contiguous float32 vector: the vector is cut into chunks of 8192 elements (the ufunc
// buffer size), every chunk is summed PAIRWISE (blocks of <= 128 with 8 strided accumulators, halving above that with
// the split rounded down to a multiple of 8) and the chunk sums are accumulated in order (numpy 2.2, verified against
// numpy itself up to 10^6 elements).  A sum of 10^6 signed float32 terms carries ~1e-5 relative rounding noise, so an
// fp64 L differs from the reference's by that much; to hand back the reference's OWN number the same tree is
// evaluated here with the same float roundings -- in parallel: the tree's shape depends on n alone, so one thread sums
// one leaf and one thread per vector replays the recursion over the leaf sums (sc_pairwise.h).  The permutation
// statistics stay fp64 (the p-values of the reference's goldens are reproduced exactly that way).
#include <algorithm>
#include <vector>

#include "sc_lee.h"
#include "sc_pairwise.h"

#define NP_SUM_CHUNK 8192u   // numpy's ufunc buffer size in elements

// leaves[i] = (start, len) of the i-th leaf of numpy's sum over m elements (chunk after chunk); *nleaves
__global__ void k32_leaves(uint32_t m, uint2 *__restrict__ leaves, uint32_t max_leaves, uint32_t *__restrict__ nleaves)
{
    uint32_t k = 0;
    for (uint32_t c0 = 0; c0 < m; c0 += NP_SUM_CHUNK) {
        const uint32_t len_c = m - c0 < NP_SUM_CHUNK ? m - c0 : NP_SUM_CHUNK;
        (void)pw_walk<float>(len_c, [&](uint32_t start, uint32_t len) {
            if (k < max_leaves) leaves[k] = make_uint2(c0 + start, len);
            ++k;
            return 0.f;
        });
    }
    *nleaves = k;
}

// numpy's sum of m float32 terms from the leaf sums `ls` (in leaf order): chunk sums accumulated in order
__device__ __forceinline__ float np_sum_from_leaves(uint32_t m, const float *__restrict__ ls)
{
    uint32_t i = 0;
    float acc = 0.f;
    for (uint32_t c0 = 0; c0 < m; c0 += NP_SUM_CHUNK) {
        const uint32_t len_c = m - c0 < NP_SUM_CHUNK ? m - c0 : NP_SUM_CHUNK;
        const float part = pw_walk<float>(len_c, [&](uint32_t, uint32_t) { return ls[i++]; });
        acc = c0 == 0 ? part : __fadd_rn(acc, part);
    }
    return acc;
}

// STAT 0: leaf sums of x over cells start ..; STAT 1: of fl(d * d), d = fl(x - mean).  thread = (leaf, gene)
template <int STAT>
__global__ __launch_bounds__(256) void k32_gene_leafsum(const double *__restrict__ X, int64_t n,
                                                        const int32_t *__restrict__ genes,
                                                        const float *__restrict__ mean32, const uint2 *__restrict__ leaves,
                                                        uint32_t nleaves, float *__restrict__ leafsum)
{
    const uint32_t leaf = blockIdx.x * blockDim.x + threadIdx.x;
    if (leaf >= nleaves) return;
    const int32_t g = genes[blockIdx.y];
    const double *col = X + (int64_t)(g >> 4) * n * SC_TILE + (g & 15);
    const uint2 lf = leaves[leaf];
    const float mu = STAT ? mean32[blockIdx.y] : 0.f;
    leafsum[(int64_t)blockIdx.y * nleaves + leaf] = pw_block<float>(lf.y, [&](uint32_t k) {
        const float x = (float)col[(int64_t)(lf.x + k) * SC_TILE];
        if (!STAT) return x;
        const float d = __fsub_rn(x, mu);
        return __fmul_rn(d, d);
    });
}

// STAT 0: mean32[k] = S(x) / n;  STAT 1: sd32[k] = sqrt(S(d * d) / n)   (IEEE float division / sqrt)
template <int STAT>
__global__ void k32_gene_combine(int64_t n, int n_genes, const float *__restrict__ leafsum, uint32_t nleaves,
                                 float *__restrict__ out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_genes) return;
    float res = np_sum_from_leaves((uint32_t)n, leafsum + (int64_t)k * nleaves);
    res = (float)__ddiv_rn((double)res, (double)(float)n);   // correctly rounded float division (53 >= 2 * 24 + 2)
    out[k] = STAT ? (float)__dsqrt_rn((double)res) : res;
}

// z32[k][cell] = fl(fl(x - mean) / sd)
__global__ __launch_bounds__(256) void k32_zscore(const double *__restrict__ X, int64_t n, const int32_t *__restrict__ genes,
                                                  const float *__restrict__ mean32, const float *__restrict__ sd32,
                                                  float *__restrict__ z32)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t g = genes[blockIdx.y];
    const float x = (float)X[(int64_t)(g >> 4) * n * SC_TILE + i * SC_TILE + (g & 15)];
    z32[(int64_t)blockIdx.y * n + i] = (float)__ddiv_rn((double)__fsub_rn(x, mean32[blockIdx.y]), (double)sd32[blockIdx.y]);
}

// lag32[k][i] = scipy's float32 csr_matvec row i of W32 @ z32[k]
__global__ __launch_bounds__(256) void k32_lag(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                               const double *__restrict__ w, const float *__restrict__ z32, int64_t n,
                                               float *__restrict__ lag32)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *z = z32 + (int64_t)blockIdx.y * n;
    float s = 0.f;
    for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) s = __fadd_rn(s, __fmul_rn((float)w[e], z[indices[e]]));
    lag32[(int64_t)blockIdx.y * n + i] = s;
}

// leaf sums of p = fl(zx * lag_y) over cells start ..   thread = (leaf, pair)
__global__ __launch_bounds__(256) void k32_pair_leafsum(const float *__restrict__ z32, const float *__restrict__ lag32,
                                                        int64_t n, const int2 *__restrict__ pair_slots,
                                                        const uint2 *__restrict__ leaves, uint32_t nleaves,
                                                        float *__restrict__ leafsum)
{
    const uint32_t leaf = blockIdx.x * blockDim.x + threadIdx.x;
    if (leaf >= nleaves) return;
    const int2 sl = pair_slots[blockIdx.y];
    if (sl.x < 0) return;
    const float *zx = z32 + (int64_t)sl.x * n, *ly = lag32 + (int64_t)sl.y * n;
    const uint2 lf = leaves[leaf];
    leafsum[(int64_t)blockIdx.y * nleaves + leaf] =
        pw_block<float>(lf.y, [&](uint32_t k) { return __fmul_rn(zx[lf.x + k], ly[lf.x + k]); });
}

__global__ void k32_pair_combine(int64_t n, const int2 *__restrict__ pair_slots, int64_t n_pairs,
                                 const float *__restrict__ leafsum, uint32_t nleaves, float *__restrict__ out)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pairs) return;
    out[q] = pair_slots[q].x < 0 ? 0.f : np_sum_from_leaves((uint32_t)n, leafsum + q * nleaves);
}

extern "C" int sc_lee_observed_f32(sc_ctx *c, const int32_t *pair_x, const int32_t *pair_y, int64_t n_pairs,
                                   float *L32_out, float *mean32_out, float *sd32_out)
{
    SC_REQUIRE(c && pair_x && pair_y && L32_out, SC_ERR_INVALID, "sc_lee_observed_f32: null pointer");
    SC_HIP(hipSetDevice(c->device));
    SC_REQUIRE(c->e_n > 0 && c->g_n == c->e_n, SC_ERR_STATE, "sc_lee_observed_f32: expression / graph missing");
    SC_REQUIRE(c->e_dtype == SC_F32, SC_ERR_STATE, "sc_lee_observed_f32: the loaded matrix is not float32");
    const int64_t n = c->e_n, G = c->e_genes;
    SC_REQUIRE(n < ((int64_t)1 << 31), SC_ERR_INVALID, "sc_lee_observed_f32: too many cells");
    if (n_pairs == 0) return SC_OK;
    SC_TRY(lee_check_genes(c, "sc_lee_observed_f32", "%s: pair %lld references a gene outside the loaded set", pair_x, pair_y, n_pairs));
    // distinct genes of the pair list (first-seen order)
    std::vector<int32_t> genes, slot((size_t)G, -1);
    for (int64_t q = 0; q < n_pairs; ++q) {
        for (int32_t g : {pair_x[q], pair_y[q]})
            if (slot[(size_t)g] < 0) { slot[(size_t)g] = (int32_t)genes.size(); genes.push_back(g); }
    }
    const int K = (int)genes.size();
    const uint32_t m = (uint32_t)n;
    const uint32_t max_leaves = m / 64 + 66;  // leaves hold >= 64 elements each, except in a ragged last chunk
    // layout of one scratch buffer: [genes K i32][mean K f32][sd K f32][nleaves u32 + pad][leaves][z32 K n][lag32 K n]
    SC_TRY(c->scratch_a.ensure(sizeof(int32_t) * (size_t)K * 3 + 16 + sizeof(uint2) * (size_t)max_leaves +
                           sizeof(float) * 2 * (size_t)K * (size_t)n, &c->mem));
    int32_t *d_genes = c->scratch_a.as<int32_t>();
    float *d_mean = reinterpret_cast<float *>(d_genes + K), *d_sd = d_mean + K;
    uint32_t *d_nl = reinterpret_cast<uint32_t *>(d_sd + K + (K & 1));
    uint2 *d_leaves = reinterpret_cast<uint2 *>(d_nl + 4);
    float *d_z = reinterpret_cast<float *>(d_leaves + max_leaves), *d_lag = d_z + (int64_t)K * n;
    SC_HIP(hipMemcpyAsync(d_genes, genes.data(), sizeof(int32_t) * (size_t)K, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k32_leaves, dim3(1), dim3(1), 0, c->stream, m, d_leaves, max_leaves, d_nl);
    uint32_t nleaves = 0;
    SC_HIP(hipMemcpyAsync(&nleaves, d_nl, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    SC_REQUIRE(nleaves <= max_leaves, SC_ERR_STATE, "sc_lee_observed_f32: leaf table overflow");
    const size_t ls_elems = (size_t)std::max<int64_t>(K, n_pairs) * (size_t)(nleaves ? nleaves : 1);
    SC_TRY(c->scratch_b.ensure(sizeof(float) * ls_elems, &c->mem));
    float *d_ls = c->scratch_b.as<float>();
    const dim3 lgrid((unsigned)ceil_div64(nleaves ? nleaves : 1, 256), (unsigned)K), cgrid((unsigned)ceil_div64(n, 256), (unsigned)K);
    const double *X = c->X.as<double>();
    if (nleaves) hipLaunchKernelGGL(k32_gene_leafsum<0>, lgrid, dim3(256), 0, c->stream, X, n, d_genes, d_mean, d_leaves, nleaves, d_ls);
    hipLaunchKernelGGL(k32_gene_combine<0>, dim3((unsigned)ceil_div64(K, 64)), dim3(64), 0, c->stream, n, K, d_ls, nleaves, d_mean);
    if (nleaves) hipLaunchKernelGGL(k32_gene_leafsum<1>, lgrid, dim3(256), 0, c->stream, X, n, d_genes, d_mean, d_leaves, nleaves, d_ls);
    hipLaunchKernelGGL(k32_gene_combine<1>, dim3((unsigned)ceil_div64(K, 64)), dim3(64), 0, c->stream, n, K, d_ls, nleaves, d_sd);
    hipLaunchKernelGGL(k32_zscore, cgrid, dim3(256), 0, c->stream, X, n, d_genes, d_mean, d_sd, d_z);
    hipLaunchKernelGGL(k32_lag, cgrid, dim3(256), 0, c->stream, c->g_indptr.as<int64_t>(), c->g_indices.as<int32_t>(),
                       c->g_data.as<double>(), d_z, n, d_lag);
    SC_HIP(hipGetLastError());
    // pairs: (slot of x, slot of y), or (-1, -1) when a gene has zero float32 variance (AC:1129: x_std == 0)
    std::vector<float> sd((size_t)K), mean((size_t)K);
    SC_HIP(hipMemcpyAsync(sd.data(), d_sd, sizeof(float) * (size_t)K, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipMemcpyAsync(mean.data(), d_mean, sizeof(float) * (size_t)K, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    std::vector<int2> ps((size_t)n_pairs);
    for (int64_t q = 0; q < n_pairs; ++q) {
        const int sx = slot[(size_t)pair_x[q]], sy = slot[(size_t)pair_y[q]];
        ps[(size_t)q] = (sd[(size_t)sx] == 0.f || sd[(size_t)sy] == 0.f) ? make_int2(-1, -1) : make_int2(sx, sy);
        if (mean32_out) { mean32_out[2 * q] = mean[(size_t)sx]; mean32_out[2 * q + 1] = mean[(size_t)sy]; }
        if (sd32_out) { sd32_out[2 * q] = sd[(size_t)sx]; sd32_out[2 * q + 1] = sd[(size_t)sy]; }
    }
    SC_TRY(c->lee_rowmap.ensure(sizeof(int2) * (size_t)n_pairs + sizeof(float) * (size_t)n_pairs, &c->mem));
    int2 *d_ps = c->lee_rowmap.as<int2>();
    float *d_out = reinterpret_cast<float *>(d_ps + n_pairs);
    SC_HIP(hipMemcpyAsync(d_ps, ps.data(), sizeof(int2) * (size_t)n_pairs, hipMemcpyHostToDevice, c->stream));
    for (int64_t q0 = 0; nleaves && q0 < n_pairs; q0 += 32768) {   // gridDim.y limit
        const int64_t qn = std::min<int64_t>(32768, n_pairs - q0);
        hipLaunchKernelGGL(k32_pair_leafsum, dim3((unsigned)ceil_div64(nleaves, 256), (unsigned)qn), dim3(256), 0, c->stream,
                           d_z, d_lag, n, d_ps + q0, d_leaves, nleaves, d_ls + q0 * nleaves);
    }
    hipLaunchKernelGGL(k32_pair_combine, dim3((unsigned)ceil_div64(n_pairs, 64)), dim3(64), 0, c->stream, n, d_ps, n_pairs,
                       d_ls, nleaves, d_out);
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(L32_out, d_out, sizeof(float) * (size_t)n_pairs, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}
