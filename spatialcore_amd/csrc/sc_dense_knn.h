// What the two exact searches in d dimensions share (sc_diffusion.hip: sc_knn_dense, the direct kernels; sc_neighbors.hip:
// sc_knn_dense_gram, the certified Gram-form filter): the limits, the widening of the caller's rows, the direct-form
// squared distance whose bits every neighbour list of the project is pinned to, the finite check and the list write-out.
// And what the two graphs on those lists share (sc_diffusion.hip: sc_diffmap_graph; sc_umap.hip: sc_fuzzy_graph): the
// symmetric union as a CSR pattern and the tail that makes a weighted graph the resident one.
#pragma once

#include <cmath>

#include "sc_topk.h"

constexpr int DF_DMAX = 64;
constexpr int DF_KMAX = 32;
constexpr int DF_QB_L = 64;       // LDS form of the direct search: queries per workgroup (their rows take 32 KiB) ...
constexpr int DF_TILE_L = 32;     // ... and candidates per tile (16 KiB)
constexpr int64_t DF_SPLIT_BELOW = 100000;   // fewer queries than this: the candidates are split over workgroups
constexpr int DF_SPLIT_WGS = 2048;           // ... aiming at about this many

// X[n][dp] <- the caller's rows widened to fp64, columns d .. dp - 1 zero
template <class T>
__global__ __launch_bounds__(256) void k_df_widen(const T *__restrict__ raw, int64_t n, int d, int dp, double *__restrict__ X)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * dp) return;
    const int64_t i = t / dp;
    const int c = (int)(t % dp);
    X[t] = c < d ? (double)raw[i * d + c] : 0.0;
}

// The direct form: the dp terms (q(c) - x(c))^2 in column order, starting from the c = 0 term, every difference, product
// and sum rounded separately (-ffp-contract=off).  q and x give column c of the two rows, from wherever they live.
// DR > 0: a row of DR columns known at compile time, unrolled (rows in registers); DR = 0: dp columns.
template <int DR, class Q, class X>
__device__ __forceinline__ double df_d2(const Q &q, const X &x, int dp)
{
    const double f0 = q(0) - x(0);
    double acc = f0 * f0;
    if constexpr (DR > 0) {
#pragma unroll
        for (int c = 1; c < DR; ++c) {
            const double f = q(c) - x(c);
            acc = acc + f * f;
        }
    } else {
        for (int c = 1; c < dp; ++c) {
            const double f = q(c) - x(c);
            acc = acc + f * f;
        }
    }
    return acc;
}

// the first k entries of a finished list, best first, to (idx, d2)[o .. o + k)
template <int K>
__device__ __forceinline__ void df_write_list(const TopK<K> &best, int k, int64_t o, int32_t *__restrict__ idx, double *__restrict__ d2)
{
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j < k) {
            idx[o + j] = best.id[j];
            d2[o + j] = best.d[j];
        }
}

template <class T>
int df_require_finite(const char *who, const T *X, int64_t count)
{
    for (int64_t p = 0; p < count; ++p)
        SC_REQUIRE(std::fabs((double)X[p]) < 0x1p500, SC_ERR_INVALID,   // so that no squared distance overflows
                   "%s: feature value %lld is not finite and below 2^500 in magnitude", who, (long long)p);
    return SC_OK;
}

// the row of stored entry e: the last i with indptr[i] <= e (no row is empty)
__device__ __forceinline__ int64_t df_row_of(const int64_t *__restrict__ indptr, int64_t n, int64_t e)
{
    int64_t lo = 0, hi = n;   // indptr[lo] <= e < indptr[hi]
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (indptr[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// sc_diffusion.hip.  df_build_union: the symmetric union of the resident lists as indptr / indices on the device (rows
// sorted by column), *nnz_out = its stored entries.  df_finish_graph: on the resident CSR with its weights w in place: row
// sums, density, transition matrix and the connected components; marks the graph valid for sc_diffmap_graph_get,
// sc_lanczos_begin and sc_louvain_begin_resident.
int df_build_union(sc_ctx *c, long long *nnz_out);
int df_finish_graph(sc_ctx *c, int64_t *n_components_out);
