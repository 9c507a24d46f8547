// What more than one unit needs of the exact search in d dimensions (sc_neighbors.hip: sc_knn_dense, the direct kernels,
// and sc_knn_dense_gram, the certified Gram-form filter): the limits and the direct-form squared distance whose bits every
// neighbour list of the project is pinned to, which sc_diffmap_graph's weights repeat.  And what the two graphs on those
// lists share (sc_diffusion.hip: sc_diffmap_graph; sc_umap.hip: sc_fuzzy_graph): the row of a stored entry, the symmetric
// union as a CSR pattern and the tail that makes a weighted graph the resident one.
#pragma once

#include "sc_ctx.h"

constexpr int DF_DMAX = 64;
constexpr int DF_KMAX = 32;

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

// sc_diffusion.hip.  df_build_union: the symmetric union of the resident lists (ctx->knn) as indptr / indices on the device
// (rows sorted by column), *nnz_out = its stored entries; df.n becomes the lists' row count.  df_finish_graph: on the
// resident CSR with its weights w in place: row sums, density, transition matrix and the connected components; marks the
// graph valid for sc_diffmap_graph_get, sc_lanczos_begin and sc_louvain_begin_resident.
int df_build_union(sc_ctx *c, long long *nnz_out);
int df_finish_graph(sc_ctx *c, int64_t *n_components_out);
