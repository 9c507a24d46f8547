// What more than one unit needs of the exact search in d dimensions (sc_neighbors.hip: sc_knn_dense, the direct kernels,
// and sc_knn_dense_gram, the certified Gram-form filter): the limits and the direct-form squared distance whose bits every
// neighbour list of the project is pinned to, which sc_diffmap_graph's weights repeat.
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
