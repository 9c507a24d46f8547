// The order of neighbour candidates and the register top-k list built on it (device helpers; sc_search.hip: the planar
// searches, sc_neighbors.hip: the search in d dimensions).  Every neighbour list of the project is pinned bit for bit, so
// the comparison that decides it is written here once.
#pragma once

#include <float.h>

#include "sc_ctx.h"

// The project's order of candidates: smaller squared distance first, ties to the lower index.
__device__ __forceinline__ bool cand_better(double d, int id, double ed, int eid)
{
    return d < ed || (d == ed && id < eid);
}

// The K best candidates of a query in registers, best first (sc_search.hip: k_knn; sc_neighbors.hip: the dense search)
template <int K>
struct TopK {
    double d[K];
    int id[K];
    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int j = 0; j < K; ++j) { d[j] = DBL_MAX; id[j] = 0x7fffffff; }
    }
    // sorted insert of a candidate known to beat the last entry
    __device__ __forceinline__ void insert(double cd, int cid)
    {
        bool b_hi = cand_better(cd, cid, d[K - 1], id[K - 1]);  // vs entry j
#pragma unroll
        for (int j = K - 1; j > 0; --j) {
            bool b_lo = cand_better(cd, cid, d[j - 1], id[j - 1]);  // vs entry j-1
            double nd = b_lo ? d[j - 1] : (b_hi ? cd : d[j]);
            int ni = b_lo ? id[j - 1] : (b_hi ? cid : id[j]);
            d[j] = nd;
            id[j] = ni;
            b_hi = b_lo;
        }
        if (b_hi) { d[0] = cd; id[0] = cid; }
    }
    __device__ __forceinline__ double kth(int k) const
    {
        double v = d[K - 1];
#pragma unroll
        for (int j = 0; j < K; ++j) v = (j == k - 1) ? d[j] : v;
        return v;
    }
};
