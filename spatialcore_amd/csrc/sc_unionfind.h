// Lock-free union-find on an int32 parent array (device helpers; sc_domains.hip, sc_diffusion.hip).  Every edge hooks the
// larger root under the smaller (atomicCAS) and finds halve their path (atomicMin), so a parent is never larger than its
// child and the root of a finished tree is the smallest index of its component: a function of the edge set, not of the
// order in which the atomics landed.
#pragma once

#include "sc_ctx.h"

__device__ __forceinline__ int32_t uf_load(const int32_t *a) { return __atomic_load_n(a, __ATOMIC_RELAXED); }

// root of x, halving the path on the way: parent[x] <- its grandparent.  atomicMin: a parent only ever moves towards the
// root, whatever other lanes write meanwhile.
__device__ __forceinline__ int32_t uf_find(int32_t *parent, int32_t x)
{
    for (;;) {
        const int32_t p = uf_load(parent + x);
        if (p == x) return x;
        const int32_t gp = uf_load(parent + p);
        if (gp != p) atomicMin(parent + x, gp);
        x = gp;
    }
}

__device__ __forceinline__ void uf_union(int32_t *parent, int32_t a, int32_t b)
{
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        if (atomicCAS(parent + hi, hi, lo) == hi) return;   // hi was still a root: hooked.  Otherwise look again.
    }
}
