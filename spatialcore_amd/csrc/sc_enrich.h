// The relabel kernels of the label-permutation tests, shared by the enrichment (sc_graph.hip) and Ripley's K
// (sc_ripley.hip): both walk a pair list whose two ends are positions of a spatially sorted processing order and need
// the permuted label of the cell at a position as one byte (one permutation) or as one 16-byte word (sixteen).
// `static`: every translation unit that includes this compiles its own copy (the library is built without -fgpu-rdc).
#pragma once

#include "sc_ctx.h"

// labp[p][r] = lab[perm_p[order[r]]] (p == n_perm: the identity, i.e. the observed labels): the permuted label of
// the cell at position r of the graph's spatially sorted processing order.  The edge kernel then needs ONE byte per
// edge end from an n-byte array (instead of a 4-byte index gather followed by a byte gather), and the two ends of an
// edge -- spatial neighbours -- sit at nearby positions: the row's k + 1 bytes come from one or two cache lines.
static __global__ __launch_bounds__(256) void k_enrich_relabel(const unsigned char *__restrict__ lab,
                                                               const int32_t *__restrict__ order,
                                                               const int32_t *__restrict__ perm, int64_t pstride, int n_perm,
                                                               int64_t n, int64_t lstride, unsigned char *__restrict__ labp)
{
    const int p = blockIdx.y;
    const int32_t *prow = p < n_perm ? perm + (int64_t)p * pstride : nullptr;
    const int64_t r0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (r0 >= n) return;
    unsigned char *dst = labp + (int64_t)p * lstride;
    uint32_t v = 0;
    for (int k = 0; k < 4 && r0 + k < n; ++k) {
        const int32_t cell = order[r0 + k];
        v |= (uint32_t)lab[prow ? prow[cell] : cell] << (8 * k);
    }
    if (r0 + 4 <= n) *reinterpret_cast<uint32_t *>(dst + r0) = v;
    else for (int k = 0; r0 + k < n; ++k) dst[r0 + k] = (unsigned char)(v >> (8 * k));
}

// lab16[g][rank[cell]] = the labels of `cell` under permutations 16 g .. 16 g + 15 (rows clamped to rows - 1)
static __global__ __launch_bounds__(256) void k_enrich_relabel16(const unsigned char *__restrict__ lab,
                                                                 const int32_t *__restrict__ rank,
                                                                 const int32_t *__restrict__ perm, int64_t pstride, int rows,
                                                                 int64_t n, uint4 *__restrict__ lab16)
{
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= n) return;
    const int g = blockIdx.y;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        const int row = 16 * g + p < rows ? 16 * g + p : rows - 1;
        w[p >> 2] |= (uint32_t)lab[perm[(int64_t)row * pstride + cell]] << (8 * (p & 3));
    }
    lab16[(int64_t)g * n + rank[cell]] = make_uint4(w[0], w[1], w[2], w[3]);
}
