// Local Moran's I with the reference's float32 arithmetic and per-cell permutation counts.  gfx950 only.
#include <math.h>
#include <stdlib.h>

#include <functional>
#include <optional>
#include <thread>
#include <vector>

#include "sc_ctx.h"
#include "sc_local.h"
#include "sc_pairwise.h"

// ------------------------------------------------------------------------------------------------
// N1: Local Moran's I (AC:804-934) with the reference's float32 arithmetic
//
// The reference standardises in float32, takes lag = W32 @ Z32 with scipy's row-sequential float32
// accumulation, and for every permutation recomputes Zs = Z[perm], lag_s = W @ Zs, I_perm = Zs * lag_s
// into a (P, N, B) tensor before counting |I_perm| >= |I| per cell in a Python loop.  Here the count
// is accumulated on the fly: thread = (cell, 4 genes of a 16-gene float tile), loop over permutations.
// ------------------------------------------------------------------------------------------------

// Z32[tile][cell][16] = (float(x) - mean32) / sd32  (two float32 roundings, AC:858); padded genes -> 0
__global__ __launch_bounds__(256) void k_lm_standardize(const double *__restrict__ X, const float *__restrict__ mean32,
                                                        const float *__restrict__ sd32, float *__restrict__ Z32,
                                                        int64_t n)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * SC_TILE) return;
    int64_t tile = blockIdx.y;
    int slot = (int)(t & 15);
    float x = (float)X[tile * n * SC_TILE + t];
    float sd = sd32[tile * SC_TILE + slot];
    // IEEE float division via double (innocuous double rounding for 24-bit operands)
    float z = (float)__ddiv_rn((double)__fsub_rn(x, mean32[tile * SC_TILE + slot]), (double)sd);
    Z32[tile * n * SC_TILE + t] = z;
}

// ---- numpy's float summation, reproduced ---------------------------------------------------------
// The reference takes the per-gene mean and E[x^2] with scipy's sparse `.mean(axis=0)` (AC:79-80,
// 102-107): (data * T(1/n)) summed per CSC column by np.add.reduceat, i.e. first stored entry +
// numpy's PAIRWISE sum of the rest (blocks of <= 128 with 8 strided accumulators, halving above
// that with the split rounded down to a multiple of 8), in the matrix dtype T.  On count data the
// per-cell |I_perm| >= |I| test is full of exact ties that are decided by the last bit of z, so the
// float32 mean and sd must be THE SAME floats; a more accurate sum is not good enough.
// The summation tree is fixed by the element count alone, so it is evaluated in parallel with the same rounding:
// (1) the stored (non-zero) values of every gene are compacted in cell order (k_npc_count / k_npc_offsets /
// k_npc_scatter: wavefront ballots over 512-cell blocks), (2) one thread per gene lists the leaves of numpy's
// recursion over elements 1.. (k_npc_leaves), (3) one thread per (gene, statistic, leaf) sums its <= 128 elements
// with the 8 strided accumulators (k_npc_leafsum), (4) one thread per (gene, statistic) replays the recursion over
// the leaf sums (k_npc_combine).  A sequential walk per gene took 1.15 s at 1M cells; this takes milliseconds.

#define NPC_CELLS 512  // cells per wavefront block of the compaction

// cnt[(tile * nblk + w) * 16 + g] = stored entries of gene slot g among the cells of block w
__global__ __launch_bounds__(256) void k_npc_count(const double *__restrict__ X, int64_t n, int64_t nblk,
                                                   uint32_t *__restrict__ cnt)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), tile = blockIdx.y;
    if (w >= nblk) return;
    const double *Xt = X + tile * n * SC_TILE;
    uint32_t mine = 0;
    for (int s = 0; s < NPC_CELLS / 64; ++s) {
        const int64_t cell = w * NPC_CELLS + 64 * s + lane;
        double v[16];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double2 t = cell < n ? reinterpret_cast<const double2 *>(Xt + cell * SC_TILE)[k] : make_double2(0.0, 0.0);
            v[2 * k] = t.x; v[2 * k + 1] = t.y;
        }
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const uint32_t c = (uint32_t)__popcll(__ballot(v[g] != 0.0));
            mine += (lane == g) ? c : 0u;
        }
    }
    if (lane < 16) cnt[(tile * nblk + w) * 16 + lane] = mine;
}

// exclusive prefix over the blocks of one gene, in place (one thread per padded gene)
__global__ void k_npc_offsets(uint32_t *__restrict__ cnt, int64_t nblk, int64_t genes_padded)
{
    const int64_t gp = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gp >= genes_padded) return;
    uint32_t *c = cnt + (gp >> 4) * nblk * 16 + (gp & 15);
    uint32_t run = 0;
    for (int64_t w = 0; w < nblk; ++w) {
        const uint32_t t = c[w * 16];
        c[w * 16] = run;
        run += t;
    }
}

// comp[gene * n + k] = k-th stored value of the gene, in cell order, as T
template <typename T>
__global__ __launch_bounds__(256) void k_npc_scatter(const double *__restrict__ X, int64_t n, int64_t nblk,
                                                     const uint32_t *__restrict__ off, T *__restrict__ comp)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), tile = blockIdx.y;
    if (w >= nblk) return;
    const double *Xt = X + tile * n * SC_TILE;
    uint32_t base[16];
#pragma unroll
    for (int g = 0; g < 16; ++g) base[g] = off[(tile * nblk + w) * 16 + g];
    for (int s = 0; s < NPC_CELLS / 64; ++s) {
        const int64_t cell = w * NPC_CELLS + 64 * s + lane;
        double v[16];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double2 t = cell < n ? reinterpret_cast<const double2 *>(Xt + cell * SC_TILE)[k] : make_double2(0.0, 0.0);
            v[2 * k] = t.x; v[2 * k + 1] = t.y;
        }
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const bool nz = v[g] != 0.0;
            const unsigned long long bal = __ballot(nz);
            // set bits of the ballot below this lane: the hardware's own mask-below-lane count (no per-lane 64-bit shift)
            const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            if (nz) comp[(tile * 16 + g) * n + base[g] + below] = (T)v[g];
            base[g] += (uint32_t)__popcll(bal);
        }
    }
}

// leaves[gene][i] = (start, len) of the i-th leaf of the recursion over elements 1 .. nnz-1; nleaves[gene]
__global__ void k_npc_leaves(const double *__restrict__ nnz, int64_t n_genes, int64_t max_leaves,
                             uint2 *__restrict__ leaves, uint32_t *__restrict__ nleaves)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_genes) return;
    const uint32_t cnt = (uint32_t)nnz[g];
    uint32_t k = 0;
    if (cnt >= 2) {
        uint2 *out = leaves + g * max_leaves;
        (void)pw_walk<float>(cnt - 1, [&](uint32_t start, uint32_t len) {
            if ((int64_t)k < max_leaves) out[k] = make_uint2(start, len);
            ++k;
            return 0.f;
        });
    }
    nleaves[g] = k;
}

// one leaf: numpy's unrolled block sum (8 strided accumulators, pairwise combine, then the tail) of
// val(i) = x_i * inv_n (statistic 0) or (x_i * x_i) * inv_n (statistic 1) over compacted elements 1 + start ..
template <typename T>
__global__ __launch_bounds__(256) void k_npc_leafsum(const T *__restrict__ comp, int64_t n,
                                                     const uint2 *__restrict__ leaves,
                                                     const uint32_t *__restrict__ nleaves, int64_t max_leaves,
                                                     T *__restrict__ leafsum)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t g = blockIdx.y;
    const int square = blockIdx.z;
    if (i >= (int64_t)nleaves[g] || i >= max_leaves) return;
    const uint2 lf = leaves[g * max_leaves + i];
    const T *a = comp + g * n + 1 + lf.x;
    const T inv_n = (T)(1.0 / (double)n);
    const uint32_t len = lf.y;
    auto val = [&](uint32_t k) { T x = a[k]; if (square) x = x * x; return x * inv_n; };
    T res;
    if (len < 8) {
        res = (T)(-0.0);
        for (uint32_t k = 0; k < len; ++k) res += val(k);
    } else {
        T r0 = val(0), r1 = val(1), r2 = val(2), r3 = val(3), r4 = val(4), r5 = val(5), r6 = val(6), r7 = val(7);
        uint32_t k = 8;
        for (; k < len - (len % 8); k += 8) {
            r0 += val(k); r1 += val(k + 1); r2 += val(k + 2); r3 += val(k + 3);
            r4 += val(k + 4); r5 += val(k + 5); r6 += val(k + 6); r7 += val(k + 7);
        }
        res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
        for (; k < len; ++k) res += val(k);
    }
    leafsum[(g * 2 + square) * max_leaves + i] = res;
}

// out[2*g] = numpy mean, out[2*g+1] = numpy mean of squares, as T: first stored entry + pairwise sum of the rest
template <typename T>
__global__ void k_npc_combine(const T *__restrict__ comp, int64_t n, const double *__restrict__ nnz,
                              const T *__restrict__ leafsum, int64_t max_leaves, int64_t n_genes,
                              T *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t g = t >> 1;
    if (g >= n_genes) return;
    const int square = (int)(t & 1);
    const uint32_t cnt = (uint32_t)nnz[g];
    const T inv_n = (T)(1.0 / (double)n);
    T res = (T)0;
    if (cnt >= 1) {
        T x = comp[g * n];
        if (square) x = x * x;
        res = x * inv_n;
        if (cnt >= 2) {
            const T *ls = leafsum + (g * 2 + square) * max_leaves;
            uint32_t k = 0;
            res = res + pw_walk<T>(cnt - 1, [&](uint32_t, uint32_t) { return ls[k++]; });
        }
    }
    out[t] = res;
}

// mean32 / sd32 exactly as AC:821-830: var = sqmean - mean^2 and sqrt in the matrix dtype T, then float32
template <typename T>
__global__ void k_lm_stats(const T *__restrict__ stats, float *__restrict__ mean32, float *__restrict__ sd32,
                           unsigned char *__restrict__ zero, int64_t n_genes, int64_t total)
{
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    if (g >= n_genes) { mean32[g] = 0.f; sd32[g] = 1.f; zero[g] = 1; return; }
    const T m = stats[2 * g], q = stats[2 * g + 1];
    const T var = q - m * m;
    // sqrt in double, rounded once: correctly rounded for a float operand (53 >= 2*24 + 2 bits); the
    // hardware v_sqrt_f32 alone is a 1-ulp approximation
    const float sd = (float)__dsqrt_rn((double)var);
    const bool z = (sd == 0.0f);
    mean32[g] = (float)m;
    sd32[g] = z ? 1.0f : sd;
    zero[g] = z ? 1 : 0;
}

// observed: lag = W32 @ Z32 (row-sequential float32, mul and add rounded separately), I = Z * lag
__global__ __launch_bounds__(256) void k_lm_observed(const long long *__restrict__ indptr,
                                                     const int32_t *__restrict__ indices,
                                                     const double *__restrict__ w, const float *__restrict__ Z32,
                                                     float *__restrict__ Lag32, float *__restrict__ I32, int64_t n)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t i = t >> 2;
    int q = (int)(t & 3);
    if (i >= n) return;
    const float4 *Zt = reinterpret_cast<const float4 *>(Z32 + (int64_t)blockIdx.y * n * SC_TILE) + q;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long e = indptr[i]; e < indptr[i + 1]; ++e) {
        const float ww = (float)w[e];
        const float4 z = Zt[(int64_t)indices[e] * 4];
        s.x = __fadd_rn(s.x, __fmul_rn(ww, z.x)); s.y = __fadd_rn(s.y, __fmul_rn(ww, z.y));
        s.z = __fadd_rn(s.z, __fmul_rn(ww, z.z)); s.w = __fadd_rn(s.w, __fmul_rn(ww, z.w));
    }
    const float4 zi = Zt[i * 4];
    const int64_t o = (int64_t)blockIdx.y * n * 4 + i * 4 + q;
    reinterpret_cast<float4 *>(Lag32)[o] = s;
    reinterpret_cast<float4 *>(I32)[o] =
        make_float4(__fmul_rn(zi.x, s.x), __fmul_rn(zi.y, s.y), __fmul_rn(zi.z, s.z), __fmul_rn(zi.w, s.w));
}

// ---- count[i][g] += #{p : |Z[perm_p[i]] * sum_e w_e Z[perm_p[col_e]]| >= |I[i]|}, in two phases per batch of
// permutations, in the graph's processing order (r02) ----
// A one-kernel form (r01) read, per permutation and cell, k + 1 permutation indices and k + 1 random 64-byte z rows
// per gene tile.  Per cell i the permuted vector y = z[perm] is all that matters: I_perm[i] = y[i] * sum_e w_e y[col_e].
// Phase A materialises y once per (permutation, tile) -- ONE random row per cell -- at the cell's position r in a
// spatially sorted order (Ys[r] = Z[perm[order[r]]]); phase B is then a LOCAL sparse product: the neighbours of a cell
// sit at nearby positions, their rows are served by L1 / L2.  The edges of a row keep their ascending-column order,
// so every sum is the reference's row-sequential float32 sum, bit for bit.
// (LM_PERM_BATCH permutations per launch: sc_local.h)

// Ys[p][tile][r][16] = Z32[tile][perm_p[order[r]]][16]      thread = (r, q), grid.y = tile, grid.z = permutation of the batch
__global__ __launch_bounds__(256) void k_lm_gather_sorted(const float *__restrict__ Z32, const int32_t *__restrict__ order,
                                                          const int32_t *__restrict__ perm, int64_t pstride, int64_t n,
                                                          int64_t tiles, float *__restrict__ Ys)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 2;
    const int q = (int)(t & 3);
    if (r >= n) return;
    const int32_t src = perm[(int64_t)blockIdx.z * pstride + order[r]];
    const float4 v = reinterpret_cast<const float4 *>(Z32 + (int64_t)blockIdx.y * n * SC_TILE)[(int64_t)src * 4 + q];
    reinterpret_cast<float4 *>(Ys + ((int64_t)blockIdx.z * tiles + blockIdx.y) * n * SC_TILE)[r * 4 + q] = v;
}

// count[tile][cell][16] += #{p in batch : |y[r] * sum_e w_e y[rank(col_e)]| >= |I[cell]|},  cell = order[r]
// The edge loop is the OUTER loop and the batch's permutations the (unrolled) inner one: the LM_PERM_BATCH row loads of
// an edge are independent and in flight together (with the permutations outside, every row load waited for the
// previous one: 6.4 ms per launch at 2.9 TB/s of fabric traffic, latency-bound), and an edge's index and weight are
// read once per batch.  Per permutation the terms are still added in the row's edge order: the reference's sum.
// (An XCD-contiguous block order was measured too: 7.6 ms instead of 6.4 with the old loop order; not kept.)
__global__ __launch_bounds__(256) void k_lm_count_sorted(const long long *__restrict__ indptr,
                                                         const int32_t *__restrict__ indices_r,
                                                         const float *__restrict__ w32, const int32_t *__restrict__ order,
                                                         const float *__restrict__ Ys, const float *__restrict__ I32,
                                                         int n_batch, int64_t tiles, int32_t *__restrict__ count, int64_t n,
                                                         int first)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 2;
    const int q = (int)(t & 3);
    if (r >= n) return;
    const int64_t i = order[r];
    const int64_t o = (int64_t)blockIdx.y * n * 4 + i * 4 + q;
    const float4 obs = reinterpret_cast<const float4 *>(I32)[o];
    const float ax = fabsf(obs.x), ay = fabsf(obs.y), az = fabsf(obs.z), aw = fabsf(obs.w);
    const long long e0 = indptr[i], e1 = indptr[i + 1];
    const int64_t pstep = tiles * n * 4;   // float4 stride between the permutations of the batch
    const float4 *Y0 = reinterpret_cast<const float4 *>(Ys + (int64_t)blockIdx.y * n * SC_TILE) + q;
    float4 s[LM_PERM_BATCH];
#pragma unroll
    for (int p = 0; p < LM_PERM_BATCH; ++p) s[p] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long e = e0; e < e1; ++e) {
        const float ww = w32[e];
        const float4 *Ye = Y0 + (int64_t)indices_r[e] * 4;
#pragma unroll
        for (int p = 0; p < LM_PERM_BATCH; ++p) {
            if (p < n_batch) {
                const float4 z = Ye[p * pstep];
                s[p].x = __fadd_rn(s[p].x, __fmul_rn(ww, z.x)); s[p].y = __fadd_rn(s[p].y, __fmul_rn(ww, z.y));
                s[p].z = __fadd_rn(s[p].z, __fmul_rn(ww, z.z)); s[p].w = __fadd_rn(s[p].w, __fmul_rn(ww, z.w));
            }
        }
    }
    int cx = 0, cy = 0, cz = 0, cw = 0;
#pragma unroll
    for (int p = 0; p < LM_PERM_BATCH; ++p) {
        if (p < n_batch) {
            const float4 zi = Y0[r * 4 + p * pstep];
            cx += fabsf(__fmul_rn(zi.x, s[p].x)) >= ax; cy += fabsf(__fmul_rn(zi.y, s[p].y)) >= ay;
            cz += fabsf(__fmul_rn(zi.z, s[p].z)) >= az; cw += fabsf(__fmul_rn(zi.w, s[p].w)) >= aw;
        }
    }
    int4 *dst = reinterpret_cast<int4 *>(count) + o;
    if (first) *dst = make_int4(cx, cy, cz, cw);
    else { const int4 c0 = *dst; *dst = make_int4(c0.x + cx, c0.y + cy, c0.z + cz, c0.w + cw); }
}

// ---- the two phases over CODE rows (r03): count data, every value an integer in [0, LM_CODES) ----
// A gene with few distinct values has few distinct z: z = table[gene][value].  The permuted matrix of a batch is then
// moved around as the uint8 rows of the scoring kernel's narrow copy (128 genes per 128-byte row instead of 16 per
// 64-byte float tile row: an eighth of the gathered, written and re-read bytes), and the float32 z of a neighbour is
// looked up in LDS when it is used.  table[gene][v] is k_lm_standardize's own expression at x = v, so every product
// and every sum is the float path's, bit for bit.  With all weights equal (a row-normalised kNN graph) a second table
// holds w * z, the product the float path rounds before it adds.
// (LM_CODES values, LM_TAB_STRIDE floats per table row, quads of LM_U8_QUAD and launches of LM_U8_BATCH_MAX permutations: sc_local.h)

// table rows in the order the kernel's threads use them: row = 8 b + q holds the gene of byte b of lane q's 16 bytes
// of a narrow row (k_pack_narrow<8>: tile 8 grp + b / 2, slot 2 q + b % 2);  tab[0] = z, tab[1] = w z
__global__ __launch_bounds__(256) void k_lm_ztab(const float *__restrict__ mean32, const float *__restrict__ sd32,
                                                 int64_t tiles16, float w, float *__restrict__ tab, int groups)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= groups * 128 * LM_TAB_STRIDE) return;
    const int v = t % LM_TAB_STRIDE, row = (t / LM_TAB_STRIDE) % 128, grp = t / (LM_TAB_STRIDE * 128);
    const int b = row >> 3, q = row & 7;
    const int64_t tile = 8 * (int64_t)grp + (b >> 1);
    float z = 0.f;
    if (tile < tiles16 && v < LM_CODES) {
        const int64_t g = tile * SC_TILE + 2 * q + (b & 1);
        z = (float)__ddiv_rn((double)__fsub_rn((float)v, mean32[g]), (double)sd32[g]);
    }
    tab[t] = z;
    tab[(size_t)groups * 128 * LM_TAB_STRIDE + t] = __fmul_rn(w, z);
}

// Ys8[p][grp][r] = X8[grp][perm_p[order[r]]]   thread = (r, q), grid.y = group, grid.z = permutation of the batch
__global__ __launch_bounds__(256) void k_lm_gather_u8(const uint4 *__restrict__ X8, const int32_t *__restrict__ order,
                                                      const int32_t *__restrict__ perm, int64_t pstride, int64_t n,
                                                      int groups, uint4 *__restrict__ Ys8)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 3;
    const int q = (int)(t & 7);
    if (r >= n) return;
    const int32_t src = perm[(int64_t)blockIdx.z * pstride + order[r]];
    Ys8[(((int64_t)blockIdx.z * groups + blockIdx.y) * n + r) * 8 + q] = X8[((int64_t)blockIdx.y * n + src) * 8 + q];
}

// count[tile][cell][16] += #{p in batch : |y[r] * sum_e w_e y[rank(col_e)]| >= |I[cell]|}, y = table[code], cell = order[r]
// thread = (r, q): the 16 genes of lane q's 16 bytes, LM_U8_QUAD permutations at a time; edges in the row's order.
template <bool UNI>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(UNI ? 4 : 3, 4))) void k_lm_count_u8(const long long *__restrict__ indptr,
                                                     const int32_t *__restrict__ indices_r, const float *__restrict__ w32,
                                                     const int32_t *__restrict__ order, const uint4 *__restrict__ Ys8,
                                                     const float *__restrict__ I32, const float *__restrict__ tab,
                                                     int n_batch, int64_t tiles, int groups, int32_t *__restrict__ count,
                                                     int64_t n, int first)
{
    __shared__ float tz[128 * LM_TAB_STRIDE];
    __shared__ float tw[UNI ? 128 * LM_TAB_STRIDE : 1];
    const int grp = blockIdx.y;
    for (int k = threadIdx.x; k < 128 * LM_TAB_STRIDE; k += 256) {
        tz[k] = tab[(size_t)grp * 128 * LM_TAB_STRIDE + k];
        if (UNI) tw[k] = tab[((size_t)groups + grp) * 128 * LM_TAB_STRIDE + k];
    }
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 3;
    const int q = (int)(t & 7);
    if (r >= n) return;
    const int64_t i = order[r];
    float a[16];
    uint32_t cnt[4] = {0u, 0u, 0u, 0u};   // 16 counts of <= LM_U8_BATCH_MAX, 8 bits each
    static_assert(LM_U8_BATCH_MAX < 256, "packed per-launch counts");
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        const int64_t tile = 8 * (int64_t)grp + (b >> 1);
        a[b] = tile < tiles ? fabsf(I32[tile * n * SC_TILE + i * SC_TILE + 2 * q + (b & 1)]) : 0.f;
    }
    const long long e0 = indptr[i], e1 = indptr[i + 1];
    const int64_t pstep = (int64_t)groups * n * 8;   // uint4 stride between the permutations of the batch
    const uint4 *Y0 = Ys8 + (int64_t)grp * n * 8 + q;
    const float *zq = tz + q * LM_TAB_STRIDE;         // + b * 8 * LM_TAB_STRIDE + value
    const float *wq = (UNI ? tw : tz) + q * LM_TAB_STRIDE;
    typedef float v2f __attribute__((ext_vector_type(2)));   // two genes per v_pk_add_f32 / v_pk_mul_f32: IEEE per component
    for (int p0 = 0; p0 < n_batch; p0 += LM_U8_QUAD) {
        v2f s[LM_U8_QUAD][8];
#pragma unroll
        for (int p = 0; p < LM_U8_QUAD; ++p)
#pragma unroll
            for (int b = 0; b < 8; ++b) s[p][b] = (v2f){0.f, 0.f};
        for (long long e = e0; e < e1; ++e) {
            const float ww = w32[e];
            const v2f ww2 = {ww, ww};
            const uint4 *Ye = Y0 + (int64_t)indices_r[e] * 8 + (int64_t)p0 * pstep;
            uint4 row[LM_U8_QUAD];
#pragma unroll
            for (int p = 0; p < LM_U8_QUAD; ++p) row[p] = p0 + p < n_batch ? Ye[p * pstep] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int p = 0; p < LM_U8_QUAD; ++p) {
                const uint32_t wd[4] = {row[p].x, row[p].y, row[p].z, row[p].w};
#pragma unroll
                for (int b = 0; b < 16; b += 2) {
                    const uint32_t v0 = (wd[b >> 2] >> (8 * (b & 3))) & 0xffu, v1 = (wd[b >> 2] >> (8 * (b & 3) + 8)) & 0xffu;
                    v2f term = {wq[b * 8 * LM_TAB_STRIDE + v0], wq[(b + 1) * 8 * LM_TAB_STRIDE + v1]};
                    if (!UNI) term = ww2 * term;          // (-ffp-contract=off: product and sum are rounded separately)
                    s[p][b >> 1] = s[p][b >> 1] + term;
                }
            }
        }
#pragma unroll
        for (int p = 0; p < LM_U8_QUAD; ++p) {
            if (p0 + p < n_batch) {
                const uint4 own = Y0[r * 8 + (int64_t)(p0 + p) * pstep];
                const uint32_t wd[4] = {own.x, own.y, own.z, own.w};
#pragma unroll
                for (int b = 0; b < 16; b += 2) {
                    const uint32_t v0 = (wd[b >> 2] >> (8 * (b & 3))) & 0xffu, v1 = (wd[b >> 2] >> (8 * (b & 3) + 8)) & 0xffu;
                    const v2f zi = {zq[b * 8 * LM_TAB_STRIDE + v0], zq[(b + 1) * 8 * LM_TAB_STRIDE + v1]};
                    const v2f ip = zi * s[p][b >> 1];
                    cnt[b >> 2] += (fabsf(ip.x) >= a[b] ? 1u : 0u) << (8 * (b & 3));
                    cnt[b >> 2] += (fabsf(ip.y) >= a[b + 1] ? 1u : 0u) << (8 * (b & 3) + 8);
                }
            }
        }
    }
#pragma unroll
    for (int tt = 0; tt < 8; ++tt) {
        const int64_t tile = 8 * (int64_t)grp + tt;
        if (tile >= tiles) continue;
        int2 *dst = reinterpret_cast<int2 *>(count + tile * n * SC_TILE + i * SC_TILE + 2 * q);
        const int ca = (int)((cnt[tt >> 1] >> (16 * (tt & 1))) & 0xffu), cb = (int)((cnt[tt >> 1] >> (16 * (tt & 1) + 8)) & 0xffu);
        if (first) *dst = make_int2(ca, cb);
        else { const int2 c0 = *dst; *dst = make_int2(c0.x + ca, c0.y + cb); }
    }
}

// tile layout [tile][cell][16] -> row-major [cell][n_genes]
template <typename T>
__global__ __launch_bounds__(256) void k_untile(const T *__restrict__ tiles, T *__restrict__ out, int64_t n,
                                                int64_t n_genes)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * n_genes) return;
    int64_t i = t / n_genes, g = t - i * n_genes;
    out[t] = tiles[(g >> 4) * n * SC_TILE + i * SC_TILE + (g & 15)];
}

// Is every loaded value an integer in [0, LM_CODES)?  (one pass over the tiles + one synchronisation; SC_LM_FLOAT_ROWS
// set: development switch, the float-row form for A/B runs and tests)
static int lm_codes_ok(sc_ctx *c, bool *ok)
{
    *ok = false;
    if (getenv("SC_LM_FLOAT_ROWS") || c->e_n >= ((int64_t)1 << 24)) return SC_OK;   // (16.7M cells: 2 GB of code rows per permutation and group)
    const int64_t G = c->e_genes, Gpad = align_up64(c->e_tiles, 8) * SC_TILE;
    SC_TRY(expr_gene_stats(c));
    std::vector<uint32_t> flags((size_t)Gpad), xmax((size_t)Gpad);
    SC_HIP(hipMemcpyAsync(flags.data(), c->g_flags.p, sizeof(uint32_t) * (size_t)Gpad, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipMemcpyAsync(xmax.data(), c->g_xmax.p, sizeof(uint32_t) * (size_t)Gpad, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    for (int64_t g = 0; g < G; ++g)
        if ((flags[(size_t)g] & 1u) || xmax[(size_t)g] >= LM_CODES) return SC_OK;
    *ok = true;
    return SC_OK;
}

// statistics in numpy's order, z, observed lag and I; then the form of the permutation counts and its buffers
int lm_prepare(sc_ctx *c, int64_t n_perm, LmJob &j)
{
    const int64_t n = c->e_n, G = c->e_genes, T = c->e_tiles;
    c->lm_valid = false;
    const size_t tile_f = (size_t)T * n * SC_TILE;
    // per-gene mean and E[x^2] with numpy's own summation order, in the matrix dtype (see k_npc_*)
    SC_TRY(expr_colsum(c, OP_NZ, c->X.as<double>(), nullptr, c->g_Inum.as<double>(), 1.0));
    SC_TRY(c->lee_out.ensure(sizeof(double) * 2 * (size_t)(T * SC_TILE), &c->mem));
    {
        const int64_t nblk = ceil_div64(n, NPC_CELLS), max_leaves = n / 32 + 64;
        const size_t tsz = c->e_dtype == SC_F32 ? sizeof(float) : sizeof(double);
        SC_TRY(c->np_cnt.ensure(sizeof(uint32_t) * (size_t)(T * nblk * 16), &c->mem));
        SC_TRY(c->np_comp.ensure(tsz * (size_t)(T * SC_TILE) * (size_t)n, &c->mem));
        SC_TRY(c->np_leaves.ensure(sizeof(uint2) * (size_t)G * (size_t)max_leaves + sizeof(uint32_t) * (size_t)G, &c->mem));
        SC_TRY(c->np_leafsum.ensure(tsz * 2 * (size_t)G * (size_t)max_leaves, &c->mem));
        uint2 *leaves = c->np_leaves.as<uint2>();
        uint32_t *nleaves = reinterpret_cast<uint32_t *>(leaves + (size_t)G * (size_t)max_leaves);
        const dim3 gw((unsigned)ceil_div64(nblk, 4), (unsigned)T);
        hipLaunchKernelGGL(k_npc_count, gw, dim3(256), 0, c->stream, c->X.as<double>(), n, nblk, c->np_cnt.as<uint32_t>());
        hipLaunchKernelGGL(k_npc_offsets, dim3((unsigned)ceil_div64(T * SC_TILE, 64)), dim3(64), 0, c->stream,
                           c->np_cnt.as<uint32_t>(), nblk, T * SC_TILE);
        hipLaunchKernelGGL(k_npc_leaves, dim3((unsigned)ceil_div64(G, 64)), dim3(64), 0, c->stream,
                           c->g_Inum.as<double>(), G, max_leaves, leaves, nleaves);
        const dim3 gl((unsigned)ceil_div64(max_leaves, 256), (unsigned)G, 2);
        if (c->e_dtype == SC_F32) {
            hipLaunchKernelGGL(k_npc_scatter<float>, gw, dim3(256), 0, c->stream, c->X.as<double>(), n, nblk,
                               c->np_cnt.as<uint32_t>(), c->np_comp.as<float>());
            hipLaunchKernelGGL(k_npc_leafsum<float>, gl, dim3(256), 0, c->stream, c->np_comp.as<float>(), n, leaves,
                               nleaves, max_leaves, c->np_leafsum.as<float>());
            hipLaunchKernelGGL(k_npc_combine<float>, dim3((unsigned)ceil_div64(2 * G, 64)), dim3(64), 0, c->stream,
                               c->np_comp.as<float>(), n, c->g_Inum.as<double>(), c->np_leafsum.as<float>(), max_leaves, G,
                               c->lee_out.as<float>());
        } else {
            hipLaunchKernelGGL(k_npc_scatter<double>, gw, dim3(256), 0, c->stream, c->X.as<double>(), n, nblk,
                               c->np_cnt.as<uint32_t>(), c->np_comp.as<double>());
            hipLaunchKernelGGL(k_npc_leafsum<double>, gl, dim3(256), 0, c->stream, c->np_comp.as<double>(), n, leaves,
                               nleaves, max_leaves, c->np_leafsum.as<double>());
            hipLaunchKernelGGL(k_npc_combine<double>, dim3((unsigned)ceil_div64(2 * G, 64)), dim3(64), 0, c->stream,
                               c->np_comp.as<double>(), n, c->g_Inum.as<double>(), c->np_leafsum.as<double>(), max_leaves,
                               G, c->lee_out.as<double>());
        }
        SC_HIP(hipGetLastError());
    }
    // float work buffers: [mean32 | sd32] in g_scale (as float), zero flags in counts, Z32/Lag32/I32 in Z/Lag
    SC_TRY(c->Z.ensure(tile_f * sizeof(double), &c->mem));    // Z32 (first half) + I32 (second half)
    SC_TRY(c->Lag.ensure(tile_f * sizeof(double), &c->mem));  // Lag32 (first half) + counts (second half)
    SC_TRY(c->counts.ensure((size_t)T * SC_TILE + 16, &c->mem));
    float *mean32 = c->g_scale.as<float>(), *sd32 = mean32 + T * SC_TILE;
    float *Z32 = c->Z.as<float>(), *I32 = Z32 + tile_f;
    float *Lag32 = c->Lag.as<float>();
    int32_t *cnt = reinterpret_cast<int32_t *>(Lag32 + tile_f);
    unsigned char *zero = c->counts.as<unsigned char>();
    if (c->e_dtype == SC_F32)
        hipLaunchKernelGGL(k_lm_stats<float>, dim3((unsigned)ceil_div64(T * SC_TILE, 256)), dim3(256), 0, c->stream,
                           c->lee_out.as<float>(), mean32, sd32, zero, G, T * SC_TILE);
    else
        hipLaunchKernelGGL(k_lm_stats<double>, dim3((unsigned)ceil_div64(T * SC_TILE, 256)), dim3(256), 0, c->stream,
                           c->lee_out.as<double>(), mean32, sd32, zero, G, T * SC_TILE);
    dim3 ge((unsigned)ceil_div64(n * SC_TILE, 256), (unsigned)T);
    hipLaunchKernelGGL(k_lm_standardize, ge, dim3(256), 0, c->stream, c->X.as<double>(), mean32, sd32, Z32, n);
    dim3 gc((unsigned)ceil_div64(n * 4, 256), (unsigned)T);
    hipLaunchKernelGGL(k_lm_observed, gc, dim3(256), 0, c->stream, c->g_indptr.as<long long>(),
                       c->g_indices.as<int32_t>(), c->g_data.as<double>(), Z32, Lag32, I32, n);
    SC_HIP(hipGetLastError());
    j.n = n; j.G = G; j.T = T; j.tile_f = tile_f;
    j.mean32 = mean32; j.sd32 = sd32; j.Z32 = Z32; j.I32 = I32; j.Lag32 = Lag32; j.cnt = cnt; j.zero = zero; j.gc = gc;
    if (n_perm <= 0) return SC_OK;
    SC_TRY(sc_graph_ensure_order(c));
    bool codes = false;
    SC_TRY(lm_codes_ok(c, &codes));
    if (codes) {
        // count data: the permuted matrix travels as uint8 code rows, z is looked up where it is used (k_lm_count_u8)
        j.mode = 1;
        j.groups = (int)ceil_div64(T, 8);
        const size_t row_bytes = (size_t)j.groups * (size_t)n * 128;
        SC_TRY(c->lm_tab.ensure(sizeof(float) * 2 * (size_t)j.groups * 128 * LM_TAB_STRIDE, &c->mem));
        int64_t batch = (int64_t)(((size_t)4 << 30) / row_bytes) / LM_U8_QUAD * LM_U8_QUAD;
        batch = batch < LM_U8_QUAD ? LM_U8_QUAD : batch > LM_U8_BATCH_MAX ? LM_U8_BATCH_MAX : batch;
        if (batch > n_perm) batch = align_up64(n_perm, LM_U8_QUAD);
        j.batch = batch;
        SC_TRY(c->lm_ys.ensure(row_bytes * (size_t)batch, &c->mem));
        SC_TRY(expr_pack_narrow(c, 8));
        j.uni = c->g_uniform_w > 0.0;
        hipLaunchKernelGGL(k_lm_ztab, dim3((unsigned)ceil_div64((int64_t)j.groups * 128 * LM_TAB_STRIDE, 256)), dim3(256), 0, c->stream,
                           mean32, sd32, T, j.uni ? (float)c->g_uniform_w : 0.f, c->lm_tab.as<float>(), j.groups);
        SC_HIP(hipGetLastError());
    } else {
        j.mode = 2;
        j.batch = LM_PERM_BATCH;
        SC_TRY(c->lm_ys.ensure(sizeof(float) * (size_t)LM_PERM_BATCH * tile_f, &c->mem));
    }
    return SC_OK;
}

// phase A of permutations [row, row + nb) of the forward table: the permuted rows of the batch, in the job's form
void lm_gather(sc_ctx *c, const LmJob &j, int64_t row, int nb)
{
    const int64_t n = j.n;
    if (j.mode == 1)
        hipLaunchKernelGGL(k_lm_gather_u8, dim3((unsigned)ceil_div64(n * 8, 256), (unsigned)j.groups, (unsigned)nb), dim3(256), 0,
                           c->stream, c->X32.as<uint4>(), c->g_order.as<int32_t>(), c->perm.as<int32_t>() + row * c->p_stride,
                           c->p_stride, n, j.groups, c->lm_ys.as<uint4>());
    else
        hipLaunchKernelGGL(k_lm_gather_sorted, dim3(j.gc.x, (unsigned)j.T, (unsigned)nb), dim3(256), 0, c->stream, j.Z32,
                           c->g_order.as<int32_t>(), c->perm.as<int32_t>() + row * c->p_stride, c->p_stride, n, j.T,
                           c->lm_ys.as<float>());
}

// counts of permutations [p0, p1) of the job (rows row0 + p of the forward table); p0 == 0 starts the counts
static int lm_count(sc_ctx *c, const LmJob &j, int64_t row0, int64_t p0, int64_t p1)
{
    const int64_t n = j.n, T = j.T;
    if (p1 <= p0) return SC_OK;
    KernelTimerScope ts(c, SC_K_LEE_PERM);
    const dim3 g8((unsigned)ceil_div64(n * 8, 256), (unsigned)j.groups);
    auto count_u8 = j.uni ? k_lm_count_u8<true> : k_lm_count_u8<false>;
    for (int64_t p = p0; p < p1; p += j.batch) {
        const int nb = (int)(p1 - p < j.batch ? p1 - p : j.batch);
        lm_gather(c, j, row0 + p, nb);
        if (j.mode == 1)
            hipLaunchKernelGGL(count_u8, g8, dim3(256), 0, c->stream, c->g_indptr.as<long long>(),
                               c->g_indices_r.as<int32_t>(), c->g_w32.as<float>(), c->g_order.as<int32_t>(),
                               c->lm_ys.as<uint4>(), j.I32, c->lm_tab.as<float>(), nb, T, j.groups, j.cnt, n, p == 0 ? 1 : 0);
        else
            hipLaunchKernelGGL(k_lm_count_sorted, j.gc, dim3(256), 0, c->stream, c->g_indptr.as<long long>(),
                               c->g_indices_r.as<int32_t>(), c->g_w32.as<float>(), c->g_order.as<int32_t>(),
                               c->lm_ys.as<float>(), j.I32, nb, T, j.cnt, n, p == 0 ? 1 : 0);
    }
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// z / lag / I of the job, each un-tiled into the row-major (cells x genes) staging buffer and copied out on stream s
int lm_copy_arrays(const LmJob &j, float *stage, hipStream_t s, bool sync_each, float *z_out, float *lag_out, float *I_out)
{
    const unsigned gu = (unsigned)ceil_div64(j.n * j.G, 256);
    const struct { const float *src; float *dst; } outs[3] = {{j.Z32, z_out}, {j.Lag32, lag_out}, {j.I32, I_out}};
    for (const auto &o : outs) {
        hipLaunchKernelGGL(k_untile<float>, dim3(gu), dim3(256), 0, s, o.src, stage, j.n, j.G);
        SC_HIP(hipMemcpyAsync(o.dst, stage, sizeof(float) * (size_t)j.n * (size_t)j.G, hipMemcpyDeviceToHost, s));
        if (sync_each) SC_HIP(hipStreamSynchronize(s));
    }
    return SC_OK;
}

// un-tile into row-major (cells x genes) staging and copy back
static int lm_finish(sc_ctx *c, const LmJob &j, int64_t n_perm, float *z_out, float *lag_out, float *I_out,
                     int32_t *count_out, uint8_t *zero_var_out, bool arrays_done = false)
{
    const int64_t n = j.n, G = j.G;
    const bool counts = n_perm > 0 && count_out;
    if (!arrays_done || counts) SC_TRY(c->lee_a.ensure(sizeof(float) * (size_t)n * (size_t)G, &c->mem));   // (staging)
    unsigned gu = (unsigned)ceil_div64(n * G, 256);
    // (arrays_done: a helper thread has copied them out beside the pipeline)
    if (!arrays_done) SC_TRY(lm_copy_arrays(j, c->lee_a.as<float>(), c->stream, false, z_out, lag_out, I_out));
    if (counts) {
        hipLaunchKernelGGL(k_untile<int32_t>, dim3(gu), dim3(256), 0, c->stream, j.cnt, c->lee_a.as<int32_t>(), n, G);
        SC_HIP(hipMemcpyAsync(count_out, c->lee_a.p, sizeof(int32_t) * (size_t)n * (size_t)G, hipMemcpyDeviceToHost,
                              c->stream));
    }
    if (zero_var_out)
        SC_HIP(hipMemcpyAsync(zero_var_out, j.zero, (size_t)G, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipGetLastError());
    SC_HIP(hipStreamSynchronize(c->stream));
    c->lm_valid = true;  // z / lag / counts stay resident for sc_local_moran_hist / sc_local_moran_classify
    c->lm_stat = LM_STAT_MORAN;
    c->lm_perms = n_perm;
    return SC_OK;
}

extern "C" int sc_local_moran(sc_ctx *c, int64_t n_perm, int64_t perm_row0, float *z_out, float *lag_out,
                              float *I_out, int32_t *count_out, uint8_t *zero_var_out)
{
    SC_REQUIRE(c && z_out && lag_out && I_out, SC_ERR_INVALID, "sc_local_moran: null pointer");
    SC_REQUIRE(n_perm >= 0 && perm_row0 >= 0, SC_ERR_INVALID, "sc_local_moran: negative size");
    SC_HIP(hipSetDevice(c->device));
    if (n_perm > 0) SC_TRY(sc_perm_forward_ensure(c));
    SC_REQUIRE(c->e_n > 0, SC_ERR_STATE, "sc_local_moran: no expression loaded");
    SC_REQUIRE(c->g_n == c->e_n, SC_ERR_STATE, "sc_local_moran: graph missing or size mismatch");
    c->lm_valid = false;
    if (n_perm > 0) {
        SC_REQUIRE(c->p_n == c->e_n && perm_row0 + n_perm <= c->p_count, SC_ERR_STATE,
                   "sc_local_moran: needs permutation rows [%lld, %lld) of length %lld", (long long)perm_row0,
                   (long long)(perm_row0 + n_perm), (long long)c->e_n);
    }
    LmJob j;
    SC_TRY(lm_prepare(c, n_perm, j));
    SC_TRY(lm_count(c, j, perm_row0, 0, n_perm));
    return lm_finish(c, j, n_perm, z_out, lag_out, I_out, count_out, zero_var_out);
}

// A thread that is joined when it is destroyed (C++17 has no std::jthread)
struct JoiningThread {
    std::thread t;
    ~JoiningThread() { if (t.joinable()) t.join(); }
};

// A job as one pipeline behind the generator (sc_local.h): n_perm numpy-exact permutations of the cells from state6 (as
// sc_perm_generate would draw them; state6 is advanced the same way, the table stays resident), generated chunk by chunk
// while the per-cell counts of the finished chunks are taken -- the generator's chain is the longest part of a call, and
// the counts hide behind it.
int lm_seeded_pipeline(sc_ctx *c, const char *who, uint64_t *state6, int64_t n_perm, LmJob &j,
                       const std::function<int(const LmJob &)> &observed,
                       const std::function<int(const LmJob &, int64_t, int64_t)> &count, float *z_out, float *lag_out,
                       float *I_out, bool *arrays_done)
{
    // r04: z, lag and I are final once the preparation has run -- three (cells x genes) float arrays, 1.2 GB at 10^6 cells x
    // 100 genes, that r03 copied to the caller's (pageable) arrays AFTER the last count, 0.1 s of a 0.5-s call.  A helper
    // thread un-tiles and copies them out on a stream of its own while the generator and the counts run (neither uses
    // the PCIe link); this thread keeps enqueuing the pipeline.
    int copier_rc = SC_OK;
    std::optional<JoiningThread> copier;   // (declared after what its thread writes; reset() joins)
    bool copier_started = false;
    *arrays_done = false;
    auto prepare = [&]() -> int {
        SC_TRY(lm_prepare(c, n_perm, j));
        if (observed) SC_TRY(observed(j));
        if (copier_started) return SC_OK;
        if (!c->stream_out) SC_HIP(hipStreamCreateWithFlags(&c->stream_out, hipStreamNonBlocking));
        SC_TRY(c->lm_out.ensure(sizeof(float) * (size_t)j.n * (size_t)j.G, &c->mem));
        hipEvent_t ready;
        SC_HIP(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
        SC_HIP(hipEventRecord(ready, c->stream));
        SC_HIP(hipStreamWaitEvent(c->stream_out, ready, 0));
        SC_HIP(hipEventDestroy(ready));
        const LmJob jj = j;
        try {   // (no thread to be had: the arrays are copied at the end, as in r03)
            copier.emplace().t = std::thread([c, jj, z_out, lag_out, I_out, &copier_rc]() {
            if (hipSetDevice(c->device) != hipSuccess) { copier_rc = SC_ERR_HIP; return; }
            // (a synchronisation per array: the staging buffer is reused by the next one)
            copier_rc = lm_copy_arrays(jj, c->lm_out.as<float>(), c->stream_out, true, z_out, lag_out, I_out);
            });
            copier_started = true;
        } catch (...) {
            copier_started = false;
        }
        return SC_OK;
    };
    auto score = [&](int64_t p0, int64_t p1) -> int { return count(j, p0, p1); };
    // a job that fails its verification is rerun with the sequential scan: the counts restart at permutation 0, and the
    // copier is joined first (the second preparation rewrites what it reads -- with the same values)
    const int rc = permgen_rerun_on_failure(
        c, [&]() { return sc_perm_pipeline(c, state6, c->e_n, n_perm, 0, 2, prepare, score); },
        [&]() { copier.reset(); return SC_OK; });
    copier.reset();
    SC_TRY(rc);
    if (copier_started && copier_rc != SC_OK) {
        sc_set_error("%s: the copy of z / lag / the statistic to the host failed", who);
        return copier_rc;
    }
    *arrays_done = copier_started;
    return SC_OK;
}

// sc_local_moran with the permutations drawn here, as one pipeline.  Same outputs as sc_perm_generate + sc_local_moran.
extern "C" int sc_local_moran_seeded(sc_ctx *c, uint64_t *state6, int64_t n_perm, float *z_out, float *lag_out,
                                     float *I_out, int32_t *count_out, uint8_t *zero_var_out)
{
    SC_REQUIRE(c && state6 && z_out && lag_out && I_out, SC_ERR_INVALID, "sc_local_moran_seeded: null pointer");
    SC_REQUIRE(n_perm >= 1 && n_perm <= (1 << 24), SC_ERR_INVALID, "sc_local_moran_seeded: n_perm=%lld out of range", (long long)n_perm);
    SC_HIP(hipSetDevice(c->device));
    SC_REQUIRE(c->e_n > 0, SC_ERR_STATE, "sc_local_moran_seeded: no expression loaded");
    SC_REQUIRE(c->g_n == c->e_n, SC_ERR_STATE, "sc_local_moran_seeded: graph missing or size mismatch");
    c->lm_valid = false;
    LmJob j;
    bool arrays_done = false;
    SC_TRY(lm_seeded_pipeline(c, "sc_local_moran_seeded", state6, n_perm, j, nullptr,
                              [c](const LmJob &job, int64_t p0, int64_t p1) { return lm_count(c, job, 0, p0, p1); }, z_out,
                              lag_out, I_out, &arrays_done));
    return lm_finish(c, j, n_perm, z_out, lag_out, I_out, count_out, zero_var_out, arrays_done);
}

// hist[gene][c] = cells of the gene with permutation count c (LDS-private per workgroup while 16 genes' worth fits)
#define LMH_LDS 12288
__global__ __launch_bounds__(256) void k_lm_hist(const int32_t *__restrict__ cnt, int64_t n, int P1,
                                                 unsigned long long *__restrict__ hist)
{
    __shared__ uint32_t h[LMH_LDS];
    const int64_t tile = blockIdx.y;
    const int32_t *ct = cnt + tile * n * SC_TILE;
    unsigned long long *ht = hist + tile * SC_TILE * P1;
    const bool priv = SC_TILE * P1 <= LMH_LDS;
    if (priv) {
        for (int k = threadIdx.x; k < SC_TILE * P1; k += 256) h[k] = 0;
        __syncthreads();
    }
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n * SC_TILE; t += (int64_t)gridDim.x * 256) {
        int c = ct[t];
        c = c < 0 ? 0 : (c >= P1 ? P1 - 1 : c);
        const int slot = (int)(t & 15);
        if (priv) atomicAdd(&h[slot * P1 + c], 1u);
        else atomicAdd(&ht[slot * P1 + c], 1ull);
    }
    if (priv) {
        __syncthreads();
        for (int k = threadIdx.x; k < SC_TILE * P1; k += 256)
            if (h[k]) atomicAdd(&ht[k], (unsigned long long)h[k]);
    }
}

int lm_hist_run(sc_ctx *c, int64_t *hist_out)
{
    const int64_t n = c->e_n, G = c->e_genes, T = c->e_tiles;
    const int P1 = (int)c->lm_perms + 1;
    const size_t tile_f = (size_t)T * n * SC_TILE;
    const int32_t *cnt = reinterpret_cast<const int32_t *>(c->Lag.as<float>() + tile_f);
    SC_TRY(c->lee_b.ensure(sizeof(unsigned long long) * (size_t)(T * SC_TILE) * (size_t)P1, &c->mem));
    SC_HIP(hipMemsetAsync(c->lee_b.p, 0, sizeof(unsigned long long) * (size_t)(T * SC_TILE) * (size_t)P1, c->stream));
    hipLaunchKernelGGL(k_lm_hist, dim3(256, (unsigned)T), dim3(256), 0, c->stream, cnt, n, P1,
                       c->lee_b.as<unsigned long long>());
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(hist_out, c->lee_b.p, sizeof(int64_t) * (size_t)G * (size_t)P1, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}

extern "C" int sc_local_moran_hist(sc_ctx *c, int64_t *hist_out)
{
    SC_REQUIRE(c && hist_out, SC_ERR_INVALID, "sc_local_moran_hist: null pointer");
    SC_REQUIRE(c->lm_valid && c->lm_stat == LM_STAT_MORAN && c->lm_perms > 0, SC_ERR_STATE,
               "sc_local_moran_hist: no sc_local_moran result with permutations");
    SC_HIP(hipSetDevice(c->device));
    return lm_hist_run(c, hist_out);
}

// p = p_tab[g][count], p_adj = padj_tab[g][count], LISA quadrant (AC:219-265): 1 HH, 2 LL, 3 HL, 4 LH from the signs of
// z and lag, 0 where p_adj >= alpha or the gene is flagged; row-major outputs
__global__ __launch_bounds__(256) void k_lm_classify(const float *__restrict__ Z32, const float *__restrict__ Lag32,
                                                     const int32_t *__restrict__ cnt, int64_t n, int64_t G, int P1,
                                                     const float *__restrict__ p_tab, const float *__restrict__ padj_tab,
                                                     const unsigned char *__restrict__ force_ns, float alpha,
                                                     float *__restrict__ p_out, float *__restrict__ padj_out,
                                                     signed char *__restrict__ q_out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * G) return;
    const int64_t i = t / G, g = t - i * G;
    const int64_t src = (g >> 4) * n * SC_TILE + i * SC_TILE + (g & 15);
    const float z = Z32[src], lag = Lag32[src];
    signed char q = 0;
    if (z > 0.f && lag > 0.f) q = 1;
    if (z < 0.f && lag < 0.f) q = 2;
    if (z > 0.f && lag < 0.f) q = 3;
    if (z < 0.f && lag > 0.f) q = 4;
    if (P1 > 0) {
        int c = cnt[src];
        c = c < 0 ? 0 : (c >= P1 ? P1 - 1 : c);
        const float pa = padj_tab[g * P1 + c];
        p_out[t] = p_tab[g * P1 + c];
        padj_out[t] = pa;
        if (pa >= alpha) q = 0;
    }
    if (force_ns[g]) q = 0;
    q_out[t] = q;
}

int lm_classify_run(sc_ctx *c, const float *p_tab, const float *padj_tab, const uint8_t *force_ns, float *p_out,
                    float *padj_out, int8_t *class_out,
                    const std::function<void(int, const float *, const float *, const unsigned char *, float *, float *,
                                             signed char *)> &classify)
{
    const int64_t n = c->e_n, G = c->e_genes;
    const int P1 = c->lm_perms > 0 ? (int)c->lm_perms + 1 : 0;
    const size_t cells = (size_t)n * (size_t)G;
    // device staging: [p | p_adj | class] row-major, tables, flags
    SC_TRY(c->lee_a.ensure(sizeof(float) * 2 * cells + cells + 64, &c->mem));
    SC_TRY(c->lee_b.ensure(sizeof(float) * 2 * (size_t)G * (size_t)(P1 > 0 ? P1 : 1) + (size_t)G + 64, &c->mem));
    float *d_p = c->lee_a.as<float>(), *d_pa = d_p + cells;
    signed char *d_q = reinterpret_cast<signed char *>(d_pa + cells);
    float *d_pt = c->lee_b.as<float>(), *d_at = d_pt + (size_t)G * (size_t)(P1 > 0 ? P1 : 1);
    unsigned char *d_f = reinterpret_cast<unsigned char *>(d_at + (size_t)G * (size_t)(P1 > 0 ? P1 : 1));
    if (P1 > 0) {
        SC_HIP(hipMemcpyAsync(d_pt, p_tab, sizeof(float) * (size_t)G * P1, hipMemcpyHostToDevice, c->stream));
        SC_HIP(hipMemcpyAsync(d_at, padj_tab, sizeof(float) * (size_t)G * P1, hipMemcpyHostToDevice, c->stream));
    }
    SC_HIP(hipMemcpyAsync(d_f, force_ns, (size_t)G, hipMemcpyHostToDevice, c->stream));
    classify(P1, d_pt, d_at, d_f, d_p, d_pa, d_q);
    SC_HIP(hipGetLastError());
    if (P1 > 0) {
        SC_HIP(hipMemcpyAsync(p_out, d_p, sizeof(float) * cells, hipMemcpyDeviceToHost, c->stream));
        SC_HIP(hipMemcpyAsync(padj_out, d_pa, sizeof(float) * cells, hipMemcpyDeviceToHost, c->stream));
    }
    SC_HIP(hipMemcpyAsync(class_out, d_q, cells, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}

extern "C" int sc_local_moran_classify(sc_ctx *c, const float *p_tab, const float *padj_tab, const uint8_t *force_ns,
                                       float alpha, float *p_out, float *padj_out, int8_t *quadrant_out)
{
    SC_REQUIRE(c && force_ns && quadrant_out, SC_ERR_INVALID, "sc_local_moran_classify: null pointer");
    SC_REQUIRE(c->lm_valid && c->lm_stat == LM_STAT_MORAN, SC_ERR_STATE, "sc_local_moran_classify: no sc_local_moran result");
    SC_HIP(hipSetDevice(c->device));
    const int64_t n = c->e_n, G = c->e_genes, T = c->e_tiles;
    if (c->lm_perms > 0) SC_REQUIRE(p_tab && padj_tab && p_out && padj_out, SC_ERR_INVALID, "sc_local_moran_classify: tables and outputs required with permutations");
    const size_t tile_f = (size_t)T * n * SC_TILE;
    const float *Z32 = c->Z.as<float>(), *Lag32 = c->Lag.as<float>();
    const int32_t *cnt = reinterpret_cast<const int32_t *>(Lag32 + tile_f);
    return lm_classify_run(c, p_tab, padj_tab, force_ns, p_out, padj_out, quadrant_out,
                           [=](int P1, const float *d_pt, const float *d_at, const unsigned char *d_f, float *d_p, float *d_pa,
                               signed char *d_q) {
                               hipLaunchKernelGGL(k_lm_classify, dim3((unsigned)ceil_div64(n * G, 256)), dim3(256), 0, c->stream,
                                                  Z32, Lag32, cnt, n, G, P1, d_pt, d_at, d_f, alpha, d_p, d_pa, d_q);
                           });
}
