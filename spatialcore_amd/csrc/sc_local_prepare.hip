// What the per-cell (LISA) statistics share and no one of them owns: the reference's float32 standardisation, the per-gene
// statistics in numpy's summation order, the observed lag and z lag, the z tables and phase A (the permuted rows of a batch
// of permutations).  The counts, the finalisation and the entry points: sc_local_stats.hip.  gfx950 only.
#include <math.h>
#include <stdlib.h>

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
    SC_TRY(c->scratch_out.ensure(sizeof(double) * 2 * (size_t)(T * SC_TILE), &c->mem));
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
                               c->scratch_out.as<float>());
        } else {
            hipLaunchKernelGGL(k_npc_scatter<double>, gw, dim3(256), 0, c->stream, c->X.as<double>(), n, nblk,
                               c->np_cnt.as<uint32_t>(), c->np_comp.as<double>());
            hipLaunchKernelGGL(k_npc_leafsum<double>, gl, dim3(256), 0, c->stream, c->np_comp.as<double>(), n, leaves,
                               nleaves, max_leaves, c->np_leafsum.as<double>());
            hipLaunchKernelGGL(k_npc_combine<double>, dim3((unsigned)ceil_div64(2 * G, 64)), dim3(64), 0, c->stream,
                               c->np_comp.as<double>(), n, c->g_Inum.as<double>(), c->np_leafsum.as<double>(), max_leaves,
                               G, c->scratch_out.as<double>());
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
    uint32_t *cnt = reinterpret_cast<uint32_t *>(Lag32 + tile_f);
    unsigned char *zero = c->counts.as<unsigned char>();
    if (c->e_dtype == SC_F32)
        hipLaunchKernelGGL(k_lm_stats<float>, dim3((unsigned)ceil_div64(T * SC_TILE, 256)), dim3(256), 0, c->stream,
                           c->scratch_out.as<float>(), mean32, sd32, zero, G, T * SC_TILE);
    else
        hipLaunchKernelGGL(k_lm_stats<double>, dim3((unsigned)ceil_div64(T * SC_TILE, 256)), dim3(256), 0, c->stream,
                           c->scratch_out.as<double>(), mean32, sd32, zero, G, T * SC_TILE);
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
        // count data: the permuted matrix travels as uint8 code rows, z is looked up where it is used (k_local_count_u8)
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
