// The per-cell (LISA) statistics: local Moran's I (the reference's, AC:804-934), Getis-Ord Gi / Gi* and local Geary's C
// (EXTENSIONS: the reference has neither).  Phase B of the per-cell permutation counts -- ONE kernel
// pair, instantiated per statistic --, the finalisation (un-tiling, histogram, classification), the pipeline behind the
// generator and the eight entry points.  Preparation, phase A and the code / float decision: sc_local_prepare.hip.
// gfx950 only.
//
// The counts, one 32-bit word per (cell, gene):
//   local Moran   #{p : |y_i * s_p| >= |I_i|}, s as Getis-Ord's, the cell's own row read after the edge loop; the word is
//                 the whole count (n_perm <= 2^24).
//   the others    ge = #{p : s_p >= s_obs}, le = #{p : s_p <= s_obs}, signed, ge in bits 0 .. 15 and le in bits 16 .. 31
//                 while they are taken (n_perm <= 65535).
//   Getis-Ord   s = row_sequential(y)_i = (((0 + w_e0 y[c_e0]) + w_e1 y[c_e1]) + ...), float32, product and sum rounded
//               separately, edges in stored order; s_obs = lag_i, the same expression on z.
//   Geary       s = sum_e fl(w_e * fl(d * d)), d = fl(y_i - y[c_e]), float32, accumulated in edge order from 0; s_obs = C_i,
//               the same expression on z.
// The standardised Getis-Ord statistic, in float64 from the float32 z_i, lag_i and weights, every operation rounded once
// (-ffp-contract=off, IEEE division and square root), stored as float32:
//   W = sum_e (double)w_e,  S1 = sum_e (double)w_e * (double)w_e      (edges in stored order, from 0)
//   Gi*:  den = sqrt(((n * S1) - (W * W)) / (n - 1));                 G = lag / den
//   Gi:   mi = (-z) / (n - 1);  vi = ((n - (z * z)) / (n - 1)) - (mi * mi);
//         den = sqrt(vi) * sqrt((((n - 1) * S1) - (W * W)) / (n - 2));  G = (lag - (W * mi)) / den
//   G = 0 where den is 0 or not finite.
// Local Geary's null expectation under the full-permutation scheme, float64:
//   E = ((2 * n) / (n - 1)) * sum_{e : c_e != i} (double)w_e          (edges in stored order, from 0)
#include <math.h>

#include <optional>
#include <thread>

#include "sc_ctx.h"
#include "sc_local.h"

// ---- observed values ---------------------------------------------------------------------------------------------------

// C[tile][cell][16] = sum_e fl(w_e * fl(d d)), d = fl(z_i - z_e)       thread = (cell, 4 genes), grid.y = tile
__global__ __launch_bounds__(256) void k_ls_geary_observed(const long long *__restrict__ indptr,
                                                           const int32_t *__restrict__ indices,
                                                           const double *__restrict__ w, const float *__restrict__ Z32,
                                                           float *__restrict__ C32, int64_t n)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = t >> 2;
    const int q = (int)(t & 3);
    if (i >= n) return;
    const float4 *Zt = reinterpret_cast<const float4 *>(Z32 + (int64_t)blockIdx.y * n * SC_TILE) + q;
    const float4 zi = Zt[i * 4];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long e = indptr[i]; e < indptr[i + 1]; ++e) {
        const float ww = (float)w[e];
        const float4 z = Zt[(int64_t)indices[e] * 4];
        const float dx = __fsub_rn(zi.x, z.x), dy = __fsub_rn(zi.y, z.y), dz = __fsub_rn(zi.z, z.z), dw = __fsub_rn(zi.w, z.w);
        s.x = __fadd_rn(s.x, __fmul_rn(ww, __fmul_rn(dx, dx))); s.y = __fadd_rn(s.y, __fmul_rn(ww, __fmul_rn(dy, dy)));
        s.z = __fadd_rn(s.z, __fmul_rn(ww, __fmul_rn(dz, dz))); s.w = __fadd_rn(s.w, __fmul_rn(ww, __fmul_rn(dw, dw)));
    }
    reinterpret_cast<float4 *>(C32)[(int64_t)blockIdx.y * n * 4 + i * 4 + q] = s;
}

__device__ __forceinline__ float ls_getis_value(double z, double lag, double W, double S1, double nn, bool star)
{
    const double ww = __dmul_rn(W, W);
    double num, den;
    if (star) {
        num = lag;
        den = __dsqrt_rn(__ddiv_rn(__dsub_rn(__dmul_rn(nn, S1), ww), nn - 1.0));
    } else {
        const double mi = __ddiv_rn(-z, nn - 1.0);
        const double vi = __dsub_rn(__ddiv_rn(__dsub_rn(nn, __dmul_rn(z, z)), nn - 1.0), __dmul_rn(mi, mi));
        den = __dmul_rn(__dsqrt_rn(vi), __dsqrt_rn(__ddiv_rn(__dsub_rn(__dmul_rn(nn - 1.0, S1), ww), nn - 2.0)));
        num = __dsub_rn(lag, __dmul_rn(W, mi));
    }
    if (den == 0.0 || !isfinite(den)) return 0.f;
    return (float)__ddiv_rn(num, den);
}

// G[tile][cell][16], float64 arithmetic on the float32 z, lag and weights (header comment)   thread = (cell, 4 genes)
__global__ __launch_bounds__(256) void k_ls_getis_value(const long long *__restrict__ indptr, const double *__restrict__ w,
                                                        const float *__restrict__ Z32, const float *__restrict__ Lag32,
                                                        float *__restrict__ G32, int64_t n, int star)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t i = t >> 2;
    const int q = (int)(t & 3);
    if (i >= n) return;
    double W = 0.0, S1 = 0.0;
    for (long long e = indptr[i]; e < indptr[i + 1]; ++e) {
        const double we = (double)(float)w[e];
        W = __dadd_rn(W, we);
        S1 = __dadd_rn(S1, __dmul_rn(we, we));
    }
    const int64_t o = (int64_t)blockIdx.y * n * 4 + i * 4 + q;
    const float4 z = reinterpret_cast<const float4 *>(Z32)[o], lag = reinterpret_cast<const float4 *>(Lag32)[o];
    const double nn = (double)n;
    const bool st = star != 0;
    reinterpret_cast<float4 *>(G32)[o] = make_float4(ls_getis_value(z.x, lag.x, W, S1, nn, st), ls_getis_value(z.y, lag.y, W, S1, nn, st),
                                                    ls_getis_value(z.z, lag.z, W, S1, nn, st), ls_getis_value(z.w, lag.w, W, S1, nn, st));
}


// ---- phase B: count[tile][cell][16] += the batch's permutations that reach the observed value -------------------------
// STAT: LM_STAT_MORAN, SC_LOCAL_GETIS or SC_LOCAL_GEARY.  Obs: I32 (local Moran, Geary's C) or Lag32 (Getis-Ord).

typedef float v2f __attribute__((ext_vector_type(2)));   // two genes per v_pk_add_f32 / v_pk_mul_f32: IEEE per component

// float rows: thread = (position r, 4 genes of a tile), cell = order[r]
// The edge loop is the OUTER loop and the batch's permutations the (unrolled) inner one: the LM_PERM_BATCH row loads of
// an edge are independent and in flight together (with the permutations outside, every row load waited for the
// previous one: 6.4 ms per launch at 2.9 TB/s of fabric traffic, latency-bound), and an edge's index and weight are
// read once per batch.  Per permutation the terms are still added in the row's edge order: the reference's sum.
// (An XCD-contiguous block order was measured too: 7.6 ms instead of 6.4 with the old loop order; not kept.)
template <int STAT>
__global__ __launch_bounds__(256) void k_local_count_sorted(const long long *__restrict__ indptr,
                                                            const int32_t *__restrict__ indices_r,
                                                            const float *__restrict__ w32, const int32_t *__restrict__ order,
                                                            const float *__restrict__ Ys, const float *__restrict__ Obs,
                                                            int n_batch, int64_t tiles, uint32_t *__restrict__ count,
                                                            int64_t n, int first)
{
    constexpr bool MORAN = STAT == LM_STAT_MORAN, GEARY = STAT == SC_LOCAL_GEARY;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 2;
    const int q = (int)(t & 3);
    if (r >= n) return;
    const int64_t i = order[r];
    const int64_t o = (int64_t)blockIdx.y * n * 4 + i * 4 + q;
    float4 obs = reinterpret_cast<const float4 *>(Obs)[o];
    if (MORAN) obs = make_float4(fabsf(obs.x), fabsf(obs.y), fabsf(obs.z), fabsf(obs.w));
    const long long e0 = indptr[i], e1 = indptr[i + 1];
    const int64_t pstep = tiles * n * 4;   // float4 stride between the permutations of the batch
    const float4 *Y0 = reinterpret_cast<const float4 *>(Ys + (int64_t)blockIdx.y * n * SC_TILE) + q;
    float4 s[LM_PERM_BATCH], own[GEARY ? LM_PERM_BATCH : 1];
#pragma unroll
    for (int p = 0; p < LM_PERM_BATCH; ++p) {
        s[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (GEARY) own[p] = p < n_batch ? Y0[r * 4 + p * pstep] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (long long e = e0; e < e1; ++e) {
        const float ww = w32[e];
        const float4 *Ye = Y0 + (int64_t)indices_r[e] * 4;
#pragma unroll
        for (int p = 0; p < LM_PERM_BATCH; ++p) {
            if (p < n_batch) {
                float4 z = Ye[p * pstep];
                if (GEARY) {
                    const float4 yi = own[GEARY ? p : 0];
                    const float dx = __fsub_rn(yi.x, z.x), dy = __fsub_rn(yi.y, z.y), dz = __fsub_rn(yi.z, z.z), dw = __fsub_rn(yi.w, z.w);
                    z = make_float4(__fmul_rn(dx, dx), __fmul_rn(dy, dy), __fmul_rn(dz, dz), __fmul_rn(dw, dw));
                }
                s[p].x = __fadd_rn(s[p].x, __fmul_rn(ww, z.x)); s[p].y = __fadd_rn(s[p].y, __fmul_rn(ww, z.y));
                s[p].z = __fadd_rn(s[p].z, __fmul_rn(ww, z.z)); s[p].w = __fadd_rn(s[p].w, __fmul_rn(ww, z.w));
            }
        }
    }
    uint32_t cx = 0, cy = 0, cz = 0, cw = 0;   // local Moran: the count; the others: ge | le << 16
#pragma unroll
    for (int p = 0; p < LM_PERM_BATCH; ++p) {
        if (p < n_batch) {
            if constexpr (MORAN) {
                const float4 zi = Y0[r * 4 + p * pstep];
                cx += fabsf(__fmul_rn(zi.x, s[p].x)) >= obs.x; cy += fabsf(__fmul_rn(zi.y, s[p].y)) >= obs.y;
                cz += fabsf(__fmul_rn(zi.z, s[p].z)) >= obs.z; cw += fabsf(__fmul_rn(zi.w, s[p].w)) >= obs.w;
            } else {
                cx += (s[p].x >= obs.x ? 1u : 0u) + (s[p].x <= obs.x ? 0x10000u : 0u);
                cy += (s[p].y >= obs.y ? 1u : 0u) + (s[p].y <= obs.y ? 0x10000u : 0u);
                cz += (s[p].z >= obs.z ? 1u : 0u) + (s[p].z <= obs.z ? 0x10000u : 0u);
                cw += (s[p].w >= obs.w ? 1u : 0u) + (s[p].w <= obs.w ? 0x10000u : 0u);
            }
        }
    }
    uint4 *dst = reinterpret_cast<uint4 *>(count) + o;
    if (first) *dst = make_uint4(cx, cy, cz, cw);
    else { const uint4 c0 = *dst; *dst = make_uint4(c0.x + cx, c0.y + cy, c0.z + cz, c0.w + cw); }
}

// z of bytes b and b + 1 of a lane's 16 code bytes: tq = table + q * LM_TAB_STRIDE  (+ b * 8 * LM_TAB_STRIDE + value)
__device__ __forceinline__ v2f lc_pair(const float *tq, const uint4 &row, int b)
{
    const uint32_t wd[4] = {row.x, row.y, row.z, row.w};
    const uint32_t v0 = (wd[b >> 2] >> (8 * (b & 3))) & 0xffu, v1 = (wd[b >> 2] >> (8 * (b & 3) + 8)) & 0xffu;
    return (v2f){tq[b * 8 * LM_TAB_STRIDE + v0], tq[(b + 1) * 8 * LM_TAB_STRIDE + v1]};
}

// code rows: thread = (position r, lane q's 16 bytes of a 128-gene code row), QUAD permutations at a time, z looked up in
// LDS per (gene, value); edges in the row's order.  With one weight for all edges (UNI) the table's w z is added, the
// product the float path rounds before it adds.  Geary has no w z table: both z are looked up, subtracted, squared and
// multiplied by the weight; it keeps its own 16 z per permutation in registers and therefore takes two permutations at a
// time.  (The occupancy bounds are local Moran's measured ones; the other two keep the compiler's default.)
template <int STAT, bool UNI>
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(STAT == LM_STAT_MORAN ? (UNI ? 4 : 3) : 1, STAT == LM_STAT_MORAN ? 4 : 8)))
void k_local_count_u8(const long long *__restrict__ indptr, const int32_t *__restrict__ indices_r,
                      const float *__restrict__ w32, const int32_t *__restrict__ order, const uint4 *__restrict__ Ys8,
                      const float *__restrict__ Obs, const float *__restrict__ tab, int n_batch, int64_t tiles, int groups,
                      uint32_t *__restrict__ count, int64_t n, int first)
{
    constexpr bool MORAN = STAT == LM_STAT_MORAN, GEARY = STAT == SC_LOCAL_GEARY;
    constexpr int QUAD = GEARY ? 2 : LM_U8_QUAD;
    static_assert(!(GEARY && UNI), "local Geary has no w z table");
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
    uint32_t cge[4] = {0u, 0u, 0u, 0u}, cle[4] = {0u, 0u, 0u, 0u};   // 16 counts of <= LM_U8_BATCH_MAX, 8 bits each (local Moran: cge only)
    static_assert(LM_U8_BATCH_MAX < 256, "packed per-launch counts");
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        const int64_t tile = 8 * (int64_t)grp + (b >> 1);
        const int64_t o = tile * n * SC_TILE + i * SC_TILE + 2 * q + (b & 1);
        a[b] = tile < tiles ? (MORAN ? fabsf(Obs[o]) : Obs[o]) : 0.f;
    }
    const long long e0 = indptr[i], e1 = indptr[i + 1];
    const int64_t pstep = (int64_t)groups * n * 8;   // uint4 stride between the permutations of the batch
    const uint4 *Y0 = Ys8 + (int64_t)grp * n * 8 + q;
    const float *zq = tz + q * LM_TAB_STRIDE;
    const float *wq = (UNI ? tw : tz) + q * LM_TAB_STRIDE;
    for (int p0 = 0; p0 < n_batch; p0 += QUAD) {
        v2f s[QUAD][8], yi[GEARY ? QUAD : 1][8];
#pragma unroll
        for (int p = 0; p < QUAD; ++p) {
#pragma unroll
            for (int b = 0; b < 8; ++b) s[p][b] = (v2f){0.f, 0.f};
            if constexpr (GEARY) {
                const uint4 own = p0 + p < n_batch ? Y0[r * 8 + (int64_t)(p0 + p) * pstep] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
                for (int b = 0; b < 16; b += 2) yi[GEARY ? p : 0][b >> 1] = lc_pair(zq, own, b);
            }
        }
        for (long long e = e0; e < e1; ++e) {
            const float ww = w32[e];
            const v2f ww2 = {ww, ww};
            const uint4 *Ye = Y0 + (int64_t)indices_r[e] * 8 + (int64_t)p0 * pstep;
            uint4 row[QUAD];
#pragma unroll
            for (int p = 0; p < QUAD; ++p) row[p] = p0 + p < n_batch ? Ye[p * pstep] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
            for (int p = 0; p < QUAD; ++p) {
                const uint32_t wd[4] = {row[p].x, row[p].y, row[p].z, row[p].w};   // (lc_pair written out: through the call this loop is scheduled differently)
#pragma unroll
                for (int b = 0; b < 16; b += 2) {
                    const uint32_t v0 = (wd[b >> 2] >> (8 * (b & 3))) & 0xffu, v1 = (wd[b >> 2] >> (8 * (b & 3) + 8)) & 0xffu;
                    v2f term = {wq[b * 8 * LM_TAB_STRIDE + v0], wq[(b + 1) * 8 * LM_TAB_STRIDE + v1]};
                    if (GEARY) {                          // (-ffp-contract=off: difference, square, product and sum are rounded separately)
                        const v2f d = yi[GEARY ? p : 0][b >> 1] - term;
                        term = ww2 * (d * d);
                    } else if (!UNI) {
                        term = ww2 * term;
                    }
                    s[p][b >> 1] = s[p][b >> 1] + term;
                }
            }
        }
#pragma unroll
        for (int p = 0; p < QUAD; ++p) {
            if (p0 + p < n_batch) {
                // local Moran multiplies by the cell's own z: its row is read here, after the edge loop
                const uint4 own = MORAN ? Y0[r * 8 + (int64_t)(p0 + p) * pstep] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
                for (int b = 0; b < 16; b += 2) {
                    const v2f sp = MORAN ? lc_pair(zq, own, b) * s[p][b >> 1] : s[p][b >> 1];
                    const float sx = MORAN ? fabsf(sp.x) : sp.x, sy = MORAN ? fabsf(sp.y) : sp.y;
                    cge[b >> 2] += (sx >= a[b] ? 1u : 0u) << (8 * (b & 3));
                    cge[b >> 2] += (sy >= a[b + 1] ? 1u : 0u) << (8 * (b & 3) + 8);
                    if constexpr (!MORAN) {
                        cle[b >> 2] += (sx <= a[b] ? 1u : 0u) << (8 * (b & 3));
                        cle[b >> 2] += (sy <= a[b + 1] ? 1u : 0u) << (8 * (b & 3) + 8);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int tt = 0; tt < 8; ++tt) {
        const int64_t tile = 8 * (int64_t)grp + tt;
        if (tile >= tiles) continue;
        uint2 *dst = reinterpret_cast<uint2 *>(count + tile * n * SC_TILE + i * SC_TILE + 2 * q);
        const int sh = 16 * (tt & 1);
        uint32_t ca = (cge[tt >> 1] >> sh) & 0xffu, cb = (cge[tt >> 1] >> (sh + 8)) & 0xffu;
        if constexpr (!MORAN) {
            ca |= ((cle[tt >> 1] >> sh) & 0xffu) << 16;
            cb |= ((cle[tt >> 1] >> (sh + 8)) & 0xffu) << 16;
        }
        if (first) *dst = make_uint2(ca, cb);
        else { const uint2 c0 = *dst; *dst = make_uint2(c0.x + ca, c0.y + cb); }
    }
}

// ---- finalisation ------------------------------------------------------------------------------------------------------

// one field of the count words, un-tiled: out[cell][gene] = (word >> shift) & mask   (tile layout [tile][cell][16])
__global__ __launch_bounds__(256) void k_local_untile_field(const uint32_t *__restrict__ cnt, int32_t *__restrict__ out,
                                                            int64_t n, int64_t n_genes, int shift, uint32_t mask)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * n_genes) return;
    const int64_t i = t / n_genes, g = t - i * n_genes;
    out[t] = (int32_t)((cnt[(g >> 4) * n * SC_TILE + i * SC_TILE + (g & 15)] >> shift) & mask);
}

// the permutation level m = min(ge, le), in place: what k_lm_hist and the classification read as the count
__global__ __launch_bounds__(256) void k_ls_fold(uint32_t *__restrict__ cnt, int64_t total)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint32_t c = cnt[t], ge = c & 0xffffu, le = c >> 16;
    cnt[t] = ge < le ? ge : le;
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


// what the class rules read (a kernel argument by value): local Moran's z and lag; the others' graph, z, lag and statistic
struct LmClassIn { const float *Z32, *Lag32; };
struct LsClassIn {
    const long long *indptr; const int32_t *indices; const double *w;
    const float *Z32, *Lag32, *S32;
};

// p = p_tab[g][level], p_adj = padj_tab[g][level] -- level: local Moran's count, min(ge, le) of the others -- and the class,
// row-major outputs.
// Local Moran, the LISA quadrant (AC:219-265): 1 HH, 2 LL, 3 HL, 4 LH from the signs of z and lag.
// Getis-Ord: 1 hot (G > 0), 2 cold (G < 0).  Geary (GeoDa): C < E positive association -- 1 high-high (z > 0, lag > 0),
// 2 low-low (z < 0, lag < 0), 3 other positive --, C > E: 4 negative.  0 where p_adj >= alpha, the gene is flagged, or the
// statistic sits on its null value (z or lag 0, G == 0, C == E).
template <int STAT, typename In>
__global__ __launch_bounds__(256) void k_local_classify(const In in, const uint32_t *__restrict__ cnt, int64_t n,
                                                        int64_t G, int P1, const float *__restrict__ p_tab,
                                                        const float *__restrict__ padj_tab,
                                                        const unsigned char *__restrict__ force_ns, float alpha,
                                                        float *__restrict__ p_out, float *__restrict__ padj_out,
                                                        signed char *__restrict__ q_out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * G) return;
    const int64_t i = t / G, g = t - i * G;
    const int64_t src = (g >> 4) * n * SC_TILE + i * SC_TILE + (g & 15);
    signed char q = 0;
    if constexpr (STAT == LM_STAT_MORAN) {
        const float z = in.Z32[src], lag = in.Lag32[src];
        if (z > 0.f && lag > 0.f) q = 1;
        if (z < 0.f && lag < 0.f) q = 2;
        if (z > 0.f && lag < 0.f) q = 3;
        if (z < 0.f && lag > 0.f) q = 4;
    } else if constexpr (STAT == SC_LOCAL_GETIS) {
        const float sv = in.S32[src];
        if (sv > 0.f) q = 1;
        if (sv < 0.f) q = 2;
    } else {
        const float sv = in.S32[src];
        double ws = 0.0;
        for (long long e = in.indptr[i]; e < in.indptr[i + 1]; ++e)
            if (in.indices[e] != i) ws = __dadd_rn(ws, (double)(float)in.w[e]);
        const double nn = (double)n;
        const double E = __dmul_rn(__ddiv_rn(__dmul_rn(2.0, nn), nn - 1.0), ws);
        const float z = in.Z32[src], lag = in.Lag32[src];
        if ((double)sv < E) q = (z > 0.f && lag > 0.f) ? 1 : (z < 0.f && lag < 0.f) ? 2 : 3;
        if ((double)sv > E) q = 4;
    }
    if (P1 > 0) {
        int64_t c;   // the level, clamped to the tables as each family's kernel always did (local Moran's word as a signed count)
        if constexpr (STAT == LM_STAT_MORAN) {
            const int s = (int)cnt[src];
            c = s < 0 ? 0 : (s >= P1 ? P1 - 1 : s);
        } else {
            const uint32_t u = cnt[src];
            c = u >= (uint32_t)P1 ? (uint32_t)P1 - 1u : u;
        }
        const float pa = padj_tab[g * P1 + c];
        p_out[t] = p_tab[g * P1 + c];
        padj_out[t] = pa;
        if (pa >= alpha) q = 0;
    }
    if (force_ns[g]) q = 0;
    q_out[t] = q;
}

// ---- host --------------------------------------------------------------------------------------------------------------

// the observed G or C into the job's I32 tiles, over the z lag that lm_prepare wrote there (local Moran's own observed value)
static int local_observed(sc_ctx *c, const LmJob &j, int stat, int star)
{
    if (stat == SC_LOCAL_GETIS)
        hipLaunchKernelGGL(k_ls_getis_value, j.gc, dim3(256), 0, c->stream, c->g_indptr.as<long long>(), c->g_data.as<double>(),
                           j.Z32, j.Lag32, j.I32, j.n, star);
    else if (stat == SC_LOCAL_GEARY)
        hipLaunchKernelGGL(k_ls_geary_observed, j.gc, dim3(256), 0, c->stream, c->g_indptr.as<long long>(),
                           c->g_indices.as<int32_t>(), c->g_data.as<double>(), j.Z32, j.I32, j.n);
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// counts of permutations [p0, p1) of the job (rows row0 + p of the forward table); p0 == 0 starts the counts
static int local_count(sc_ctx *c, const LmJob &j, int stat, int64_t row0, int64_t p0, int64_t p1)
{
    const int64_t n = j.n, T = j.T;
    if (p1 <= p0) return SC_OK;
    KernelTimerScope ts(c, SC_K_LEE_PERM);
    const float *obs = stat == SC_LOCAL_GETIS ? j.Lag32 : j.I32;
    const dim3 g8((unsigned)ceil_div64(n * 8, 256), (unsigned)j.groups);
    auto count_u8 = stat == SC_LOCAL_GEARY   ? k_local_count_u8<SC_LOCAL_GEARY, false>
                    : stat == SC_LOCAL_GETIS ? (j.uni ? k_local_count_u8<SC_LOCAL_GETIS, true> : k_local_count_u8<SC_LOCAL_GETIS, false>)
                                             : (j.uni ? k_local_count_u8<LM_STAT_MORAN, true> : k_local_count_u8<LM_STAT_MORAN, false>);
    auto count_f = stat == SC_LOCAL_GEARY   ? k_local_count_sorted<SC_LOCAL_GEARY>
                   : stat == SC_LOCAL_GETIS ? k_local_count_sorted<SC_LOCAL_GETIS> : k_local_count_sorted<LM_STAT_MORAN>;
    for (int64_t p = p0; p < p1; p += j.batch) {
        const int nb = (int)(p1 - p < j.batch ? p1 - p : j.batch);
        lm_gather(c, j, row0 + p, nb);
        if (j.mode == 1)
            hipLaunchKernelGGL(count_u8, g8, dim3(256), 0, c->stream, c->g_indptr.as<long long>(),
                               c->g_indices_r.as<int32_t>(), c->g_w32.as<float>(), c->g_order.as<int32_t>(),
                               c->lm_ys.as<uint4>(), obs, c->lm_tab.as<float>(), nb, T, j.groups, j.cnt, n, p == 0 ? 1 : 0);
        else
            hipLaunchKernelGGL(count_f, j.gc, dim3(256), 0, c->stream, c->g_indptr.as<long long>(),
                               c->g_indices_r.as<int32_t>(), c->g_w32.as<float>(), c->g_order.as<int32_t>(),
                               c->lm_ys.as<float>(), obs, nb, T, j.cnt, n, p == 0 ? 1 : 0);
    }
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// arrays and counts to the host -- local Moran: its count through ge_out, le_out null; the others: the two tails, then the
// words folded to m = min(ge, le) for the histogram and the classification
static int local_finish(sc_ctx *c, const LmJob &j, int stat, int star, int64_t n_perm, float *z_out, float *lag_out,
                        float *stat_out, int32_t *ge_out, int32_t *le_out, uint8_t *zero_var_out, bool arrays_done)
{
    const int64_t n = j.n, G = j.G;
    const size_t cells = (size_t)n * (size_t)G;
    const bool moran = stat == LM_STAT_MORAN;
    const bool counts = n_perm > 0 && (ge_out || le_out);
    if (!arrays_done || counts) SC_TRY(c->scratch_a.ensure(sizeof(float) * cells, &c->mem));   // (staging)
    const unsigned gu = (unsigned)ceil_div64(n * G, 256);
    // (arrays_done: a helper thread has copied them out beside the pipeline)
    if (!arrays_done) SC_TRY(lm_copy_arrays(j, c->scratch_a.as<float>(), c->stream, false, z_out, lag_out, stat_out));
    if (n_perm > 0) {
        int32_t *const outs[2] = {ge_out, le_out};
        for (int h = 0; h < 2; ++h) {
            if (!outs[h]) continue;
            hipLaunchKernelGGL(k_local_untile_field, dim3(gu), dim3(256), 0, c->stream, j.cnt, c->scratch_a.as<int32_t>(), n, G,
                               16 * h, moran ? 0xffffffffu : 0xffffu);
            SC_HIP(hipMemcpyAsync(outs[h], c->scratch_a.p, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, c->stream));
        }
        if (!moran)
            hipLaunchKernelGGL(k_ls_fold, dim3((unsigned)ceil_div64((int64_t)j.tile_f, 256)), dim3(256), 0, c->stream, j.cnt,
                               (int64_t)j.tile_f);
    }
    if (zero_var_out) SC_HIP(hipMemcpyAsync(zero_var_out, j.zero, (size_t)G, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipGetLastError());
    SC_HIP(hipStreamSynchronize(c->stream));
    c->lm_valid = true;   // z / lag / statistic / count or m stay resident for the _hist and _classify calls of the family
    c->lm_stat = stat;
    c->lm_star = star != 0;
    c->lm_perms = n_perm;
    return SC_OK;
}

// behind sc_local_moran and sc_local_stat (which check their own arguments): rows [perm_row0, perm_row0 + n_perm) of the table
static int local_run(sc_ctx *c, const char *who, int stat, int star, int64_t n_perm, int64_t perm_row0, float *z_out,
                     float *lag_out, float *stat_out, int32_t *ge_out, int32_t *le_out, uint8_t *zero_var_out)
{
    SC_REQUIRE(n_perm >= 0 && perm_row0 >= 0, SC_ERR_INVALID, "%s: negative size", who);
    SC_HIP(hipSetDevice(c->device));
    if (n_perm > 0) SC_TRY(sc_perm_forward_ensure(c));
    SC_REQUIRE(c->e_n > 0, SC_ERR_STATE, "%s: no expression loaded", who);
    SC_REQUIRE(c->g_n == c->e_n, SC_ERR_STATE, "%s: graph missing or size mismatch", who);
    c->lm_valid = false;
    if (n_perm > 0) {
        SC_REQUIRE(c->p_n == c->e_n && perm_row0 + n_perm <= c->p_count, SC_ERR_STATE,
                   "%s: needs permutation rows [%lld, %lld) of length %lld", who, (long long)perm_row0,
                   (long long)(perm_row0 + n_perm), (long long)c->e_n);
    }
    LmJob j;
    SC_TRY(lm_prepare(c, n_perm, j));
    SC_TRY(local_observed(c, j, stat, star));
    SC_TRY(local_count(c, j, stat, perm_row0, 0, n_perm));
    return local_finish(c, j, stat, star, n_perm, z_out, lag_out, stat_out, ge_out, le_out, zero_var_out, false);
}

// A thread that is joined when it is destroyed (C++17 has no std::jthread)
struct JoiningThread {
    std::thread t;
    ~JoiningThread() { if (t.joinable()) t.join(); }
};

// behind the two _seeded entries: the job as one pipeline behind the generator -- n_perm numpy-exact permutations of the
// cells from state6 (as sc_perm_generate would draw them; state6 is advanced the same way, the table stays resident),
// generated chunk by chunk while the per-cell counts of the finished chunks are taken -- the generator's chain is the
// longest part of a call, and the counts hide behind it.  Same outputs as sc_perm_generate + the unseeded call.
static int local_run_seeded(sc_ctx *c, const char *who, int stat, int star, uint64_t *state6, int64_t n_perm, float *z_out,
                            float *lag_out, float *stat_out, int32_t *ge_out, int32_t *le_out, uint8_t *zero_var_out)
{
    SC_HIP(hipSetDevice(c->device));
    SC_REQUIRE(c->e_n > 0, SC_ERR_STATE, "%s: no expression loaded", who);
    SC_REQUIRE(c->g_n == c->e_n, SC_ERR_STATE, "%s: graph missing or size mismatch", who);
    c->lm_valid = false;
    LmJob j;
    // r04: z, lag and the statistic are final once the preparation has run -- three (cells x genes) float arrays, 1.2 GB at
    // 10^6 cells x 100 genes, that r03 copied to the caller's (pageable) arrays AFTER the last count, 0.1 s of a 0.5-s call.
    // A helper thread un-tiles and copies them out on a stream of its own while the generator and the counts run (neither
    // uses the PCIe link); this thread keeps enqueuing the pipeline.
    int copier_rc = SC_OK;
    std::optional<JoiningThread> copier;   // (declared after what its thread writes; reset() joins)
    bool copier_started = false;
    auto prepare = [&]() -> int {
        SC_TRY(lm_prepare(c, n_perm, j));
        SC_TRY(local_observed(c, j, stat, star));
        if (copier_started) return SC_OK;
        SC_TRY(c->streams.ensure(SR_FINALISE));
        SC_TRY(c->lm_out.ensure(sizeof(float) * (size_t)j.n * (size_t)j.G, &c->mem));
        hipEvent_t ready;
        SC_HIP(hipEventCreateWithFlags(&ready, hipEventDisableTiming));
        SC_HIP(hipEventRecord(ready, c->stream));
        SC_HIP(hipStreamWaitEvent(c->stream_out, ready, 0));
        SC_HIP(hipEventDestroy(ready));
        const LmJob jj = j;
        try {   // (no thread to be had: the arrays are copied at the end, as in r03)
            copier.emplace().t = std::thread([c, jj, z_out, lag_out, stat_out, &copier_rc]() {
            if (hipSetDevice(c->device) != hipSuccess) { copier_rc = SC_ERR_HIP; return; }
            // (a synchronisation per array: the staging buffer is reused by the next one)
            copier_rc = lm_copy_arrays(jj, c->lm_out.as<float>(), c->stream_out, true, z_out, lag_out, stat_out);
            });
            copier_started = true;
        } catch (...) {
            copier_started = false;
        }
        return SC_OK;
    };
    auto score = [&](int64_t p0, int64_t p1) -> int { return local_count(c, j, stat, 0, p0, p1); };
    // a job that fails its verification is rerun with the sequential scan: the counts restart at permutation 0, and the
    // copier is joined first (the second preparation rewrites what it reads -- with the same values)
    const int rc = permgen_rerun_on_failure(
        c, [&]() { return sc_perm_pipeline(c, state6, c->e_n, n_perm, 0, 2, nullptr, prepare, score); },
        [&]() { copier.reset(); return SC_OK; });
    copier.reset();
    SC_TRY(rc);
    if (copier_started && copier_rc != SC_OK) {
        sc_set_error("%s: the copy of z / lag / the statistic to the host failed", who);
        return copier_rc;
    }
    return local_finish(c, j, stat, star, n_perm, z_out, lag_out, stat_out, ge_out, le_out, zero_var_out, copier_started);
}

// behind the two _hist entries: hist[gene][c] = cells of the gene whose resident count (or level m) is c, c = 0 .. lm_perms
static int local_hist(sc_ctx *c, const char *family, bool moran, int64_t *hist_out)
{
    SC_REQUIRE(c && hist_out, SC_ERR_INVALID, "%s_hist: null pointer", family);
    SC_REQUIRE(c->lm_valid && (c->lm_stat == LM_STAT_MORAN) == moran && c->lm_perms > 0, SC_ERR_STATE,
               "%s_hist: no %s result with permutations", family, family);
    SC_HIP(hipSetDevice(c->device));
    const int64_t n = c->e_n, G = c->e_genes, T = c->e_tiles;
    const int P1 = (int)c->lm_perms + 1;
    const size_t tile_f = (size_t)T * n * SC_TILE;
    const int32_t *cnt = reinterpret_cast<const int32_t *>(c->Lag.as<float>() + tile_f);
    SC_TRY(c->scratch_b.ensure(sizeof(unsigned long long) * (size_t)(T * SC_TILE) * (size_t)P1, &c->mem));
    SC_HIP(hipMemsetAsync(c->scratch_b.p, 0, sizeof(unsigned long long) * (size_t)(T * SC_TILE) * (size_t)P1, c->stream));
    hipLaunchKernelGGL(k_lm_hist, dim3(256, (unsigned)T), dim3(256), 0, c->stream, cnt, n, P1,
                       c->scratch_b.as<unsigned long long>());
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(hist_out, c->scratch_b.p, sizeof(int64_t) * (size_t)G * (size_t)P1, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}

// behind the two _classify entries: tables and flags to the device, the resident statistic's kernel over row-major device
// arrays, results back to the host
static int local_classify(sc_ctx *c, const char *family, bool moran, const float *p_tab, const float *padj_tab,
                          const uint8_t *force_ns, float alpha, float *p_out, float *padj_out, int8_t *class_out)
{
    SC_REQUIRE(c && force_ns && class_out, SC_ERR_INVALID, "%s_classify: null pointer", family);
    SC_REQUIRE(c->lm_valid && (c->lm_stat == LM_STAT_MORAN) == moran, SC_ERR_STATE, "%s_classify: no %s result", family, family);
    if (!moran) SC_REQUIRE(c->g_n == c->e_n, SC_ERR_STATE, "%s_classify: graph missing or size mismatch", family);
    SC_HIP(hipSetDevice(c->device));
    if (c->lm_perms > 0)
        SC_REQUIRE(p_tab && padj_tab && p_out && padj_out, SC_ERR_INVALID, "%s_classify: tables and outputs required with permutations", family);
    const int64_t n = c->e_n, G = c->e_genes;
    const int P1 = c->lm_perms > 0 ? (int)c->lm_perms + 1 : 0;
    const size_t cells = (size_t)n * (size_t)G, tile_f = (size_t)c->e_tiles * n * SC_TILE;
    const float *Z32 = c->Z.as<float>(), *S32 = Z32 + tile_f, *Lag32 = c->Lag.as<float>();
    const uint32_t *cnt = reinterpret_cast<const uint32_t *>(Lag32 + tile_f);
    // device staging: [p | p_adj | class] row-major, tables, flags
    SC_TRY(c->scratch_a.ensure(sizeof(float) * 2 * cells + cells + 64, &c->mem));
    SC_TRY(c->scratch_b.ensure(sizeof(float) * 2 * (size_t)G * (size_t)(P1 > 0 ? P1 : 1) + (size_t)G + 64, &c->mem));
    float *d_p = c->scratch_a.as<float>(), *d_pa = d_p + cells;
    signed char *d_q = reinterpret_cast<signed char *>(d_pa + cells);
    float *d_pt = c->scratch_b.as<float>(), *d_at = d_pt + (size_t)G * (size_t)(P1 > 0 ? P1 : 1);
    unsigned char *d_f = reinterpret_cast<unsigned char *>(d_at + (size_t)G * (size_t)(P1 > 0 ? P1 : 1));
    if (P1 > 0) {
        SC_HIP(hipMemcpyAsync(d_pt, p_tab, sizeof(float) * (size_t)G * P1, hipMemcpyHostToDevice, c->stream));
        SC_HIP(hipMemcpyAsync(d_at, padj_tab, sizeof(float) * (size_t)G * P1, hipMemcpyHostToDevice, c->stream));
    }
    SC_HIP(hipMemcpyAsync(d_f, force_ns, (size_t)G, hipMemcpyHostToDevice, c->stream));
    auto launch = [&](auto kernel, auto in) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div64(n * G, 256)), dim3(256), 0, c->stream, in, cnt, n, G, P1, d_pt, d_at,
                           d_f, alpha, d_p, d_pa, d_q);
    };
    if (moran)
        launch(k_local_classify<LM_STAT_MORAN, LmClassIn>, LmClassIn{Z32, Lag32});
    else
        launch(c->lm_stat == SC_LOCAL_GEARY ? k_local_classify<SC_LOCAL_GEARY, LsClassIn> : k_local_classify<SC_LOCAL_GETIS, LsClassIn>,
               LsClassIn{c->g_indptr.as<long long>(), c->g_indices.as<int32_t>(), c->g_data.as<double>(), Z32, Lag32, S32});
    SC_HIP(hipGetLastError());
    if (P1 > 0) {
        SC_HIP(hipMemcpyAsync(p_out, d_p, sizeof(float) * cells, hipMemcpyDeviceToHost, c->stream));
        SC_HIP(hipMemcpyAsync(padj_out, d_pa, sizeof(float) * cells, hipMemcpyDeviceToHost, c->stream));
    }
    SC_HIP(hipMemcpyAsync(class_out, d_q, cells, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}

// ---- the entry points: each checks its own arguments and forwards -------------------------------------------------------

extern "C" int sc_local_moran(sc_ctx *c, int64_t n_perm, int64_t perm_row0, float *z_out, float *lag_out,
                              float *I_out, int32_t *count_out, uint8_t *zero_var_out)
{
    SC_REQUIRE(c && z_out && lag_out && I_out, SC_ERR_INVALID, "sc_local_moran: null pointer");
    return local_run(c, "sc_local_moran", LM_STAT_MORAN, 0, n_perm, perm_row0, z_out, lag_out, I_out, count_out, nullptr,
                     zero_var_out);
}

extern "C" int sc_local_moran_seeded(sc_ctx *c, uint64_t *state6, int64_t n_perm, float *z_out, float *lag_out,
                                     float *I_out, int32_t *count_out, uint8_t *zero_var_out)
{
    SC_REQUIRE(c && state6 && z_out && lag_out && I_out, SC_ERR_INVALID, "sc_local_moran_seeded: null pointer");
    SC_REQUIRE(n_perm >= 1 && n_perm <= (1 << 24), SC_ERR_INVALID, "sc_local_moran_seeded: n_perm=%lld out of range", (long long)n_perm);
    return local_run_seeded(c, "sc_local_moran_seeded", LM_STAT_MORAN, 0, state6, n_perm, z_out, lag_out, I_out, count_out,
                            nullptr, zero_var_out);
}

extern "C" int sc_local_moran_hist(sc_ctx *c, int64_t *hist_out) { return local_hist(c, "sc_local_moran", true, hist_out); }

extern "C" int sc_local_moran_classify(sc_ctx *c, const float *p_tab, const float *padj_tab, const uint8_t *force_ns,
                                       float alpha, float *p_out, float *padj_out, int8_t *quadrant_out)
{
    return local_classify(c, "sc_local_moran", true, p_tab, padj_tab, force_ns, alpha, p_out, padj_out, quadrant_out);
}

static int ls_check(sc_ctx *c, const char *who, int stat, int64_t n_perm, const void *z, const void *lag, const void *st)
{
    SC_REQUIRE(c && z && lag && st, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(stat == SC_LOCAL_GETIS || stat == SC_LOCAL_GEARY, SC_ERR_INVALID, "%s: unknown statistic %d", who, stat);
    SC_REQUIRE(n_perm <= 65535, SC_ERR_INVALID, "%s: n_perm=%lld above 65535 (the two tails share one 32-bit word)", who,
               (long long)n_perm);
    return SC_OK;
}

extern "C" int sc_local_stat(sc_ctx *c, int32_t stat, int32_t star, int64_t n_perm, int64_t perm_row0, float *z_out,
                             float *lag_out, float *stat_out, int32_t *count_ge_out, int32_t *count_le_out,
                             uint8_t *zero_var_out)
{
    SC_TRY(ls_check(c, "sc_local_stat", stat, n_perm, z_out, lag_out, stat_out));
    return local_run(c, "sc_local_stat", stat, star, n_perm, perm_row0, z_out, lag_out, stat_out, count_ge_out, count_le_out,
                     zero_var_out);
}

extern "C" int sc_local_stat_seeded(sc_ctx *c, int32_t stat, int32_t star, uint64_t *state6, int64_t n_perm, float *z_out,
                                    float *lag_out, float *stat_out, int32_t *count_ge_out, int32_t *count_le_out,
                                    uint8_t *zero_var_out)
{
    SC_TRY(ls_check(c, "sc_local_stat_seeded", stat, n_perm, z_out, lag_out, stat_out));
    SC_REQUIRE(state6 && n_perm >= 1, SC_ERR_INVALID, "sc_local_stat_seeded: needs a generator state and n_perm >= 1");
    return local_run_seeded(c, "sc_local_stat_seeded", stat, star, state6, n_perm, z_out, lag_out, stat_out, count_ge_out,
                            count_le_out, zero_var_out);
}

extern "C" int sc_local_stat_hist(sc_ctx *c, int64_t *hist_out) { return local_hist(c, "sc_local_stat", false, hist_out); }

extern "C" int sc_local_stat_classify(sc_ctx *c, const float *p_tab, const float *padj_tab, const uint8_t *force_ns,
                                      float alpha, float *p_out, float *padj_out, int8_t *class_out)
{
    return local_classify(c, "sc_local_stat", false, p_tab, padj_tab, force_ns, alpha, p_out, padj_out, class_out);
}
