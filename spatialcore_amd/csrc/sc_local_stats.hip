// Getis-Ord Gi / Gi* and local Geary's C per cell, with two-tail permutation counts (EXTENSION: the reference has neither;
// DESIGN.md 4.6h).  Phase B of the per-cell counts for the two statistics; preparation, phase A, the code / float decision
// and the histogram are local Moran's (sc_local.h).  gfx950 only.
//
// The counts: ge = #{p : s_p >= s_obs}, le = #{p : s_p <= s_obs}, signed, both in one 32-bit word per (cell, gene) while
// they are taken (ge in bits 0 .. 15, le in bits 16 .. 31: n_perm <= 65535), in the buffer that holds local Moran's counts.
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

// ---- phase B over float rows -------------------------------------------------------------------------------------------
// As k_lm_count_sorted: thread = (position r, 4 genes of a tile), the edge loop outside and the batch's permutations
// (unrolled) inside, every sum in the row's edge order.  Obs is Lag32 (Getis-Ord) or the C tiles (Geary).
template <int STAT>
__global__ __launch_bounds__(256) void k_ls_count_sorted(const long long *__restrict__ indptr,
                                                         const int32_t *__restrict__ indices_r,
                                                         const float *__restrict__ w32, const int32_t *__restrict__ order,
                                                         const float *__restrict__ Ys, const float *__restrict__ Obs,
                                                         int n_batch, int64_t tiles, uint32_t *__restrict__ count, int64_t n,
                                                         int first)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = t >> 2;
    const int q = (int)(t & 3);
    if (r >= n) return;
    const int64_t i = order[r];
    const int64_t o = (int64_t)blockIdx.y * n * 4 + i * 4 + q;
    const float4 obs = reinterpret_cast<const float4 *>(Obs)[o];
    const long long e0 = indptr[i], e1 = indptr[i + 1];
    const int64_t pstep = tiles * n * 4;   // float4 stride between the permutations of the batch
    const float4 *Y0 = reinterpret_cast<const float4 *>(Ys + (int64_t)blockIdx.y * n * SC_TILE) + q;
    float4 s[LM_PERM_BATCH], own[STAT == SC_LOCAL_GEARY ? LM_PERM_BATCH : 1];
#pragma unroll
    for (int p = 0; p < LM_PERM_BATCH; ++p) {
        s[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (STAT == SC_LOCAL_GEARY) own[p] = p < n_batch ? Y0[r * 4 + p * pstep] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (long long e = e0; e < e1; ++e) {
        const float ww = w32[e];
        const float4 *Ye = Y0 + (int64_t)indices_r[e] * 4;
#pragma unroll
        for (int p = 0; p < LM_PERM_BATCH; ++p) {
            if (p < n_batch) {
                float4 z = Ye[p * pstep];
                if (STAT == SC_LOCAL_GEARY) {
                    const float4 yi = own[STAT == SC_LOCAL_GEARY ? p : 0];
                    const float dx = __fsub_rn(yi.x, z.x), dy = __fsub_rn(yi.y, z.y), dz = __fsub_rn(yi.z, z.z), dw = __fsub_rn(yi.w, z.w);
                    z = make_float4(__fmul_rn(dx, dx), __fmul_rn(dy, dy), __fmul_rn(dz, dz), __fmul_rn(dw, dw));
                }
                s[p].x = __fadd_rn(s[p].x, __fmul_rn(ww, z.x)); s[p].y = __fadd_rn(s[p].y, __fmul_rn(ww, z.y));
                s[p].z = __fadd_rn(s[p].z, __fmul_rn(ww, z.z)); s[p].w = __fadd_rn(s[p].w, __fmul_rn(ww, z.w));
            }
        }
    }
    uint32_t cx = 0, cy = 0, cz = 0, cw = 0;   // ge | le << 16
#pragma unroll
    for (int p = 0; p < LM_PERM_BATCH; ++p) {
        if (p < n_batch) {
            cx += (s[p].x >= obs.x ? 1u : 0u) + (s[p].x <= obs.x ? 0x10000u : 0u);
            cy += (s[p].y >= obs.y ? 1u : 0u) + (s[p].y <= obs.y ? 0x10000u : 0u);
            cz += (s[p].z >= obs.z ? 1u : 0u) + (s[p].z <= obs.z ? 0x10000u : 0u);
            cw += (s[p].w >= obs.w ? 1u : 0u) + (s[p].w <= obs.w ? 0x10000u : 0u);
        }
    }
    uint4 *dst = reinterpret_cast<uint4 *>(count) + o;
    if (first) *dst = make_uint4(cx, cy, cz, cw);
    else { const uint4 c0 = *dst; *dst = make_uint4(c0.x + cx, c0.y + cy, c0.z + cz, c0.w + cw); }
}

// ---- phase B over code rows --------------------------------------------------------------------------------------------
// As k_lm_count_u8: thread = (position r, lane q's 16 bytes of a 128-gene code row), QUAD permutations at a time, z looked
// up in LDS per (gene, value).  Getis-Ord with one weight for all edges (UNI) adds the table's w z, the product the float
// path rounds before it adds.  Geary has no w z table: both z are looked up, subtracted, squared and multiplied by the
// weight; it keeps its own 16 z per permutation in registers and therefore takes two permutations at a time.
template <int STAT, bool UNI>
__global__ __launch_bounds__(256) void k_ls_count_u8(const long long *__restrict__ indptr,
                                                     const int32_t *__restrict__ indices_r, const float *__restrict__ w32,
                                                     const int32_t *__restrict__ order, const uint4 *__restrict__ Ys8,
                                                     const float *__restrict__ Obs, const float *__restrict__ tab,
                                                     int n_batch, int64_t tiles, int groups, uint32_t *__restrict__ count,
                                                     int64_t n, int first)
{
    constexpr bool GEARY = STAT == SC_LOCAL_GEARY;
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
    uint32_t cge[4] = {0u, 0u, 0u, 0u}, cle[4] = {0u, 0u, 0u, 0u};   // 16 counts of <= LM_U8_BATCH_MAX each, 8 bits each
    static_assert(LM_U8_BATCH_MAX < 256, "packed per-launch counts");
#pragma unroll
    for (int b = 0; b < 16; ++b) {
        const int64_t tile = 8 * (int64_t)grp + (b >> 1);
        a[b] = tile < tiles ? Obs[tile * n * SC_TILE + i * SC_TILE + 2 * q + (b & 1)] : 0.f;
    }
    const long long e0 = indptr[i], e1 = indptr[i + 1];
    const int64_t pstep = (int64_t)groups * n * 8;   // uint4 stride between the permutations of the batch
    const uint4 *Y0 = Ys8 + (int64_t)grp * n * 8 + q;
    const float *zq = tz + q * LM_TAB_STRIDE;         // + b * 8 * LM_TAB_STRIDE + value
    const float *wq = (UNI ? tw : tz) + q * LM_TAB_STRIDE;
    typedef float v2f __attribute__((ext_vector_type(2)));   // two genes per v_pk_add_f32 / v_pk_mul_f32: IEEE per component
    for (int p0 = 0; p0 < n_batch; p0 += QUAD) {
        v2f s[QUAD][8], yi[GEARY ? QUAD : 1][8];
#pragma unroll
        for (int p = 0; p < QUAD; ++p) {
#pragma unroll
            for (int b = 0; b < 8; ++b) s[p][b] = (v2f){0.f, 0.f};
            if constexpr (GEARY) {
                const uint4 own = p0 + p < n_batch ? Y0[r * 8 + (int64_t)(p0 + p) * pstep] : make_uint4(0u, 0u, 0u, 0u);
                const uint32_t wd[4] = {own.x, own.y, own.z, own.w};
#pragma unroll
                for (int b = 0; b < 16; b += 2) {
                    const uint32_t v0 = (wd[b >> 2] >> (8 * (b & 3))) & 0xffu, v1 = (wd[b >> 2] >> (8 * (b & 3) + 8)) & 0xffu;
                    yi[GEARY ? p : 0][b >> 1] = (v2f){zq[b * 8 * LM_TAB_STRIDE + v0], zq[(b + 1) * 8 * LM_TAB_STRIDE + v1]};
                }
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
                const uint32_t wd[4] = {row[p].x, row[p].y, row[p].z, row[p].w};
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
#pragma unroll
                for (int b = 0; b < 16; b += 2) {
                    const v2f sp = s[p][b >> 1];
                    cge[b >> 2] += (sp.x >= a[b] ? 1u : 0u) << (8 * (b & 3));
                    cge[b >> 2] += (sp.y >= a[b + 1] ? 1u : 0u) << (8 * (b & 3) + 8);
                    cle[b >> 2] += (sp.x <= a[b] ? 1u : 0u) << (8 * (b & 3));
                    cle[b >> 2] += (sp.y <= a[b + 1] ? 1u : 0u) << (8 * (b & 3) + 8);
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
        const uint32_t ca = ((cge[tt >> 1] >> sh) & 0xffu) | (((cle[tt >> 1] >> sh) & 0xffu) << 16);
        const uint32_t cb = ((cge[tt >> 1] >> (sh + 8)) & 0xffu) | (((cle[tt >> 1] >> (sh + 8)) & 0xffu) << 16);
        if (first) *dst = make_uint2(ca, cb);
        else { const uint2 c0 = *dst; *dst = make_uint2(c0.x + ca, c0.y + cb); }
    }
}

// ---- finalisation ------------------------------------------------------------------------------------------------------

// one tail of the packed counts, un-tiled: out[cell][gene] = (word >> shift) & 0xffff
__global__ __launch_bounds__(256) void k_ls_untile_tail(const uint32_t *__restrict__ cnt, int32_t *__restrict__ out, int64_t n,
                                                        int64_t n_genes, int shift)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * n_genes) return;
    const int64_t i = t / n_genes, g = t - i * n_genes;
    out[t] = (int32_t)((cnt[(g >> 4) * n * SC_TILE + i * SC_TILE + (g & 15)] >> shift) & 0xffffu);
}

// the permutation level m = min(ge, le), in place: what k_lm_hist and the classification read as the count
__global__ __launch_bounds__(256) void k_ls_fold(uint32_t *__restrict__ cnt, int64_t total)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint32_t c = cnt[t], ge = c & 0xffffu, le = c >> 16;
    cnt[t] = ge < le ? ge : le;
}

// p = p_tab[g][m], p_adj = padj_tab[g][m] and the class, row-major outputs.
// Getis-Ord: 1 hot (G > 0), 2 cold (G < 0).  Geary (GeoDa): C < E positive association -- 1 high-high (z > 0, lag > 0),
// 2 low-low (z < 0, lag < 0), 3 other positive --, C > E: 4 negative.  0 where p_adj >= alpha, the gene is flagged, or the
// statistic sits on its null value (G == 0, C == E).
template <int STAT>
__global__ __launch_bounds__(256) void k_ls_classify(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                     const double *__restrict__ w, const float *__restrict__ Z32,
                                                     const float *__restrict__ Lag32, const float *__restrict__ S32,
                                                     const uint32_t *__restrict__ cnt, int64_t n, int64_t G, int P1,
                                                     const float *__restrict__ p_tab, const float *__restrict__ padj_tab,
                                                     const unsigned char *__restrict__ force_ns, float alpha,
                                                     float *__restrict__ p_out, float *__restrict__ padj_out,
                                                     signed char *__restrict__ q_out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * G) return;
    const int64_t i = t / G, g = t - i * G;
    const int64_t src = (g >> 4) * n * SC_TILE + i * SC_TILE + (g & 15);
    const float sv = S32[src];
    signed char q = 0;
    if (STAT == SC_LOCAL_GETIS) {
        if (sv > 0.f) q = 1;
        if (sv < 0.f) q = 2;
    } else {
        double ws = 0.0;
        for (long long e = indptr[i]; e < indptr[i + 1]; ++e)
            if (indices[e] != i) ws = __dadd_rn(ws, (double)(float)w[e]);
        const double nn = (double)n;
        const double E = __dmul_rn(__ddiv_rn(__dmul_rn(2.0, nn), nn - 1.0), ws);
        const float z = Z32[src], lag = Lag32[src];
        if ((double)sv < E) q = (z > 0.f && lag > 0.f) ? 1 : (z < 0.f && lag < 0.f) ? 2 : 3;
        if ((double)sv > E) q = 4;
    }
    if (P1 > 0) {
        uint32_t c = cnt[src];
        c = c >= (uint32_t)P1 ? (uint32_t)P1 - 1u : c;
        const float pa = padj_tab[g * P1 + c];
        p_out[t] = p_tab[g * P1 + c];
        padj_out[t] = pa;
        if (pa >= alpha) q = 0;
    }
    if (force_ns[g]) q = 0;
    q_out[t] = q;
}

// ---- host --------------------------------------------------------------------------------------------------------------

// the observed statistic into the job's I32 tiles (over local Moran's z lag, which these statistics do not use)
static int ls_observed(sc_ctx *c, const LmJob &j, int stat, int star)
{
    if (stat == SC_LOCAL_GETIS)
        hipLaunchKernelGGL(k_ls_getis_value, j.gc, dim3(256), 0, c->stream, c->g_indptr.as<long long>(), c->g_data.as<double>(),
                           j.Z32, j.Lag32, j.I32, j.n, star);
    else
        hipLaunchKernelGGL(k_ls_geary_observed, j.gc, dim3(256), 0, c->stream, c->g_indptr.as<long long>(),
                           c->g_indices.as<int32_t>(), c->g_data.as<double>(), j.Z32, j.I32, j.n);
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// two-tail counts of permutations [p0, p1) of the job (rows row0 + p of the forward table); p0 == 0 starts the counts
static int ls_count(sc_ctx *c, const LmJob &j, int stat, int64_t row0, int64_t p0, int64_t p1)
{
    const int64_t n = j.n, T = j.T;
    if (p1 <= p0) return SC_OK;
    KernelTimerScope ts(c, SC_K_LEE_PERM);
    const bool geary = stat == SC_LOCAL_GEARY;
    const float *obs = geary ? j.I32 : j.Lag32;
    uint32_t *cnt = reinterpret_cast<uint32_t *>(j.cnt);
    const dim3 g8((unsigned)ceil_div64(n * 8, 256), (unsigned)j.groups);
    auto count_u8 = geary ? k_ls_count_u8<SC_LOCAL_GEARY, false>
                          : j.uni ? k_ls_count_u8<SC_LOCAL_GETIS, true> : k_ls_count_u8<SC_LOCAL_GETIS, false>;
    auto count_f = geary ? k_ls_count_sorted<SC_LOCAL_GEARY> : k_ls_count_sorted<SC_LOCAL_GETIS>;
    for (int64_t p = p0; p < p1; p += j.batch) {
        const int nb = (int)(p1 - p < j.batch ? p1 - p : j.batch);
        lm_gather(c, j, row0 + p, nb);
        if (j.mode == 1)
            hipLaunchKernelGGL(count_u8, g8, dim3(256), 0, c->stream, c->g_indptr.as<long long>(),
                               c->g_indices_r.as<int32_t>(), c->g_w32.as<float>(), c->g_order.as<int32_t>(),
                               c->lm_ys.as<uint4>(), obs, c->lm_tab.as<float>(), nb, T, j.groups, cnt, n, p == 0 ? 1 : 0);
        else
            hipLaunchKernelGGL(count_f, j.gc, dim3(256), 0, c->stream, c->g_indptr.as<long long>(),
                               c->g_indices_r.as<int32_t>(), c->g_w32.as<float>(), c->g_order.as<int32_t>(),
                               c->lm_ys.as<float>(), obs, nb, T, cnt, n, p == 0 ? 1 : 0);
    }
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// arrays and the two tails to the host, then the counts folded to m = min(ge, le) for the histogram and the classification
static int ls_finish(sc_ctx *c, const LmJob &j, int stat, int star, int64_t n_perm, float *z_out, float *lag_out,
                     float *stat_out, int32_t *ge_out, int32_t *le_out, uint8_t *zero_var_out, bool arrays_done)
{
    const int64_t n = j.n, G = j.G;
    const size_t cells = (size_t)n * (size_t)G;
    SC_TRY(c->lee_a.ensure(sizeof(float) * cells, &c->mem));   // (staging)
    const unsigned gu = (unsigned)ceil_div64(n * G, 256);
    if (!arrays_done) SC_TRY(lm_copy_arrays(j, c->lee_a.as<float>(), c->stream, false, z_out, lag_out, stat_out));
    if (n_perm > 0) {
        uint32_t *cnt = reinterpret_cast<uint32_t *>(j.cnt);
        int32_t *const outs[2] = {ge_out, le_out};
        for (int h = 0; h < 2; ++h) {
            if (!outs[h]) continue;
            hipLaunchKernelGGL(k_ls_untile_tail, dim3(gu), dim3(256), 0, c->stream, cnt, c->lee_a.as<int32_t>(), n, G, 16 * h);
            SC_HIP(hipMemcpyAsync(outs[h], c->lee_a.p, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, c->stream));
        }
        hipLaunchKernelGGL(k_ls_fold, dim3((unsigned)ceil_div64((int64_t)j.tile_f, 256)), dim3(256), 0, c->stream, cnt,
                           (int64_t)j.tile_f);
    }
    if (zero_var_out) SC_HIP(hipMemcpyAsync(zero_var_out, j.zero, (size_t)G, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipGetLastError());
    SC_HIP(hipStreamSynchronize(c->stream));
    c->lm_valid = true;   // z / lag / statistic / m stay resident for sc_local_stat_hist / sc_local_stat_classify
    c->lm_stat = stat;
    c->lm_star = star != 0;
    c->lm_perms = n_perm;
    return SC_OK;
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
    SC_REQUIRE(n_perm >= 0 && perm_row0 >= 0, SC_ERR_INVALID, "sc_local_stat: negative size");
    SC_HIP(hipSetDevice(c->device));
    if (n_perm > 0) SC_TRY(sc_perm_forward_ensure(c));
    SC_REQUIRE(c->e_n > 0, SC_ERR_STATE, "sc_local_stat: no expression loaded");
    SC_REQUIRE(c->g_n == c->e_n, SC_ERR_STATE, "sc_local_stat: graph missing or size mismatch");
    c->lm_valid = false;
    if (n_perm > 0) {
        SC_REQUIRE(c->p_n == c->e_n && perm_row0 + n_perm <= c->p_count, SC_ERR_STATE,
                   "sc_local_stat: needs permutation rows [%lld, %lld) of length %lld", (long long)perm_row0,
                   (long long)(perm_row0 + n_perm), (long long)c->e_n);
    }
    LmJob j;
    SC_TRY(lm_prepare(c, n_perm, j));
    SC_TRY(ls_observed(c, j, stat, star));
    SC_TRY(ls_count(c, j, stat, perm_row0, 0, n_perm));
    return ls_finish(c, j, stat, star, n_perm, z_out, lag_out, stat_out, count_ge_out, count_le_out, zero_var_out, false);
}

extern "C" int sc_local_stat_seeded(sc_ctx *c, int32_t stat, int32_t star, uint64_t *state6, int64_t n_perm, float *z_out,
                                    float *lag_out, float *stat_out, int32_t *count_ge_out, int32_t *count_le_out,
                                    uint8_t *zero_var_out)
{
    SC_TRY(ls_check(c, "sc_local_stat_seeded", stat, n_perm, z_out, lag_out, stat_out));
    SC_REQUIRE(state6 && n_perm >= 1, SC_ERR_INVALID, "sc_local_stat_seeded: needs a generator state and n_perm >= 1");
    SC_HIP(hipSetDevice(c->device));
    SC_REQUIRE(c->e_n > 0, SC_ERR_STATE, "sc_local_stat_seeded: no expression loaded");
    SC_REQUIRE(c->g_n == c->e_n, SC_ERR_STATE, "sc_local_stat_seeded: graph missing or size mismatch");
    c->lm_valid = false;
    LmJob j;
    bool arrays_done = false;
    SC_TRY(lm_seeded_pipeline(c, "sc_local_stat_seeded", state6, n_perm, j,
                              [=](const LmJob &job) { return ls_observed(c, job, stat, star); },
                              [=](const LmJob &job, int64_t p0, int64_t p1) { return ls_count(c, job, stat, 0, p0, p1); },
                              z_out, lag_out, stat_out, &arrays_done));
    return ls_finish(c, j, stat, star, n_perm, z_out, lag_out, stat_out, count_ge_out, count_le_out, zero_var_out, arrays_done);
}

extern "C" int sc_local_stat_hist(sc_ctx *c, int64_t *hist_out)
{
    SC_REQUIRE(c && hist_out, SC_ERR_INVALID, "sc_local_stat_hist: null pointer");
    SC_REQUIRE(c->lm_valid && c->lm_stat != LM_STAT_MORAN && c->lm_perms > 0, SC_ERR_STATE,
               "sc_local_stat_hist: no sc_local_stat result with permutations");
    SC_HIP(hipSetDevice(c->device));
    return lm_hist_run(c, hist_out);
}

extern "C" int sc_local_stat_classify(sc_ctx *c, const float *p_tab, const float *padj_tab, const uint8_t *force_ns,
                                      float alpha, float *p_out, float *padj_out, int8_t *class_out)
{
    SC_REQUIRE(c && force_ns && class_out, SC_ERR_INVALID, "sc_local_stat_classify: null pointer");
    SC_REQUIRE(c->lm_valid && c->lm_stat != LM_STAT_MORAN, SC_ERR_STATE, "sc_local_stat_classify: no sc_local_stat result");
    SC_REQUIRE(c->g_n == c->e_n, SC_ERR_STATE, "sc_local_stat_classify: graph missing or size mismatch");
    SC_HIP(hipSetDevice(c->device));
    if (c->lm_perms > 0) SC_REQUIRE(p_tab && padj_tab && p_out && padj_out, SC_ERR_INVALID, "sc_local_stat_classify: tables and outputs required with permutations");
    const int64_t n = c->e_n, G = c->e_genes, T = c->e_tiles;
    const size_t tile_f = (size_t)T * n * SC_TILE;
    const float *Z32 = c->Z.as<float>(), *S32 = Z32 + tile_f, *Lag32 = c->Lag.as<float>();
    const uint32_t *cnt = reinterpret_cast<const uint32_t *>(Lag32 + tile_f);
    auto kernel = c->lm_stat == SC_LOCAL_GEARY ? k_ls_classify<SC_LOCAL_GEARY> : k_ls_classify<SC_LOCAL_GETIS>;
    return lm_classify_run(c, p_tab, padj_tab, force_ns, p_out, padj_out, class_out,
                           [=](int P1, const float *d_pt, const float *d_at, const unsigned char *d_f, float *d_p, float *d_pa,
                               signed char *d_q) {
                               hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div64(n * G, 256)), dim3(256), 0, c->stream,
                                                  c->g_indptr.as<long long>(), c->g_indices.as<int32_t>(), c->g_data.as<double>(),
                                                  Z32, Lag32, S32, cnt, n, G, P1, d_pt, d_at, d_f, alpha, d_p, d_pa, d_q);
                           });
}
