// A8 at scale: Lee's L for many gene pairs in ONE call (BASELINE configs[2]: 100 x 100 pairs, 1M cells).  gfx950 only.
//
// Reference: lees_l (AC:1113-1155) loops over the pairs in Python; per pair it standardises the two columns,
// takes L = sum_i z_x[i] (W z_y)[i] (AC:307-315) and then P times shuffles z_y with ONE generator shared by all pairs
// and redoes the sparse mat-vec (AC:322-328); p = (#{|L_perm| >= |L|} + 1) / (P + 1) (AC:331-332).
// Here, for all pairs at once:
//   * every distinct gene is standardised once (fp64 z-scores, population sd), lag = W Z and U = W^T Z are one
//     tile-SpMM each;
//   * the observed statistics are a dense contraction over the cells, L[x][y] = sum_i Z[i][x] Lag[i][y]: the one true
//     GEMM on the path, done 16 x 16 genes at a time with v_mfma_f64_16x16x4_f64 straight from the 128-byte tile rows
//     (lane l loads element [cell l >> 4][gene l & 15] of both operands: a fully coalesced 512-byte load per MFMA);
//   * the permutation statistic of pair (x, y) is the gather-dot sum_j U[j][x] z_y[perm[j]]; the numpy-exact
//     rows -- a fresh block of P per live pair, in pair order, zero-variance pairs draw nothing (AC:1129-1140) -- come
//     out of the same generator pipeline as sc_moran_seeded and are scored chunk by chunk while the generator runs; the
//     counts are reduced on the device (no host round trip per pair).
// Behind the batched forms: Lee's L one pair at a time on the resident table (sc_lee), at the end of this file.  The
// float32-faithful observed value is in sc_lee_f32.hip, local Lee in sc_lee_local.hip; sc_lee.h is what they share.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "sc_lee.h"

// out[k][cell] = T[tile(genes[k])][cell][slot(genes[k])]: gene-major contiguous copies of the genes a kernel gathers from
__global__ __launch_bounds__(256) void k_gene_major(const double *__restrict__ T, int64_t n, const int32_t *__restrict__ genes,
                                                    double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t g = genes[blockIdx.y];
    out[(int64_t)blockIdx.y * n + i] = T[(int64_t)(g >> 4) * n * SC_TILE + i * SC_TILE + (g & 15)];
}

// ---- observed statistics: C[tile pair][16 x][16 y] = sum over cells of Z_xtile[cell][x] * Lag_ytile[cell][y] ----
#define LEE_OBS_CELLS 16384   // cells per workgroup (4 wavefronts x 4096)

typedef double v4f64 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void k_lee_observed_mfma(const double *__restrict__ Z, const double *__restrict__ Lag,
                                                           int64_t n, const int2 *__restrict__ tile_pairs,
                                                           double *__restrict__ partial)
{
    __shared__ double red[4][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int2 tp = tile_pairs[blockIdx.y];
    const double *A = Z + (int64_t)tp.x * n * SC_TILE, *B = Lag + (int64_t)tp.y * n * SC_TILE;
    const int64_t c0 = (int64_t)blockIdx.x * LEE_OBS_CELLS + (int64_t)wave * (LEE_OBS_CELLS / 4);
    int64_t c1 = c0 + LEE_OBS_CELLS / 4;
    if (c1 > n) c1 = n;
    v4f64 acc = {0.0, 0.0, 0.0, 0.0};
    // A[i = gene x = lane & 15][k = cell lane >> 4], B[k = cell lane >> 4][j = gene y = lane & 15]: both are element
    // [cell][gene] of a tile row, i.e. word `lane` of the 4-row block
    for (int64_t c = c0; c < c1; c += 4) {
        const int64_t cell = c + (lane >> 4);
        const double a = cell < c1 ? A[cell * SC_TILE + (lane & 15)] : 0.0;
        const double b = cell < c1 ? B[cell * SC_TILE + (lane & 15)] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    // D[row = (lane >> 4) + 4 reg][col = lane & 15]  (row = gene x, col = gene y)
#pragma unroll
    for (int v = 0; v < 4; ++v) red[wave][((lane >> 4) + 4 * v) * 16 + (lane & 15)] = acc[v];
    __syncthreads();
    const int t = threadIdx.x;
    partial[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 + t] = (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
}

// obs[pair] = sum over cell blocks (ascending) of the pair's element of its tile pair
__global__ __launch_bounds__(256) void k_lee_observed_pick(const double *__restrict__ partial, int blocks,
                                                           const int32_t *__restrict__ pair_tp,
                                                           const int32_t *__restrict__ pair_x,
                                                           const int32_t *__restrict__ pair_y, int64_t n_pairs,
                                                           double *__restrict__ obs)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_pairs) return;
    const int tp = pair_tp[q];
    if (tp < 0) { obs[q] = 0.0; return; }
    const int e = (pair_x[q] & 15) * 16 + (pair_y[q] & 15);
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += partial[((int64_t)tp * blocks + b) * 256 + e];
    obs[q] = s;
}

// ---- the per-pair permutation statistic: partial[row][block] = sum_{j in block} u[j] * z[perm_row[j]] ----
// Row r of a launch belongs to pair (row0 + r) / rows_per_pair of the slot table: (slot of u_x in Uc, slot of z_y in Zc),
// n doubles per slot; 32-bit, a generator job has fewer than 2^32 rows.  A single pair (lee_pair_*) is a one-entry table
// over its own vectors.  PERMUTED = false is the identity permutation: sc_lee's observed L.
#define LEE_ROW_CELLS 8192   // cells per workgroup.  sc_lee and sc_lee_seeded agree bit for bit because they add the same blocks.

template <bool PERMUTED>
__global__ __launch_bounds__(256) void k_lee_rows(const double *__restrict__ Uc, const double *__restrict__ Zc, int64_t n,
                                                  const int32_t *__restrict__ perm, int64_t pstride,
                                                  const int2 *__restrict__ pair_slots, unsigned row0, unsigned rows_per_pair,
                                                  double *__restrict__ partial)
{
    __shared__ double sh[256];
    const int row = blockIdx.y;
    const int2 sl = pair_slots[(row0 + row) / rows_per_pair];
    const double *u = Uc + (int64_t)sl.x * n, *z = Zc + (int64_t)sl.y * n;
    const int32_t *prow = perm + (int64_t)row * pstride;
    const int64_t j0 = (int64_t)blockIdx.x * LEE_ROW_CELLS;
    const int64_t j1 = j0 + LEE_ROW_CELLS < n ? j0 + LEE_ROW_CELLS : n;
    double acc = 0.0;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += 256) acc = fma(u[j], z[PERMUTED ? prow[j] : j], acc);
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(int64_t)row * gridDim.x + blockIdx.x] = sh[0];
}

// sum[row] = sum_b partial[row][b] (ascending) into out (optional).  COUNT: count[pair(row)] += |sum| >= |obs[pair]|
// (integer: exact, order-free), the pair being pair_of[(row0 + row) / rows_per_pair]
template <bool COUNT>
__global__ __launch_bounds__(256) void k_lee_row_sums(const double *__restrict__ partial, int blocks, int rows,
                                                      const int32_t *__restrict__ pair_of, unsigned row0, unsigned rows_per_pair,
                                                      const double *__restrict__ obs, unsigned long long *__restrict__ count,
                                                      double *__restrict__ out)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += partial[(int64_t)r * blocks + b];
    if (COUNT) {
        const int q = pair_of[(row0 + r) / rows_per_pair];
        if (fabs(s) >= fabs(obs[q])) atomicAdd(&count[q], 1ull);
    }
    if (out) out[r] = s;
}

// ---- what the entry points share ----

int lee_check_genes(const sc_ctx *c, const char *name, const char *fmt, const int32_t *a, const int32_t *b, int64_t k)
{
    const int64_t G = c->e_genes;
    for (int64_t q = 0; q < k; ++q)
        SC_REQUIRE(a[q] >= 0 && a[q] < G && (!b || (b[q] >= 0 && b[q] < G)), SC_ERR_INVALID, fmt, name, (long long)q);
    return SC_OK;
}

int lee_operands(sc_ctx *c, int transposed, std::vector<double> *var)
{
    const size_t tiles_bytes = (size_t)c->e_tiles * (size_t)c->e_n * SC_TILE * sizeof(double);
    SC_TRY(sc_expr_zscores(c));
    SC_TRY(c->Lag.ensure(tiles_bytes, &c->mem));
    SC_TRY(sc_lag_tiles(c, c->g_indptr, c->g_indices, c->g_data, c->Z.as<double>(), c->Lag.as<double>()));
    if (transposed >= 1) SC_TRY(sc_graph_ensure_transpose(c));
    if (transposed >= 2) {
        SC_TRY(c->lee_U.ensure(tiles_bytes, &c->mem));
        SC_TRY(sc_lag_tiles(c, c->gt_indptr, c->gt_indices, c->gt_data, c->Z.as<double>(), c->lee_U.as<double>()));
    }
    if (var) {
        var->resize((size_t)c->e_genes);
        SC_HIP(hipMemcpyAsync(var->data(), c->g_var.p, sizeof(double) * var->size(), hipMemcpyDeviceToHost, c->stream));
        SC_HIP(hipStreamSynchronize(c->stream));
    }
    return SC_OK;
}

void lee_gene_major(sc_ctx *c, const double *T, const int32_t *d_genes, int k, double *out)
{
    hipLaunchKernelGGL(k_gene_major, dim3((unsigned)ceil_div64(c->e_n, 256), (unsigned)k), dim3(256), 0, c->stream, T, c->e_n,
                       d_genes, out);
}

// The observed stage of the batched forms.  L of n_pairs pairs into c->lee_obs and their counts zeroed (c->lee_cnt, with
// room for lee_counted_pipeline's copy): one MFMA contraction of Zt against Lagt per tile pair of tps, then pair q picks
// element (px[q] & 15, py[q] & 15) of tile pair tp[q] (tp[q] < 0: L = 0).  The host arrays are read until c->stream is
// next synchronised.
static int lee_observed(sc_ctx *c, const double *Zt, const double *Lagt, const std::vector<int2> &tps, const int32_t *tp,
                        const int32_t *px, const int32_t *py, int64_t n_pairs)
{
    const int64_t n = c->e_n;
    const int oblocks = (int)ceil_div64(n, LEE_OBS_CELLS);
    SC_TRY(c->lee_obs.ensure(sizeof(double) * (size_t)n_pairs, &c->mem));
    SC_TRY(c->lee_cnt.ensure(sizeof(unsigned long long) * (size_t)n_pairs * 2, &c->mem));
    SC_HIP(hipMemsetAsync(c->lee_cnt.p, 0, sizeof(unsigned long long) * (size_t)n_pairs, c->stream));
    // small index arrays: [tp | px | py] then the tile pairs
    SC_TRY(c->scratch_idx.ensure(sizeof(int32_t) * (size_t)(3 * n_pairs) + sizeof(int2) * (tps.size() + 1), &c->mem));
    int32_t *d_tp = c->scratch_idx.as<int32_t>(), *d_px = d_tp + n_pairs, *d_py = d_px + n_pairs;
    int2 *d_tps = reinterpret_cast<int2 *>(d_py + n_pairs + (n_pairs & 1));
    SC_HIP(hipMemcpyAsync(d_tp, tp, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(d_px, px, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(d_py, py, sizeof(int32_t) * (size_t)n_pairs, hipMemcpyHostToDevice, c->stream));
    if (!tps.empty()) {
        SC_HIP(hipMemcpyAsync(d_tps, tps.data(), sizeof(int2) * tps.size(), hipMemcpyHostToDevice, c->stream));
        SC_TRY(c->lee_part.ensure(sizeof(double) * tps.size() * (size_t)oblocks * 256, &c->mem));
        hipLaunchKernelGGL(k_lee_observed_mfma, dim3((unsigned)oblocks, (unsigned)tps.size()), dim3(256), 0, c->stream, Zt, Lagt,
                           n, d_tps, c->lee_part.as<double>());
    }
    hipLaunchKernelGGL(k_lee_observed_pick, dim3((unsigned)ceil_div64(n_pairs, 256)), dim3(256), 0, c->stream,
                       c->lee_part.as<double>(), oblocks, d_tp, d_px, d_py, n_pairs, c->lee_obs.as<double>());
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// A generator job of `rows` permutations scored chunk by chunk into the n_cnt counts of c->lee_cnt.  The block-parallel
// scan verifies itself at the end of a job; if that fails (never seen without the fault injection mode) the counts are
// rolled back to what they were before the job and it is rerun with the sequential scan.
static int lee_counted_pipeline(sc_ctx *c, uint64_t *state6, int64_t rows, int64_t n_cnt,
                                const std::function<int(int64_t, int64_t)> &score)
{
    unsigned long long *cnt = c->lee_cnt.as<unsigned long long>(), *backup = cnt + n_cnt;
    const size_t bytes = sizeof(unsigned long long) * (size_t)n_cnt;
    SC_HIP(hipMemcpyAsync(backup, cnt, bytes, hipMemcpyDeviceToDevice, c->stream));
    return permgen_rerun_on_failure(
        c, [&]() { return sc_perm_pipeline(c, state6, c->e_n, rows, 0, 2, nullptr, nullptr, score); },
        [&]() -> int {
            SC_HIP(hipMemcpyAsync(cnt, backup, bytes, hipMemcpyDeviceToDevice, c->stream));
            return SC_OK;
        });
}

// L and the counts (widened to int64) of n_pairs pairs to the host
static int lee_download(sc_ctx *c, int64_t n_pairs, double *L_out, int64_t *count_abs_ge_out)
{
    std::vector<unsigned long long> cnt((size_t)n_pairs);
    SC_HIP(hipMemcpyAsync(L_out, c->lee_obs.p, sizeof(double) * (size_t)n_pairs, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipMemcpyAsync(cnt.data(), c->lee_cnt.p, sizeof(unsigned long long) * (size_t)n_pairs, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    for (int64_t q = 0; q < n_pairs; ++q) count_abs_ge_out[q] = (int64_t)cnt[(size_t)q];
    return SC_OK;
}

extern "C" int sc_lee_seeded(sc_ctx *c, uint64_t *state6, const int32_t *pair_x, const int32_t *pair_y, int64_t n_pairs,
                             int64_t n_perm, double *L_out, int64_t *count_abs_ge_out, double *L_perm_out)
{
    SC_REQUIRE(c && pair_x && pair_y && L_out && count_abs_ge_out, SC_ERR_INVALID, "sc_lee_seeded: null pointer");
    SC_REQUIRE(n_pairs >= 0 && n_perm >= 0, SC_ERR_INVALID, "sc_lee_seeded: negative size");
    SC_REQUIRE(n_perm == 0 || state6, SC_ERR_INVALID, "sc_lee_seeded: generator state required when n_perm > 0");
    SC_HIP(hipSetDevice(c->device));
    SC_REQUIRE(c->e_n > 0, SC_ERR_STATE, "sc_lee_seeded: no expression loaded");
    SC_REQUIRE(c->g_n == c->e_n, SC_ERR_STATE, "sc_lee_seeded: graph missing or size mismatch");
    const int64_t n = c->e_n, T = c->e_tiles, G = c->e_genes;
    SC_TRY(lee_check_genes(c, "sc_lee_seeded", "%s: pair %lld references a gene outside the loaded set", pair_x, pair_y, n_pairs));
    if (n_pairs == 0) return SC_OK;
    std::vector<double> var;
    SC_TRY(lee_operands(c, n_perm > 0 ? 2 : 0, &var));

    // ---- observed L of every pair: MFMA contraction per distinct (x tile, y tile) ----
    std::vector<int32_t> pair_tp((size_t)n_pairs, -1), live;
    std::vector<int2> tps;
    {
        std::vector<int64_t> keys;
        for (int64_t q = 0; q < n_pairs; ++q)
            if (var[(size_t)pair_x[q]] > 0.0 && var[(size_t)pair_y[q]] > 0.0) {
                live.push_back((int32_t)q);
                keys.push_back((int64_t)(pair_x[q] >> 4) * T + (pair_y[q] >> 4));
            }
        std::vector<int64_t> uniq(keys);
        std::sort(uniq.begin(), uniq.end());
        uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
        for (int64_t k : uniq) tps.push_back(make_int2((int)(k / T), (int)(k % T)));
        for (size_t i = 0; i < live.size(); ++i)
            pair_tp[(size_t)live[i]] = (int32_t)(std::lower_bound(uniq.begin(), uniq.end(), keys[i]) - uniq.begin());
    }
    const int64_t n_live = (int64_t)live.size();
    SC_TRY(lee_observed(c, c->Z.as<double>(), c->Lag.as<double>(), tps, pair_tp.data(), pair_x, pair_y, n_pairs));

    if (n_perm > 0 && n_live > 0) {
        // ---- gene-major copies of the u_x / z_y vectors the permutation kernel reads; per live pair its slots and its index ----
        std::vector<int32_t> xs, ys, slot_x((size_t)G, -1), slot_y((size_t)G, -1);
        std::vector<int2> slots;
        for (int32_t q : live) {
            if (slot_x[(size_t)pair_x[q]] < 0) { slot_x[(size_t)pair_x[q]] = (int32_t)xs.size(); xs.push_back(pair_x[q]); }
            if (slot_y[(size_t)pair_y[q]] < 0) { slot_y[(size_t)pair_y[q]] = (int32_t)ys.size(); ys.push_back(pair_y[q]); }
            slots.push_back(make_int2(slot_x[(size_t)pair_x[q]], slot_y[(size_t)pair_y[q]]));
        }
        SC_TRY(c->lee_Uc.ensure(sizeof(double) * xs.size() * (size_t)n, &c->mem));
        SC_TRY(c->lee_Zc.ensure(sizeof(double) * ys.size() * (size_t)n, &c->mem));
        SC_TRY(c->scratch_a.ensure(sizeof(int32_t) * (xs.size() + ys.size()), &c->mem));
        SC_TRY(c->lee_rowmap.ensure((sizeof(int2) + sizeof(int32_t)) * (size_t)n_live, &c->mem));
        int32_t *d_xs = c->scratch_a.as<int32_t>(), *d_ys = d_xs + xs.size();
        int2 *d_slots = c->lee_rowmap.as<int2>();
        int32_t *d_live = reinterpret_cast<int32_t *>(d_slots + n_live);
        SC_HIP(hipMemcpyAsync(d_xs, xs.data(), sizeof(int32_t) * xs.size(), hipMemcpyHostToDevice, c->stream));
        SC_HIP(hipMemcpyAsync(d_ys, ys.data(), sizeof(int32_t) * ys.size(), hipMemcpyHostToDevice, c->stream));
        SC_HIP(hipMemcpyAsync(d_slots, slots.data(), sizeof(int2) * (size_t)n_live, hipMemcpyHostToDevice, c->stream));
        SC_HIP(hipMemcpyAsync(d_live, live.data(), sizeof(int32_t) * (size_t)n_live, hipMemcpyHostToDevice, c->stream));
        lee_gene_major(c, c->lee_U.as<double>(), d_xs, (int)xs.size(), c->lee_Uc.as<double>());
        lee_gene_major(c, c->Z.as<double>(), d_ys, (int)ys.size(), c->lee_Zc.as<double>());
        SC_HIP(hipGetLastError());
        SC_HIP(hipStreamSynchronize(c->stream));  // the index arrays are host vectors

        // ---- permutations: sub-jobs of whole pairs, each a generator / scoring pipeline that continues the stream.
        // Live pair l0 + i owns rows [i n_perm, (i + 1) n_perm) of its job ----
        const int64_t max_rows = std::max<int64_t>(n_perm, (int64_t)(2.2e9 / (double)n));   // ~40 GB of generator scratch
        const int64_t pairs_per_job = std::max<int64_t>(1, max_rows / n_perm);
        const int pblocks = (int)ceil_div64(n, LEE_ROW_CELLS);
        const int64_t job_rows_max = std::min(n_live, pairs_per_job) * n_perm;
        SC_TRY(c->scratch_b.ensure(sizeof(double) * (size_t)PERM_CHUNK * (size_t)pblocks, &c->mem));
        if (L_perm_out) SC_TRY(c->lee_lperm.ensure(sizeof(double) * (size_t)job_rows_max, &c->mem));
        for (int64_t l0 = 0; l0 < n_live; l0 += pairs_per_job) {
            const int64_t l1 = std::min(n_live, l0 + pairs_per_job), rows = (l1 - l0) * n_perm;
            auto score = [&](int64_t p0, int64_t p1) -> int {
                const int cnt = (int)(p1 - p0);
                {
                    KernelTimerScope ts(c, SC_K_LEE_PERM);
                    hipLaunchKernelGGL(k_lee_rows<true>, dim3((unsigned)pblocks, (unsigned)cnt), dim3(256), 0, c->stream,
                                       c->lee_Uc.as<double>(), c->lee_Zc.as<double>(), n,
                                       c->perm.as<int32_t>() + p0 * c->p_stride, c->p_stride, d_slots + l0, (unsigned)p0, (unsigned)n_perm,
                                       c->scratch_b.as<double>());
                }
                hipLaunchKernelGGL(k_lee_row_sums<true>, dim3((unsigned)ceil_div64(cnt, 256)), dim3(256), 0, c->stream,
                                   c->scratch_b.as<double>(), pblocks, cnt, d_live + l0, (unsigned)p0, (unsigned)n_perm,
                                   c->lee_obs.as<double>(), c->lee_cnt.as<unsigned long long>(),
                                   L_perm_out ? c->lee_lperm.as<double>() + p0 : (double *)nullptr);
                SC_HIP(hipGetLastError());
                return SC_OK;
            };
            SC_TRY(lee_counted_pipeline(c, state6, rows, n_pairs, score));
            if (L_perm_out) {
                std::vector<double> lp((size_t)rows);
                SC_HIP(hipMemcpy(lp.data(), c->lee_lperm.p, sizeof(double) * (size_t)rows, hipMemcpyDeviceToHost));
                for (int64_t l = l0; l < l1; ++l)
                    memcpy(L_perm_out + (int64_t)live[(size_t)l] * n_perm, lp.data() + (l - l0) * n_perm,
                           sizeof(double) * (size_t)n_perm);
            }
        }
    }
    SC_TRY(lee_download(c, n_pairs, L_out, count_abs_ge_out));
    for (int64_t q = 0; q < n_pairs; ++q) {
        if (pair_tp[(size_t)q] >= 0) continue;   // a zero-variance pair: L = 0, every L_perm = 0, p = 1
        L_out[q] = 0.0;
        count_abs_ge_out[q] = n_perm;
        if (L_perm_out)
            for (int64_t p = 0; p < n_perm; ++p) L_perm_out[q * n_perm + p] = 0.0;
    }
    return SC_OK;
}

// ------------------------------------------------------------------------------------------------
// EXTENSION: all pairs of an x-gene list and a y-gene list under SHARED permutations.
//
// The reference draws a fresh block of permutations for every pair, which makes a 100 x 100 screen cost 2 x 10^6
// permutations of the cells (sc_lee_seeded: 36 ms per pair, generator-bound).  When ONE block of P permutations is
// shared by all pairs (each pair's null is still "y shuffled against x"; the nulls of different pairs are correlated),
// the permutation statistics of the whole grid are P dense contractions over the cells,
//     L_p[x][y] = sum_j U[j][x] * Zy[perm_p[j]][y],
// i.e. the permutation x gene batch becomes a true GEMM with a row-gathered B operand: fp64 matrix cores
// (v_mfma_f64_16x16x4_f64), A = 16 x-genes of 4 cells (coalesced 512 bytes), B = 16 y-genes of the 4 permuted cells
// (four gathered 128-byte rows).  A wavefront keeps the accumulators of up to 8 x-tiles, so every gathered row is
// used for 128 x-genes.
// ------------------------------------------------------------------------------------------------

// out tiles [t][cell][16] = column genes[16 t + s] of the source tiles (0 beyond n_genes)
__global__ __launch_bounds__(256) void k_repack_tiles(const double *__restrict__ T, int64_t n, const int32_t *__restrict__ genes,
                                                      int n_genes, double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t cell = t >> 4;
    const int s = (int)(t & 15);
    if (cell >= n) return;
    const int k = blockIdx.y * 16 + s;
    double v = 0.0;
    if (k < n_genes) { const int32_t g = genes[k]; v = T[(int64_t)(g >> 4) * n * SC_TILE + cell * SC_TILE + (g & 15)]; }
    out[(int64_t)blockIdx.y * n * SC_TILE + cell * SC_TILE + s] = v;
}

#define LEE_SH_CELLS 16384   // cells per workgroup (4 wavefronts x 4096)
#define LEE_SH_XT 8          // x tiles per wavefront pass

// partial[p][yt][xt][block][256]: sums over the block's cells of U_xt[cell][x] * Zy_yt[perm_p[cell]][y]
__global__ __launch_bounds__(256) void k_lee_shared_mfma(const double *__restrict__ Ux, const double *__restrict__ Zy,
                                                         int64_t n, const int32_t *__restrict__ perm, int64_t pstride,
                                                         int xt0, int xt_n, int x_tiles, int y_tiles,
                                                         double *__restrict__ partial)
{
    __shared__ double red[4][256];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int yt = blockIdx.y, p = blockIdx.z;
    const double *B = Zy + (int64_t)yt * n * SC_TILE;
    const int32_t *prow = perm + (int64_t)p * pstride;
    const int64_t c0 = (int64_t)blockIdx.x * LEE_SH_CELLS + (int64_t)wave * (LEE_SH_CELLS / 4);
    int64_t c1 = c0 + LEE_SH_CELLS / 4;
    if (c1 > n) c1 = n;
    v4f64 acc[LEE_SH_XT];
#pragma unroll
    for (int k = 0; k < LEE_SH_XT; ++k) acc[k] = v4f64{0.0, 0.0, 0.0, 0.0};
    for (int64_t c = c0; c < c1; c += 4) {
        const int64_t cell = c + (lane >> 4);
        const bool live = cell < c1;
        const double b = live ? B[(int64_t)prow[cell] * SC_TILE + (lane & 15)] : 0.0;
#pragma unroll
        for (int k = 0; k < LEE_SH_XT; ++k) {
            if (k < xt_n) {
                const double a = live ? Ux[(int64_t)(xt0 + k) * n * SC_TILE + cell * SC_TILE + (lane & 15)] : 0.0;
                acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[k], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < LEE_SH_XT; ++k) {   // (unrolled: a runtime index into acc[] would put it in scratch)
        if (k < xt_n) {                       // uniform for the whole workgroup
            __syncthreads();
#pragma unroll
            for (int v = 0; v < 4; ++v) red[wave][((lane >> 4) + 4 * v) * 16 + (lane & 15)] = acc[k][v];
            __syncthreads();
            const int t = threadIdx.x;
            partial[((((int64_t)p * y_tiles + yt) * x_tiles + xt0 + k) * gridDim.x + blockIdx.x) * 256 + t] =
                (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]);
        }
    }
}

// L_p[x][y] = sum over blocks (ascending); count[x][y] += |L_p| >= |obs[x][y]|; optional copy of L_p
__global__ __launch_bounds__(256) void k_lee_shared_count(const double *__restrict__ partial, int blocks, int x_tiles, int y_tiles,
                                                          int n_x, int n_y, int n_perm_chunk, const double *__restrict__ obs,
                                                          unsigned long long *__restrict__ count, double *__restrict__ lperm_out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per = (int64_t)n_x * n_y;
    if (t >= per * n_perm_chunk) return;
    const int p = (int)(t / per);
    const int x = (int)((t % per) / n_y), y = (int)(t % n_y);
    const double *src = partial + ((((int64_t)p * y_tiles + (y >> 4)) * x_tiles + (x >> 4)) * blocks) * 256 + (x & 15) * 16 + (y & 15);
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += src[(int64_t)b * 256];
    if (fabs(s) >= fabs(obs[(int64_t)x * n_y + y])) atomicAdd(&count[(int64_t)x * n_y + y], 1ull);
    if (lperm_out) lperm_out[t] = s;
}

extern "C" int sc_lee_shared(sc_ctx *c, uint64_t *state6, const int32_t *genes_x, int32_t n_x, const int32_t *genes_y,
                             int32_t n_y, int64_t n_perm, double *L_out, int64_t *count_abs_ge_out, double *L_perm_out)
{
    SC_REQUIRE(c && genes_x && genes_y && L_out && count_abs_ge_out, SC_ERR_INVALID, "sc_lee_shared: null pointer");
    SC_REQUIRE(n_x >= 1 && n_y >= 1 && n_perm >= 0, SC_ERR_INVALID, "sc_lee_shared: bad sizes");
    SC_HIP(hipSetDevice(c->device));
    SC_REQUIRE(c->e_n > 0 && c->g_n == c->e_n, SC_ERR_STATE, "sc_lee_shared: expression / graph missing");
    // state6 == NULL: the shared block is rows [0, n_perm) of the RESIDENT table (e.g. sc_perm_generate_counter's)
    SC_REQUIRE(n_perm == 0 || state6 || (c->p_count >= n_perm && c->p_n == c->e_n), SC_ERR_STATE,
               "sc_lee_shared: no generator state and no resident table of %lld rows", (long long)n_perm);
    const int64_t n = c->e_n;
    SC_TRY(lee_check_genes(c, "sc_lee_shared", "%s: x gene out of range", genes_x, nullptr, n_x));
    SC_TRY(lee_check_genes(c, "sc_lee_shared", "%s: y gene out of range", genes_y, nullptr, n_y));
    const size_t tile_bytes = (size_t)n * SC_TILE * sizeof(double);
    const int XT = (n_x + 15) / 16, YT = (n_y + 15) / 16;
    const int64_t per = (int64_t)n_x * n_y;
    // z-scores (zero-variance genes -> 0: their L and every L_perm are 0, count = n_perm, p = 1), lag, U
    SC_TRY(lee_operands(c, 2, nullptr));
    // compact tile sets: Zx (observed), Ux (permutations) over the x genes; LagY (observed), Zy (permutations) over the y genes
    SC_TRY(c->lee_Uc.ensure((size_t)(2 * XT) * tile_bytes, &c->mem));
    SC_TRY(c->lee_Zc.ensure((size_t)(2 * YT) * tile_bytes, &c->mem));
    SC_TRY(c->scratch_a.ensure(sizeof(int32_t) * (size_t)(n_x + n_y), &c->mem));
    int32_t *d_gx = c->scratch_a.as<int32_t>(), *d_gy = d_gx + n_x;
    SC_HIP(hipMemcpyAsync(d_gx, genes_x, sizeof(int32_t) * (size_t)n_x, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(d_gy, genes_y, sizeof(int32_t) * (size_t)n_y, hipMemcpyHostToDevice, c->stream));
    double *Zx = c->lee_Uc.as<double>(), *Ux = Zx + (size_t)XT * n * SC_TILE;
    double *LagY = c->lee_Zc.as<double>(), *Zy = LagY + (size_t)YT * n * SC_TILE;
    const unsigned gcell = (unsigned)ceil_div64(n * 16, 256);
    hipLaunchKernelGGL(k_repack_tiles, dim3(gcell, (unsigned)XT), dim3(256), 0, c->stream, c->Z.as<double>(), n, d_gx, (int)n_x, Zx);
    hipLaunchKernelGGL(k_repack_tiles, dim3(gcell, (unsigned)XT), dim3(256), 0, c->stream, c->lee_U.as<double>(), n, d_gx, (int)n_x, Ux);
    hipLaunchKernelGGL(k_repack_tiles, dim3(gcell, (unsigned)YT), dim3(256), 0, c->stream, c->Lag.as<double>(), n, d_gy, (int)n_y, LagY);
    hipLaunchKernelGGL(k_repack_tiles, dim3(gcell, (unsigned)YT), dim3(256), 0, c->stream, c->Z.as<double>(), n, d_gy, (int)n_y, Zy);
    // observed grid: every tile pair of the compact sets; pair (x, y) of the grid reads tile pair (x >> 4) * YT + (y >> 4)
    std::vector<int2> tps;
    for (int a = 0; a < XT; ++a) for (int b = 0; b < YT; ++b) tps.push_back(make_int2(a, b));
    std::vector<int32_t> tp((size_t)per), px((size_t)per), py((size_t)per);
    for (int x = 0; x < n_x; ++x)
        for (int y = 0; y < n_y; ++y) {
            tp[(size_t)x * n_y + y] = (x >> 4) * YT + (y >> 4);
            px[(size_t)x * n_y + y] = x;
            py[(size_t)x * n_y + y] = y;
        }
    // (c->lee_part holds the observed partials, then a chunk's: sized for both before the first kernel writes it)
    const int sblocks = (int)ceil_div64(n, LEE_SH_CELLS);
    const int64_t chunk_max = n_perm < PERM_CHUNK ? (n_perm > 0 ? n_perm : 1) : PERM_CHUNK;
    const size_t part_obs = tps.size() * (size_t)ceil_div64(n, LEE_OBS_CELLS) * 256, part_perm = (size_t)chunk_max * YT * XT * sblocks * 256;
    SC_TRY(c->lee_part.ensure(sizeof(double) * std::max(part_obs, part_perm), &c->mem));
    SC_TRY(lee_observed(c, Zx, LagY, tps, tp.data(), px.data(), py.data(), per));
    SC_HIP(hipStreamSynchronize(c->stream));   // the index arrays are host vectors
    if (n_perm > 0) {
        if (L_perm_out) SC_TRY(c->lee_lperm.ensure(sizeof(double) * (size_t)per * (size_t)n_perm, &c->mem));
        auto score = [&](int64_t p0, int64_t p1) -> int {
            const int cnt = (int)(p1 - p0);
            for (int xt0 = 0; xt0 < XT; xt0 += LEE_SH_XT) {
                const int xt_n = XT - xt0 < LEE_SH_XT ? XT - xt0 : LEE_SH_XT;
                KernelTimerScope ts(c, SC_K_LEE_PERM);
                hipLaunchKernelGGL(k_lee_shared_mfma, dim3((unsigned)sblocks, (unsigned)YT, (unsigned)cnt), dim3(256), 0, c->stream,
                                   Ux, Zy, n, c->perm.as<int32_t>() + p0 * c->p_stride, c->p_stride, xt0, xt_n, XT, YT,
                                   c->lee_part.as<double>());
            }
            hipLaunchKernelGGL(k_lee_shared_count, dim3((unsigned)ceil_div64(per * cnt, 256)), dim3(256), 0, c->stream,
                               c->lee_part.as<double>(), sblocks, XT, YT, (int)n_x, (int)n_y, cnt, c->lee_obs.as<double>(),
                               c->lee_cnt.as<unsigned long long>(),
                               L_perm_out ? c->lee_lperm.as<double>() + p0 * per : (double *)nullptr);
            SC_HIP(hipGetLastError());
            return SC_OK;
        };
        if (!state6) {   // the resident table, chunk by chunk
            SC_TRY(sc_perm_forward_ensure(c));
            for (int64_t p0 = 0; p0 < n_perm; p0 += PERM_CHUNK) SC_TRY(score(p0, p0 + PERM_CHUNK < n_perm ? p0 + PERM_CHUNK : n_perm));
        } else {
            SC_TRY(lee_counted_pipeline(c, state6, n_perm, per, score));
        }
        if (L_perm_out)
            SC_HIP(hipMemcpyAsync(L_perm_out, c->lee_lperm.p, sizeof(double) * (size_t)per * (size_t)n_perm, hipMemcpyDeviceToHost, c->stream));
    }
    return lee_download(c, per, L_out, count_abs_ge_out);
}

// ------------------------------------------------------------------------------------------------
// A8: Lee's L, one pair at a time on contiguous vectors (sc_lee: the resident permutation table; sc_lee_local_seeded's
// global statistic).  The observed L is the fma dot product of k_lee_rows, not the MFMA contraction.
// ------------------------------------------------------------------------------------------------

int lee_pair_alloc(sc_ctx *c, const int32_t *xy, int64_t n_pairs, int64_t P_max, size_t extra, LeePair &j)
{
    const int64_t n = j.n = c->e_n;
    SC_TRY(c->scratch_a.ensure(sizeof(double) * ((size_t)n * 4 + extra), &c->mem));
    j.zx = c->scratch_a.as<double>(); j.zy = j.zx + n; j.lagy = j.zx + 2 * n; j.u = j.zx + 3 * n;
    SC_TRY(c->scratch_b.ensure(sizeof(double) * (size_t)ceil_div64(n, LEE_ROW_CELLS) * (size_t)(P_max + 1), &c->mem));   // [row][block]
    SC_TRY(c->scratch_out.ensure(sizeof(double) * (size_t)(P_max + 1), &c->mem));
    SC_TRY(c->lee_rowmap.ensure(sizeof(int2) + sizeof(int32_t) * 2 * (size_t)n_pairs, &c->mem));
    j.d_slot = c->lee_rowmap.as<int2>();
    j.d_xy = reinterpret_cast<const int32_t *>(j.d_slot + 1);
    SC_HIP(hipMemsetAsync(c->lee_rowmap.p, 0, sizeof(int2), c->stream));
    SC_HIP(hipMemcpyAsync(c->lee_rowmap.as<int2>() + 1, xy, sizeof(int32_t) * 2 * (size_t)n_pairs, hipMemcpyHostToDevice, c->stream));
    return SC_OK;
}

// (every row of the job, the observed one at index P included, is pair 0 of the one-entry table)
int lee_pair_prepare(sc_ctx *c, LeePair &j, int64_t q, int64_t P)
{
    const int64_t n = j.n;
    const int blocks = (int)ceil_div64(n, LEE_ROW_CELLS);
    j.P = P;
    lee_gene_major(c, c->Z.as<double>(), j.d_xy + 2 * q, 2, j.zx);   // z_x | z_y
    lee_gene_major(c, c->Lag.as<double>(), j.d_xy + 2 * q + 1, 1, j.lagy);
    hipLaunchKernelGGL(k_lee_rows<false>, dim3((unsigned)blocks), dim3(256), 0, c->stream, j.zx, j.lagy, n, (const int32_t *)nullptr,
                       (int64_t)0, j.d_slot, (unsigned)P, (unsigned)P + 1, c->scratch_b.as<double>() + (size_t)P * blocks);
    if (P > 0)   // u = W^T z_x: SpMV with the transposed graph on the contiguous vector
        sc_launch_spmv_vec(c, c->gt_indptr.as<int64_t>(), c->gt_indices.as<int32_t>(), c->gt_data.as<double>(), j.zx, j.u, n);
    SC_HIP(hipGetLastError());
    return SC_OK;
}

int lee_pair_score(sc_ctx *c, const LeePair &j, int64_t row0, int64_t p0, int64_t p1)
{
    const int blocks = (int)ceil_div64(j.n, LEE_ROW_CELLS);
    hipLaunchKernelGGL(k_lee_rows<true>, dim3((unsigned)blocks, (unsigned)(p1 - p0)), dim3(256), 0, c->stream, j.u, j.zy, j.n,
                       c->perm.as<int32_t>() + (row0 + p0) * c->p_stride, c->p_stride, j.d_slot, (unsigned)p0, (unsigned)j.P + 1,
                       c->scratch_b.as<double>() + (size_t)p0 * blocks);
    SC_HIP(hipGetLastError());
    return SC_OK;
}

int lee_pair_finish(sc_ctx *c, LeePair &j, double *L, int64_t *count_abs_ge, double *L_perm)
{
    const int rows = (int)j.P + 1;
    j.sums.resize((size_t)rows);
    hipLaunchKernelGGL(k_lee_row_sums<false>, dim3((unsigned)ceil_div64(rows, 256)), dim3(256), 0, c->stream,
                       c->scratch_b.as<double>(), (int)ceil_div64(j.n, LEE_ROW_CELLS), rows, (const int32_t *)nullptr, 0u,
                       1u, (const double *)nullptr, (unsigned long long *)nullptr, c->scratch_out.as<double>());
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(j.sums.data(), c->scratch_out.p, sizeof(double) * (size_t)rows, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    *L = j.sums[(size_t)j.P];
    int64_t cnt = 0;
    for (int64_t p = 0; p < j.P; ++p) cnt += fabs(j.sums[(size_t)p]) >= fabs(*L) ? 1 : 0;
    if (count_abs_ge) *count_abs_ge = cnt;
    if (L_perm) memcpy(L_perm, j.sums.data(), sizeof(double) * (size_t)j.P);
    return SC_OK;
}

extern "C" int sc_lee(sc_ctx *c, const int32_t *pair_x, const int32_t *pair_y, const int64_t *perm_offset,
                      int64_t n_pairs, int64_t n_perm, double *L_out, int64_t *count_abs_ge_out,
                      double *L_perm_out)
{
    SC_REQUIRE(c && pair_x && pair_y && L_out, SC_ERR_INVALID, "sc_lee: null pointer");
    SC_REQUIRE(n_pairs >= 0 && n_perm >= 0, SC_ERR_INVALID, "sc_lee: negative size");
    SC_HIP(hipSetDevice(c->device));
    if (n_perm > 0) SC_TRY(sc_perm_forward_ensure(c));
    SC_REQUIRE(c->e_n > 0, SC_ERR_STATE, "sc_lee: no expression loaded");
    SC_REQUIRE(c->g_n == c->e_n, SC_ERR_STATE, "sc_lee: graph missing or size mismatch");
    SC_REQUIRE(n_perm == 0 || perm_offset, SC_ERR_INVALID, "sc_lee: perm_offset required when n_perm > 0");
    SC_TRY(lee_check_genes(c, "sc_lee", "%s: pair %lld references a gene outside the loaded set", pair_x, pair_y, n_pairs));
    for (int64_t q = 0; q < n_pairs; ++q)
        if (n_perm > 0 && perm_offset[q] >= 0)
            SC_REQUIRE(c->p_n == c->e_n && perm_offset[q] + n_perm <= c->p_count, SC_ERR_STATE,
                       "sc_lee: pair %lld needs permutation rows [%lld, %lld) but the table has %lld",
                       (long long)q, (long long)perm_offset[q], (long long)(perm_offset[q] + n_perm),
                       (long long)c->p_count);
    std::vector<double> var;
    SC_TRY(lee_operands(c, n_perm > 0 ? 1 : 0, &var));
    if (n_pairs == 0) return SC_OK;
    std::vector<int32_t> xy((size_t)(2 * n_pairs));
    for (int64_t q = 0; q < n_pairs; ++q) { xy[(size_t)(2 * q)] = pair_x[q]; xy[(size_t)(2 * q + 1)] = pair_y[q]; }
    LeePair j;
    SC_TRY(lee_pair_alloc(c, xy.data(), n_pairs, n_perm, 0, j));
    for (int64_t q = 0; q < n_pairs; ++q) {
        const bool live = var[(size_t)pair_x[q]] > 0.0 && var[(size_t)pair_y[q]] > 0.0;
        const bool do_perm = live && n_perm > 0 && perm_offset[q] >= 0;
        if (!do_perm && L_perm_out)
            for (int64_t p = 0; p < n_perm; ++p) L_perm_out[q * n_perm + p] = 0.0;
        if (!live) {   // a zero-variance pair: L = 0, p = 1
            L_out[q] = 0.0;
            if (count_abs_ge_out) count_abs_ge_out[q] = n_perm;
            continue;
        }
        SC_TRY(lee_pair_prepare(c, j, q, do_perm ? n_perm : 0));
        if (do_perm) {
            KernelTimerScope ts(c, SC_K_LEE_PERM);
            SC_TRY(lee_pair_score(c, j, perm_offset[q], 0, n_perm));
        }
        SC_TRY(lee_pair_finish(c, j, L_out + q, count_abs_ge_out ? count_abs_ge_out + q : nullptr,
                               do_perm && L_perm_out ? L_perm_out + q * n_perm : nullptr));
    }
    return SC_OK;
}
