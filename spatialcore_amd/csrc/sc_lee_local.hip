// N2: Local Lee's L for one pair (AC:1394-1413): z-scores, lag = W z_y, L_local = z_x * lag, and the optional per-cell
// permutation count  #{p : |float32(z_x[i] * (W z_y[perm_p])[i])| >= |L_local[i]|}  (sc_lee_local); and the pair body of
// lees_l_local -- the global statistic and the per-cell counts behind one generator job (sc_lee_local_seeded).  gfx950 only.
#include <math.h>

#include <vector>

#include "sc_lee.h"

__global__ __launch_bounds__(256) void k_vec_mul(const double *__restrict__ a, const double *__restrict__ b,
                                                 double *__restrict__ out, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = __dmul_rn(a[i], b[i]);
}

// The count in two phases per batch of permutations, in the graph's processing order (see k_lm_gather_sorted):
// ys[p][r] = z_y[perm_p[order[r]]] once per permutation, then a LOCAL sparse product.  (A one-kernel form, r01,
// fetched 900 GB for 999 permutations of 1M cells: 7 random 8-byte reads per cell and permutation, 128 bytes each.)
#define LL_PERM_BATCH 16

__global__ __launch_bounds__(256) void k_lee_local_gather(const double *__restrict__ zy, const int32_t *__restrict__ order,
                                                          const int32_t *__restrict__ perm, int64_t pstride, int64_t n,
                                                          double *__restrict__ ys)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    ys[(int64_t)blockIdx.y * n + r] = zy[perm[(int64_t)blockIdx.y * pstride + order[r]]];
}

__global__ __launch_bounds__(256) void k_lee_local_count_sorted(const long long *__restrict__ indptr,
                                                                const int32_t *__restrict__ indices_r,
                                                                const double *__restrict__ w, const int32_t *__restrict__ order,
                                                                const double *__restrict__ zx,
                                                                const double *__restrict__ ys,
                                                                const double *__restrict__ Llocal, int n_batch,
                                                                int32_t *__restrict__ count, int64_t n, int first)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const int64_t i = order[r];
    const long long e0 = indptr[i], e1 = indptr[i + 1];
    const double x = zx[i], obs = fabs(Llocal[i]);
    double s[LL_PERM_BATCH];
#pragma unroll
    for (int p = 0; p < LL_PERM_BATCH; ++p) s[p] = 0.0;
    for (long long e = e0; e < e1; ++e) {      // edge loop outside, permutations unrolled inside: independent loads in flight
        const double ww = w[e];
        const double *ye = ys + indices_r[e];
#pragma unroll
        for (int p = 0; p < LL_PERM_BATCH; ++p)
            if (p < n_batch) s[p] = __dadd_rn(s[p], __dmul_rn(ww, ye[(int64_t)p * n]));
    }
    int cnt = 0;
#pragma unroll
    for (int p = 0; p < LL_PERM_BATCH; ++p)
        if (p < n_batch) {
            // the reference stores the permuted values in a float32 array before comparing (AC:1402,1408)
            const double lp = (double)(float)__dmul_rn(x, s[p]);
            cnt += fabs(lp) >= obs;
        }
    count[i] = first ? cnt : count[i] + cnt;
}


// The vectors of one local Lee job (sc_lee_local, sc_lee_local_seeded), n each
struct LlJob { int64_t n = 0; double *zx = nullptr, *zy = nullptr, *lag = nullptr, *L = nullptr; int32_t *cnt = nullptr; };

// From the job's z_x and z_y: lag = W z_y, L_local = z_x * lag; and what the per-cell counts of n_perm permutations need
static int ll_prepare(sc_ctx *c, int64_t n_perm, const LlJob &j)
{
    const int64_t n = j.n;
    sc_launch_spmv_vec(c, c->g_indptr.as<int64_t>(), c->g_indices.as<int32_t>(), c->g_data.as<double>(), j.zy, j.lag, n);
    hipLaunchKernelGGL(k_vec_mul, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, c->stream, j.zx, j.lag, j.L, n);
    if (n_perm > 0) {
        SC_TRY(sc_graph_ensure_order(c));
        SC_TRY(c->lm_ys.ensure(sizeof(double) * (size_t)LL_PERM_BATCH * (size_t)n, &c->mem));
    }
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// counts of permutations [p0, p1) of the job (rows row0 + p of the forward table); p0 == 0 starts the counts
static int ll_count(sc_ctx *c, const LlJob &j, int64_t row0, int64_t p0, int64_t p1)
{
    const int64_t n = j.n;
    const unsigned gcol = (unsigned)ceil_div64(n, 256);
    for (int64_t p = p0; p < p1; p += LL_PERM_BATCH) {
        const int nb = (int)(p1 - p < LL_PERM_BATCH ? p1 - p : LL_PERM_BATCH);
        hipLaunchKernelGGL(k_lee_local_gather, dim3(gcol, (unsigned)nb), dim3(256), 0, c->stream, j.zy,
                           c->g_order.as<int32_t>(), c->perm.as<int32_t>() + (row0 + p) * c->p_stride, c->p_stride,
                           n, c->lm_ys.as<double>());
        hipLaunchKernelGGL(k_lee_local_count_sorted, dim3(gcol), dim3(256), 0, c->stream, c->g_indptr.as<long long>(),
                           c->g_indices_r.as<int32_t>(), c->g_data.as<double>(), c->g_order.as<int32_t>(), j.zx,
                           c->lm_ys.as<double>(), j.L, nb, j.cnt, n, p == 0 ? 1 : 0);
    }
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// the job's arrays to the host (count_out: optional), enqueued: the caller synchronises
static int ll_download(sc_ctx *c, const LlJob &j, double *zx_out, double *lag_out, double *L_local_out, int32_t *count_out)
{
    const size_t n = (size_t)j.n;
    SC_HIP(hipMemcpyAsync(zx_out, j.zx, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipMemcpyAsync(lag_out, j.lag, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipMemcpyAsync(L_local_out, j.L, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    if (count_out) SC_HIP(hipMemcpyAsync(count_out, j.cnt, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    return SC_OK;
}

extern "C" int sc_lee_local(sc_ctx *c, int32_t gene_x, int32_t gene_y, int64_t n_perm, int64_t perm_row0,
                            double *zx_out, double *lag_out, double *L_local_out, int32_t *count_out)
{
    SC_REQUIRE(c && zx_out && lag_out && L_local_out, SC_ERR_INVALID, "sc_lee_local: null pointer");
    SC_HIP(hipSetDevice(c->device));
    if (n_perm > 0) SC_TRY(sc_perm_forward_ensure(c));
    SC_REQUIRE(c->e_n > 0, SC_ERR_STATE, "sc_lee_local: no expression loaded");
    SC_REQUIRE(c->g_n == c->e_n, SC_ERR_STATE, "sc_lee_local: graph missing or size mismatch");
    SC_TRY(lee_check_genes(c, "sc_lee_local", "%s: gene index outside the loaded set", &gene_x, &gene_y, 1));
    if (n_perm > 0) {
        SC_REQUIRE(count_out, SC_ERR_INVALID, "sc_lee_local: count_out required when n_perm > 0");
        SC_REQUIRE(c->p_n == c->e_n && perm_row0 >= 0 && perm_row0 + n_perm <= c->p_count, SC_ERR_STATE,
                   "sc_lee_local: needs permutation rows [%lld, %lld)", (long long)perm_row0,
                   (long long)(perm_row0 + n_perm));
    }
    const int64_t n = c->e_n;
    const int32_t xy[2] = {gene_x, gene_y};   // (read until the synchronisation below)
    SC_TRY(sc_expr_zscores(c));
    SC_TRY(c->scratch_a.ensure(sizeof(double) * ((size_t)n * 5 + 1), &c->mem));   // four vectors, the counts, the two genes
    LlJob j;
    j.n = n; j.zx = c->scratch_a.as<double>(); j.zy = j.zx + n; j.lag = j.zx + 2 * n; j.L = j.zx + 3 * n;
    j.cnt = reinterpret_cast<int32_t *>(j.zx + 4 * n);
    int32_t *d_xy = reinterpret_cast<int32_t *>(j.zx + 5 * n);
    SC_HIP(hipMemcpyAsync(d_xy, xy, sizeof(xy), hipMemcpyHostToDevice, c->stream));
    lee_gene_major(c, c->Z.as<double>(), d_xy, 2, j.zx);   // z_x | z_y
    SC_TRY(ll_prepare(c, n_perm, j));
    if (n_perm > 0) {
        KernelTimerScope ts(c, SC_K_LEE_PERM);
        SC_TRY(ll_count(c, j, perm_row0, 0, n_perm));
    }
    SC_TRY(ll_download(c, j, zx_out, lag_out, L_local_out, n_perm > 0 ? count_out : nullptr));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}

// r04: the pair body of lees_l_local as ONE pipeline (r03's verdict: a generator call and two device calls per pair, each
// waiting for the one before).  Equal to
//     sc_perm_generate(state6, n, n_perm_global + n_perm_local);  sc_lee(x, y, offset 0, n_perm_global);
//     sc_lee_local(x, y, n_perm_local, perm_row0 = n_perm_global)
// -- the same kernels on the same rows, results bit for bit, the generator state advanced by the same draws -- with the
// permuted sums of the global statistic and the per-cell counts taken chunk by chunk behind the generator (which is 85 % of
// the three calls' time at 10^6 cells), like sc_local_moran_seeded.  The global statistic is sc_lee's own pair job
// (lee_pair_*), scored a chunk at a time; its z_x and z_y are the local job's vectors too.
extern "C" int sc_lee_local_seeded(sc_ctx *c, uint64_t *state6, int32_t gene_x, int32_t gene_y, int64_t n_perm_global,
                                   int64_t n_perm_local, double *L_out, int64_t *count_abs_ge_out, double *zx_out,
                                   double *lag_out, double *L_local_out, int32_t *count_out)
{
    SC_REQUIRE(c && state6 && L_out && zx_out && lag_out && L_local_out, SC_ERR_INVALID, "sc_lee_local_seeded: null pointer");
    SC_REQUIRE(n_perm_global >= 0 && n_perm_local >= 0 && n_perm_global + n_perm_local >= 1 &&
               n_perm_global + n_perm_local <= (1 << 24), SC_ERR_INVALID, "sc_lee_local_seeded: permutation counts out of range");
    SC_REQUIRE(n_perm_local == 0 || count_out, SC_ERR_INVALID, "sc_lee_local_seeded: count_out required when n_perm_local > 0");
    SC_REQUIRE(n_perm_global == 0 || count_abs_ge_out, SC_ERR_INVALID, "sc_lee_local_seeded: count_abs_ge_out required when n_perm_global > 0");
    SC_HIP(hipSetDevice(c->device));
    SC_REQUIRE(c->e_n > 0, SC_ERR_STATE, "sc_lee_local_seeded: no expression loaded");
    SC_REQUIRE(c->g_n == c->e_n, SC_ERR_STATE, "sc_lee_local_seeded: graph missing or size mismatch");
    SC_TRY(lee_check_genes(c, "sc_lee_local_seeded", "%s: gene index outside the loaded set", &gene_x, &gene_y, 1));
    const int64_t n = c->e_n, Pg = n_perm_global, Pl = n_perm_local;
    const int32_t xy[2] = {gene_x, gene_y};   // (read until the synchronisation of lee_pair_finish)
    LeePair g;
    LlJob j;
    auto prepare = [&]() -> int {
        std::vector<double> var;
        SC_TRY(lee_operands(c, Pg > 0 ? 1 : 0, &var));
        SC_REQUIRE(var[(size_t)gene_x] > 0.0 && var[(size_t)gene_y] > 0.0, SC_ERR_INVALID,
                   "sc_lee_local_seeded: a gene of the pair has zero variance");
        SC_TRY(lee_pair_alloc(c, xy, 1, Pg, (size_t)n * 3, g));   // behind the pair's vectors: lag, L_local, the counts
        j.n = n; j.zx = g.zx; j.zy = g.zy; j.lag = g.zx + 4 * n; j.L = g.zx + 5 * n;
        j.cnt = reinterpret_cast<int32_t *>(g.zx + 6 * n);
        SC_TRY(lee_pair_prepare(c, g, 0, Pg));
        return ll_prepare(c, Pl, j);
    };
    auto score = [&](int64_t p0, int64_t p1) -> int {
        KernelTimerScope ts(c, SC_K_LEE_PERM);
        const int64_t a1 = p1 < Pg ? p1 : Pg, b0 = p0 > Pg ? p0 : Pg;
        if (p0 < a1) SC_TRY(lee_pair_score(c, g, 0, p0, a1));           // rows of the global statistic
        if (b0 < p1) SC_TRY(ll_count(c, j, Pg, b0 - Pg, p1 - Pg));      // rows of the per-cell counts
        return SC_OK;
    };
    // a job that fails its verification is rerun with the sequential scan: everything restarts at permutation 0 (the
    // first rows' flag restarts the counts)
    SC_TRY(permgen_rerun_on_failure(c, [&]() { return sc_perm_pipeline(c, state6, n, Pg + Pl, 0, 2, nullptr, prepare, score); }, nullptr));
    SC_TRY(ll_download(c, j, zx_out, lag_out, L_local_out, Pl > 0 ? count_out : nullptr));
    return lee_pair_finish(c, g, L_out, count_abs_ge_out, nullptr);
}
