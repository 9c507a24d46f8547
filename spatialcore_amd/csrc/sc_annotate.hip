// sc_annotate.hip -- sc_annot_*: CellTypist-style prediction and training on a sparse cells x genes matrix: a
// StandardScaler, a clip at 10 and one-vs-rest L2 logistic regression (restated in the same order by
// tests/annotation_restated.py).
//
// The standardised matrix Z = min((X - mean) / scale, 10) is never formed: a zero entry gives z0_g = -mean_g / scale_g, so
// Z = 1 z0^T + D with D on X's own pattern, d_ig = z_ig - z0_g.  A product with a T x G table is then a base row
// (bias_t + sum_g z0_g w_tg, formed on the host in gene order) plus a sum over the stored entries.
//
// fp64 throughout, -ffp-contract=off, no floating-point atomics.  ONE summation order per sum:
//  - over a row's stored entries: index (= column) order, starting from the base;
//  - over a gene column's stored entries (rows ascending): chunks of 512 entries, each in index order from 0, the chunk sums
//    in chunk order;
//  - over cells: chunks of 1024 cells, each in index order from 0, the chunk sums in chunk order;
//  - over the classes of one cell (the epilogue): class t = 64 b + l sits in lane l; every lane adds its own values for b
//    ascending from 0, the lane sums (zero for a lane without a class) meet in the adjacent-pair tree over the group's tp
//    lanes (lane l takes lane l ^ 1, then l ^ 2, ...); maxima and minima are order-free, the argmax is the first.
// None of this depends on the grid.
//
// Lanes = classes: a group of tp lanes (T rounded up to a power of two, 64 for T > 64) serves one row or one column chunk
// and loops over NB = ceil(T / 64) blocks of 64 classes; a workgroup of 256 threads holds 256 / tp groups.
#include <climits>
#include <cmath>
#include <vector>

#include "sc_colsort.h"
#include "sc_csr_input.h"
#include "sc_ctx.h"
#include "sc_lane_group.h"

namespace {

constexpr int AN_TPB = 256;
constexpr int AN_TMAX = 256;
constexpr int AN_CELL_CHUNK = 1024;   // cells per partial of the sums over cells
constexpr double AN_CLIP = 10.0;      // CellTypist clips the standardised values from above
enum { AN_COUNTS = 0, AN_LOG1P = 1, AN_LOG1P_RENORM = 2 };
enum { AN_OUT_ROWS = 0, AN_OUT_PREDICT = 1 };

__device__ __forceinline__ double an_group_min(double v, int tp)
{
    for (int h = 1; h < tp; h <<= 1) {
        const double o = __shfl_xor(v, h, 64);
        v = o < v ? o : v;
    }
    return v;
}
// the largest value of the group and the smallest class that holds it
__device__ __forceinline__ void an_group_argmax(double &v, int &idx, int tp)
{
    for (int h = 1; h < tp; h <<= 1) {
        const double ov = __shfl_xor(v, h, 64);
        const int oi = __shfl_xor(idx, h, 64);
        if (ov > v || (ov == v && oi < idx)) {
            v = ov;
            idx = oi;
        }
    }
}
__device__ __forceinline__ double an_expit(double u) { return 1.0 / (1.0 + exp(-u)); }

// ---- set-up ------------------------------------------------------------------------------------------------------
// per row (one thread): the normalised fp64 values.  AN_LOG1P: as they are; AN_COUNTS: log1p(x / rowsum * 1e4);
// AN_LOG1P_RENORM: the same on expm1(x).  The row sum runs over the stored entries in index order; where it is 0 (every
// stored value of the row is 0) the values stay 0.
template <class V>
__global__ __launch_bounds__(256) void k_an_normalise(const int64_t *__restrict__ indptr, const V *__restrict__ raw, int64_t n, int mode,
                                                      double *__restrict__ val)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t p0 = indptr[i], p1 = indptr[i + 1];
    if (mode == AN_LOG1P) {
        for (int64_t p = p0; p < p1; ++p) val[p] = (double)raw[p];
        return;
    }
    double sum = 0.0;
    for (int64_t p = p0; p < p1; ++p) {
        const double x = (double)raw[p];
        sum = sum + (mode == AN_LOG1P_RENORM ? expm1(x) : x);
    }
    for (int64_t p = p0; p < p1; ++p) {
        const double x = (double)raw[p];
        const double e = mode == AN_LOG1P_RENORM ? expm1(x) : x;
        val[p] = sum > 0.0 ? log1p((e / sum) * 1e4) : 0.0;   // a row of stored zeros is an empty row
    }
}
// per column chunk (one thread): pass 0 the sum of the chunk's values, pass 1 the sum of (x - mean_g)^2, in index order
__global__ __launch_bounds__(256) void k_an_colstat_chunks(const int64_t *__restrict__ colptr, const int64_t *__restrict__ cptr,
                                                           const int32_t *__restrict__ cgene, const double *__restrict__ cval,
                                                           int64_t chunks, int pass, const double *__restrict__ mean,
                                                           double *__restrict__ part)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= chunks) return;
    const ColChunk ch = col_chunk(colptr, cptr, cgene, c);
    const double m = pass ? mean[ch.g] : 0.0;
    double s = 0.0;
    for (int64_t p = ch.p0; p < ch.p1; ++p) {
        const double d = cval[p] - m;
        s = pass ? s + d * d : s + d;
    }
    part[c] = s;
}
// per gene (one thread), chunk sums in chunk order.  Pass 0: mean = sum / n.  Pass 1: the population variance with the
// zeros counted, var = (sum + (n - stored) mean^2) / n; scale = sqrt(var), 1 where sklearn calls the feature constant
// (var <= n eps var + (n mean eps)^2, which covers var == 0); z0 = -mean / scale.
__global__ __launch_bounds__(256) void k_an_colstat_finish(const int64_t *__restrict__ colptr, const int64_t *__restrict__ cptr,
                                                           const double *__restrict__ part, int G, int64_t n, int pass,
                                                           double *__restrict__ mean, double *__restrict__ scale,
                                                           double *__restrict__ z0)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    double s = 0.0;
    for (int64_t c = cptr[g]; c < cptr[g + 1]; ++c) s = s + part[c];
    const double dn = (double)n;
    if (!pass) {
        mean[g] = s / dn;
        return;
    }
    const double m = mean[g];
    const double zeros = (double)(n - (colptr[g + 1] - colptr[g]));
    const double var = (s + zeros * (m * m)) / dn;
    const double eps = 2.220446049250313e-16;
    const double nme = dn * m * eps;
    const double sc = var <= dn * eps * var + nme * nme ? 1.0 : sqrt(var);
    scale[g] = sc;
    z0[g] = (0.0 - m) / sc;
}
// per stored entry: d = min((x - mean_g) / scale_g, 10) - z0_g, in place.  `gene` is int32 (row order) or the sorted keys
template <class I>
__global__ __launch_bounds__(256) void k_an_dvals(const I *__restrict__ gene, int64_t nnz, const double *__restrict__ mean,
                                                  const double *__restrict__ scale, const double *__restrict__ z0,
                                                  double *__restrict__ val)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const int64_t g = (int64_t)gene[p];
    double z = (val[p] - mean[g]) / scale[g];
    z = z < AN_CLIP ? z : AN_CLIP;
    val[p] = z - z0[g];
}

// ---- the per-cell epilogue ---------------------------------------------------------------------------------------------
// The reference's transform_confidence of one row: f[b] is the value of class 64 b + l.  out = {raw, zscore, softmax,
// minmax}, identical in every lane of the group.
template <int NB>
__device__ __forceinline__ void an_confidences(const double (&f)[NB], int T, int tp, int l, double (&out)[4])
{
    double best = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int cls = b * 64 + l;
        if (cls < T && f[b] > best) {
            best = f[b];
            bi = cls;
        }
    }
    an_group_argmax(best, bi, tp);
    const double dT = (double)T;
    double sum = 0.0;
#pragma unroll
    for (int b = 0; b < NB; ++b)
        if (b * 64 + l < T) sum = sum + f[b];
    const double mean = group_sum(sum, tp) / dT;
    double ss = 0.0, se = 0.0, mn = INFINITY;
#pragma unroll
    for (int b = 0; b < NB; ++b)
        if (b * 64 + l < T) {
            const double d = f[b] - mean;
            ss = ss + d * d;
            se = se + exp(f[b] - best);
            mn = f[b] < mn ? f[b] : mn;
        }
    double sd = sqrt(group_sum(ss, tp) / dT);
    if (sd < 1e-10) sd = 1.0;
    se = group_sum(se, tp);
    mn = an_group_min(mn, tp);
    double range = best - mn;
    if (range < 1e-10) range = 1.0;
    out[0] = best;
    out[1] = an_expit((best - mean) / sd);
    out[2] = 1.0 / se;
    out[3] = (best - mn) / range;
}

// ---- the sparse passes --------------------------------------------------------------------------------------------------
// A lane's part of a row of a [rows][T] table: the values of its classes 64 b + l (0.0 past T), and their accumulation
template <int NB>
struct AnRow {
    double v[NB];
};
template <int NB>
__device__ __forceinline__ AnRow<NB> an_row_of(const double *__restrict__ table, int64_t row, int T, int l)
{
    AnRow<NB> r;
#pragma unroll
    for (int b = 0; b < NB; ++b) r.v[b] = b * 64 + l < T ? table[row * T + b * 64 + l] : 0.0;
    return r;
}
template <int NB>
__device__ __forceinline__ void an_row_add(double (&acc)[NB], double x, const AnRow<NB> &r)
{
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = acc[b] + x * r.v[b];
}

// Row pass, one group per cell: acc_t = base_t, then + d_ig table[g][t] over the row's stored entries in index order, four
// table rows in flight (lane_group_walk).
// AN_OUT_ROWS: out64[i][t] = acc_t.  AN_OUT_PREDICT: label = first argmax of the fp64 scores, conf[0] = expit(max),
// out32[i][t] = the float32 score (may be NULL), conf[1 .. 4] = the four transforms of the float32-rounded row.
template <int NB, int OUT>
__global__ __launch_bounds__(256) void k_an_rows(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                 const double *__restrict__ dval, int64_t n, int T, int tp,
                                                 const double *__restrict__ table, const double *__restrict__ base,
                                                 double *__restrict__ out64, float *__restrict__ out32,
                                                 int32_t *__restrict__ label, double *__restrict__ conf)
{
    const int t = threadIdx.x, grp = t / tp, l = t % tp;
    const int64_t i = (int64_t)blockIdx.x * (AN_TPB / tp) + grp;
    if (i >= n) return;   // the whole group leaves
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = b * 64 + l < T ? base[b * 64 + l] : 0.0;
    lane_group_walk(indices, dval, indptr[i], indptr[i + 1], tp, l, [&](int32_t g) { return an_row_of<NB>(table, g, T, l); },
                    [&](double x, const AnRow<NB> &w) { an_row_add<NB>(acc, x, w); });
    if (OUT == AN_OUT_ROWS) {
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (b * 64 + l < T) out64[i * T + b * 64 + l] = acc[b];
        return;
    }
    double best = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int cls = b * 64 + l;
        if (cls < T && acc[b] > best) {
            best = acc[b];
            bi = cls;
        }
    }
    an_group_argmax(best, bi, tp);
    double f[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const float r = (float)acc[b];
        f[b] = (double)r;
        if (out32 && b * 64 + l < T) out32[i * T + b * 64 + l] = r;
    }
    double tr[4];
    an_confidences<NB>(f, T, tp, l, tr);
    if (l == 0) {
        label[i] = bi;
        conf[i] = an_expit(best);
        conf[n + i] = tr[0];
        conf[2 * n + i] = tr[1];
        conf[3 * n + i] = tr[2];
        conf[4 * n + i] = tr[3];
    }
}
// transform_confidence of any n x T matrix (float32 values are widened): one group per row, conf[4][n]
template <int NB, class V>
__global__ __launch_bounds__(256) void k_an_transform(const V *__restrict__ scores, int64_t n, int T, int tp, double *__restrict__ conf)
{
    const int t = threadIdx.x, grp = t / tp, l = t % tp;
    const int64_t i = (int64_t)blockIdx.x * (AN_TPB / tp) + grp;
    if (i >= n) return;
    double f[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) f[b] = b * 64 + l < T ? (double)scores[i * T + b * 64 + l] : 0.0;
    double tr[4];
    an_confidences<NB>(f, T, tp, l, tr);
    if (l == 0) {
        conf[i] = tr[0];
        conf[n + i] = tr[1];
        conf[2 * n + i] = tr[2];
        conf[3 * n + i] = tr[3];
    }
}

// ---- training: kernels over n x T ----------------------------------------------------------------------------------------
// One thread per (cell chunk, class), the chunk's cells in index order.  R_it = s_i (expit(S_it) - y_it);
// rpart[chunk][t] = sum R_it, lpart[chunk][t] = sum s_i (softplus(S_it) - y_it S_it).
__global__ __launch_bounds__(256) void k_an_resid(const double *__restrict__ S, const int32_t *__restrict__ labels,
                                                  const double *__restrict__ sw, int64_t n, int T, int64_t cell_chunks,
                                                  double *__restrict__ R, double *__restrict__ rpart, double *__restrict__ lpart)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= cell_chunks * T) return;
    const int64_t c = q / T;
    const int t = (int)(q % T);
    const int64_t c0 = c * AN_CELL_CHUNK, c1 = c0 + AN_CELL_CHUNK < n ? c0 + AN_CELL_CHUNK : n;
    double rs = 0.0, ls = 0.0;
    for (int64_t i = c0; i < c1; ++i) {
        const double u = S[i * T + t], s = sw[i];
        const double y = labels[i] == t ? 1.0 : 0.0;
        const double r = s * (an_expit(u) - y);
        R[i * T + t] = r;
        rs = rs + r;
        const double sp = (u > 0.0 ? u : 0.0) + log1p(exp(-fabs(u)));
        ls = ls + s * (sp - y * u);
    }
    rpart[q] = rs;
    lpart[q] = ls;
}
// The line search's derivatives at S + alpha_t Dir: d1part[chunk][t] = sum s_i (expit(u) - y) dir,
// d2part[chunk][t] = sum s_i expit(u) (1 - expit(u)) dir^2
__global__ __launch_bounds__(256) void k_an_line(const double *__restrict__ S, const double *__restrict__ Dir,
                                                 const int32_t *__restrict__ labels, const double *__restrict__ sw,
                                                 const double *__restrict__ alpha, int64_t n, int T, int64_t cell_chunks,
                                                 double *__restrict__ d1part, double *__restrict__ d2part)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= cell_chunks * T) return;
    const int64_t c = q / T;
    const int t = (int)(q % T);
    const int64_t c0 = c * AN_CELL_CHUNK, c1 = c0 + AN_CELL_CHUNK < n ? c0 + AN_CELL_CHUNK : n;
    const double a = alpha[t];
    double d1 = 0.0, d2 = 0.0;
    for (int64_t i = c0; i < c1; ++i) {
        const double dir = Dir[i * T + t], s = sw[i];
        const double u = S[i * T + t] + a * dir;
        const double y = labels[i] == t ? 1.0 : 0.0;
        const double sg = an_expit(u);
        d1 = d1 + (s * (sg - y)) * dir;
        d2 = d2 + (s * (sg * (1.0 - sg))) * (dir * dir);
    }
    d1part[q] = d1;
    d2part[q] = d2;
}
__global__ __launch_bounds__(256) void k_an_step(double *__restrict__ S, const double *__restrict__ Dir, const double *__restrict__ alpha,
                                                 int64_t total, int T)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total) return;
    S[q] = S[q] + alpha[q % T] * Dir[q];
}
// Gradient pass: one group per column chunk; part[chunk][t] = sum over the chunk's entries of d_ig R_it, index order
template <int NB>
__global__ __launch_bounds__(256) void k_an_gradcols(const int64_t *__restrict__ colptr, const int32_t *__restrict__ crow,
                                                     const double *__restrict__ cval, const int64_t *__restrict__ cptr,
                                                     const int32_t *__restrict__ cgene, int64_t chunks, int T, int tp,
                                                     const double *__restrict__ R, double *__restrict__ part)
{
    const int t = threadIdx.x, grp = t / tp, l = t % tp;
    const int64_t c = (int64_t)blockIdx.x * (AN_TPB / tp) + grp;
    if (c >= chunks) return;   // the whole group leaves
    const ColChunk ch = col_chunk(colptr, cptr, cgene, c);
    double acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.0;
    // as the row pass: four rows of R in flight
    lane_group_walk(crow, cval, ch.p0, ch.p1, tp, l, [&](int32_t i) { return an_row_of<NB>(R, i, T, l); },
                    [&](double x, const AnRow<NB> &r) { an_row_add<NB>(acc, x, r); });
#pragma unroll
    for (int b = 0; b < NB; ++b)
        if (b * 64 + l < T) part[c * T + b * 64 + l] = acc[b];
}
// grad[t][g] = (the gene's chunk sums in chunk order) + z0_g rsum_t, grad[t][G] = rsum_t: one thread per (gene, class)
__global__ __launch_bounds__(256) void k_an_gradfinish(const int64_t *__restrict__ cptr, const double *__restrict__ part, int G, int T,
                                                       const double *__restrict__ z0, const double *__restrict__ rsum,
                                                       double *__restrict__ grad)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (int64_t)G * T) return;
    const int64_t g = q / T;
    const int t = (int)(q % T);
    double num = 0.0;
    for (int64_t c = cptr[g]; c < cptr[g + 1]; ++c) num = num + part[c * T + t];
    grad[(int64_t)t * (G + 1) + g] = num + z0[g] * rsum[t];
    if (g == 0) grad[(int64_t)t * (G + 1) + G] = rsum[t];
}

// ---- host --------------------------------------------------------------------------------------------------------------
struct AnnotData {   // the matrix on the device (m.val: the D values in row order), the scaler
    CsrDevice m;
    DBuf mean, scale, z0, table, base;
};

int an_lanes(int T) { return lanes_for(T, 2, 64); }

// the envelope and the canonical CSR, on the host
int an_check_matrix(const char *who, const int64_t *indptr, const int32_t *indices, const void *data, int dtype, int64_t n,
                    int32_t G, int32_t mode, int32_t T, int64_t min_nnz, int64_t *nnz_out)
{
    SC_REQUIRE(indptr, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "%s: dtype must be SC_F32 or SC_F64", who);
    SC_REQUIRE(n >= 1 && n <= INT32_MAX, SC_ERR_INVALID, "%s: need 1 <= n <= 2^31 - 1, got %lld", who, (long long)n);
    SC_REQUIRE(G >= 1 && G <= 32768, SC_ERR_INVALID, "%s: need 1 <= n_genes <= 32768, got %d", who, G);
    SC_REQUIRE(T >= 2 && T <= AN_TMAX, SC_ERR_INVALID, "%s: need 2 <= classes <= %d, got %d", who, AN_TMAX, T);
    SC_REQUIRE(mode == AN_COUNTS || mode == AN_LOG1P || mode == AN_LOG1P_RENORM, SC_ERR_INVALID,
               "%s: mode must be 0 (counts), 1 (log1p) or 2 (log1p, renormalise), got %d", who, mode);
    int64_t nnz = 0;
    SC_TRY(csr_check_offsets(who, indptr, n, &nnz));
    SC_REQUIRE(nnz >= min_nnz && nnz <= (int64_t)UINT32_MAX, SC_ERR_INVALID, "%s: need %lld <= stored entries <= 2^32 - 1, got %lld", who,
               (long long)min_nnz, (long long)nnz);
    SC_REQUIRE(nnz == 0 || (indices && data), SC_ERR_INVALID, "%s: null pointer", who);
    SC_TRY(csr_check_columns(who, indptr, indices, n, G, "n_genes"));
    SC_TRY(csr_check_values(who, data, dtype, nnz, true, ""));
    *nnz_out = nnz;
    return SC_OK;
}

// uploads the CSR and enqueues the normalisation into d.m.val
int an_upload(sc_ctx *c, AnnotData &d, const int64_t *indptr, const int32_t *indices, const void *data, int dtype, int64_t n,
              int G, int mode, int64_t nnz)
{
    hipStream_t s = c->stream;
    SC_TRY(d.m.upload(c, indptr, indices, data, dtype, n, nnz));
    SC_TRY(d.mean.ensure(sizeof(double) * (size_t)G, &c->mem));
    SC_TRY(d.scale.ensure(sizeof(double) * (size_t)G, &c->mem));
    SC_TRY(d.z0.ensure(sizeof(double) * (size_t)G, &c->mem));
    KernelTimerScope ts(c, SC_K_ANNOT_SETUP);
    const dim3 per_row((unsigned)ceil_div64(n, 256)), tpb(256);
    if (dtype == SC_F32) hipLaunchKernelGGL(k_an_normalise<float>, per_row, tpb, 0, s, d.m.indptr.as<int64_t>(), d.m.raw.as<float>(), n, mode, d.m.val.as<double>());
    else hipLaunchKernelGGL(k_an_normalise<double>, per_row, tpb, 0, s, d.m.indptr.as<int64_t>(), d.m.raw.as<double>(), n, mode, d.m.val.as<double>());
    return SC_OK;
}

// table[g][t] = coef[t][g] and base[t] = bias[t] + (sum_g z0_g coef[t][g], gene order from 0), formed on the host and
// uploaded; the host vectors must outlive the copy, so the caller waits or keeps them
int an_set_table(sc_ctx *c, AnnotData &d, const double *coef, const double *bias, const double *z0, int G, int T,
                 std::vector<double> &tab, std::vector<double> &base)
{
    tab.resize((size_t)G * T);
    base.resize((size_t)T);
    for (int t = 0; t < T; ++t) {
        double b = 0.0;
        for (int g = 0; g < G; ++g) {
            const double w = coef[(size_t)t * G + g];
            tab[(size_t)g * T + t] = w;
            b = b + z0[g] * w;
        }
        base[t] = bias[t] + b;
    }
    SC_TRY(d.table.ensure(sizeof(double) * (size_t)G * T, &c->mem));
    SC_TRY(d.base.ensure(sizeof(double) * (size_t)T, &c->mem));
    SC_HIP(hipMemcpyAsync(d.table.p, tab.data(), sizeof(double) * (size_t)G * T, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(d.base.p, base.data(), sizeof(double) * (size_t)T, hipMemcpyHostToDevice, c->stream));
    return SC_OK;
}

template <int OUT>
void an_launch_rows(sc_ctx *c, const AnnotData &d, int64_t n, int T, double *out64, float *out32, int32_t *label, double *conf)
{
    const int tp = an_lanes(T), nb = (T + 63) / 64;
    const dim3 grid((unsigned)ceil_div64(n, AN_TPB / tp)), block(AN_TPB);
    const int64_t *ip = d.m.indptr.as<int64_t>();
    const int32_t *ix = d.m.indices.as<int32_t>();
    const double *v = d.m.val.as<double>(), *tab = d.table.as<double>(), *base = d.base.as<double>();
    switch (nb) {
    case 1: hipLaunchKernelGGL((k_an_rows<1, OUT>), grid, block, 0, c->stream, ip, ix, v, n, T, tp, tab, base, out64, out32, label, conf); break;
    case 2: hipLaunchKernelGGL((k_an_rows<2, OUT>), grid, block, 0, c->stream, ip, ix, v, n, T, tp, tab, base, out64, out32, label, conf); break;
    case 3: hipLaunchKernelGGL((k_an_rows<3, OUT>), grid, block, 0, c->stream, ip, ix, v, n, T, tp, tab, base, out64, out32, label, conf); break;
    default: hipLaunchKernelGGL((k_an_rows<4, OUT>), grid, block, 0, c->stream, ip, ix, v, n, T, tp, tab, base, out64, out32, label, conf); break;
    }
}

template <class V>
void an_launch_transform(sc_ctx *c, const V *scores, int64_t n, int T, double *conf)
{
    const int tp = an_lanes(T), nb = (T + 63) / 64;
    const dim3 grid((unsigned)ceil_div64(n, AN_TPB / tp)), block(AN_TPB);
    switch (nb) {
    case 1: hipLaunchKernelGGL((k_an_transform<1, V>), grid, block, 0, c->stream, scores, n, T, tp, conf); break;
    case 2: hipLaunchKernelGGL((k_an_transform<2, V>), grid, block, 0, c->stream, scores, n, T, tp, conf); break;
    case 3: hipLaunchKernelGGL((k_an_transform<3, V>), grid, block, 0, c->stream, scores, n, T, tp, conf); break;
    default: hipLaunchKernelGGL((k_an_transform<4, V>), grid, block, 0, c->stream, scores, n, T, tp, conf); break;
    }
}

}  // namespace

// the training problem resident between sc_annot_train_begin and sc_annot_train_end
struct AnnotTrain : Resident {
    AnnotData d;
    ColSort cs;
    DBuf labels, sw, S, Dir, R, cellpart, cellsum, colpart, grad, alpha;
    int64_t cell_chunks = 0;   // the cells and the stored entries: d.m.n, d.m.nnz
    int G = 0, T = 0;
    bool have_scores = false, have_dir = false;
    std::vector<double> z0, tab, base;
};
static AnnotTrain *an_state(const sc_ctx *c) { return resident<AnnotTrain>(c->an); }

extern "C" int sc_annot_predict(sc_ctx *c, const int64_t *indptr, const int32_t *indices, const void *data, int dtype, int64_t n,
                                int32_t n_genes, int32_t mode, int32_t T, const double *coef, const double *intercept,
                                const double *mean, const double *scale, float *scores_out, int32_t *labels_out, double *conf_out)
{
    const char *who = "sc_annot_predict";
    SC_REQUIRE(c && coef && intercept && mean && scale && labels_out && conf_out, SC_ERR_INVALID, "%s: null pointer", who);
    int64_t nnz = 0;
    SC_TRY(an_check_matrix(who, indptr, indices, data, dtype, n, n_genes, mode, T, 0, &nnz));   // a batch of empty cells is legal
    const int G = n_genes;
    std::vector<double> z0((size_t)G), tab, base;
    for (int g = 0; g < G; ++g) {
        SC_REQUIRE(std::isfinite(mean[g]) && mean[g] >= 0.0 && std::isfinite(scale[g]) && scale[g] > 0.0, SC_ERR_INVALID,
                   "%s: gene %d needs a finite mean >= 0 and a finite scale > 0", who, g);
        z0[g] = (0.0 - mean[g]) / scale[g];
    }
    for (int64_t q = 0; q < (int64_t)T * G; ++q) SC_REQUIRE(std::isfinite(coef[q]), SC_ERR_INVALID, "%s: coefficients must be finite", who);
    for (int t = 0; t < T; ++t) SC_REQUIRE(std::isfinite(intercept[t]), SC_ERR_INVALID, "%s: intercepts must be finite", who);

    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    AnnotData d;
    DBuf o32, lab, conf;
    StreamWaitOnExit wait{c->stream};   // after the buffers and z0 / tab / base, which the copies read
    SC_TRY(an_upload(c, d, indptr, indices, data, dtype, n, G, mode, nnz));
    SC_HIP(hipMemcpyAsync(d.mean.p, mean, sizeof(double) * (size_t)G, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(d.scale.p, scale, sizeof(double) * (size_t)G, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(d.z0.p, z0.data(), sizeof(double) * (size_t)G, hipMemcpyHostToDevice, s));
    SC_TRY(an_set_table(c, d, coef, intercept, z0.data(), G, T, tab, base));
    if (scores_out) SC_TRY(o32.ensure(sizeof(float) * (size_t)n * T, &c->mem));
    SC_TRY(lab.ensure(sizeof(int32_t) * (size_t)n, &c->mem));
    SC_TRY(conf.ensure(sizeof(double) * (size_t)n * 5, &c->mem));
    if (nnz) {
        KernelTimerScope ts(c, SC_K_ANNOT_SETUP);
        hipLaunchKernelGGL(k_an_dvals<int32_t>, dim3((unsigned)ceil_div64(nnz, 256)), dim3(256), 0, s, d.m.indices.as<int32_t>(), nnz,
                           d.mean.as<double>(), d.scale.as<double>(), d.z0.as<double>(), d.m.val.as<double>());
    }
    {
        KernelTimerScope ts(c, SC_K_ANNOT_PREDICT);
        an_launch_rows<AN_OUT_PREDICT>(c, d, n, T, nullptr, scores_out ? o32.as<float>() : nullptr, lab.as<int32_t>(), conf.as<double>());
    }
    SC_HIP(hipGetLastError());
    if (scores_out) SC_HIP(hipMemcpyAsync(scores_out, o32.p, sizeof(float) * (size_t)n * T, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(labels_out, lab.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(conf_out, conf.p, sizeof(double) * (size_t)n * 5, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}

extern "C" int sc_annot_transform(sc_ctx *c, const void *scores, int dtype, int64_t n, int32_t T, double *conf_out)
{
    const char *who = "sc_annot_transform";
    SC_REQUIRE(c && scores && conf_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "%s: dtype must be SC_F32 or SC_F64", who);
    SC_REQUIRE(n >= 1 && n <= INT32_MAX, SC_ERR_INVALID, "%s: need 1 <= n <= 2^31 - 1, got %lld", who, (long long)n);
    SC_REQUIRE(T >= 2 && T <= AN_TMAX, SC_ERR_INVALID, "%s: need 2 <= classes <= %d, got %d", who, AN_TMAX, T);
    for (int64_t q = 0; q < n * T; ++q) {
        const double x = dtype == SC_F32 ? (double)((const float *)scores)[q] : ((const double *)scores)[q];
        SC_REQUIRE(std::isfinite(x), SC_ERR_INVALID, "%s: score %lld is not finite", who, (long long)q);
    }
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    DBuf in, conf;
    StreamWaitOnExit wait{c->stream};
    const size_t bytes = (dtype == SC_F32 ? sizeof(float) : sizeof(double)) * (size_t)n * T;
    SC_TRY(in.ensure(bytes, &c->mem));
    SC_TRY(conf.ensure(sizeof(double) * (size_t)n * 4, &c->mem));
    SC_HIP(hipMemcpyAsync(in.p, scores, bytes, hipMemcpyHostToDevice, s));
    {
        KernelTimerScope ts(c, SC_K_ANNOT_PREDICT);
        if (dtype == SC_F32) an_launch_transform<float>(c, in.as<float>(), n, T, conf.as<double>());
        else an_launch_transform<double>(c, in.as<double>(), n, T, conf.as<double>());
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(conf_out, conf.p, sizeof(double) * (size_t)n * 4, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}

extern "C" int sc_annot_train_begin(sc_ctx *c, const int64_t *indptr, const int32_t *indices, const void *data, int dtype, int64_t n,
                                    int32_t n_genes, int32_t mode, int32_t T, const int32_t *labels, const double *weights,
                                    double *mean_out, double *scale_out)
{
    const char *who = "sc_annot_train_begin";
    SC_REQUIRE(c && labels && weights && mean_out && scale_out, SC_ERR_INVALID, "%s: null pointer", who);
    int64_t nnz = 0;
    SC_TRY(an_check_matrix(who, indptr, indices, data, dtype, n, n_genes, mode, T, 1, &nnz));
    for (int64_t i = 0; i < n; ++i) {
        SC_REQUIRE(labels[i] >= 0 && labels[i] < T, SC_ERR_INVALID, "%s: label of cell %lld is outside [0, classes)", who, (long long)i);
        SC_REQUIRE(std::isfinite(weights[i]) && weights[i] > 0.0, SC_ERR_INVALID, "%s: weight of cell %lld must be finite and > 0", who,
                   (long long)i);
    }
    SC_HIP(hipSetDevice(c->device));
    sc_resident_drop(c, c->an);
    c->an.reset(new AnnotTrain());
    AnnotTrain &a = *an_state(c);
    hipStream_t s = c->stream;
    const int G = n_genes;
    a.G = G, a.T = T, a.cell_chunks = ceil_div64(n, AN_CELL_CHUNK);
#define AN_TRY(call) do { int rc_ = (call); if (rc_ != SC_OK) { sc_resident_drop(c, c->an); return rc_; } } while (0)
    AN_TRY(an_upload(c, a.d, indptr, indices, data, dtype, n, G, mode, nnz));
    AN_TRY(colsort_alloc(c, a.cs, nnz, G));
    AN_TRY(a.labels.ensure(sizeof(int32_t) * (size_t)n, &c->mem));
    AN_TRY(a.sw.ensure(sizeof(double) * (size_t)n, &c->mem));
    AN_TRY(a.S.ensure(sizeof(double) * (size_t)n * T, &c->mem));
    AN_TRY(a.Dir.ensure(sizeof(double) * (size_t)n * T, &c->mem));
    AN_TRY(a.R.ensure(sizeof(double) * (size_t)n * T, &c->mem));
    AN_TRY(a.cellpart.ensure(sizeof(double) * (size_t)a.cell_chunks * T * 2, &c->mem));
    AN_TRY(a.cellsum.ensure(sizeof(double) * (size_t)T * 2, &c->mem));
    AN_TRY(a.grad.ensure(sizeof(double) * (size_t)T * (G + 1), &c->mem));
    AN_TRY(a.alpha.ensure(sizeof(double) * (size_t)T, &c->mem));
    if (hipMemcpyAsync(a.labels.p, labels, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(a.sw.p, weights, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess) {
        sc_set_error("%s: upload failed", who);
        sc_resident_drop(c, c->an);
        return SC_ERR_HIP;
    }
    {
        KernelTimerScope ts(c, SC_K_ANNOT_SETUP);
        AN_TRY(colsort_enqueue(c, a.cs, a.d.m.indptr.as<int64_t>(), a.d.m.indices.as<int32_t>(), a.d.m.val.as<double>(), n, G, nnz));
    }
    AN_TRY(colsort_finish(c, a.cs, G, nnz, who));
    const int64_t chunks = a.cs.chunks;
    AN_TRY(a.colpart.ensure(sizeof(double) * (size_t)chunks * T, &c->mem));
    {
        KernelTimerScope ts(c, SC_K_ANNOT_SETUP);
        const dim3 per_chunk((unsigned)ceil_div64(chunks, 256)), per_gene((unsigned)ceil_div64(G, 256)), per_entry((unsigned)ceil_div64(nnz, 256)), tpb(256);
        const int64_t *colptr = a.cs.colptr.as<int64_t>(), *cptr = a.cs.cptr.as<int64_t>();
        double *part = a.colpart.as<double>(), *mean = a.d.mean.as<double>(), *scale = a.d.scale.as<double>(), *z0 = a.d.z0.as<double>();
        for (int pass = 0; pass < 2; ++pass) {
            hipLaunchKernelGGL(k_an_colstat_chunks, per_chunk, tpb, 0, s, colptr, cptr, a.cs.cgene.as<int32_t>(), a.cs.cval.as<double>(), chunks,
                               pass, mean, part);
            hipLaunchKernelGGL(k_an_colstat_finish, per_gene, tpb, 0, s, colptr, cptr, part, G, n, pass, mean, scale, z0);
        }
        hipLaunchKernelGGL(k_an_dvals<int32_t>, per_entry, tpb, 0, s, a.d.m.indices.as<int32_t>(), nnz, mean, scale, z0, a.d.m.val.as<double>());
        hipLaunchKernelGGL(k_an_dvals<unsigned long long>, per_entry, tpb, 0, s, a.cs.gene.as<unsigned long long>(), nnz, mean, scale, z0,
                           a.cs.cval.as<double>());
    }
    a.z0.resize((size_t)G);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(mean_out, a.d.mean.p, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(scale_out, a.d.scale.p, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(a.z0.data(), a.d.z0.p, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        sc_set_error("%s: set-up failed on the device: %s", who, hipGetErrorString(hipGetLastError()));
        sc_resident_drop(c, c->an);
        return SC_ERR_HIP;
    }
#undef AN_TRY
    return SC_OK;
}

// which = 0: S = Z coef^T + bias (the scores of the coefficients); which = 1: Dir = Z coef^T + bias (a direction's product)
extern "C" int sc_annot_train_forward(sc_ctx *c, const double *coef, const double *bias, int32_t which)
{
    const char *who = "sc_annot_train_forward";
    SC_REQUIRE(c && coef && bias, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(c->an, SC_ERR_STATE, "%s: no training problem is resident (sc_annot_train_begin)", who);
    SC_REQUIRE(which == 0 || which == 1, SC_ERR_INVALID, "%s: which must be 0 (scores) or 1 (direction), got %d", who, which);
    AnnotTrain &a = *an_state(c);
    for (int64_t q = 0; q < (int64_t)a.T * a.G; ++q) SC_REQUIRE(std::isfinite(coef[q]), SC_ERR_INVALID, "%s: coefficients must be finite", who);
    for (int t = 0; t < a.T; ++t) SC_REQUIRE(std::isfinite(bias[t]), SC_ERR_INVALID, "%s: biases must be finite", who);
    SC_HIP(hipSetDevice(c->device));
    SC_HIP(hipStreamSynchronize(c->stream));   // the table's host copy of the previous call is free again
    SC_TRY(an_set_table(c, a.d, coef, bias, a.z0.data(), a.G, a.T, a.tab, a.base));
    {
        KernelTimerScope ts(c, SC_K_ANNOT_ROWS);
        an_launch_rows<AN_OUT_ROWS>(c, a.d, a.d.m.n, a.T, which ? a.Dir.as<double>() : a.S.as<double>(), nullptr, nullptr, nullptr);
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipStreamSynchronize(c->stream));
    (which ? a.have_dir : a.have_scores) = true;
    return SC_OK;
}

extern "C" int sc_annot_train_grad(sc_ctx *c, double *grad_out, double *loss_out)
{
    const char *who = "sc_annot_train_grad";
    SC_REQUIRE(c && grad_out && loss_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(c->an && an_state(c)->have_scores, SC_ERR_STATE, "%s: no scores are resident (sc_annot_train_forward with which = 0)", who);
    AnnotTrain &a = *an_state(c);
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int T = a.T, G = a.G, tp = an_lanes(T), nb = (T + 63) / 64;
    const int64_t cc = a.cell_chunks, chunks = a.cs.chunks;
    double *rpart = a.cellpart.as<double>(), *lpart = rpart + cc * T, *rsum = a.cellsum.as<double>(), *lsum = rsum + T;
    {
        KernelTimerScope ts(c, SC_K_ANNOT_GRAD);
        const dim3 tpb(AN_TPB), per_t((unsigned)ceil_div64(T, AN_TPB));
        hipLaunchKernelGGL(k_an_resid, dim3((unsigned)ceil_div64(cc * T, AN_TPB)), tpb, 0, s, a.S.as<double>(), a.labels.as<int32_t>(),
                           a.sw.as<double>(), a.d.m.n, T, cc, a.R.as<double>(), rpart, lpart);
        hipLaunchKernelGGL(k_chunk_add, per_t, tpb, 0, s, rpart, cc, T, rsum);
        hipLaunchKernelGGL(k_chunk_add, per_t, tpb, 0, s, lpart, cc, T, lsum);
        const dim3 grid((unsigned)ceil_div64(chunks, AN_TPB / tp));
        const int64_t *colptr = a.cs.colptr.as<int64_t>(), *cptr = a.cs.cptr.as<int64_t>();
        const int32_t *crow = a.cs.crow.as<int32_t>(), *cgene = a.cs.cgene.as<int32_t>();
        const double *cval = a.cs.cval.as<double>(), *R = a.R.as<double>();
        double *part = a.colpart.as<double>();
        switch (nb) {
        case 1: hipLaunchKernelGGL(k_an_gradcols<1>, grid, tpb, 0, s, colptr, crow, cval, cptr, cgene, chunks, T, tp, R, part); break;
        case 2: hipLaunchKernelGGL(k_an_gradcols<2>, grid, tpb, 0, s, colptr, crow, cval, cptr, cgene, chunks, T, tp, R, part); break;
        case 3: hipLaunchKernelGGL(k_an_gradcols<3>, grid, tpb, 0, s, colptr, crow, cval, cptr, cgene, chunks, T, tp, R, part); break;
        default: hipLaunchKernelGGL(k_an_gradcols<4>, grid, tpb, 0, s, colptr, crow, cval, cptr, cgene, chunks, T, tp, R, part); break;
        }
        hipLaunchKernelGGL(k_an_gradfinish, dim3((unsigned)ceil_div64((int64_t)G * T, AN_TPB)), tpb, 0, s, cptr, part, G, T, a.d.z0.as<double>(),
                           rsum, a.grad.as<double>());
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(grad_out, a.grad.p, sizeof(double) * (size_t)T * (G + 1), hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(loss_out, lsum, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}

static int an_upload_alpha(sc_ctx *c, AnnotTrain &a, const char *who, const double *alpha)
{
    for (int t = 0; t < a.T; ++t) SC_REQUIRE(std::isfinite(alpha[t]), SC_ERR_INVALID, "%s: step lengths must be finite", who);
    SC_HIP(hipMemcpyAsync(a.alpha.p, alpha, sizeof(double) * (size_t)a.T, hipMemcpyHostToDevice, c->stream));
    return SC_OK;
}

extern "C" int sc_annot_train_line(sc_ctx *c, const double *alpha, double *d1_out, double *d2_out)
{
    const char *who = "sc_annot_train_line";
    SC_REQUIRE(c && alpha && d1_out && d2_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(c->an && an_state(c)->have_scores && an_state(c)->have_dir, SC_ERR_STATE, "%s: needs resident scores and a direction product", who);
    AnnotTrain &a = *an_state(c);
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    SC_TRY(an_upload_alpha(c, a, who, alpha));
    const int T = a.T;
    const int64_t cc = a.cell_chunks;
    double *p1 = a.cellpart.as<double>(), *p2 = p1 + cc * T, *s1 = a.cellsum.as<double>(), *s2 = s1 + T;
    {
        KernelTimerScope ts(c, SC_K_ANNOT_LINE);
        const dim3 tpb(AN_TPB), per_t((unsigned)ceil_div64(T, AN_TPB));
        hipLaunchKernelGGL(k_an_line, dim3((unsigned)ceil_div64(cc * T, AN_TPB)), tpb, 0, s, a.S.as<double>(), a.Dir.as<double>(),
                           a.labels.as<int32_t>(), a.sw.as<double>(), a.alpha.as<double>(), a.d.m.n, T, cc, p1, p2);
        hipLaunchKernelGGL(k_chunk_add, per_t, tpb, 0, s, p1, cc, T, s1);
        hipLaunchKernelGGL(k_chunk_add, per_t, tpb, 0, s, p2, cc, T, s2);
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(d1_out, s1, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(d2_out, s2, sizeof(double) * (size_t)T, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}

extern "C" int sc_annot_train_step(sc_ctx *c, const double *alpha)
{
    const char *who = "sc_annot_train_step";
    SC_REQUIRE(c && alpha, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(c->an && an_state(c)->have_scores && an_state(c)->have_dir, SC_ERR_STATE, "%s: needs resident scores and a direction product", who);
    AnnotTrain &a = *an_state(c);
    SC_HIP(hipSetDevice(c->device));
    SC_TRY(an_upload_alpha(c, a, who, alpha));
    const int64_t total = a.d.m.n * a.T;
    {
        KernelTimerScope ts(c, SC_K_ANNOT_STEP);
        hipLaunchKernelGGL(k_an_step, dim3((unsigned)ceil_div64(total, AN_TPB)), dim3(AN_TPB), 0, c->stream, a.S.as<double>(), a.Dir.as<double>(),
                           a.alpha.as<double>(), total, a.T);
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}

extern "C" int sc_annot_train_end(sc_ctx *c)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "sc_annot_train_end: null pointer");
    SC_HIP(hipSetDevice(c->device));
    sc_resident_drop(c, c->an);
    return SC_OK;
}
