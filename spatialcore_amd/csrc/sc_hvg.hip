// sc_hvg.hip -- sc_hvg_pearson: per-gene variance of the analytic Pearson residuals of a sparse cells x genes count matrix
// (Lause, Berens & Kobak 2021; restated line by line by tests/hvg_restated.py: ordered()).
//
// Nothing is densified.  The two sums of a gene, S1 = sum_i r_ig and S2 = sum_i r_ig^2 over all n cells, are split into
//  - the dense zero term: r0_ig, the residual the pair would have if x_ig were 0, summed over ALL n cells.  It needs only
//    the row sums s (8 bytes per cell) and p_g.  A thread owns a gene, a workgroup HVG_BLK genes and one slice of cells;
//    the slice length is a function of n alone (hvg_slice_rows).  k_chunk_add adds the slices in slice order.
//  - the sparse correction: (r - r0, r^2 - r0^2) per stored entry, over the column-sorted copy (sc_colsort.h) in chunks of
//    COL_CHUNK entries, a thread per chunk in index order; k_hvg_finish adds a gene's chunks in chunk order.
// fp64 throughout, no floating-point atomics, nothing depends on the device's configuration.  The one expression order:
//    s_i   = 0.0 + the row's stored values in index order
//    t_g   = 0.0 + the gene's chunk sums in chunk order, a chunk sum = 0.0 + its values in row order (q_g: of x * x)
//    T     = 0.0 + a[0] + ... + a[255], a[j] = 0.0 + t_j + t_(j + 256) + ...            (k_hvg_total)
//    p_g   = t_g / T,  mu = s_i * p_g,  v = mu * (1.0 + mu * (1.0 / theta))               (1.0 / theta once, on the host)
//    z(x)  = (x - mu) / sqrt(v),  r = min(max(z(x), -clip), clip),  r0 = max(z(0.0), -clip);  mu == 0: r = r0 = 0
//    S1_g  = D1 + C1, D1 = 0.0 + slice sums in slice order (a slice sum = 0.0 + r0 in cell order), C1 = 0.0 + chunk sums
//            of (r - r0) in chunk order; S2_g the same with r0 * r0 and r * r - r0 * r0
//    mean  = S1 / n,  var = max(S2 / n - mean * mean, 0.0)
// Division and square root are the correctly rounded ones; -ffp-contract=off keeps every multiply and add apart.
#include <climits>
#include <cmath>

#include "sc_colsort.h"
#include "sc_csr_input.h"
#include "sc_ctx.h"

namespace {

constexpr int HVG_BLK = 256;                // genes per workgroup of the dense term, one per thread
constexpr int64_t HVG_SLICE = 1024;         // cells per slice of the dense term ...
constexpr int64_t HVG_MAX_SLICES = 4096;    // ... doubled, tripled, ... once n needs more slices than this
constexpr int HVG_GMAX = 32768;             // sc_colsort.h's chunk scan is one thread

inline int64_t hvg_slice_rows(int64_t n) { return HVG_SLICE * ceil_div64(n, HVG_SLICE * HVG_MAX_SLICES); }

// the residual of a count x at mean mu > 0
__device__ __forceinline__ double hvg_z(double x, double mu, double inv_theta)
{
    const double v = mu * (1.0 + mu * inv_theta);
    return (x - mu) / sqrt(v);
}

// per row (one thread): the fp64 values and the row sum in index order
template <class V>
__global__ __launch_bounds__(256) void k_hvg_rows(const int64_t *__restrict__ indptr, const V *__restrict__ raw, int64_t n,
                                                  double *__restrict__ val, double *__restrict__ s)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double sum = 0.0;
    for (int64_t p = indptr[i]; p < indptr[i + 1]; ++p) {
        const double x = (double)raw[p];
        val[p] = x;
        sum = sum + x;
    }
    s[i] = sum;
}

// per column chunk (one thread): part[c] = sum x, part[chunks + c] = sum x * x, in row order
__global__ __launch_bounds__(256) void k_hvg_colsum_chunks(const int64_t *__restrict__ colptr, const int64_t *__restrict__ cptr,
                                                           const int32_t *__restrict__ cgene, const double *__restrict__ cval,
                                                           int64_t chunks, double *__restrict__ part)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= chunks) return;
    const ColChunk ch = col_chunk(colptr, cptr, cgene, c);
    double a = 0.0, b = 0.0;
    for (int64_t p = ch.p0; p < ch.p1; ++p) {
        const double x = cval[p];
        a = a + x;
        b = b + x * x;
    }
    part[c] = a;
    part[chunks + c] = b;
}

// per gene (one thread): out[g] = part[c], out[G + g] = part[chunks + c] over the gene's chunks in chunk order
__global__ __launch_bounds__(256) void k_hvg_gene_add(const int64_t *__restrict__ cptr, const double *__restrict__ part, int64_t chunks,
                                                      int G, double *__restrict__ out)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    double a = 0.0, b = 0.0;
    for (int64_t c = cptr[g]; c < cptr[g + 1]; ++c) {
        a = a + part[c];
        b = b + part[chunks + c];
    }
    out[g] = a;
    out[G + g] = b;
}

// one workgroup of 256: thread j adds t_j, t_(j + 256), ... in order; thread 0 adds the 256 sums in order
__global__ __launch_bounds__(256) void k_hvg_total(const double *__restrict__ t, int G, double *__restrict__ total)
{
    __shared__ double a[256];
    double s = 0.0;
    for (int g = threadIdx.x; g < G; g += 256) s = s + t[g];
    a[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double T = 0.0;
    for (int j = 0; j < 256; ++j) T = T + a[j];
    total[0] = T;
}

// ---- the dense zero term: grid (gene blocks, slices) ---------------------------------------------------------------------
// Every lane of a wavefront reads the same s[i]: a uniform address, one scalar load per cell and wavefront.
__global__ __launch_bounds__(HVG_BLK) void k_hvg_dense(const double *__restrict__ s, const double *__restrict__ t,
                                                       const double *__restrict__ total, int64_t n, int G, int64_t slice_rows,
                                                       double inv_theta, double clip, double *__restrict__ dpart)
{
    const int g = blockIdx.x * HVG_BLK + threadIdx.x;
    if (g >= G) return;
    const double p = t[g] / total[0];
    const double lo = 0.0 - clip;
    const int64_t i0 = (int64_t)blockIdx.y * slice_rows;
    const int64_t i1 = i0 + slice_rows < n ? i0 + slice_rows : n;
    double a = 0.0, b = 0.0;
#pragma unroll 4
    for (int64_t i = i0; i < i1; ++i) {
        const double mu = s[i] * p;
        const double z = hvg_z(0.0, mu, inv_theta);   // mu == 0: NaN, dropped by the last select; no branch in the loop
        double r0 = z > lo ? z : lo;
        r0 = mu > 0.0 ? r0 : 0.0;
        a = a + r0;
        b = b + r0 * r0;
    }
    double *out = dpart + (int64_t)blockIdx.y * 2 * G;
    out[g] = a;
    out[G + g] = b;
}

// ---- the sparse correction: per column chunk (one thread), part[c] = sum (r - r0), part[chunks + c] = sum (r r - r0 r0) ----
__global__ __launch_bounds__(256) void k_hvg_correct_chunks(const int64_t *__restrict__ colptr, const int64_t *__restrict__ cptr,
                                                            const int32_t *__restrict__ cgene, const int32_t *__restrict__ crow,
                                                            const double *__restrict__ cval, int64_t chunks,
                                                            const double *__restrict__ s, const double *__restrict__ t,
                                                            const double *__restrict__ total, double inv_theta, double clip,
                                                            double *__restrict__ part)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= chunks) return;
    const ColChunk ch = col_chunk(colptr, cptr, cgene, c);
    const double p = t[ch.g] / total[0];
    const double lo = 0.0 - clip;
    double a = 0.0, b = 0.0;
    for (int64_t q = ch.p0; q < ch.p1; ++q) {
        const double mu = s[crow[q]] * p;
        double r = 0.0, r0 = 0.0;
        if (mu > 0.0) {
            const double z0 = hvg_z(0.0, mu, inv_theta);
            r0 = z0 > lo ? z0 : lo;
            const double z = hvg_z(cval[q], mu, inv_theta);
            r = z > lo ? z : lo;
            r = r < clip ? r : clip;
        }
        a = a + (r - r0);
        b = b + (r * r - r0 * r0);
    }
    part[c] = a;
    part[chunks + c] = b;
}

// per gene (one thread): dsum = the slice sums added in slice order (k_chunk_add), the gene's chunk sums in chunk order, the
// mean and the variance
__global__ __launch_bounds__(256) void k_hvg_finish(const int64_t *__restrict__ cptr, const double *__restrict__ dsum,
                                                    const double *__restrict__ part, int64_t chunks, int G, int64_t n,
                                                    double *__restrict__ mean_out, double *__restrict__ var_out)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    double c1 = 0.0, c2 = 0.0;
    for (int64_t c = cptr[g]; c < cptr[g + 1]; ++c) {
        c1 = c1 + part[c];
        c2 = c2 + part[chunks + c];
    }
    const double dn = (double)n;
    const double m = (dsum[g] + c1) / dn;
    const double var = (dsum[G + g] + c2) / dn - m * m;
    mean_out[g] = m;
    var_out[g] = var > 0.0 ? var : 0.0;
}

// a call's own buffers
struct HvgBufs {
    CsrDevice m;
    ColSort cs;
    DBuf s, sums, total, part, dpart, dsum, out;
};

// true if any stored value is > 0
template <class V>
bool hvg_any_positive(const V *data, int64_t nnz)
{
    for (int64_t p = 0; p < nnz; ++p)
        if (data[p] > (V)0) return true;
    return false;
}

}  // namespace

extern "C" int sc_hvg_pearson(sc_ctx *c, const int64_t *indptr, const int32_t *indices, const void *data, int dtype, int64_t n,
                              int32_t n_genes, double theta, double clip, double *sum_out, double *sumsq_out,
                              double *resid_mean_out, double *resid_var_out)
{
    const char *who = "sc_hvg_pearson";
    SC_REQUIRE(c && indptr && sum_out && sumsq_out && resid_mean_out && resid_var_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "%s: dtype must be SC_F32 or SC_F64", who);
    SC_REQUIRE(n >= 2 && n <= INT32_MAX, SC_ERR_INVALID, "%s: need 2 <= n <= 2^31 - 1, got %lld", who, (long long)n);
    SC_REQUIRE(n_genes >= 1 && n_genes <= HVG_GMAX, SC_ERR_INVALID, "%s: need 1 <= n_genes <= %d, got %d", who, HVG_GMAX, n_genes);
    SC_REQUIRE(theta > 0.0, SC_ERR_INVALID, "%s: theta must be > 0 (infinity: Poisson)", who);
    SC_REQUIRE(clip > 0.0, SC_ERR_INVALID, "%s: clip must be > 0", who);
    int64_t nnz = 0;
    SC_TRY(csr_check_offsets(who, indptr, n, &nnz));
    SC_REQUIRE(nnz <= (int64_t)UINT32_MAX, SC_ERR_INVALID, "%s: need stored entries <= 2^32 - 1, got %lld", who, (long long)nnz);
    SC_REQUIRE(nnz == 0 || (indices && data), SC_ERR_INVALID, "%s: null pointer", who);
    SC_TRY(csr_check_columns(who, indptr, indices, n, n_genes, "n_genes"));
    SC_TRY(csr_check_values(who, data, dtype, nnz, true, " (Pearson residuals need counts)"));
    SC_REQUIRE(dtype == SC_F32 ? hvg_any_positive((const float *)data, nnz) : hvg_any_positive((const double *)data, nnz), SC_ERR_INVALID,
               "%s: the matrix is all zero", who);

    SC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int G = n_genes;
    const double inv_theta = 1.0 / theta;
    const int64_t slice_rows = hvg_slice_rows(n), slices = ceil_div64(n, slice_rows);
    HvgBufs b;
    StreamWaitOnExit wait{c->stream};   // after the buffers: an early return may leave work on them in flight
    SC_TRY(b.m.upload(c, indptr, indices, data, dtype, n, nnz));
    SC_TRY(colsort_alloc(c, b.cs, nnz, G));
    SC_TRY(b.s.ensure(sizeof(double) * (size_t)n, &c->mem));
    SC_TRY(b.sums.ensure(sizeof(double) * (size_t)G * 2, &c->mem));
    SC_TRY(b.total.ensure(sizeof(double), &c->mem));
    SC_TRY(b.dpart.ensure(sizeof(double) * (size_t)slices * 2 * G, &c->mem));
    SC_TRY(b.dsum.ensure(sizeof(double) * (size_t)G * 2, &c->mem));
    SC_TRY(b.out.ensure(sizeof(double) * (size_t)G * 2, &c->mem));
    const dim3 tpb(256), per_row((unsigned)ceil_div64(n, 256)), per_gene((unsigned)ceil_div64(G, 256));
    {
        KernelTimerScope ts(c, SC_K_HVG_SETUP);
        if (dtype == SC_F32)
            hipLaunchKernelGGL(k_hvg_rows<float>, per_row, tpb, 0, st, b.m.indptr.as<int64_t>(), b.m.raw.as<float>(), n, b.m.val.as<double>(), b.s.as<double>());
        else
            hipLaunchKernelGGL(k_hvg_rows<double>, per_row, tpb, 0, st, b.m.indptr.as<int64_t>(), b.m.raw.as<double>(), n, b.m.val.as<double>(), b.s.as<double>());
        SC_TRY(colsort_enqueue(c, b.cs, b.m.indptr.as<int64_t>(), b.m.indices.as<int32_t>(), b.m.val.as<double>(), n, G, nnz));
    }
    SC_TRY(colsort_finish(c, b.cs, G, nnz, who));   // waits: the caller's arrays are free again
    const int64_t chunks = b.cs.chunks;
    SC_TRY(b.part.ensure(sizeof(double) * (size_t)chunks * 2, &c->mem));
    const dim3 per_chunk((unsigned)ceil_div64(chunks, 256));
    const int64_t *colptr = b.cs.colptr.as<int64_t>(), *cptr = b.cs.cptr.as<int64_t>();
    const int32_t *cgene = b.cs.cgene.as<int32_t>();
    double *t = b.sums.as<double>(), *total = b.total.as<double>(), *part = b.part.as<double>();
    {
        KernelTimerScope ts(c, SC_K_HVG_SETUP);
        hipLaunchKernelGGL(k_hvg_colsum_chunks, per_chunk, tpb, 0, st, colptr, cptr, cgene, b.cs.cval.as<double>(), chunks, part);
        hipLaunchKernelGGL(k_hvg_gene_add, per_gene, tpb, 0, st, cptr, part, chunks, G, t);
        hipLaunchKernelGGL(k_hvg_total, dim3(1), tpb, 0, st, t, G, total);
    }
    {
        KernelTimerScope ts(c, SC_K_HVG_DENSE);
        hipLaunchKernelGGL(k_hvg_dense, dim3((unsigned)ceil_div64(G, HVG_BLK), (unsigned)slices), dim3(HVG_BLK), 0, st, b.s.as<double>(), t, total, n, G,
                           slice_rows, inv_theta, clip, b.dpart.as<double>());
        hipLaunchKernelGGL(k_chunk_add, dim3((unsigned)ceil_div64(2 * G, 256)), tpb, 0, st, b.dpart.as<double>(), slices, 2 * G, b.dsum.as<double>());
    }
    {
        KernelTimerScope ts(c, SC_K_HVG_SPARSE);
        hipLaunchKernelGGL(k_hvg_correct_chunks, per_chunk, tpb, 0, st, colptr, cptr, cgene, b.cs.crow.as<int32_t>(), b.cs.cval.as<double>(), chunks,
                           b.s.as<double>(), t, total, inv_theta, clip, part);
        hipLaunchKernelGGL(k_hvg_finish, per_gene, tpb, 0, st, cptr, b.dsum.as<double>(), part, chunks, G, n, b.out.as<double>(),
                           b.out.as<double>() + G);
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(sum_out, t, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost, st));
    SC_HIP(hipMemcpyAsync(sumsq_out, t + G, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost, st));
    SC_HIP(hipMemcpyAsync(resid_mean_out, b.out.p, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost, st));
    SC_HIP(hipMemcpyAsync(resid_var_out, b.out.as<double>() + G, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost, st));
    SC_HIP(hipStreamSynchronize(st));
    return SC_OK;
}
