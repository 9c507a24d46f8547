// sc_pca.hip -- sc_pca_*: exact covariance PCA of a sparse cells x genes matrix (restated by
// tests/pca_restated.py).  What touches the n cells runs here: the optional normalisation, the Gram matrix X^T X with its
// column sums, and the projection X V^T - offset.  The G x G eigenproblem between the two is the host's (pca/decompose.py).
//
// fp64 throughout, no floating-point atomics, nothing depends on the device's configuration:
//  - the Gram matrix is cut into PCA_BLK x PCA_BLK blocks (upper triangle only) and the rows into S slices of R rows,
//    R = max(PCA_SLICE_ROWS, ceil(n / smax) rounded up to PCA_CHUNK) with smax = max(1, PCA_MAX_WG / blocks), S = ceil(n / R):
//    functions of (n, G) alone.  One workgroup owns (block, slice).  It densifies PCA_CHUNK rows at a time from the CSR into
//    two LDS column panels (zeroed per chunk; rows past the slice and columns past G stay zero) and accumulates 16 x 16 tiles
//    with v_mfma_f64_16x16x4_f64, four rows per k-step, the k-steps in ascending row order.  k_pca_block_ptr first finds, per
//    row, where each 128-column block begins, so that a workgroup reads only the entries inside its panels.
//    k_pca_gram_reduce adds the S slice sums of an element in ascending slice order and mirrors it.
//  - column sums: the workgroups of the diagonal blocks add their panel's rows in ascending order (from 0.0; a zero adds
//    nothing), one sum per (slice, column); k_pca_colsum adds the slice sums in ascending order.
//  - projection: one group of tp lanes (K rounded up to a power of two, at least 2) per row, lane = component, the row's
//    stored entries in index order with multiply and add rounded separately (-ffp-contract=off), then - offset.  A group
//    fetches tp entries at once and hands them round, four table rows in flight (sc_lane_group.h).
#include <climits>
#include <cmath>
#include <vector>

#include "sc_csr_input.h"
#include "sc_ctx.h"
#include "sc_lane_group.h"

namespace {

constexpr int PCA_TPB = 256;
constexpr int PCA_GMAX = 4096;          // the host solves a G x G eigenproblem, the device holds partial G x G sums
constexpr int PCA_KMAX = 64;            // sc_knn_dense's D_MAX: every result feeds diffusion_map
constexpr int PCA_BLK = 128;            // columns per Gram block: 8 x 8 MFMA tiles, 4 x 4 per wavefront
constexpr int PCA_CHUNK = 32;           // rows densified at a time
constexpr int PCA_LD = PCA_BLK + 16;    // LDS row stride in doubles: rows k, k + 1 of a k-step fall into different bank halves
constexpr int64_t PCA_SLICE_ROWS = 16384;
constexpr int PCA_MAX_WG = 2048;        // bounds blocks x slices, i.e. the partial sums at 2048 x 128 KiB

typedef double v4f64 __attribute__((ext_vector_type(4)));

// per row (one thread): val = (double)raw, or log1p(x / rowsum * target_sum) with the row sum in index order
template <class V>
__global__ __launch_bounds__(256) void k_pca_values(const int64_t *__restrict__ indptr, const V *__restrict__ raw, int64_t n, int normalize,
                                                    double target_sum, double *__restrict__ val)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t p0 = indptr[i], p1 = indptr[i + 1];
    if (!normalize) {
        for (int64_t p = p0; p < p1; ++p) val[p] = (double)raw[p];
        return;
    }
    double sum = 0.0;
    for (int64_t p = p0; p < p1; ++p) sum = sum + (double)raw[p];
    for (int64_t p = p0; p < p1; ++p) val[p] = sum > 0.0 ? log1p(((double)raw[p] / sum) * target_sum) : 0.0;
}

// ---- the Gram matrix ---------------------------------------------------------------------------------------------------
// bptr[row][b] = the position of row's first stored entry whose column is >= 128 b, b = 0 .. nb (b = nb: the row's end), so
// that a workgroup reads of every row only the run of entries inside its panels.  One thread per (row, b), a binary search
// in the row's ascending columns; positions fit 32 bits (stored entries <= 2^32 - 1).
__global__ __launch_bounds__(256) void k_pca_block_ptr(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices, int64_t n,
                                                       int nb, uint32_t *__restrict__ bptr)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n * (nb + 1)) return;
    const int64_t row = q / (nb + 1);
    const int target = (int)(q % (nb + 1)) * PCA_BLK;
    int64_t lo = indptr[row], hi = indptr[row + 1];
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (indices[mid] < target) lo = mid + 1;
        else hi = mid;
    }
    bptr[q] = (uint32_t)lo;
}

// grid (upper blocks, slices).  Wavefront w owns the 64 x 64 quarter (w >> 1, w & 1) of the block: 4 x 4 tiles, 16 fp64
// accumulators of 4 values.  Operand maps of v_mfma_f64_16x16x4_f64 (as k_lee_observed_mfma): A[i = lane & 15][k = lane >> 4],
// B[k = lane >> 4][j = lane & 15]; here A[i][k] = X[row k][column i of panel a], B[k][j] = X[row k][column j of panel b], both
// element [k0 + (lane >> 4)][tile * 16 + (lane & 15)] of a panel.  Result D[row = (lane >> 4) + 4 v][col = lane & 15].
// On a diagonal block panel b is panel a, and the quarter below the diagonal (w = 2) is left out: nobody reads it.
__global__ __launch_bounds__(256) void k_pca_gram(const uint32_t *__restrict__ bptr, const int32_t *__restrict__ indices,
                                                  const double *__restrict__ val, int64_t n, int64_t slice_rows,
                                                  const int2 *__restrict__ blocks, int nb, double *__restrict__ partial,
                                                  double *__restrict__ colpart)
{
    __shared__ double P[2 * PCA_CHUNK * PCA_LD];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int2 blk = blocks[blockIdx.x];
    const bool diag = blk.x == blk.y;
    const int wi = wave >> 1, wj = wave & 1;
    const bool idle = diag && wi > wj;
    const int ca0 = blk.x * PCA_BLK, cb0 = blk.y * PCA_BLK;
    const int boff = diag ? 0 : PCA_CHUNK * PCA_LD;
    const int64_t s0 = (int64_t)blockIdx.y * slice_rows;
    const int64_t s1 = s0 + slice_rows < n ? s0 + slice_rows : n;
    v4f64 acc[4][4];
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) acc[x][y] = v4f64{0.0, 0.0, 0.0, 0.0};
    double cs = 0.0;
    const int fill = diag ? PCA_CHUNK * PCA_LD : 2 * PCA_CHUNK * PCA_LD;
    for (int64_t r0 = s0; r0 < s1; r0 += PCA_CHUNK) {
        for (int q = t; q < fill; q += PCA_TPB) P[q] = 0.0;
        __syncthreads();
        // A wavefront densifies eight rows: of each row only the run of entries inside a panel's 128 columns (bptr), one
        // entry per lane, so at most two trips.  A canonical row stores a column once: no two lanes write one word
        const int rows_here = (int)(s1 - r0 < PCA_CHUNK ? s1 - r0 : PCA_CHUNK);
#pragma unroll
        for (int q = 0; q < PCA_CHUNK / 4; ++q) {
            const int lr = wave * (PCA_CHUNK / 4) + q;
            if (lr >= rows_here) break;   // the whole wavefront
            const uint32_t *bp = bptr + (r0 + lr) * (nb + 1);
            const int64_t a0 = bp[blk.x], a1 = bp[blk.x + 1];
            for (int64_t p = a0 + lane; p < a1; p += 64) P[lr * PCA_LD + (indices[p] - ca0)] = val[p];
            if (!diag) {
                const int64_t b0 = bp[blk.y], b1 = bp[blk.y + 1];
                for (int64_t p = b0 + lane; p < b1; p += 64) P[boff + lr * PCA_LD + (indices[p] - cb0)] = val[p];
            }
        }
        __syncthreads();
        if (diag && t < PCA_BLK)
            for (int r = 0; r < PCA_CHUNK; ++r) cs = cs + P[r * PCA_LD + t];
        if (!idle) {
            for (int k0 = 0; k0 < PCA_CHUNK; k0 += 4) {
                const int rowoff = (k0 + (lane >> 4)) * PCA_LD + (lane & 15);
                double a[4], b[4];
#pragma unroll
                for (int x = 0; x < 4; ++x) a[x] = P[rowoff + (wi * 4 + x) * 16];
#pragma unroll
                for (int y = 0; y < 4; ++y) b[y] = P[boff + rowoff + (wj * 4 + y) * 16];
#pragma unroll
                for (int x = 0; x < 4; ++x)
#pragma unroll
                    for (int y = 0; y < 4; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[x], b[y], acc[x][y], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    if (diag && t < PCA_BLK) colpart[((int64_t)blockIdx.y * nb + blk.x) * PCA_BLK + t] = cs;
    if (idle) return;
    double *out = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (PCA_BLK * PCA_BLK);
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                out[((wi * 4 + x) * 16 + (lane >> 4) + 4 * v) * PCA_BLK + (wj * 4 + y) * 16 + (lane & 15)] = acc[x][y][v];
}

// gram[i][j] = gram[j][i] = the slice sums of element (i, j), i <= j, in ascending slice order.  grid (64, upper blocks)
__global__ __launch_bounds__(256) void k_pca_gram_reduce(const double *__restrict__ partial, const int2 *__restrict__ blocks, int nq,
                                                         int slices, int G, double *__restrict__ gram)
{
    const int e = blockIdx.x * PCA_TPB + threadIdx.x;
    const int2 blk = blocks[blockIdx.y];
    const int i = blk.x * PCA_BLK + e / PCA_BLK, j = blk.y * PCA_BLK + e % PCA_BLK;
    if (i >= G || j >= G || i > j) return;
    double s = 0.0;
    for (int k = 0; k < slices; ++k) s = s + partial[((int64_t)k * nq + blockIdx.y) * (PCA_BLK * PCA_BLK) + e];
    gram[(int64_t)i * G + j] = s;
    gram[(int64_t)j * G + i] = s;
}

__global__ __launch_bounds__(256) void k_pca_colsum(const double *__restrict__ colpart, int nb, int slices, int G, double *__restrict__ colsum)
{
    const int g = blockIdx.x * PCA_TPB + threadIdx.x;
    if (g >= G) return;
    double s = 0.0;
    for (int k = 0; k < slices; ++k) s = s + colpart[((int64_t)k * nb + g / PCA_BLK) * PCA_BLK + g % PCA_BLK];
    colsum[g] = s;
}

// ---- the projection ----------------------------------------------------------------------------------------------------
// One group of tp lanes per row, lane l = component l; table[g][K] is V transposed.  256 / tp rows per workgroup.
template <class O>
__global__ __launch_bounds__(256) void k_pca_rows(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                  const double *__restrict__ val, int64_t n, int K, int tp,
                                                  const double *__restrict__ table, const double *__restrict__ offset,
                                                  O *__restrict__ out)
{
    const int t = threadIdx.x, grp = t / tp, l = t % tp;
    const int64_t i = (int64_t)blockIdx.x * (PCA_TPB / tp) + grp;
    if (i >= n) return;   // the whole group leaves
    const bool mine = l < K;
    double acc = 0.0;
    lane_group_walk(indices, val, indptr[i], indptr[i + 1], tp, l, [&](int32_t g) { return mine ? table[(int64_t)g * K + l] : 0.0; },
                    [&](double x, double w) { acc = acc + x * w; });
    if (mine) out[i * K + l] = (O)(acc - offset[l]);
}

}  // namespace

// the matrix resident between sc_pca_begin and sc_pca_end, and the scratch of _gram and _project
struct PcaState : Resident {
    CsrDevice m;   // m.raw only inside sc_pca_begin
    DBuf bptr, blocks, partial, colpart, gram, colsum, table, offset, out;
    int G = 0;
};
static PcaState *pca_state(const sc_ctx *c) { return resident<PcaState>(c->pca); }

extern "C" int sc_pca_begin(sc_ctx *c, const int64_t *indptr, const int32_t *indices, const void *data, int dtype, int64_t n,
                            int32_t n_genes, int32_t normalize, double target_sum)
{
    const char *who = "sc_pca_begin";
    SC_REQUIRE(c && indptr, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "%s: dtype must be SC_F32 or SC_F64", who);
    SC_REQUIRE(n >= 2 && n <= INT32_MAX, SC_ERR_INVALID, "%s: need 2 <= n <= 2^31 - 1, got %lld", who, (long long)n);
    SC_REQUIRE(n_genes >= 1 && n_genes <= PCA_GMAX, SC_ERR_INVALID, "%s: need 1 <= n_genes <= %d, got %d", who, PCA_GMAX, n_genes);
    SC_REQUIRE(!normalize || (std::isfinite(target_sum) && target_sum > 0.0), SC_ERR_INVALID, "%s: target_sum must be finite and > 0", who);
    int64_t nnz = 0;
    SC_TRY(csr_check_offsets(who, indptr, n, &nnz));
    SC_REQUIRE(nnz <= (int64_t)UINT32_MAX, SC_ERR_INVALID, "%s: need stored entries <= 2^32 - 1, got %lld", who, (long long)nnz);
    SC_REQUIRE(nnz == 0 || (indices && data), SC_ERR_INVALID, "%s: null pointer", who);
    SC_TRY(csr_check_columns(who, indptr, indices, n, n_genes, "n_genes"));
    SC_TRY(csr_check_values(who, data, dtype, nnz, normalize != 0, " (normalize needs counts)"));

    SC_HIP(hipSetDevice(c->device));
    sc_resident_drop(c, c->pca);
    c->pca.reset(new PcaState());
    PcaState &s = *pca_state(c);
    hipStream_t st = c->stream;
    s.G = n_genes;
    const int rc = s.m.upload(c, indptr, indices, data, dtype, n, nnz);
    if (rc != SC_OK) {
        sc_resident_drop(c, c->pca);
        return rc;
    }
    {
        KernelTimerScope ts(c, SC_K_PCA_SETUP);
        const dim3 per_row((unsigned)ceil_div64(n, PCA_TPB)), tpb(PCA_TPB);
        if (dtype == SC_F32)
            hipLaunchKernelGGL(k_pca_values<float>, per_row, tpb, 0, st, s.m.indptr.as<int64_t>(), s.m.raw.as<float>(), n, normalize, target_sum, s.m.val.as<double>());
        else
            hipLaunchKernelGGL(k_pca_values<double>, per_row, tpb, 0, st, s.m.indptr.as<int64_t>(), s.m.raw.as<double>(), n, normalize, target_sum, s.m.val.as<double>());
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {   // the caller's arrays are free again
        sc_set_error("%s: upload failed on the device: %s", who, hipGetErrorString(hipGetLastError()));
        sc_resident_drop(c, c->pca);
        return SC_ERR_HIP;
    }
    s.m.raw.release();
    return SC_OK;
}

extern "C" int sc_pca_values(sc_ctx *c, double *values_out)
{
    const char *who = "sc_pca_values";
    SC_REQUIRE(c && values_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(c->pca, SC_ERR_STATE, "%s: no matrix is resident (sc_pca_begin)", who);
    const CsrDevice &m = pca_state(c)->m;
    if (!m.nnz) return SC_OK;
    SC_HIP(hipSetDevice(c->device));
    SC_HIP(hipMemcpyAsync(values_out, m.val.p, sizeof(double) * (size_t)m.nnz, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}

extern "C" int sc_pca_gram(sc_ctx *c, double *colsum_out, double *gram_out)
{
    const char *who = "sc_pca_gram";
    SC_REQUIRE(c && colsum_out && gram_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(c->pca, SC_ERR_STATE, "%s: no matrix is resident (sc_pca_begin)", who);
    PcaState &s = *pca_state(c);
    SC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int G = s.G, nb = (G + PCA_BLK - 1) / PCA_BLK, nq = nb * (nb + 1) / 2;
    std::vector<int2> blocks;
    for (int bi = 0; bi < nb; ++bi)
        for (int bj = bi; bj < nb; ++bj) blocks.push_back(int2{bi, bj});
    // the slices: a function of (n, G) alone
    const int64_t smax = PCA_MAX_WG / nq > 1 ? PCA_MAX_WG / nq : 1;
    const int64_t even = align_up64(ceil_div64(s.m.n, smax), PCA_CHUNK);
    const int64_t slice_rows = even > PCA_SLICE_ROWS ? even : PCA_SLICE_ROWS;
    const int slices = (int)ceil_div64(s.m.n, slice_rows);
    SC_TRY(s.bptr.ensure(sizeof(uint32_t) * (size_t)s.m.n * (nb + 1), &c->mem));
    SC_TRY(s.blocks.ensure(sizeof(int2) * (size_t)nq, &c->mem));
    SC_TRY(s.partial.ensure(sizeof(double) * (size_t)slices * nq * PCA_BLK * PCA_BLK, &c->mem));
    SC_TRY(s.colpart.ensure(sizeof(double) * (size_t)slices * nb * PCA_BLK, &c->mem));
    SC_TRY(s.gram.ensure(sizeof(double) * (size_t)G * G, &c->mem));
    SC_TRY(s.colsum.ensure(sizeof(double) * (size_t)G, &c->mem));
    SC_HIP(hipMemcpyAsync(s.blocks.p, blocks.data(), sizeof(int2) * (size_t)nq, hipMemcpyHostToDevice, st));
    {
        KernelTimerScope ts(c, SC_K_PCA_GRAM);
        hipLaunchKernelGGL(k_pca_block_ptr, dim3((unsigned)ceil_div64(s.m.n * (nb + 1), PCA_TPB)), dim3(PCA_TPB), 0, st, s.m.indptr.as<int64_t>(),
                           s.m.indices.as<int32_t>(), s.m.n, nb, s.bptr.as<uint32_t>());
        hipLaunchKernelGGL(k_pca_gram, dim3((unsigned)nq, (unsigned)slices), dim3(PCA_TPB), 0, st, s.bptr.as<uint32_t>(), s.m.indices.as<int32_t>(),
                           s.m.val.as<double>(), s.m.n, slice_rows, s.blocks.as<int2>(), nb, s.partial.as<double>(), s.colpart.as<double>());
        hipLaunchKernelGGL(k_pca_gram_reduce, dim3(PCA_BLK * PCA_BLK / PCA_TPB, (unsigned)nq), dim3(PCA_TPB), 0, st, s.partial.as<double>(),
                           s.blocks.as<int2>(), nq, slices, G, s.gram.as<double>());
        hipLaunchKernelGGL(k_pca_colsum, dim3((unsigned)ceil_div64(G, PCA_TPB)), dim3(PCA_TPB), 0, st, s.colpart.as<double>(), nb, slices, G,
                           s.colsum.as<double>());
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(gram_out, s.gram.p, sizeof(double) * (size_t)G * G, hipMemcpyDeviceToHost, st));
    SC_HIP(hipMemcpyAsync(colsum_out, s.colsum.p, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost, st));
    SC_HIP(hipStreamSynchronize(st));   // `blocks` lives until here
    return SC_OK;
}

extern "C" int sc_pca_project(sc_ctx *c, const double *V, const double *offset, int32_t K, int out_dtype, void *scores_out)
{
    const char *who = "sc_pca_project";
    SC_REQUIRE(c && V && offset && scores_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(K >= 1 && K <= PCA_KMAX, SC_ERR_INVALID, "%s: need 1 <= K <= %d, got %d", who, PCA_KMAX, K);
    SC_REQUIRE(out_dtype == SC_F32 || out_dtype == SC_F64, SC_ERR_INVALID, "%s: out_dtype must be SC_F32 or SC_F64", who);
    SC_REQUIRE(c->pca, SC_ERR_STATE, "%s: no matrix is resident (sc_pca_begin)", who);
    PcaState &s = *pca_state(c);
    const int G = s.G;
    std::vector<double> tab((size_t)G * K);
    for (int k = 0; k < K; ++k) {
        SC_REQUIRE(std::isfinite(offset[k]), SC_ERR_INVALID, "%s: offset[%d] is not finite", who, k);
        for (int g = 0; g < G; ++g) {
            const double w = V[(size_t)k * G + g];
            SC_REQUIRE(std::isfinite(w), SC_ERR_INVALID, "%s: loading %lld is not finite", who, (long long)((size_t)k * G + g));
            tab[(size_t)g * K + k] = w;
        }
    }
    SC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t os = out_dtype == SC_F32 ? sizeof(float) : sizeof(double);
    SC_TRY(s.table.ensure(sizeof(double) * (size_t)G * K, &c->mem));
    SC_TRY(s.offset.ensure(sizeof(double) * (size_t)K, &c->mem));
    SC_TRY(s.out.ensure(os * (size_t)s.m.n * K, &c->mem));
    SC_HIP(hipMemcpyAsync(s.table.p, tab.data(), sizeof(double) * (size_t)G * K, hipMemcpyHostToDevice, st));
    SC_HIP(hipMemcpyAsync(s.offset.p, offset, sizeof(double) * (size_t)K, hipMemcpyHostToDevice, st));
    {
        KernelTimerScope ts(c, SC_K_PCA_PROJECT);
        const int tp = lanes_for(K, 2, PCA_KMAX);
        const dim3 grid((unsigned)ceil_div64(s.m.n, PCA_TPB / tp)), block(PCA_TPB);
        if (out_dtype == SC_F32)
            hipLaunchKernelGGL(k_pca_rows<float>, grid, block, 0, st, s.m.indptr.as<int64_t>(), s.m.indices.as<int32_t>(), s.m.val.as<double>(), s.m.n, K, tp,
                               s.table.as<double>(), s.offset.as<double>(), s.out.as<float>());
        else
            hipLaunchKernelGGL(k_pca_rows<double>, grid, block, 0, st, s.m.indptr.as<int64_t>(), s.m.indices.as<int32_t>(), s.m.val.as<double>(), s.m.n, K, tp,
                               s.table.as<double>(), s.offset.as<double>(), s.out.as<double>());
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(scores_out, s.out.p, os * (size_t)s.m.n * K, hipMemcpyDeviceToHost, st));
    SC_HIP(hipStreamSynchronize(st));   // `tab` lives until here
    return SC_OK;
}

extern "C" int sc_pca_end(sc_ctx *c)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "sc_pca_end: null pointer");
    if (!c->pca) return SC_OK;
    SC_HIP(hipSetDevice(c->device));
    sc_resident_drop(c, c->pca);
    return SC_OK;
}
