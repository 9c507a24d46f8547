// Expression tiles: upload, per-gene column reductions, centring / z-scores, the spatial lag of the tiles, and the
// narrow exact copies of the raw values.  gfx950 only.
//
// Device layout (DESIGN.md "Data layout"): genes are grouped in tiles of SC_TILE = 16; a tile is
// [cell][16] fp64, i.e. one 128-byte row per cell.  A permutation step `lag[perm[i]]` then gathers
// one full cache line that serves 16 genes at once, and the contiguous operand z[i] is a coalesced
// 128-byte row.
#include <math.h>

#include <vector>

#include "sc_ctx.h"

// ------------------------------------------------------------------------------------------------
// expression upload
// ------------------------------------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(256) void k_scatter_csr(const int64_t *__restrict__ indptr,
                                                      const int32_t *__restrict__ indices,
                                                      const T *__restrict__ data,
                                                      const int32_t *__restrict__ colmap,
                                                      double *__restrict__ X, int64_t rows,
                                                      int64_t n, int64_t n_vars, int64_t row0)
{
    // one wavefront per matrix row; lanes stride over the row's stored entries.
    // X points at the chunk's first row inside tile 0; n is the full cell count (tile stride).
    int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    int lane = threadIdx.x & 63;
    if (row >= rows) return;
    int64_t e0 = indptr[row] - row0, e1 = indptr[row + 1] - row0;
    for (int64_t e = e0 + lane; e < e1; e += 64) {
        int32_t c = indices[e];
        if ((uint32_t)c >= (uint64_t)n_vars) continue;
        int32_t slot = colmap[c];
        if (slot >= 0)
            X[(int64_t)(slot >> 4) * n * SC_TILE + row * SC_TILE + (slot & 15)] = (double)data[e];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_gather_dense(const T *__restrict__ data, int64_t ld,
                                                       const int32_t *__restrict__ gene_cols,
                                                       int64_t n_genes, double *__restrict__ X,
                                                       int64_t n, int64_t row_lo, int64_t rows)
{
    // thread = (row, slot) of one tile (blockIdx.y); padded slots are written as 0
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t r = t >> 4;
    int s = (int)(t & 15);
    if (r >= rows) return;
    int64_t g = (int64_t)blockIdx.y * SC_TILE + s;
    double v = 0.0;
    if (g < n_genes) v = (double)data[r * ld + gene_cols[g]];
    X[(int64_t)blockIdx.y * n * SC_TILE + (row_lo + r) * SC_TILE + s] = v;
}

static int expr_alloc(sc_ctx *c, int64_t n, int64_t n_genes)
{
    SC_REQUIRE(n >= 1 && n <= 0x7fffffffLL, SC_ERR_INVALID, "n_cells=%lld out of range", (long long)n);
    SC_REQUIRE(n_genes >= 1 && n_genes <= (1 << 24), SC_ERR_INVALID, "n_genes=%lld out of range",
               (long long)n_genes);
    int64_t tiles = ceil_div64(n_genes, SC_TILE);
    size_t bytes = (size_t)tiles * n * SC_TILE * sizeof(double);
    SC_TRY(c->X.ensure(bytes, &c->mem));
    size_t gb = (size_t)align_up64(tiles, 8) * SC_TILE * sizeof(double);  // the narrow-source kernels read whole groups
    SC_TRY(c->g_mean.ensure(gb, &c->mem));
    SC_TRY(c->g_var.ensure(gb, &c->mem));
    SC_TRY(c->g_z2.ensure(gb, &c->mem));
    SC_TRY(c->g_scale.ensure(gb, &c->mem));
    SC_TRY(c->g_Inum.ensure(gb, &c->mem));
    SC_TRY(c->g_xsum.ensure(gb, &c->mem));
    SC_TRY(c->g_meanc.ensure(gb, &c->mem));
    SC_TRY(c->g_lat.ensure(gb, &c->mem));
    c->e_n = n;
    c->e_genes = n_genes;
    c->e_tiles = tiles;
    c->narrow_bits = 64;
    c->lat_any = false;
    c->lm_valid = false;
    c->prep_early = false;
    return SC_OK;
}


extern "C" int sc_expr_set_csr(sc_ctx *c, const int64_t *indptr, const int32_t *indices,
                               const void *data, int dtype, int64_t n, int64_t n_vars,
                               const int32_t *gene_cols, int64_t n_genes)
{
    SC_REQUIRE(c && indptr && gene_cols, SC_ERR_INVALID, "sc_expr_set_csr: null pointer");
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "sc_expr_set_csr: bad dtype %d", dtype);
    SC_REQUIRE(n_vars >= 1 && n_vars <= 0x7fffffffLL, SC_ERR_INVALID, "n_vars out of range");
    SC_HIP(hipSetDevice(c->device));
    c->e_n = 0;
    SC_TRY(expr_alloc(c, n, n_genes));
    c->e_dtype = dtype;
    SC_REQUIRE(indptr[0] == 0, SC_ERR_INVALID, "sc_expr_set_csr: indptr[0] must be 0");
    for (int64_t i = 0; i < n; ++i)
        SC_REQUIRE(indptr[i + 1] >= indptr[i], SC_ERR_INVALID, "sc_expr_set_csr: indptr not monotone at row %lld",
                   (long long)i);
    int64_t nnz = indptr[n];
    SC_REQUIRE(nnz == 0 || (indices && data), SC_ERR_INVALID, "sc_expr_set_csr: null indices/data");
    std::vector<int32_t> colmap((size_t)n_vars, -1);
    for (int64_t g = 0; g < n_genes; ++g) {
        SC_REQUIRE(gene_cols[g] >= 0 && gene_cols[g] < n_vars, SC_ERR_INVALID, "gene column %d out of range",
                   gene_cols[g]);
        SC_REQUIRE(colmap[gene_cols[g]] < 0, SC_ERR_INVALID, "gene column %d listed twice", gene_cols[g]);
        colmap[gene_cols[g]] = (int32_t)g;
    }
    SC_TRY(c->e_colmap.ensure(sizeof(int32_t) * (size_t)n_vars, &c->mem));
    SC_HIP(hipMemcpyAsync(c->e_colmap.p, colmap.data(), sizeof(int32_t) * (size_t)n_vars,
                          hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemsetAsync(c->X.p, 0, (size_t)c->e_tiles * n * SC_TILE * sizeof(double), c->stream));
    SC_TRY(c->e_tmp_indptr.ensure(sizeof(int64_t) * (size_t)(n + 1), &c->mem));
    SC_HIP(hipMemcpyAsync(c->e_tmp_indptr.p, indptr, sizeof(int64_t) * (size_t)(n + 1),
                          hipMemcpyHostToDevice, c->stream));
    // stream the stored entries through the device in row chunks of <= 256 Mi entries
    const int64_t max_chunk = (int64_t)1 << 28;
    size_t esz = dtype == SC_F32 ? 4 : 8;
    int64_t r0 = 0;
    while (r0 < n) {
        int64_t r1 = r0 + 1;
        while (r1 < n && indptr[r1 + 1] - indptr[r0] <= max_chunk) ++r1;
        int64_t e0 = indptr[r0], cnt = indptr[r1] - e0;
        if (cnt > 0) {
            SC_TRY(c->e_tmp_indices.ensure(sizeof(int32_t) * (size_t)cnt, &c->mem));
            SC_TRY(c->e_tmp_data.ensure(esz * (size_t)cnt, &c->mem));
            SC_HIP(hipMemcpyAsync(c->e_tmp_indices.p, indices + e0, sizeof(int32_t) * (size_t)cnt,
                                  hipMemcpyHostToDevice, c->stream));
            SC_HIP(hipMemcpyAsync(c->e_tmp_data.p, (const char *)data + esz * (size_t)e0, esz * (size_t)cnt,
                                  hipMemcpyHostToDevice, c->stream));
            int64_t rows = r1 - r0;
            unsigned grid = (unsigned)ceil_div64(rows * 64, 256);
            const int64_t *ip = c->e_tmp_indptr.as<int64_t>() + r0;
            double *Xr = c->X.as<double>() + r0 * SC_TILE;
            // Xr is offset by r0 rows inside every tile: tile stride stays n*16
            if (dtype == SC_F32)
                hipLaunchKernelGGL(k_scatter_csr<float>, dim3(grid), dim3(256), 0, c->stream, ip,
                                   c->e_tmp_indices.as<int32_t>(), c->e_tmp_data.as<float>(),
                                   c->e_colmap.as<int32_t>(), Xr, rows, n, n_vars, e0);
            else
                hipLaunchKernelGGL(k_scatter_csr<double>, dim3(grid), dim3(256), 0, c->stream, ip,
                                   c->e_tmp_indices.as<int32_t>(), c->e_tmp_data.as<double>(),
                                   c->e_colmap.as<int32_t>(), Xr, rows, n, n_vars, e0);
            SC_HIP(hipGetLastError());
            // the staging buffers are reused by the next chunk
            SC_HIP(hipStreamSynchronize(c->stream));
        }
        r0 = r1;
    }
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}

extern "C" int sc_expr_set_dense(sc_ctx *c, const void *data, int dtype, int64_t n, int64_t n_vars,
                                 const int32_t *gene_cols, int64_t n_genes)
{
    SC_REQUIRE(c && data && gene_cols, SC_ERR_INVALID, "sc_expr_set_dense: null pointer");
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "sc_expr_set_dense: bad dtype %d", dtype);
    SC_REQUIRE(n_vars >= 1, SC_ERR_INVALID, "n_vars out of range");
    SC_HIP(hipSetDevice(c->device));
    c->e_n = 0;
    SC_TRY(expr_alloc(c, n, n_genes));
    c->e_dtype = dtype;
    for (int64_t g = 0; g < n_genes; ++g)
        SC_REQUIRE(gene_cols[g] >= 0 && gene_cols[g] < n_vars, SC_ERR_INVALID, "gene column %d out of range",
                   gene_cols[g]);
    SC_TRY(c->e_colmap.ensure(sizeof(int32_t) * (size_t)n_genes, &c->mem));
    SC_HIP(hipMemcpyAsync(c->e_colmap.p, gene_cols, sizeof(int32_t) * (size_t)n_genes, hipMemcpyHostToDevice,
                          c->stream));
    size_t esz = dtype == SC_F32 ? 4 : 8;
    // row chunks of <= 1 GiB of source data
    int64_t rows_per = ((int64_t)1 << 30) / (int64_t)(esz * (size_t)n_vars);
    if (rows_per < 1) rows_per = 1;
    for (int64_t r0 = 0; r0 < n; r0 += rows_per) {
        int64_t rows = (n - r0 < rows_per) ? n - r0 : rows_per;
        size_t bytes = esz * (size_t)rows * (size_t)n_vars;
        SC_TRY(c->e_tmp_data.ensure(bytes, &c->mem));
        SC_HIP(hipMemcpyAsync(c->e_tmp_data.p, (const char *)data + esz * (size_t)r0 * (size_t)n_vars, bytes,
                              hipMemcpyHostToDevice, c->stream));
        dim3 grid((unsigned)ceil_div64(rows * SC_TILE, 256), (unsigned)c->e_tiles);
        if (dtype == SC_F32)
            hipLaunchKernelGGL(k_gather_dense<float>, grid, dim3(256), 0, c->stream, c->e_tmp_data.as<float>(),
                               n_vars, c->e_colmap.as<int32_t>(), n_genes, c->X.as<double>(), n, r0, rows);
        else
            hipLaunchKernelGGL(k_gather_dense<double>, grid, dim3(256), 0, c->stream,
                               c->e_tmp_data.as<double>(), n_vars, c->e_colmap.as<int32_t>(), n_genes,
                               c->X.as<double>(), n, r0, rows);
        SC_HIP(hipGetLastError());
        SC_HIP(hipStreamSynchronize(c->stream));
    }
    return SC_OK;
}

// ------------------------------------------------------------------------------------------------
// per-gene column reductions over tiles (deterministic two-stage tree)
// ------------------------------------------------------------------------------------------------

#define RED_ROWS_PER_BLOCK 4096

// partial[tile][chunk][16] = sum over the chunk's rows of op(A[row][slot], B[row][slot])
// (OP_SQC: (A[row][slot] - B[tile * 16 + slot])^2, B = the per-gene means: the squares of Z = X - mean without storing Z)
template <int OP>
__global__ __launch_bounds__(256) void k_colsum_partial(const double *__restrict__ A,
                                                        const double *__restrict__ B,
                                                        double *__restrict__ partial, int64_t n)
{
    __shared__ double sh[256];
    const int64_t tile = blockIdx.y;
    const int slot = threadIdx.x & 15, rg = threadIdx.x >> 4;  // 16 row groups
    const double *a = A + tile * n * SC_TILE;
    const double *b = (OP == OP_MUL) ? B + tile * n * SC_TILE : nullptr;
    const double centre = (OP == OP_SQC) ? B[tile * SC_TILE + slot] : 0.0;
    int64_t r0 = (int64_t)blockIdx.x * RED_ROWS_PER_BLOCK;
    int64_t r1 = r0 + RED_ROWS_PER_BLOCK < n ? r0 + RED_ROWS_PER_BLOCK : n;
    double acc = 0.0;
    for (int64_t r = r0 + rg; r < r1; r += 16) {
        double v = a[r * SC_TILE + slot];
        if (OP == OP_SQC) v = v - centre;
        if (OP == OP_SQ || OP == OP_SQC) v = v * v;
        if (OP == OP_NZ) v = (v != 0.0) ? 1.0 : 0.0;
        if (OP == OP_MUL) v = v * b[r * SC_TILE + slot];
        acc += v;
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s >= 16; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 16) partial[(tile * gridDim.x + blockIdx.x) * SC_TILE + threadIdx.x] = sh[threadIdx.x];
}

// out[tile*16+slot] = (sum over chunks, ascending) / div; out_raw (optional) gets the sum itself.
// A true division, as numpy's mean takes it: sum * (1/n) turns a constant column c into c(1 +- eps) for ~15 % of
// the cell counts n, and a zero-variance gene would then look alive.
__global__ void k_colsum_final(const double *__restrict__ partial, double *__restrict__ out,
                               double *__restrict__ out_raw, int chunks, double div)
{
    int tile = blockIdx.x, slot = threadIdx.x;
    double s = 0.0;
    for (int ch = 0; ch < chunks; ++ch) s += partial[((int64_t)tile * chunks + ch) * SC_TILE + slot];
    if (out_raw) out_raw[tile * SC_TILE + slot] = s;
    out[tile * SC_TILE + slot] = s / div;
}

// second stage on its own: partial = [tile][chunk][16] sums that another kernel left (k_lag_u8's column sums)
int expr_colsum_chunks(sc_ctx *c, const double *partial, int chunks, double *out, double div, double *out_raw)
{
    hipLaunchKernelGGL(k_colsum_final, dim3((unsigned)c->e_tiles), dim3(SC_TILE), 0, c->stream, partial, out, out_raw,
                       chunks, div);
    SC_HIP(hipGetLastError());
    return SC_OK;
}

int expr_colsum(sc_ctx *c, int op, const double *A, const double *B, double *out, double div, double *out_raw)
{
    int64_t n = c->e_n;
    int chunks = (int)ceil_div64(n, RED_ROWS_PER_BLOCK);
    SC_TRY(c->red_tmp.ensure(sizeof(double) * (size_t)c->e_tiles * chunks * SC_TILE, &c->mem));
    auto partial = op == OP_ID ? k_colsum_partial<OP_ID> : op == OP_MUL ? k_colsum_partial<OP_MUL>
                 : op == OP_NZ ? k_colsum_partial<OP_NZ> : k_colsum_partial<OP_SQC>;
    hipLaunchKernelGGL(partial, dim3(chunks, (unsigned)c->e_tiles), dim3(256), 0, c->stream, A, B,
                       c->red_tmp.as<double>(), n);
    return expr_colsum_chunks(c, c->red_tmp.as<double>(), chunks, out, div, out_raw);
}

// Z = X - mean   (mode 0, scanpy's z)      |  Z = Z / sd  (mode 1, in place; Lee's z-score AC:1142)
__global__ __launch_bounds__(256) void k_center(const double *__restrict__ X, const double *__restrict__ mean,
                                                double *__restrict__ Z, int64_t n)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * SC_TILE) return;
    int64_t tile = blockIdx.y;
    int slot = (int)(t & 15);
    Z[tile * n * SC_TILE + t] = X[tile * n * SC_TILE + t] - mean[tile * SC_TILE + slot];
}

__global__ __launch_bounds__(256) void k_div_sd(double *__restrict__ Z, const double *__restrict__ var,
                                                int64_t n)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * SC_TILE) return;
    int64_t tile = blockIdx.y;
    int slot = (int)(t & 15);
    double v = var[tile * SC_TILE + slot];
    double sd = sqrt(v);
    // zero-variance genes are standardised to 0 (AC:1357-1359)
    Z[tile * n * SC_TILE + t] = (v > 0.0) ? Z[tile * n * SC_TILE + t] / sd : 0.0;
}

// mean (+ raw column sums), z2 = sum (X - mean)^2, var = z2 / n
int expr_moments(sc_ctx *c)
{
    SC_REQUIRE(c->e_n > 0, SC_ERR_STATE, "no expression loaded (call sc_expr_set_* first)");
    const int64_t n = c->e_n;
    SC_TRY(expr_colsum(c, OP_ID, c->X.as<double>(), nullptr, c->g_mean.as<double>(), (double)n, c->g_xsum.as<double>()));
    SC_TRY(expr_colsum(c, OP_SQC, c->X.as<double>(), c->g_mean.as<double>(), c->g_var.as<double>(), (double)n, c->g_z2.as<double>()));
    return SC_OK;
}

// Z = X - centre (per gene)
int expr_write_z(sc_ctx *c, const double *centre)
{
    c->lm_valid = false;  // Z is about to be rewritten
    const int64_t n = c->e_n;
    SC_TRY(c->Z.ensure((size_t)c->e_tiles * n * SC_TILE * sizeof(double), &c->mem));
    dim3 grid((unsigned)ceil_div64(n * SC_TILE, 256), (unsigned)c->e_tiles);
    hipLaunchKernelGGL(k_center, grid, dim3(256), 0, c->stream, c->X.as<double>(), centre, c->Z.as<double>(), n);
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// mean, Z = X - mean, z2 = sum Z^2, var = z2 / n
static int expr_center(sc_ctx *c)
{
    SC_TRY(expr_moments(c));
    return expr_write_z(c, c->g_mean.as<double>());
}

extern "C" int sc_expr_stats(sc_ctx *c, double *mean_out, double *var_out)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "null context");
    SC_HIP(hipSetDevice(c->device));
    SC_TRY(expr_center(c));
    if (mean_out)
        SC_HIP(hipMemcpyAsync(mean_out, c->g_mean.p, sizeof(double) * (size_t)c->e_genes, hipMemcpyDeviceToHost,
                              c->stream));
    if (var_out)
        SC_HIP(hipMemcpyAsync(var_out, c->g_var.p, sizeof(double) * (size_t)c->e_genes, hipMemcpyDeviceToHost,
                              c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}

// ------------------------------------------------------------------------------------------------
// A3: spatial lag  Lag[i][g] = sum_e w[e] * Z[col[e]][g]   (row-sequential, mul and add rounded
// separately, like scanpy's `(i_data * z[i_indices]).sum()` and scipy's csr_matvec)
// ------------------------------------------------------------------------------------------------

// unit[gene] != 0 (optional): the gene's rows are summed with weight 1 instead of w[e] -- the unweighted neighbour sums S
// of an integer-lattice gene (Z holds its raw counts then), exact integers in fp64.
//
// Processing order (r03): thread groups walk the cells in the graph's spatially sorted order (`order`: the bin-sorted
// order of the points the graph was built from; identity for a graph of unknown geometry) and each XCD -- blockIdx.x % 8
// under round-robin placement, speed only -- takes one contiguous eighth of that order, so the neighbour rows a
// workgroup gathers were fetched by its neighbours a moment ago and sit in THAT XCD's L2.  In input order (r02) every
// neighbour row came from the Infinity Cache or HBM again: 12.5 ms and 8-16 x the compulsory fetch traffic per launch at
// bench size.  The sums are per row, in edge order: the results do not depend on the processing order.
__global__ __launch_bounds__(256) void k_lag(const int64_t *__restrict__ indptr,
                                             const int32_t *__restrict__ indices,
                                             const double *__restrict__ w, const double *__restrict__ Z,
                                             double *__restrict__ Lag, int64_t n, const double *__restrict__ unit,
                                             const int32_t *__restrict__ order)
{
    // 8 threads per cell, each owning 2 of the tile's 16 genes (one 16-byte slice of the row)
    const int64_t per_xcd = (int64_t)(gridDim.x >> 3);                 // gridDim.x is a multiple of 8
    const int64_t blk = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    const int64_t t = blk * blockDim.x + threadIdx.x;
    const int64_t pos = t >> 3;
    int q = (int)(t & 7);
    if (pos >= n) return;
    const int64_t i = order ? order[pos] : pos;
    const double2 *Zt = reinterpret_cast<const double2 *>(Z + (int64_t)blockIdx.y * n * SC_TILE);
    double2 *Lt = reinterpret_cast<double2 *>(Lag + (int64_t)blockIdx.y * n * SC_TILE);
    const bool ux = unit && unit[(int64_t)blockIdx.y * SC_TILE + 2 * q] != 0.0;
    const bool uy = unit && unit[(int64_t)blockIdx.y * SC_TILE + 2 * q + 1] != 0.0;
    int64_t e0 = indptr[i], e1 = indptr[i + 1];
    double sx = 0.0, sy = 0.0;
    for (int64_t e = e0; e < e1; ++e) {
        int32_t j = indices[e];
        double ww = w[e];
        double2 z = Zt[(int64_t)j * 8 + q];
        sx = __dadd_rn(sx, __dmul_rn(ux ? 1.0 : ww, z.x));
        sy = __dadd_rn(sy, __dmul_rn(uy ? 1.0 : ww, z.y));
    }
    Lt[i * 8 + q] = make_double2(sx, sy);
}

int sc_lag_tiles(sc_ctx *c, const DBuf &indptr, const DBuf &indices, const DBuf &data, const double *Z, double *out,
                 const double *unit)
{
    int64_t n = c->e_n;
    const int32_t *order = sc_processing_order(c, n);
    KernelTimerScope ts(c, SC_K_LAG);
    hipLaunchKernelGGL(k_lag, dim3((unsigned)align_up64(ceil_div64(n * 8, 256), 8), (unsigned)c->e_tiles), dim3(256), 0,
                       c->stream, indptr.as<int64_t>(), indices.as<int32_t>(), data.as<double>(), Z, out, n, unit, order);
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// population-sd z-scores of the loaded genes in c->Z (zero-variance genes -> 0, AC:1357-1359; c->g_var holds the variances)
int sc_expr_zscores(sc_ctx *c)
{
    SC_TRY(expr_center(c));
    hipLaunchKernelGGL(k_div_sd, dim3((unsigned)ceil_div64(c->e_n * SC_TILE, 256), (unsigned)c->e_tiles), dim3(256), 0,
                       c->stream, c->Z.as<double>(), c->g_var.as<double>(), c->e_n);
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// Value class of every gene in one pass over the tiles: flags[g] bit 0 = some value is not an integer in [0, 255],
// bit 1 = ... not an integer in [0, 65535], bit 2 = ... not a float32 (NaN included); xmax[g] = largest integer count
// (0xffffffff as soon as a value is no integer in [0, 2^32))
__global__ __launch_bounds__(256) void k_gene_stats(const double *__restrict__ X, int64_t n, uint32_t *__restrict__ flags,
                                                    uint32_t *__restrict__ xmax)
{
    __shared__ uint32_t sh_f[256], sh_m[256];
    const int64_t tile = blockIdx.y;
    const int slot = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const double *a = X + tile * n * SC_TILE;
    const int64_t r0 = (int64_t)blockIdx.x * RED_ROWS_PER_BLOCK;
    const int64_t r1 = r0 + RED_ROWS_PER_BLOCK < n ? r0 + RED_ROWS_PER_BLOCK : n;
    uint32_t f = 0u, m = 0u;
    for (int64_t r = r0 + rg; r < r1; r += 16) {
        const double v = a[r * SC_TILE + slot];
        const bool isint = v >= 0.0 && v <= 4294967295.0 && (double)(uint32_t)v == v;
        const uint32_t u = isint ? (uint32_t)v : 0xffffffffu;
        f |= (u <= 255u ? 0u : 1u) | (u <= 65535u ? 0u : 2u) | ((double)(float)v == v ? 0u : 4u);
        m = u > m ? u : m;
    }
    sh_f[threadIdx.x] = f;
    sh_m[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s >= 16; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sh_f[threadIdx.x] |= sh_f[threadIdx.x + s];
            sh_m[threadIdx.x] = sh_m[threadIdx.x] > sh_m[threadIdx.x + s] ? sh_m[threadIdx.x] : sh_m[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < 16) {
        if (sh_f[threadIdx.x]) atomicOr(&flags[tile * SC_TILE + threadIdx.x], sh_f[threadIdx.x]);
        atomicMax(&xmax[tile * SC_TILE + threadIdx.x], sh_m[threadIdx.x]);
    }
}

// the value-class pass into c->g_flags / c->g_xmax ([tiles padded to 8][16] each), enqueued; the caller copies them out
int expr_gene_stats(sc_ctx *c)
{
    const int64_t n = c->e_n, T = c->e_tiles;
    const size_t bytes = sizeof(uint32_t) * (size_t)(align_up64(T, 8) * SC_TILE);
    SC_TRY(c->g_flags.ensure(bytes, &c->mem));
    SC_TRY(c->g_xmax.ensure(bytes, &c->mem));
    SC_HIP(hipMemsetAsync(c->g_flags.p, 0, bytes, c->stream));
    SC_HIP(hipMemsetAsync(c->g_xmax.p, 0, bytes, c->stream));
    hipLaunchKernelGGL(k_gene_stats, dim3((unsigned)ceil_div64(n, RED_ROWS_PER_BLOCK), (unsigned)T), dim3(256), 0, c->stream,
                       c->X.as<double>(), n, c->g_flags.as<uint32_t>(), c->g_xmax.as<uint32_t>());
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// Narrow[group][cell][q][t][e] = X[TG * group + t][cell][2 q + e] as uint8 / uint16 / float (every value fits: k_gene_stats)
template <int BITS>
__global__ __launch_bounds__(256) void k_pack_narrow(const double *__restrict__ X, uint4 *__restrict__ out, int64_t n,
                                                     int64_t tiles16)
{
    constexpr int TG = BITS == 8 ? 8 : BITS == 16 ? 4 : 2;
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;  // (cell, q)
    if (t >= n * 8) return;
    const int64_t cell = t >> 3;
    const int q = (int)(t & 7);
    uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int tt = 0; tt < TG; ++tt) {
        const int64_t t16 = TG * (int64_t)blockIdx.y + tt;
        if (t16 >= tiles16) continue;
        const double2 v = reinterpret_cast<const double2 *>(X + t16 * n * SC_TILE + cell * SC_TILE)[q];
        if (BITS == 8) {
            const uint32_t a = (uint32_t)(v.x >= 0.0 && v.x <= 255.0 ? v.x : 0.0), b = (uint32_t)(v.y >= 0.0 && v.y <= 255.0 ? v.y : 0.0);
            o[tt >> 1] |= (a | (b << 8)) << (16 * (tt & 1));
        } else if (BITS == 16) {
            const uint32_t a = (uint32_t)(v.x >= 0.0 && v.x <= 65535.0 ? v.x : 0.0), b = (uint32_t)(v.y >= 0.0 && v.y <= 65535.0 ? v.y : 0.0);
            o[tt] = a | (b << 16);
        } else {
            const float a = (float)v.x, b = (float)v.y;
            o[2 * tt] = __float_as_uint(a);
            o[2 * tt + 1] = __float_as_uint(b);
        }
    }
    out[((int64_t)blockIdx.y * n + cell) * 8 + q] = make_uint4(o[0], o[1], o[2], o[3]);
}

// c->X32 = the narrow copy of every loaded gene, bits = 8 / 16 / 32 (the buffer is sized for the widest of them)
int expr_pack_narrow(sc_ctx *c, int bits)
{
    const int64_t n = c->e_n, T = c->e_tiles;
    SC_TRY(c->X32.ensure(sizeof(float) * (size_t)((T + 1) / 2) * n * 32, &c->mem));   // >= the uint16 / uint8 copies
    const int tg = bits == 8 ? 8 : bits == 16 ? 4 : 2;
    const dim3 grid((unsigned)ceil_div64(n * 8, 256), (unsigned)ceil_div64(T, tg));
    auto pack = bits == 8 ? k_pack_narrow<8> : bits == 16 ? k_pack_narrow<16> : k_pack_narrow<32>;
    hipLaunchKernelGGL(pack, grid, dim3(256), 0, c->stream, c->X.as<double>(), c->X32.as<uint4>(), n, T);
    SC_HIP(hipGetLastError());
    return SC_OK;
}
