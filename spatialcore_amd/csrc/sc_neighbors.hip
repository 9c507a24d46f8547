// sc_neighbors.hip -- sc_knn_dense_gram: the exact k nearest neighbours of sc_knn_dense, bit for bit, found through a
// Gram-form filter on the fp64 matrix cores (restated by tests/neighbors_restated.py).  gfx950 only.
//
// A neighbour list is pinned to the direct form d2 = sum_c (x_ic - x_jc)^2 (sc_dense_knn.h: df_d2), which a Gram-form
// distance |x|^2 + |y|^2 - 2 x.y does not reproduce.  So the Gram form only FILTERS, with a proven bound:
//   1. norms       n_i = sum_c x_ic^2 (fp64, column order; any order satisfies the bound)
//   2. filter      g_ij = x_i . x_j by v_mfma_f64_16x16x4_f64, s_ij = (n_i + n_j) - 2 g_ij,
//                  E_ij = c_E 2^-52 (n_i + n_j) + 2^-1000 with c_E = 4 dp + 32, lo_ij = s_ij - E_ij <= d2_dev(i, j);
//                  a query keeps its L = k + slack smallest (lo, j), a total order: the kept SET depends on nothing else
//   3. re-rank     the direct-form d2 of the kept candidates, the k best by cand_better; D = the k-th of them.  The row is
//                  certified iff it kept fewer than L candidates or D < lo_(L) strictly: every candidate not kept has
//                  d2_dev >= lo >= lo_(L) > D
//   4. fallback    the uncertified rows, compacted into a list, scan every candidate in the direct form
// An uncertified row costs time and never correctness; the lists, the widened X and knn_valid are left in ctx->df exactly
// as sc_knn_dense leaves them.
#include <cfloat>

#include "sc_dense_knn.h"

namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr int NB_TPB = 512;       // filter: 8 wavefronts of 16 queries (one B operand block each) ...
constexpr int NB_QB = 128;        // ... = queries per workgroup
constexpr int NB_TC = 64;         // candidates per LDS tile: 4 A operand blocks, taken two at a time
constexpr int NB_CAP = 80;        // entries of a query's survivor buffer; compacted to L when fewer than 32 are free
constexpr int NB_SLACK_MAX = 16;  // so that L <= 48 = NB_CAP - 32: a compacted buffer always has room for the next step
constexpr int NB_SLACK_DEFAULT = 8;
// path 0 (profiles/neighbors_sweep.json): the filter from this many cells on -- padded widths above 32, where the
// direct search reads its queries from LDS, and widths 24 and 32; narrower rows stay on the direct register kernels
constexpr int64_t NB_GRAM_FROM_WIDE = 10000;
constexpr int64_t NB_GRAM_FROM = 100000;

__global__ __launch_bounds__(256) void k_nb_norms(const double *__restrict__ X, int64_t n, int dp, double *__restrict__ nrm)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *x = X + i * dp;
    double s = x[0] * x[0];
    for (int c = 1; c < dp; ++c) s = s + x[c] * x[c];
    nrm[i] = s;
}

__global__ void k_nb_zero(int32_t *__restrict__ counter) { *counter = 0; }

// One wavefront sorts a query's survivor buffer (m <= NB_CAP entries) by (lo, j) and keeps the first min(m, L): every lane
// ranks up to two entries against all m, read as broadcasts; the ranks of a total order are distinct, so the kept entries
// land on distinct slots.  All reads precede the first write (one wavefront, program order).  With m >= L the L-th key
// becomes the query's threshold.
__device__ __forceinline__ void nb_compact(volatile double *lo, volatile int *id, volatile int *cnt, volatile double *thr, int L, int lane)
{
    const int m = *cnt;
    const bool h0 = lane < m, h1 = lane + 64 < m;
    const double l0 = h0 ? lo[lane] : 0.0, l1 = h1 ? lo[lane + 64] : 0.0;
    const int j0 = h0 ? id[lane] : 0, j1 = h1 ? id[lane + 64] : 0;
    int r0 = 0, r1 = 0;
    for (int e = 0; e < m; ++e) {
        const double le = lo[e];
        const int je = id[e];
        r0 += cand_better(le, je, l0, j0) ? 1 : 0;
        r1 += cand_better(le, je, l1, j1) ? 1 : 0;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (h0 && r0 < L) { lo[r0] = l0; id[r0] = j0; }
    if (h1 && r1 < L) { lo[r1] = l1; id[r1] = j1; }
    if (h0 && r0 == L - 1) *thr = l0;
    if (h1 && r1 == L - 1) *thr = l1;
    if (lane == 0) *cnt = m < L ? m : L;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Workgroup b filters the queries [b * NB_QB, (b + 1) * NB_QB) against every candidate.  Operand maps of
// v_mfma_f64_16x16x4_f64 (as k_pca_gram): A[i = lane & 15][k = lane >> 4] = candidate i of a block, column 4 s + k, from the
// LDS tile (row stride DP + 2 doubles: the 32 lanes of a half read 32 different 8-byte banks); B[k = lane >> 4][j = lane & 15]
// = query j of the wavefront, column 4 s + k, in registers for the whole launch.  Result D[row = (lane >> 4) + 4 v][col =
// lane & 15]: lane holds candidates (lane >> 4) + 4 v of the block for query lane & 15, so a query's 16 results sit in 4
// lanes of ONE wavefront and its survivor buffer is that wavefront's alone: appends are LDS integer atomics, compaction
// needs no workgroup barrier.  The next tile is fetched into registers while this one is multiplied.
// Writes kept[q][0 .. m) (sorted by (lo, j)), kcnt[q] = m <= L and klo[q] = the L-th key (m == L).
template <int DP>
__global__ __launch_bounds__(NB_TPB) void k_nb_filter(const double *__restrict__ X, const double *__restrict__ nrm, int64_t n, int L,
                                                      double ce, int32_t *__restrict__ kept, int32_t *__restrict__ kcnt,
                                                      double *__restrict__ klo)
{
    constexpr int LD = DP + 2, KS = DP / 4, PRE = NB_TC * DP / NB_TPB;
    __shared__ double tile[NB_TC * LD];
    __shared__ double tn[NB_TC];
    __shared__ double blo[NB_QB * NB_CAP];
    __shared__ int bj[NB_QB * NB_CAP];
    __shared__ int bcnt[NB_QB];
    __shared__ double bthr[NB_QB];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int kk = lane >> 4;
    const int ql = wave * 16 + (lane & 15);
    const int64_t qi = (int64_t)blockIdx.x * NB_QB + ql;
    double b[KS];
#pragma unroll
    for (int s = 0; s < KS; ++s) b[s] = qi < n ? X[qi * DP + 4 * s + kk] : 0.0;
    const double nq = qi < n ? nrm[qi] : 0.0;
    if (t < NB_QB) {
        bcnt[t] = 0;
        bthr[t] = (int64_t)blockIdx.x * NB_QB + t < n ? DBL_MAX : -DBL_MAX;   // a query past the end keeps nothing
    }
    double thr = qi < n ? DBL_MAX : -DBL_MAX;
    const int64_t tiles = (n + NB_TC - 1) / NB_TC;
    double pre[PRE], pren = 0.0;
    auto fetch = [&](int64_t base) {
#pragma unroll
        for (int r = 0; r < PRE; ++r) {
            const int e = t + r * NB_TPB;
            pre[r] = base + e / DP < n ? X[base * DP + e] : 0.0;
        }
        if (t < NB_TC) pren = base + t < n ? nrm[base + t] : 0.0;
    };
    fetch(0);
    for (int64_t ti = 0; ti < tiles; ++ti) {
        const int64_t base = ti * NB_TC;
        __syncthreads();
#pragma unroll
        for (int r = 0; r < PRE; ++r) {
            const int e = t + r * NB_TPB;
            tile[(e / DP) * LD + e % DP] = pre[r];
        }
        if (t < NB_TC) tn[t] = pren;
        __syncthreads();
        if (ti + 1 < tiles) fetch(base + NB_TC);
        for (int half = 0; half < NB_TC / 32; ++half) {
            v4f64 acc[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                acc[u] = v4f64{0.0, 0.0, 0.0, 0.0};
                const double *arow = tile + ((half * 2 + u) * 16 + (lane & 15)) * LD + kk;
#pragma unroll
                for (int s = 0; s < KS; ++s) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(arow[4 * s], b[s], acc[u], 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int cl = (half * 2 + u) * 16 + kk + 4 * v;
                    const int64_t cj = base + cl;
                    const double tt = nq + tn[cl];
                    const double sg = tt - 2.0 * acc[u][v];
                    const double lo = sg - (ce * tt + 0x1p-1000);
                    if (cj < n && cj != qi && lo <= thr) {
                        const int pos = atomicAdd(&bcnt[ql], 1);   // < NB_CAP: at most 32 appends since the buffer held <= NB_CAP - 32
                        blo[ql * NB_CAP + pos] = lo;
                        bj[ql * NB_CAP + pos] = (int)cj;
                    }
                }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int have = ((volatile int *)bcnt)[ql];
            unsigned full = (unsigned)(__ballot(have > NB_CAP - 32) & 0xffffull);   // lanes 0 .. 15: the wavefront's queries
            if (full) {
                while (full) {
                    const int q = wave * 16 + __builtin_ctz(full);
                    full &= full - 1;
                    nb_compact(blo + q * NB_CAP, bj + q * NB_CAP, bcnt + q, bthr + q, L, lane);
                }
                thr = ((volatile double *)bthr)[ql];
            }
        }
    }
    for (int u = 0; u < 16; ++u) {
        const int q = wave * 16 + u;
        const int64_t gq = (int64_t)blockIdx.x * NB_QB + q;
        if (gq >= n) break;   // the whole wavefront
        nb_compact(blo + q * NB_CAP, bj + q * NB_CAP, bcnt + q, bthr + q, L, lane);
        const int m = ((volatile int *)bcnt)[q];
        if (lane < m) kept[gq * L + lane] = ((volatile int *)bj)[q * NB_CAP + lane];
        if (lane == 0) {
            kcnt[gq] = m;
            klo[gq] = m == L ? ((volatile double *)blo)[q * NB_CAP + L - 1] : 0.0;
        }
    }
}

// One thread per query: the direct-form d2 of its kept candidates, the k best, the certificate.  An uncertified row goes
// on the fallback list (an integer atomic: the order of the list changes no result).
template <int K>
__global__ __launch_bounds__(256) void k_nb_rerank(const double *__restrict__ X, int64_t n, int dp, int k, int L,
                                                   const int32_t *__restrict__ kept, const int32_t *__restrict__ kcnt,
                                                   const double *__restrict__ klo, int32_t *__restrict__ idx, double *__restrict__ d2,
                                                   int32_t *__restrict__ rows, int32_t *__restrict__ nrows)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double *a = X + i * dp;
    const int m = kcnt[i];
    TopK<K> best;
    best.init();
    for (int p = 0; p < m; ++p) {
        const int cid = kept[i * L + p];
        const double *x = X + (int64_t)cid * dp;
        const double acc = df_d2<0>([&](int c) { return a[c]; }, [&](int c) { return x[c]; }, dp);
        if (cand_better(acc, cid, best.d[K - 1], best.id[K - 1])) best.insert(acc, cid);
    }
    df_write_list(best, k, i * k, idx, d2);
    if (!(m < L || best.kth(k) < klo[i])) rows[atomicAdd(nrows, 1)] = (int32_t)i;
}

// The fallback: k_df_knn_lds (sc_diffusion.hip) for the listed queries only -- one thread per listed query, its row in
// LDS, workgroup (x, y) scans the candidates [y * split_len, (y + 1) * split_len) in tiles; the K-list of that split goes to
// (pidx, pd2)[y][list position][k].
template <int K>
__global__ __launch_bounds__(DF_QB_L) void k_nb_fallback(const double *__restrict__ X, int64_t n, int dp, int k,
                                                         const int32_t *__restrict__ rows, int64_t nrows, int64_t split_len,
                                                         int32_t *__restrict__ pidx, double *__restrict__ pd2)
{
    __shared__ double qs[DF_DMAX * DF_QB_L];
    __shared__ double tile[DF_TILE_L * DF_DMAX];
    const int t = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * DF_QB_L + t;
    const int64_t i = r < nrows ? rows[r] : -1;
    const int64_t c0 = (int64_t)blockIdx.y * split_len;
    const int64_t c1 = c0 + split_len < n ? c0 + split_len : n;
    for (int c = 0; c < dp; ++c) qs[c * DF_QB_L + t] = i >= 0 ? X[i * dp + c] : 0.0;
    TopK<K> best;
    best.init();
    for (int64_t b = c0; b < c1; b += DF_TILE_L) {
        const int cnt = (int)(c1 - b < DF_TILE_L ? c1 - b : DF_TILE_L);
        __syncthreads();
        for (int e = t; e < cnt * dp; e += DF_QB_L) tile[e] = X[b * dp + e];
        __syncthreads();
        if (i >= 0) {
            for (int j = 0; j < cnt; ++j) {
                const double *x = tile + j * dp;
                const double acc = df_d2<0>([&](int c) { return qs[c * DF_QB_L + t]; }, [&](int c) { return x[c]; }, dp);
                const int cid = (int)(b + j);
                if (cid != (int)i && cand_better(acc, cid, best.d[K - 1], best.id[K - 1])) best.insert(acc, cid);
            }
        }
    }
    if (i < 0) return;
    df_write_list(best, k, ((int64_t)blockIdx.y * nrows + r) * k, pidx, pd2);
}

// the k best of a listed query's `splits` lists, written over its row of the result
template <int K>
__global__ __launch_bounds__(256) void k_nb_fallback_merge(const int32_t *__restrict__ pidx, const double *__restrict__ pd2,
                                                           const int32_t *__restrict__ rows, int64_t nrows, int k, int splits,
                                                           int32_t *__restrict__ idx, double *__restrict__ d2)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    TopK<K> best;
    best.init();
    for (int s = 0; s < splits; ++s) {
        const int64_t o = ((int64_t)s * nrows + r) * k;
        for (int j = 0; j < k; ++j) {
            const double cd = pd2[o + j];
            const int cid = pidx[o + j];
            if (cand_better(cd, cid, best.d[K - 1], best.id[K - 1])) best.insert(cd, cid);
        }
    }
    df_write_list(best, k, (int64_t)rows[r] * k, idx, d2);
}

void nb_launch_filter(sc_ctx *c, int64_t n, int dp, int L, double ce)
{
    sc_ctx::Diffusion &f = c->df;
    const dim3 grid((unsigned)ceil_div64(n, NB_QB)), block(NB_TPB);
    const double *X = f.X.as<double>(), *nrm = f.gnorm.as<double>();
    int32_t *kept = f.gkept.as<int32_t>(), *kcnt = f.gcnt.as<int32_t>();
    double *klo = f.glo.as<double>();
    switch (dp) {
    case 8: hipLaunchKernelGGL(k_nb_filter<8>, grid, block, 0, c->stream, X, nrm, n, L, ce, kept, kcnt, klo); break;
    case 16: hipLaunchKernelGGL(k_nb_filter<16>, grid, block, 0, c->stream, X, nrm, n, L, ce, kept, kcnt, klo); break;
    case 24: hipLaunchKernelGGL(k_nb_filter<24>, grid, block, 0, c->stream, X, nrm, n, L, ce, kept, kcnt, klo); break;
    case 32: hipLaunchKernelGGL(k_nb_filter<32>, grid, block, 0, c->stream, X, nrm, n, L, ce, kept, kcnt, klo); break;
    case 40: hipLaunchKernelGGL(k_nb_filter<40>, grid, block, 0, c->stream, X, nrm, n, L, ce, kept, kcnt, klo); break;
    case 48: hipLaunchKernelGGL(k_nb_filter<48>, grid, block, 0, c->stream, X, nrm, n, L, ce, kept, kcnt, klo); break;
    case 56: hipLaunchKernelGGL(k_nb_filter<56>, grid, block, 0, c->stream, X, nrm, n, L, ce, kept, kcnt, klo); break;
    default: hipLaunchKernelGGL(k_nb_filter<64>, grid, block, 0, c->stream, X, nrm, n, L, ce, kept, kcnt, klo); break;
    }
}

template <int K>
void nb_launch_rerank(sc_ctx *c, int64_t n, int dp, int k, int L)
{
    sc_ctx::Diffusion &f = c->df;
    hipLaunchKernelGGL(k_nb_rerank<K>, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, c->stream, f.X.as<double>(), n, dp, k, L,
                       f.gkept.as<int32_t>(), f.gcnt.as<int32_t>(), f.glo.as<double>(), f.idx.as<int32_t>(), f.d2.as<double>(),
                       f.grows.as<int32_t>() + 1, f.grows.as<int32_t>());
}

template <int K>
void nb_launch_fallback(sc_ctx *c, int64_t n, int dp, int k, int64_t nrows, int S, int64_t split_len)
{
    sc_ctx::Diffusion &f = c->df;
    const int32_t *rows = f.grows.as<int32_t>() + 1;
    hipLaunchKernelGGL(k_nb_fallback<K>, dim3((unsigned)ceil_div64(nrows, DF_QB_L), (unsigned)S), dim3(DF_QB_L), 0, c->stream,
                       f.X.as<double>(), n, dp, k, rows, nrows, split_len, f.pidx.as<int32_t>(), f.pd2.as<double>());
    hipLaunchKernelGGL(k_nb_fallback_merge<K>, dim3((unsigned)ceil_div64(nrows, 256)), dim3(256), 0, c->stream, f.pidx.as<int32_t>(),
                       f.pd2.as<double>(), rows, nrows, k, S, f.idx.as<int32_t>(), f.d2.as<double>());
}

}  // namespace

extern "C" int sc_knn_dense_gram(sc_ctx *c, const void *X, int dtype, int64_t n, int32_t d, int32_t k, int32_t path, int32_t slack,
                                 int32_t *idx_out, double *d2_out, int64_t *info_out)
{
    SC_REQUIRE(c && X && info_out, SC_ERR_INVALID, "sc_knn_dense_gram: null pointer");
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "sc_knn_dense_gram: dtype must be SC_F32 or SC_F64");
    SC_REQUIRE(d >= 1 && d <= DF_DMAX, SC_ERR_INVALID, "sc_knn_dense_gram: need 1 <= d <= %d, got %d", DF_DMAX, d);
    SC_REQUIRE(k >= 2 && k <= DF_KMAX, SC_ERR_INVALID, "sc_knn_dense_gram: need 2 <= k <= %d, got %d", DF_KMAX, k);
    SC_REQUIRE(n > k && n <= INT32_MAX, SC_ERR_INVALID, "sc_knn_dense_gram: need k < n <= 2^31 - 1, got n=%lld, k=%d", (long long)n, k);
    SC_REQUIRE(n * k <= ((int64_t)1 << 29), SC_ERR_INVALID, "sc_knn_dense_gram: need n * k <= 2^29, got %lld", (long long)(n * k));
    SC_REQUIRE(path >= 0 && path <= 2, SC_ERR_INVALID, "sc_knn_dense_gram: path must be 0 (the library's choice), 1 (direct) or 2 (Gram filter), got %d",
               path);
    SC_REQUIRE(slack >= 0 && slack <= NB_SLACK_MAX, SC_ERR_INVALID, "sc_knn_dense_gram: need 0 <= slack <= %d, got %d", NB_SLACK_MAX, slack);
    const int dp = (int)align_up64(d, 8);
    if (path == 0) path = (dp > 32 && n >= NB_GRAM_FROM_WIDE) || (dp >= 24 && n >= NB_GRAM_FROM) ? 2 : 1;
    if (path == 1) {   // the direct kernels: the call is sc_knn_dense, which reads the values once for its own finite check
        SC_TRY(sc_knn_dense(c, X, dtype, n, d, k, 0, idx_out, d2_out));
        info_out[0] = 1;
        info_out[1] = k;
        info_out[2] = 0;
        info_out[3] = 0;
        return SC_OK;
    }
    if (dtype == SC_F32) SC_TRY(df_require_finite("sc_knn_dense_gram", (const float *)X, n * d));
    else SC_TRY(df_require_finite("sc_knn_dense_gram", (const double *)X, n * d));

    SC_HIP(hipSetDevice(c->device));
    sc_ctx::Diffusion &f = c->df;
    hipStream_t s = c->stream;
    f.knn_valid = f.graph_valid = f.lanczos_valid = false;
    const int L = k + (slack ? slack : NB_SLACK_DEFAULT);
    const double ce = (double)(4 * dp + 32) * 0x1p-52;
    const size_t es = dtype == SC_F32 ? sizeof(float) : sizeof(double);
    SC_TRY(f.raw.ensure(es * (size_t)(n * d), &c->mem));
    SC_TRY(f.X.ensure(sizeof(double) * (size_t)(n * dp), &c->mem));
    SC_TRY(f.idx.ensure(sizeof(int32_t) * (size_t)(n * k), &c->mem));
    SC_TRY(f.d2.ensure(sizeof(double) * (size_t)(n * k), &c->mem));
    SC_TRY(f.gnorm.ensure(sizeof(double) * (size_t)n, &c->mem));
    SC_TRY(f.gkept.ensure(sizeof(int32_t) * (size_t)(n * L), &c->mem));
    SC_TRY(f.gcnt.ensure(sizeof(int32_t) * (size_t)n, &c->mem));
    SC_TRY(f.glo.ensure(sizeof(double) * (size_t)n, &c->mem));
    SC_TRY(f.grows.ensure(sizeof(int32_t) * (size_t)(n + 1), &c->mem));   // [0]: the number of listed rows, then the rows
    SC_HIP(hipMemcpyAsync(f.raw.p, X, es * (size_t)(n * d), hipMemcpyHostToDevice, s));
    const dim3 widen((unsigned)ceil_div64(n * dp, 256)), rows((unsigned)ceil_div64(n, 256)), tpb(256);
    if (dtype == SC_F32) hipLaunchKernelGGL(k_df_widen<float>, widen, tpb, 0, s, f.raw.as<float>(), n, (int)d, dp, f.X.as<double>());
    else hipLaunchKernelGGL(k_df_widen<double>, widen, tpb, 0, s, f.raw.as<double>(), n, (int)d, dp, f.X.as<double>());
    int32_t nrows32 = 0;
    {
        KernelTimerScope ts(c, SC_K_NEIGHBORS_GRAM);
        hipLaunchKernelGGL(k_nb_norms, rows, tpb, 0, s, f.X.as<double>(), n, dp, f.gnorm.as<double>());
        hipLaunchKernelGGL(k_nb_zero, dim3(1), dim3(1), 0, s, f.grows.as<int32_t>());
        nb_launch_filter(c, n, dp, L, ce);
        if (k <= 8) nb_launch_rerank<8>(c, n, dp, k, L);
        else if (k <= 16) nb_launch_rerank<16>(c, n, dp, k, L);
        else nb_launch_rerank<32>(c, n, dp, k, L);
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(&nrows32, f.grows.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    const int64_t nrows = nrows32;
    SC_REQUIRE(nrows >= 0 && nrows <= n, SC_ERR_HIP, "sc_knn_dense_gram: %lld uncertified rows out of range", (long long)nrows);
    if (nrows > 0) {
        // the candidate ranges of sc_knn_dense's LDS form, by the number of listed rows
        int64_t want = nrows < DF_SPLIT_BELOW ? DF_SPLIT_WGS / ceil_div64(nrows, DF_QB_L) : 1;
        if (want < 1) want = 1;
        const int64_t split_len = align_up64(ceil_div64(n, want), DF_TILE_L);
        const int S = (int)ceil_div64(n, split_len);
        SC_TRY(f.pidx.ensure(sizeof(int32_t) * (size_t)(nrows * k) * S, &c->mem));
        SC_TRY(f.pd2.ensure(sizeof(double) * (size_t)(nrows * k) * S, &c->mem));
        KernelTimerScope ts(c, SC_K_NEIGHBORS_GRAM);
        if (k <= 8) nb_launch_fallback<8>(c, n, dp, k, nrows, S, split_len);
        else if (k <= 16) nb_launch_fallback<16>(c, n, dp, k, nrows, S, split_len);
        else nb_launch_fallback<32>(c, n, dp, k, nrows, S, split_len);
    }
    SC_HIP(hipGetLastError());
    if (idx_out) SC_HIP(hipMemcpyAsync(idx_out, f.idx.p, sizeof(int32_t) * (size_t)(n * k), hipMemcpyDeviceToHost, s));
    if (d2_out) SC_HIP(hipMemcpyAsync(d2_out, f.d2.p, sizeof(double) * (size_t)(n * k), hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    f.n = n;
    f.d = dp;
    f.k = k;
    f.knn_valid = true;
    info_out[0] = 2;
    info_out[1] = L;
    info_out[2] = n - nrows;
    info_out[3] = nrows;
    return SC_OK;
}
