// sc_neighbors.hip -- the exact k nearest neighbours in d <= 64 dimensions, two ways to the same bits (DESIGN.md 4.6m, 4.6q;
// restated by tests/diffusion_restated.py: knn, and tests/neighbors_restated.py).  gfx950 only.
//   sc_knn_dense        the direct kernels: every query scans every candidate
//   sc_knn_dense_gram   a Gram-form filter on the fp64 matrix cores, certified row by row; the direct kernels for the rest
//   sc_knn_cross        both again in their cross form: the queries are a second array, no candidate is excluded
// The first two leave the widened features and the lists in ctx->knn for sc_diffmap_graph and sc_fuzzy_graph; the third
// leaves its lists there for sc_cross_vote and sc_cross_regress (sc_ingest.hip) and nothing that reads as a self graph.
//
// fp64 throughout, -ffp-contract=off, no floating-point atomics.  A squared distance has ONE order: the d terms
// (x_ic - x_jc)^2 in column order, starting from the c = 0 term (sc_dense_knn.h: df_d2; the device rows are padded with
// zeros to a multiple of 8 columns; a padded term adds +0 to a non-negative sum, which changes no bit).  The lists are the
// k smallest (d2, index) pairs, a total order, so they do not depend on how the candidates were split over workgroups.
//
// A neighbour list is pinned to that direct form, which a Gram-form distance |x|^2 + |y|^2 - 2 x.y does not reproduce.  So
// the Gram form only FILTERS, with a proven bound:
//   1. norms       n_i = sum_c x_ic^2 (fp64, column order; any order satisfies the bound)
//   2. filter      g_ij = x_i . x_j by v_mfma_f64_16x16x4_f64, s_ij = (n_i + n_j) - 2 g_ij,
//                  E_ij = c_E 2^-52 (n_i + n_j) + 2^-1000 with c_E = 4 dp + 32, lo_ij = s_ij - E_ij <= d2_dev(i, j);
//                  a query keeps its L = k + slack smallest (lo, j), a total order: the kept SET depends on nothing else
//   3. re-rank     the direct-form d2 of the kept candidates, the k best by cand_better; D = the k-th of them.  The row is
//                  certified iff it kept fewer than L candidates or D < lo_(L) strictly: every candidate not kept has
//                  d2_dev >= lo >= lo_(L) > D
//   4. fallback    the uncertified rows, compacted into a list, scan every candidate in the direct form
// An uncertified row costs time and never correctness.
#include <cfloat>
#include <cmath>
#include <type_traits>

#include "sc_dense_knn.h"
#include "sc_list_graph.h"
#include "sc_topk.h"

// X[n][dp] <- the caller's rows widened to fp64, columns d .. dp - 1 zero
template <class T>
__global__ __launch_bounds__(256) void k_df_widen(const T *__restrict__ raw, int64_t n, int d, int dp, double *__restrict__ X)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * dp) return;
    const int64_t i = t / dp;
    const int c = (int)(t % dp);
    X[t] = c < d ? (double)raw[i * d + c] : 0.0;
}

namespace {

typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr int DF_DREG = 32;       // widest (padded) feature row a thread keeps in registers; wider rows live in LDS
constexpr int DF_QB = 256;        // register form: queries per workgroup ...
constexpr int DF_TILE = 128;      // ... and candidates staged in LDS at a time
constexpr int DF_QB_L = 64;       // LDS form: queries per workgroup (their rows take 32 KiB) ...
constexpr int DF_TILE_L = 32;     // ... and candidates per tile (16 KiB)
constexpr int64_t DF_SPLIT_BELOW = 100000;   // fewer queries than this: the candidates are split over workgroups
constexpr int DF_SPLIT_WGS = 2048;           // ... aiming at about this many
constexpr int NB_TPB = 512;       // filter: 8 wavefronts of 16 queries (one B operand block each) ...
constexpr int NB_QB = 128;        // ... = queries per workgroup
constexpr int NB_TC = 64;         // candidates per LDS tile: 4 A operand blocks, taken two at a time
constexpr int NB_CAP = 80;        // entries of a query's survivor buffer; compacted to L when fewer than 32 are free
constexpr int NB_SLACK_MAX = 16;  // so that L <= 48 = NB_CAP - 32: a compacted buffer always has room for the next step
constexpr int NB_SLACK_DEFAULT = 8;
// path 0 (profiles/neighbors_sweep.json, profiles/ingest_sweep.json): the filter from this many queries
// on (its grid is one workgroup per 128 queries; the direct search splits the candidates instead) and from this many
// (query, candidate) pairs on -- padded widths above 32, where the direct search reads its queries from LDS, and widths
// 24 and 32; narrower rows stay on the direct register kernels.  With n queries among themselves: from 10,000 and from
// 100,000 cells.
constexpr int64_t NB_GRAM_QUERIES_FROM = 10000;
constexpr int64_t NB_GRAM_PAIRS_FROM_WIDE = 100000000;      // 10^8
constexpr int64_t NB_GRAM_PAIRS_FROM = 10000000000;         // 10^10

// The two forms of every search kernel.  Self form: the queries are the candidates' own rows, and a query skips itself;
// the kernel takes no further argument.  Cross form: the kernel's argument list ends with the queries' array Q (and,
// where it has no query count of its own, their number nq), and no candidate is skipped.  The extra arguments are a
// parameter pack QA, empty in the self form, so that the self kernels keep their argument list and their device code.
__device__ __forceinline__ const double *dk_qrows(const double *X) { return X; }
template <class... R>
__device__ __forceinline__ const double *dk_qrows(const double *, const double *Q, R...) { return Q; }
__device__ __forceinline__ int64_t dk_qcount(int64_t n) { return n; }
template <class... R>
__device__ __forceinline__ int64_t dk_qcount(int64_t, const double *, int64_t nq, R...) { return nq; }
__device__ __forceinline__ const double *dk_qnorms(const double *nrm) { return nrm; }
__device__ __forceinline__ const double *dk_qnorms(const double *, const double *, int64_t, const double *qnrm) { return qnrm; }

// the first k entries of a finished list, best first, to (idx, d2)[o .. o + k)
template <int K>
__device__ __forceinline__ void df_write_list(const TopK<K> &best, int k, int64_t o, int32_t *__restrict__ idx, double *__restrict__ d2)
{
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j < k) {
            idx[o + j] = best.id[j];
            d2[o + j] = best.d[j];
        }
}

// One thread per query, its row in DR registers; workgroup (x, y) scans the candidates [y * split_len, (y + 1) * split_len)
// in tiles staged through LDS and read as broadcasts.  Writes the K-list of that split, best first, to
// (pidx, pd2)[y][query][k]; entries a short split could not fill keep TopK's sentinel (DBL_MAX, INT_MAX).  QA: (Q, nq).
template <int K, int DR, class... QA>
__global__ __launch_bounds__(DF_QB) void k_df_knn_reg(const double *__restrict__ X, int64_t n, int k, int64_t split_len,
                                                      int32_t *__restrict__ pidx, double *__restrict__ pd2, QA... qa)
{
    constexpr bool SELF = sizeof...(QA) == 0;
    __shared__ double tile[DF_TILE * DR];
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * DF_QB + t;
    const int64_t c0 = (int64_t)blockIdx.y * split_len;
    const int64_t c1 = c0 + split_len < n ? c0 + split_len : n;
    const double *Q = dk_qrows(X, qa...);
    const int64_t nq = dk_qcount(n, qa...);
    double q[DR];
#pragma unroll
    for (int c = 0; c < DR; ++c) q[c] = i < nq ? Q[i * DR + c] : 0.0;
    TopK<K> best;
    best.init();
    for (int64_t b = c0; b < c1; b += DF_TILE) {
        const int cnt = (int)(c1 - b < DF_TILE ? c1 - b : DF_TILE);
        __syncthreads();
        for (int e = t; e < cnt * DR; e += DF_QB) tile[e] = X[b * DR + e];
        __syncthreads();
        if (i < nq) {
            for (int j = 0; j < cnt; ++j) {
                const double *x = tile + j * DR;
                const double acc = df_d2<DR>([&](int c) { return q[c]; }, [&](int c) { return x[c]; }, DR);
                const int cid = (int)(b + j);
                if ((!SELF || cid != (int)i) && cand_better(acc, cid, best.d[K - 1], best.id[K - 1])) best.insert(acc, cid);
            }
        }
    }
    if (i >= nq) return;
    df_write_list(best, k, ((int64_t)blockIdx.y * nq + i) * k, pidx, pd2);
}

// The same with the queries' rows in LDS (column c of the workgroup's queries is one conflict-free row of 64 doubles):
// 32 < dp <= 64, where the registers of the row next to a 32-entry list would spill.  Slot r = blockIdx.x * DF_QB_L + t of
// the nq queries stands for query r (LISTED = false, nq = n: the direct search) or for query rows[r] (LISTED = true: the
// fallback of the Gram filter, at any width); the K-list of a split goes to (pidx, pd2)[y][slot][k].  QA: (Q, the number of all queries, unused: nq counts the slots).
template <int K, bool LISTED, class... QA>
__global__ __launch_bounds__(DF_QB_L) void k_df_knn_lds(const double *__restrict__ X, int64_t n, int dp, int k, int64_t split_len,
                                                        int32_t *__restrict__ pidx, double *__restrict__ pd2,
                                                        const int32_t *__restrict__ rows, int64_t nq, QA... qa)
{
    constexpr bool SELF = sizeof...(QA) == 0;
    const double *Q = dk_qrows(X, qa...);
    __shared__ double qs[DF_DMAX * DF_QB_L];
    __shared__ double tile[DF_TILE_L * DF_DMAX];
    const int t = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * DF_QB_L + t;
    const bool on = r < nq;
    int64_t i = r;
    if constexpr (LISTED) i = on ? rows[r] : 0;
    const int64_t c0 = (int64_t)blockIdx.y * split_len;
    const int64_t c1 = c0 + split_len < n ? c0 + split_len : n;
    for (int c = 0; c < dp; ++c) qs[c * DF_QB_L + t] = on ? Q[i * dp + c] : 0.0;
    TopK<K> best;
    best.init();
    for (int64_t b = c0; b < c1; b += DF_TILE_L) {
        const int cnt = (int)(c1 - b < DF_TILE_L ? c1 - b : DF_TILE_L);
        __syncthreads();
        for (int e = t; e < cnt * dp; e += DF_QB_L) tile[e] = X[b * dp + e];
        __syncthreads();
        if (on) {
            for (int j = 0; j < cnt; ++j) {
                const double *x = tile + j * dp;
                const double acc = df_d2<0>([&](int c) { return qs[c * DF_QB_L + t]; }, [&](int c) { return x[c]; }, dp);
                const int cid = (int)(b + j);
                if ((!SELF || cid != (int)i) && cand_better(acc, cid, best.d[K - 1], best.id[K - 1])) best.insert(acc, cid);
            }
        }
    }
    if (!on) return;
    df_write_list(best, k, ((int64_t)blockIdx.y * nq + r) * k, pidx, pd2);
}

// the k best of the `splits` lists of slot r, by the same comparison (a sentinel never beats anything), to row r of the
// result or, LISTED, to row rows[r]
template <int K, bool LISTED>
__global__ __launch_bounds__(256) void k_df_knn_merge(const int32_t *__restrict__ pidx, const double *__restrict__ pd2, int64_t nq,
                                                      int k, int splits, int32_t *__restrict__ idx, double *__restrict__ d2,
                                                      const int32_t *__restrict__ rows)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nq) return;
    TopK<K> best;
    best.init();
    for (int s = 0; s < splits; ++s) {
        const int64_t o = ((int64_t)s * nq + r) * k;
        for (int j = 0; j < k; ++j) {
            const double cd = pd2[o + j];
            const int cid = pidx[o + j];
            if (cand_better(cd, cid, best.d[K - 1], best.id[K - 1])) best.insert(cd, cid);
        }
    }
    int64_t i = r;
    if constexpr (LISTED) i = rows[r];
    df_write_list(best, k, i * k, idx, d2);
}

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
// Writes kept[q][0 .. m) (sorted by (lo, j)), kcnt[q] = m <= L and klo[q] = the L-th key (m == L).  QA: (Q, nq, their norms).
template <int DP, class... QA>
__global__ __launch_bounds__(NB_TPB) void k_nb_filter(const double *__restrict__ X, const double *__restrict__ nrm, int64_t n, int L,
                                                      double ce, int32_t *__restrict__ kept, int32_t *__restrict__ kcnt,
                                                      double *__restrict__ klo, QA... qa)
{
    constexpr bool SELF = sizeof...(QA) == 0;
    constexpr int LD = DP + 2, KS = DP / 4, PRE = NB_TC * DP / NB_TPB;
    const double *Q = dk_qrows(X, qa...);
    const double *qnrm = dk_qnorms(nrm, qa...);
    const int64_t nqs = dk_qcount(n, qa...);
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
    for (int s = 0; s < KS; ++s) b[s] = qi < nqs ? Q[qi * DP + 4 * s + kk] : 0.0;
    const double nq = qi < nqs ? qnrm[qi] : 0.0;
    if (t < NB_QB) {
        bcnt[t] = 0;
        bthr[t] = (int64_t)blockIdx.x * NB_QB + t < nqs ? DBL_MAX : -DBL_MAX;   // a query past the end keeps nothing
    }
    double thr = qi < nqs ? DBL_MAX : -DBL_MAX;
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
                    if (cj < n && (!SELF || cj != qi) && lo <= thr) {
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
        if (gq >= nqs) break;   // the whole wavefront
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
// on the fallback list (an integer atomic: the order of the list changes no result), which k_df_knn_lds<K, true> scans.
// QA: (Q, nq).
template <int K, class... QA>
__global__ __launch_bounds__(256) void k_nb_rerank(const double *__restrict__ X, int64_t n, int dp, int k, int L,
                                                   const int32_t *__restrict__ kept, const int32_t *__restrict__ kcnt,
                                                   const double *__restrict__ klo, int32_t *__restrict__ idx, double *__restrict__ d2,
                                                   int32_t *__restrict__ rows, int32_t *__restrict__ nrows, QA... qa)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= dk_qcount(n, qa...)) return;
    const double *a = dk_qrows(X, qa...) + i * dp;
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

// ---- host ---------------------------------------------------------------------------------------------------------
// What a search runs on: nq queries among the n candidate rows of c->knn.X, padded to dp columns.  The self search has
// nq = n and launches the kernels' self form; the cross search hands every launcher the kernels' extra arguments
// (c->knn.Q, nq) as the pack `qa`, which is empty in the self search.
struct DkShape { int64_t n, nq; int dp, k; };

// (qa..., the queries' norms) in the cross form
template <class... QA>
void nb_launch_filter(sc_ctx *c, const DkShape &sh, int L, double ce, QA... qa)
{
    sc_ctx::DenseKnn &f = c->knn;
    const dim3 grid((unsigned)ceil_div64(sh.nq, NB_QB)), block(NB_TPB);
    const double *X = f.X.as<double>(), *nrm = f.gnorm.as<double>();
    const int64_t n = sh.n;
    int32_t *kept = f.gkept.as<int32_t>(), *kcnt = f.gcnt.as<int32_t>();
    double *klo = f.glo.as<double>();
    switch (sh.dp) {
    case 8: hipLaunchKernelGGL((k_nb_filter<8, QA...>), grid, block, 0, c->stream, X, nrm, n, L, ce, kept, kcnt, klo, qa...); break;
    case 16: hipLaunchKernelGGL((k_nb_filter<16, QA...>), grid, block, 0, c->stream, X, nrm, n, L, ce, kept, kcnt, klo, qa...); break;
    case 24: hipLaunchKernelGGL((k_nb_filter<24, QA...>), grid, block, 0, c->stream, X, nrm, n, L, ce, kept, kcnt, klo, qa...); break;
    case 32: hipLaunchKernelGGL((k_nb_filter<32, QA...>), grid, block, 0, c->stream, X, nrm, n, L, ce, kept, kcnt, klo, qa...); break;
    case 40: hipLaunchKernelGGL((k_nb_filter<40, QA...>), grid, block, 0, c->stream, X, nrm, n, L, ce, kept, kcnt, klo, qa...); break;
    case 48: hipLaunchKernelGGL((k_nb_filter<48, QA...>), grid, block, 0, c->stream, X, nrm, n, L, ce, kept, kcnt, klo, qa...); break;
    case 56: hipLaunchKernelGGL((k_nb_filter<56, QA...>), grid, block, 0, c->stream, X, nrm, n, L, ce, kept, kcnt, klo, qa...); break;
    default: hipLaunchKernelGGL((k_nb_filter<64, QA...>), grid, block, 0, c->stream, X, nrm, n, L, ce, kept, kcnt, klo, qa...); break;
    }
}

template <int K, class... QA>
void nb_launch_rerank(sc_ctx *c, const DkShape &sh, int L, QA... qa)
{
    sc_ctx::DenseKnn &f = c->knn;
    hipLaunchKernelGGL((k_nb_rerank<K, QA...>), dim3((unsigned)ceil_div64(sh.nq, 256)), dim3(256), 0, c->stream, f.X.as<double>(), sh.n,
                       sh.dp, sh.k, L, f.gkept.as<int32_t>(), f.gcnt.as<int32_t>(), f.glo.as<double>(), f.idx.as<int32_t>(),
                       f.d2.as<double>(), f.grows.as<int32_t>() + 1, f.grows.as<int32_t>(), qa...);
}

// call f with K = 8, 16 or 32 as a std::integral_constant: the shortest list of TopK's three that holds k entries
template <class F>
void dk_by_k(int k, F &&f)
{
    if (k <= 8) f(std::integral_constant<int, 8>());
    else if (k <= 16) f(std::integral_constant<int, 16>());
    else f(std::integral_constant<int, 32>());
}

// The candidate ranges of a scan by nq queries in blocks of qb: `forced` of them, or (0) about DF_SPLIT_WGS workgroups'
// worth below DF_SPLIT_BELOW queries and one range above.  A range is whole tiles, the last one whatever is left of n.
struct DkSplit { int64_t len; int S; };
DkSplit dk_split(int64_t nq, int qb, int tile, int64_t n, int forced)
{
    int64_t want = forced;
    if (want == 0) want = nq < DF_SPLIT_BELOW ? DF_SPLIT_WGS / ceil_div64(nq, qb) : 1;
    if (want < 1) want = 1;
    const int64_t len = align_up64(ceil_div64(n, want), tile);
    return {len, (int)ceil_div64(n, len)};
}

template <int K, class... QA>
void df_launch_search(sc_ctx *c, const DkShape &sh, int splits, int64_t split_len, int32_t *pidx, double *pd2, QA... qa)
{
    const double *X = c->knn.X.as<double>();
    const int64_t n = sh.n;
    const int k = sh.k;
    if (sh.dp > DF_DREG) {
        const dim3 grid((unsigned)ceil_div64(sh.nq, DF_QB_L), (unsigned)splits);
        hipLaunchKernelGGL((k_df_knn_lds<K, false, QA...>), grid, dim3(DF_QB_L), 0, c->stream, X, n, sh.dp, k, split_len, pidx, pd2,
                           (const int32_t *)nullptr, sh.nq, qa...);
        return;
    }
    const dim3 grid((unsigned)ceil_div64(sh.nq, DF_QB), (unsigned)splits), block(DF_QB);
    switch (sh.dp) {
    case 8: hipLaunchKernelGGL((k_df_knn_reg<K, 8, QA...>), grid, block, 0, c->stream, X, n, k, split_len, pidx, pd2, qa...); break;
    case 16: hipLaunchKernelGGL((k_df_knn_reg<K, 16, QA...>), grid, block, 0, c->stream, X, n, k, split_len, pidx, pd2, qa...); break;
    case 24: hipLaunchKernelGGL((k_df_knn_reg<K, 24, QA...>), grid, block, 0, c->stream, X, n, k, split_len, pidx, pd2, qa...); break;
    default: hipLaunchKernelGGL((k_df_knn_reg<K, 32, QA...>), grid, block, 0, c->stream, X, n, k, split_len, pidx, pd2, qa...); break;
    }
}

template <int K, bool LISTED>
void df_launch_merge(sc_ctx *c, int64_t nq, int k, int splits, const int32_t *rows)
{
    hipLaunchKernelGGL((k_df_knn_merge<K, LISTED>), dim3((unsigned)ceil_div64(nq, 256)), dim3(256), 0, c->stream, c->knn.pidx.as<int32_t>(),
                       c->knn.pd2.as<double>(), nq, k, splits, c->knn.idx.as<int32_t>(), c->knn.d2.as<double>(), rows);
}

template <class T>
int df_require_finite(const char *who, const T *X, int64_t count)
{
    for (int64_t p = 0; p < count; ++p)
        SC_REQUIRE(std::fabs((double)X[p]) < 0x1p500, SC_ERR_INVALID,   // so that no squared distance overflows
                   "%s: feature value %lld is not finite and below 2^500 in magnitude", who, (long long)p);
    return SC_OK;
}

// ---- what the entry points share: the gates (self: dk_check, cross: dx_check), and the three steps around the search itself
int dk_check(const char *who, sc_ctx *c, const void *X, int dtype, int64_t n, int32_t d, int32_t k)
{
    SC_REQUIRE(c && X, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "%s: dtype must be SC_F32 or SC_F64", who);
    SC_REQUIRE(d >= 1 && d <= DF_DMAX, SC_ERR_INVALID, "%s: need 1 <= d <= %d, got %d", who, DF_DMAX, d);
    SC_REQUIRE(k >= 2 && k <= DF_KMAX, SC_ERR_INVALID, "%s: need 2 <= k <= %d, got %d", who, DF_KMAX, k);
    SC_REQUIRE(n > k && n <= INT32_MAX, SC_ERR_INVALID, "%s: need k < n <= 2^31 - 1, got n=%lld, k=%d", who, (long long)n, k);
    SC_REQUIRE(n * k <= ((int64_t)1 << 29), SC_ERR_INVALID, "%s: need n * k <= 2^29, got %lld", who, (long long)(n * k));
    return SC_OK;
}

// the last refusal of an entry point, after its own argument checks: it reads all n * d values, once per call
int dk_check_finite(const char *who, const void *X, int dtype, int64_t count)
{
    return dtype == SC_F32 ? df_require_finite(who, (const float *)X, count) : df_require_finite(who, (const double *)X, count);
}

// the gate of the cross search: two arrays, and a list may hold every reference row (k = n_ref) or one (k = 1)
int dx_check(const char *who, sc_ctx *c, const void *R, int dtype_r, int64_t n_ref, const void *Q, int dtype_q, int64_t n_query,
             int32_t d, int32_t k)
{
    SC_REQUIRE(c && R && Q, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE((dtype_r == SC_F32 || dtype_r == SC_F64) && (dtype_q == SC_F32 || dtype_q == SC_F64), SC_ERR_INVALID,
               "%s: dtype_r and dtype_q must be SC_F32 or SC_F64", who);
    SC_REQUIRE(d >= 1 && d <= DF_DMAX, SC_ERR_INVALID, "%s: need 1 <= d <= %d, got %d", who, DF_DMAX, d);
    SC_REQUIRE(k >= 1 && k <= DF_KMAX, SC_ERR_INVALID, "%s: need 1 <= k <= %d, got %d", who, DF_KMAX, k);
    SC_REQUIRE(n_ref >= k && n_ref <= INT32_MAX, SC_ERR_INVALID, "%s: need k <= n_ref <= 2^31 - 1, got n_ref=%lld, k=%d", who,
               (long long)n_ref, k);
    SC_REQUIRE(n_query >= 1 && n_query <= ((int64_t)1 << 29) / k, SC_ERR_INVALID, "%s: need 1 <= n_query and n_query * k <= 2^29, got n_query=%lld, k=%d",
               who, (long long)n_query, k);
    return SC_OK;
}

// raw[n][d] of the caller -> X[n][dp] on the device
int dk_upload(sc_ctx *c, const void *X, int dtype, int64_t n, int d, int dp, DBuf &raw, DBuf &wide)
{
    hipStream_t s = c->stream;
    const size_t es = dtype == SC_F32 ? sizeof(float) : sizeof(double);
    SC_TRY(raw.ensure(es * (size_t)(n * d), &c->mem));
    SC_TRY(wide.ensure(sizeof(double) * (size_t)(n * dp), &c->mem));
    SC_HIP(hipMemcpyAsync(raw.p, X, es * (size_t)(n * d), hipMemcpyHostToDevice, s));
    const dim3 widen((unsigned)ceil_div64(n * dp, 256)), tpb(256);
    if (dtype == SC_F32) hipLaunchKernelGGL(k_df_widen<float>, widen, tpb, 0, s, raw.as<float>(), n, d, dp, wide.as<double>());
    else hipLaunchKernelGGL(k_df_widen<double>, widen, tpb, 0, s, raw.as<double>(), n, d, dp, wide.as<double>());
    return SC_OK;
}

// a new search: nothing that stood on the old lists stays valid, of either kind; the lists' buffers, the upload(s), the
// rows widened to dp columns.  Q = null: the self search.
int dk_begin(sc_ctx *c, const DkShape &sh, int d, const void *X, int dtype, const void *Q, int dtype_q)
{
    SC_HIP(hipSetDevice(c->device));
    sc_ctx::DenseKnn &f = c->knn;
    lg_invalidate(c, true);
    f.cross = false;
    SC_TRY(f.idx.ensure(sizeof(int32_t) * (size_t)(sh.nq * sh.k), &c->mem));
    SC_TRY(f.d2.ensure(sizeof(double) * (size_t)(sh.nq * sh.k), &c->mem));
    SC_TRY(dk_upload(c, X, dtype, sh.n, d, sh.dp, f.raw, f.X));
    if (Q) SC_TRY(dk_upload(c, Q, dtype_q, sh.nq, d, sh.dp, f.qraw, f.Q));
    return SC_OK;
}

// the direct search on the resident rows: with one candidate range straight into the result, else partial lists and a merge
template <class... QA>
int dk_direct(sc_ctx *c, const DkShape &sh, int splits, QA... qa)
{
    sc_ctx::DenseKnn &f = c->knn;
    const bool lds = sh.dp > DF_DREG;
    const int64_t nq = sh.nq;
    const DkSplit sp = dk_split(nq, lds ? DF_QB_L : DF_QB, lds ? DF_TILE_L : DF_TILE, sh.n, splits);
    if (sp.S > 1) {
        SC_TRY(f.pidx.ensure(sizeof(int32_t) * (size_t)(nq * sh.k) * sp.S, &c->mem));
        SC_TRY(f.pd2.ensure(sizeof(double) * (size_t)(nq * sh.k) * sp.S, &c->mem));
    }
    KernelTimerScope ts(c, SC_K_DIFF_KNN);
    int32_t *pidx = sp.S > 1 ? f.pidx.as<int32_t>() : f.idx.as<int32_t>();
    double *pd2 = sp.S > 1 ? f.pd2.as<double>() : f.d2.as<double>();
    dk_by_k(sh.k, [&](auto K) {
        df_launch_search<decltype(K)::value>(c, sh, sp.S, sp.len, pidx, pd2, qa...);
        if (sp.S > 1) df_launch_merge<decltype(K)::value, false>(c, nq, sh.k, sp.S, nullptr);
    });
    return SC_OK;
}

// the queries' norms for the filter: the candidates' own in the self search, a second array in the cross search
void nb_query_norms(sc_ctx *, int) {}
void nb_query_norms(sc_ctx *c, int dp, const double *Q, int64_t nq)
{
    hipLaunchKernelGGL(k_nb_norms, dim3((unsigned)ceil_div64(nq, 256)), dim3(256), 0, c->stream, Q, nq, dp, c->knn.qnorm.as<double>());
}

// steps 1 to 4 of the Gram path on the resident rows; *nrows_out = the rows that went through the fallback
template <class... QA>
int nb_filtered(const char *who, sc_ctx *c, const DkShape &sh, int L, int64_t *nrows_out, QA... qa)
{
    sc_ctx::DenseKnn &f = c->knn;
    hipStream_t s = c->stream;
    const int64_t n = sh.n, nq = sh.nq;
    const int dp = sh.dp, k = sh.k;
    const double ce = (double)(4 * dp + 32) * 0x1p-52;
    SC_TRY(f.gnorm.ensure(sizeof(double) * (size_t)n, &c->mem));
    if (sizeof...(QA)) SC_TRY(f.qnorm.ensure(sizeof(double) * (size_t)nq, &c->mem));
    SC_TRY(f.gkept.ensure(sizeof(int32_t) * (size_t)(nq * L), &c->mem));
    SC_TRY(f.gcnt.ensure(sizeof(int32_t) * (size_t)nq, &c->mem));
    SC_TRY(f.glo.ensure(sizeof(double) * (size_t)nq, &c->mem));
    SC_TRY(f.grows.ensure(sizeof(int32_t) * (size_t)(nq + 1), &c->mem));   // [0]: the number of listed rows, then the rows
    const int32_t *rows = f.grows.as<int32_t>() + 1;
    int32_t nrows32 = 0;
    {
        KernelTimerScope ts(c, SC_K_NEIGHBORS_GRAM);
        hipLaunchKernelGGL(k_nb_norms, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, s, f.X.as<double>(), n, dp, f.gnorm.as<double>());
        nb_query_norms(c, dp, qa...);
        hipLaunchKernelGGL(k_nb_zero, dim3(1), dim3(1), 0, s, f.grows.as<int32_t>());
        if constexpr (sizeof...(QA) > 0) nb_launch_filter(c, sh, L, ce, qa..., (const double *)f.qnorm.as<double>());
        else nb_launch_filter(c, sh, L, ce);
        dk_by_k(k, [&](auto K) { nb_launch_rerank<decltype(K)::value>(c, sh, L, qa...); });
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(&nrows32, f.grows.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    const int64_t nrows = nrows32;
    SC_REQUIRE(nrows >= 0 && nrows <= nq, SC_ERR_HIP, "%s: %lld uncertified rows out of range", who, (long long)nrows);
    *nrows_out = nrows;
    if (nrows == 0) return SC_OK;
    // the fallback: the LDS form of the direct search for the listed rows, its candidate ranges by their number
    const DkSplit sp = dk_split(nrows, DF_QB_L, DF_TILE_L, n, 0);
    SC_TRY(f.pidx.ensure(sizeof(int32_t) * (size_t)(nrows * k) * sp.S, &c->mem));
    SC_TRY(f.pd2.ensure(sizeof(double) * (size_t)(nrows * k) * sp.S, &c->mem));
    KernelTimerScope ts(c, SC_K_NEIGHBORS_GRAM);
    dk_by_k(k, [&](auto K) {
        hipLaunchKernelGGL((k_df_knn_lds<decltype(K)::value, true, QA...>), dim3((unsigned)ceil_div64(nrows, DF_QB_L), (unsigned)sp.S),
                           dim3(DF_QB_L), 0, s, f.X.as<double>(), n, dp, k, sp.len, f.pidx.as<int32_t>(), f.pd2.as<double>(), rows, nrows,
                           qa...);
        df_launch_merge<decltype(K)::value, true>(c, nrows, k, sp.S, rows);
    });
    return SC_OK;
}

// the lists to the caller, if asked for, and resident: for the graphs (self) or for the gathers of sc_ingest.hip (cross)
int dk_end(sc_ctx *c, const DkShape &sh, bool cross, int32_t *idx_out, double *d2_out)
{
    sc_ctx::DenseKnn &f = c->knn;
    const size_t cells = (size_t)(sh.nq * sh.k);
    SC_HIP(hipGetLastError());
    if (idx_out) SC_HIP(hipMemcpyAsync(idx_out, f.idx.p, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, c->stream));
    if (d2_out) SC_HIP(hipMemcpyAsync(d2_out, f.d2.p, sizeof(double) * cells, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    f.n = sh.n;
    f.nq = sh.nq;
    f.d = sh.dp;
    f.k = sh.k;
    (cross ? f.cross : f.valid) = true;
    return SC_OK;
}

// the search itself in the form the pack asks for: path 1 = the direct kernels over `splits` candidate ranges, 2 = the filter
template <class... QA>
int dk_run(const char *who, sc_ctx *c, const DkShape &sh, int path, int splits, int L, int64_t *nrows, QA... qa)
{
    return path == 1 ? dk_direct(c, sh, splits, qa...) : nb_filtered(who, c, sh, L, nrows, qa...);
}

// what the entry points share once each has checked its own arguments: the finite check(s), the upload, the search
// (path 0: the size rule's choice by the numbers of queries and of pairs; `slack` spare list entries on path 2), the lists out;
// info_out (may be null): path taken, list length, rows certified, rows through the fallback.  Q = null: the self search.
int dk_search(const char *who, sc_ctx *c, const void *X, int dtype, int64_t n, const void *Q, int dtype_q, int64_t nq, int d, int k,
              int path, int splits, int slack, int32_t *idx_out, double *d2_out, int64_t *info_out)
{
    if (Q) {   // the message names the array
        SC_TRY(dk_check_finite((std::string(who) + ", R").c_str(), X, dtype, n * d));
        SC_TRY(dk_check_finite((std::string(who) + ", Q").c_str(), Q, dtype_q, nq * d));
    } else {
        SC_TRY(dk_check_finite(who, X, dtype, n * d));
    }
    const DkShape sh{n, Q ? nq : n, (int)align_up64(d, 8), k};
    const int64_t pairs = sh.nq * n;
    if (path == 0)
        path = sh.nq >= NB_GRAM_QUERIES_FROM && ((sh.dp > 32 && pairs >= NB_GRAM_PAIRS_FROM_WIDE) || (sh.dp >= 24 && pairs >= NB_GRAM_PAIRS_FROM))
                   ? 2 : 1;
    const int L = path == 1 ? k : k + (slack ? slack : NB_SLACK_DEFAULT);
    int64_t nrows = 0;
    SC_TRY(dk_begin(c, sh, d, X, dtype, Q, dtype_q));
    if (Q) SC_TRY(dk_run(who, c, sh, path, splits, L, &nrows, (const double *)c->knn.Q.as<double>(), sh.nq));
    else SC_TRY(dk_run(who, c, sh, path, splits, L, &nrows));
    SC_TRY(dk_end(c, sh, Q != nullptr, idx_out, d2_out));
    if (info_out) {
        info_out[0] = path;
        info_out[1] = L;
        info_out[2] = path == 1 ? 0 : sh.nq - nrows;
        info_out[3] = nrows;
    }
    return SC_OK;
}

}  // namespace

// an entry point: the shared gate, the refusals of its own arguments, the shared body -- the order a call is refused in
extern "C" int sc_knn_dense(sc_ctx *c, const void *X, int dtype, int64_t n, int32_t d, int32_t k, int32_t splits, int32_t *idx_out,
                            double *d2_out)
{
    const char *who = "sc_knn_dense";
    SC_TRY(dk_check(who, c, X, dtype, n, d, k));
    SC_REQUIRE(splits >= 0 && splits <= 65535, SC_ERR_INVALID, "%s: need 0 <= splits <= 65535, got %d", who, splits);
    return dk_search(who, c, X, dtype, n, nullptr, 0, 0, d, k, 1, splits, 0, idx_out, d2_out, nullptr);
}

extern "C" int sc_knn_dense_gram(sc_ctx *c, const void *X, int dtype, int64_t n, int32_t d, int32_t k, int32_t path, int32_t slack,
                                 int32_t *idx_out, double *d2_out, int64_t *info_out)
{
    const char *who = "sc_knn_dense_gram";
    SC_REQUIRE(info_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_TRY(dk_check(who, c, X, dtype, n, d, k));
    SC_REQUIRE(path >= 0 && path <= 2, SC_ERR_INVALID, "%s: path must be 0 (the library's choice), 1 (direct) or 2 (Gram filter), got %d", who,
               path);
    SC_REQUIRE(slack >= 0 && slack <= NB_SLACK_MAX, SC_ERR_INVALID, "%s: need 0 <= slack <= %d, got %d", who, NB_SLACK_MAX, slack);
    return dk_search(who, c, X, dtype, n, nullptr, 0, 0, d, k, path, 0, slack, idx_out, d2_out, info_out);
}

extern "C" int sc_knn_cross(sc_ctx *c, const void *R, int dtype_r, int64_t n_ref, const void *Q, int dtype_q, int64_t n_query, int32_t d,
                            int32_t k, int32_t path, int32_t slack, int32_t *idx_out, double *d2_out, int64_t *info_out)
{
    const char *who = "sc_knn_cross";
    SC_REQUIRE(info_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_TRY(dx_check(who, c, R, dtype_r, n_ref, Q, dtype_q, n_query, d, k));
    SC_REQUIRE(path >= 0 && path <= 2, SC_ERR_INVALID, "%s: path must be 0 (the library's choice), 1 (direct) or 2 (Gram filter), got %d", who,
               path);
    SC_REQUIRE(slack >= 0 && slack <= NB_SLACK_MAX, SC_ERR_INVALID, "%s: need 0 <= slack <= %d, got %d", who, NB_SLACK_MAX, slack);
    return dk_search(who, c, R, dtype_r, n_ref, Q, dtype_q, n_query, d, k, path, 0, slack, idx_out, d2_out, info_out);
}
