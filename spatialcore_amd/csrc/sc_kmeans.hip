// sc_kmeans.hip -- k-means++ seeding and Lloyd iterations for identify_niches (NB:299-522).
//
// The reference runs sklearn's KMeans(init="k-means++", n_init, max_iter, random_state).fit_predict on the
// neighbourhood profiles.  This file replays sklearn 1.7.2's algorithm step for step:
//  - the host centres nothing and draws nothing: X_mean, tol and every uniform of every run come from numpy;
//    the device subtracts X_mean elementwise (one rounding in the input type, as `X -= X_mean`);
//  - all n_init runs advance together: every pass over X serves every run still active;
//  - seeding: D^2 = (-2 x.c + |c|^2) + |x|^2 in fp64, stored in the input type and clipped at 0; the prefix sum
//    that the draws are searched in and every potential are ONE fixed summation order (below), fp64, rounded to the
//    input type once (the correctly rounded value of sklearn's float32 `D^2 @ w`);
//  - Lloyd: fp64 distances, first index on ties, per-workgroup fp64 partial sums reduced in a fixed order (no
//    floating-point atomics): the result is a function of the inputs alone, bit for bit.
//
// Summation order of a potential ("hsum"): points in chunks of 64 consecutive indices, each chunk summed
// sequentially; the 64 chunks of a group (4096 points) summed sequentially; the groups summed sequentially.  The
// prefix value at point i is (P2[g-1] + P1[g][j-1]) + P0[g][j][e] (group g, chunk j, element e); a draw v is searched
// level by level (first group whose running total reaches v, then the chunk, then the element; the last one of a
// level when rounding leaves v above it; n - 1 when v exceeds the total).  tests/kmeans_restated.py states the same.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "sc_ctx.h"

namespace {

constexpr int KM_CH = 64;              // points per chunk = threads of a seeding workgroup
constexpr int KM_GRP = KM_CH * KM_CH;  // points per group
constexpr int KM_LMAX = 32;            // local trials per seeding round: 2 + int(log(K)) <= 23 for K < 2^31
constexpr int KM_TPB = 256;            // points per Lloyd tile = threads of a Lloyd workgroup
constexpr int KM_FAST = 64;            // C <= 64 and K <= 64: centres in LDS, the point's row in registers

// per-run state words
enum { ST_ACTIVE = 0, ST_STRICT, ST_ITER, ST_RELOC, ST_CHANGED, ST_WORDS = 8 };

template <class T>
__global__ __launch_bounds__(256) void k_km_center(const T *__restrict__ X, const T *__restrict__ mean, int64_t n, int C,
                                                   T *__restrict__ Xc, double *__restrict__ xn)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int c = 0; c < C; ++c) {
        const T v = X[i * C + c] - mean[c];
        Xc[i * C + c] = v;
        s = s + (double)v * (double)v;
    }
    xn[i] = s;
}

// D^2 of point p to the point q as sklearn's _euclidean_distances (squared, fp64 arithmetic, result in T, >= 0)
template <class T>
__device__ __forceinline__ T km_d2(const T *__restrict__ Xc, const double *__restrict__ xn, int C, int64_t p, int64_t q)
{
    double dot = 0.0;
    for (int c = 0; c < C; ++c) dot = dot + (double)Xc[p * C + c] * (double)Xc[q * C + c];
    const double d = (-2.0 * dot + xn[q]) + xn[p];
    const T t = (T)d;
    return t < (T)0 ? (T)0 : t;
}

// Seeding, step 1 of a round: fold the centre chosen last (centre[r]) into D^2 (first: D^2 = its distances) and
// write the chunk sums S0 and group sums S1.  grid (G, R), 64 threads: thread j owns chunk j of group g.
template <class T>
__global__ __launch_bounds__(64) void k_seed_scan(const T *__restrict__ Xc, const double *__restrict__ xn, int64_t n, int C,
                                                  T *__restrict__ D2, const int64_t *__restrict__ centre, int first,
                                                  double *__restrict__ S0, double *__restrict__ S1)
{
    __shared__ double s[KM_CH];
    const int r = blockIdx.y, j = threadIdx.x;
    const int64_t g = blockIdx.x, G = gridDim.x;
    const int64_t q = centre[r];
    T *d2 = D2 + (int64_t)r * n;
    double acc = 0.0;
    const int64_t p0 = (g * KM_CH + j) * KM_CH;
    for (int e = 0; e < KM_CH; ++e) {
        const int64_t p = p0 + e;
        if (p >= n) break;
        const T d = km_d2(Xc, xn, C, p, q);
        const T v = first ? d : (d < d2[p] ? d : d2[p]);
        d2[p] = v;
        acc = acc + (double)v;
    }
    S0[((int64_t)r * G + g) * KM_CH + j] = acc;
    s[j] = acc;
    __syncthreads();
    if (j == 0) {
        double t = 0.0;
        for (int k = 0; k < KM_CH; ++k) t = t + s[k];
        S1[(int64_t)r * G + g] = t;
    }
}

// Seeding, step 2: pot = T(total); candidate t = searchsorted(prefix, u_t * pot).  grid R, thread t < L.
template <class T>
__global__ __launch_bounds__(64) void k_seed_search(const double *__restrict__ S0, const double *__restrict__ S1,
                                                    const T *__restrict__ D2, int64_t n, int64_t G,
                                                    const double *__restrict__ u, int64_t u_stride, int L,
                                                    int64_t *__restrict__ cand, double *__restrict__ pot_out)
{
    const int r = blockIdx.x, t = threadIdx.x;
    if (t >= L) return;
    const double *s1 = S1 + (int64_t)r * G;
    double total = 0.0;
    for (int64_t g = 0; g < G; ++g) total = total + s1[g];
    const double pot = (double)(T)total;
    if (t == 0) pot_out[r] = pot;
    const double v = u[(int64_t)r * u_stride + t] * pot;
    double run = 0.0, prev = 0.0;
    int64_t g = 0;
    for (; g < G; ++g) {
        prev = run;
        run = run + s1[g];
        if (run >= v) break;
    }
    int64_t idx;
    if (g == G) {
        idx = n - 1;
    } else {
        const double *s0 = S0 + ((int64_t)r * G + g) * KM_CH;
        const double base2 = prev;
        double p1 = 0.0, p1prev = 0.0;
        int j = 0;
        for (; j < KM_CH; ++j) {
            p1prev = p1;
            p1 = p1 + s0[j];
            if (base2 + p1 >= v) break;
        }
        if (j == KM_CH) j = KM_CH - 1;   // p1prev: the prefix before the last chunk
        const double base1 = j == 0 ? base2 : base2 + p1prev;
        const T *d2 = D2 + (int64_t)r * n;
        const int64_t c0 = (g * KM_CH + j) * KM_CH;
        double p0 = 0.0;
        int e = 0;
        for (; e < KM_CH; ++e) {
            const int64_t p = c0 + e;
            p0 = p0 + (p < n ? (double)d2[p] : 0.0);
            if (base1 + p0 >= v) break;
        }
        if (e == KM_CH) e = KM_CH - 1;
        idx = c0 + e;
        if (idx > n - 1) idx = n - 1;
    }
    cand[(int64_t)r * KM_LMAX + t] = idx;
}

// Seeding, step 3: per candidate, the group sums of min(D^2, d^2(., candidate)).  grid (G, R), 64 threads.
template <class T>
__global__ __launch_bounds__(64) void k_seed_cand(const T *__restrict__ Xc, const double *__restrict__ xn, int64_t n, int C,
                                                  const T *__restrict__ D2, const int64_t *__restrict__ cand, int L,
                                                  double *__restrict__ cpart)
{
    __shared__ double s[KM_LMAX][KM_CH];
    const int r = blockIdx.y, j = threadIdx.x;
    const int64_t g = blockIdx.x, G = gridDim.x;
    const T *d2 = D2 + (int64_t)r * n;
    const int64_t p0 = (g * KM_CH + j) * KM_CH;
    for (int t = 0; t < L; ++t) {
        const int64_t q = cand[(int64_t)r * KM_LMAX + t];
        double acc = 0.0;
        for (int e = 0; e < KM_CH; ++e) {
            const int64_t p = p0 + e;
            if (p >= n) break;
            const T d = km_d2(Xc, xn, C, p, q);
            const T m = d < d2[p] ? d : d2[p];
            acc = acc + (double)m;
        }
        s[t][j] = acc;
    }
    __syncthreads();
    if (j < L) {
        double tot = 0.0;
        for (int k = 0; k < KM_CH; ++k) tot = tot + s[j][k];
        cpart[((int64_t)r * KM_LMAX + j) * G + g] = tot;
    }
}

// Seeding, step 4: candidate potentials rounded to T, the first smallest wins.  grid R, thread t < L.
template <class T>
__global__ __launch_bounds__(64) void k_seed_best(const double *__restrict__ cpart, int64_t G, int L,
                                                  const int64_t *__restrict__ cand, int64_t *__restrict__ centre,
                                                  int64_t *__restrict__ seeds, int K, int round)
{
    __shared__ T pots[KM_LMAX];
    const int r = blockIdx.x, t = threadIdx.x;
    if (t < L) {
        const double *cp = cpart + ((int64_t)r * KM_LMAX + t) * G;
        double tot = 0.0;
        for (int64_t g = 0; g < G; ++g) tot = tot + cp[g];
        pots[t] = (T)tot;
    }
    __syncthreads();
    if (t == 0) {
        int b = 0;
        for (int k = 1; k < L; ++k)
            if (pots[k] < pots[b]) b = k;
        const int64_t id = cand[(int64_t)r * KM_LMAX + b];
        centre[r] = id;
        seeds[(int64_t)r * K + round] = id;
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_km_init(const T *__restrict__ Xc, int64_t n, int C, int K,
                                                 const int64_t *__restrict__ seeds, T *__restrict__ cent,
                                                 int32_t *__restrict__ labels, int64_t *__restrict__ state)
{
    const int r = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (int64_t)K * C) {
        const int64_t k = i / C, c = i % C;
        cent[(int64_t)r * K * C + i] = Xc[seeds[(int64_t)r * K + k] * C + c];
    }
    if (i < n) labels[(int64_t)r * n + i] = -1;
    if (i < ST_WORDS) state[(int64_t)r * ST_WORDS + i] = i == ST_ACTIVE ? 1 : 0;
}

// One Lloyd E-step for every run (grid (NB, R), 256 threads, tiles of 256 points in grid-stride order).
// mode 0: assign (fp64 distances, first index on ties), count changed labels, accumulate per-workgroup fp64 sums
//         and counts of the new partition (thread-owned (cluster, feature) pairs, points in index order);
// mode 1: the final pass -- runs that converged strictly keep their labels, the others are reassigned against the
//         final centres (sklearn's update_centers=False pass); per-workgroup inertia partials.
// FAST: C <= 64 and K <= 64 -- centres in LDS, the point's row in registers.
template <class T, bool FAST>
__global__ __launch_bounds__(256) void k_km_estep(const T *__restrict__ Xc, int64_t n, int C, int K,
                                                  const T *__restrict__ cent, int32_t *__restrict__ labels,
                                                  const int64_t *__restrict__ state, int mode, double *__restrict__ part,
                                                  int64_t *__restrict__ cnt, int64_t *__restrict__ chg,
                                                  double *__restrict__ inert)
{
    __shared__ double sc[FAST ? KM_FAST * KM_FAST : 1];
    __shared__ int32_t slab[KM_TPB];
    __shared__ double sred[KM_TPB];
    __shared__ int64_t sredi[KM_TPB];
    const int r = blockIdx.y, tid = threadIdx.x;
    const int64_t b = blockIdx.x, NB = gridDim.x;
    const int64_t *st = state + (int64_t)r * ST_WORDS;
    if (mode == 0 && !st[ST_ACTIVE]) return;
    const bool reassign = mode == 0 || !st[ST_STRICT];
    const int KC = K * C;
    const T *ce = cent + (int64_t)r * KC;
    int32_t *lab = labels + (int64_t)r * n;
    if (FAST) {
        for (int i = tid; i < KC; i += KM_TPB) sc[i] = (double)ce[i];
        __syncthreads();
    }
    double *pp = part + ((int64_t)r * NB + b) * KC;
    int64_t *cc = cnt + ((int64_t)r * NB + b) * K;
    int64_t changed = 0;
    double in_acc = 0.0;
    for (int64_t tile = b; tile * KM_TPB < n; tile += NB) {
        const int64_t p = tile * KM_TPB + tid;
        int l = -1;
        double dmin = 0.0;
        if (p < n) {
            const T *x = Xc + p * C;
            if (reassign) {
                double best = INFINITY;
                int bk = 0;
                if (FAST) {
                    double xr[KM_FAST];
#pragma unroll
                    for (int c = 0; c < KM_FAST; ++c) xr[c] = c < C ? (double)x[c] : 0.0;
                    for (int k = 0; k < K; ++k) {
                        double d = 0.0;
#pragma unroll
                        for (int c = 0; c < KM_FAST; ++c) {
                            if (c < C) {
                                const double t = xr[c] - sc[k * C + c];
                                d = d + t * t;
                            }
                        }
                        if (d < best) { best = d; bk = k; }
                    }
                } else {
                    for (int k = 0; k < K; ++k) {
                        double d = 0.0;
                        for (int c = 0; c < C; ++c) {
                            const double t = (double)x[c] - (double)ce[(int64_t)k * C + c];
                            d = d + t * t;
                        }
                        if (d < best) { best = d; bk = k; }
                    }
                }
                l = bk;
                dmin = best;
                if (mode == 0 && lab[p] != l) ++changed;
                lab[p] = l;
            } else {
                l = lab[p];
                double d = 0.0;
                for (int c = 0; c < C; ++c) {
                    const double t = (double)x[c] - (double)ce[(int64_t)l * C + c];
                    d = d + t * t;
                }
                dmin = d;
            }
            in_acc = in_acc + dmin;
        }
        if (mode == 0) {
            slab[tid] = l;
            __syncthreads();
            const int m = (int)min((int64_t)KM_TPB, n - tile * KM_TPB);
            const T *xt = Xc + tile * KM_TPB * C;
            for (int pr = tid; pr < KC; pr += KM_TPB) {
                const int k = pr / C, c = pr % C;
                double acc = tile == b ? 0.0 : pp[pr];
                for (int q = 0; q < m; ++q)
                    if (slab[q] == k) acc = acc + (double)xt[(int64_t)q * C + c];
                pp[pr] = acc;
            }
            for (int k = tid; k < K; k += KM_TPB) {
                int64_t cn = tile == b ? 0 : cc[k];
                for (int q = 0; q < m; ++q) cn += slab[q] == k;
                cc[k] = cn;
            }
            __syncthreads();
        }
    }
    // fixed-order block reductions: the per-thread values in LDS, thread 0 adds them in thread order
    sred[tid] = in_acc;
    sredi[tid] = changed;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        int64_t ch = 0;
        for (int k = 0; k < KM_TPB; ++k) { s = s + sred[k]; ch += sredi[k]; }
        if (mode == 0) chg[(int64_t)r * NB + b] = ch;
        else inert[(int64_t)r * NB + b] = s;
    }
}

// New centres, centre shift and the convergence rule of sklearn's Lloyd loop for one run (256 threads).
template <class T>
__device__ void km_apply(int r, const double *__restrict__ sums, const int64_t *__restrict__ counts, T *__restrict__ cent,
                         int64_t *__restrict__ state, int K, int C, double tol, int max_iter, double *sred)
{
    const int tid = threadIdx.x, KC = K * C;
    T *ce = cent + (int64_t)r * KC;
    const double *su = sums + (int64_t)r * KC;
    const int64_t *co = counts + (int64_t)r * K;
    double sh = 0.0;
    for (int pr = tid; pr < KC; pr += KM_TPB) {
        const int k = pr / C;
        const T nv = co[k] > 0 ? (T)(su[pr] / (double)co[k]) : (T)su[pr];   // an emptied cluster keeps its sum
        const double dd = (double)nv - (double)ce[pr];
        sh = sh + dd * dd;
        ce[pr] = nv;
    }
    sred[tid] = sh;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int k = 0; k < KM_TPB; ++k) s = s + sred[k];
        int64_t *st = state + (int64_t)r * ST_WORDS;
        st[ST_ITER] += 1;
        if (st[ST_CHANGED] == 0) {
            st[ST_STRICT] = 1;
            st[ST_ACTIVE] = 0;
        } else if (s <= tol || st[ST_ITER] >= max_iter) {
            st[ST_ACTIVE] = 0;
        }
    }
}

// Second stage of a Lloyd iteration: the workgroups' partials in workgroup order -> sums / counts; a run with an
// empty cluster stops here (ST_RELOC) for the host's relocation step.  grid R, 256 threads.
template <class T>
__global__ __launch_bounds__(256) void k_km_reduce(const double *__restrict__ part, const int64_t *__restrict__ cnt,
                                                   const int64_t *__restrict__ chg, int64_t NB, double *__restrict__ sums,
                                                   int64_t *__restrict__ counts, T *__restrict__ cent,
                                                   int64_t *__restrict__ state, int K, int C, double tol, int max_iter)
{
    __shared__ double sred[KM_TPB];
    __shared__ int empty;
    const int r = blockIdx.x, tid = threadIdx.x, KC = K * C;
    int64_t *st = state + (int64_t)r * ST_WORDS;
    if (!st[ST_ACTIVE]) return;
    if (tid == 0) empty = 0;
    __syncthreads();
    for (int pr = tid; pr < KC; pr += KM_TPB) {
        double s = 0.0;
        for (int64_t b = 0; b < NB; ++b) s = s + part[((int64_t)r * NB + b) * KC + pr];
        sums[(int64_t)r * KC + pr] = s;
    }
    for (int k = tid; k < K; k += KM_TPB) {
        int64_t s = 0;
        for (int64_t b = 0; b < NB; ++b) s += cnt[((int64_t)r * NB + b) * K + k];
        counts[(int64_t)r * K + k] = s;
        if (s == 0) empty = 1;
    }
    if (tid == 0) {
        int64_t s = 0;
        for (int64_t b = 0; b < NB; ++b) s += chg[(int64_t)r * NB + b];
        st[ST_CHANGED] = s;
    }
    __syncthreads();
    if (empty) {
        if (tid == 0) st[ST_RELOC] = 1;
        return;
    }
    km_apply<T>(r, sums, counts, cent, state, K, C, tol, max_iter, sred);
}

// After the host relocated the empty clusters of run r (sums / counts rewritten): the rest of the iteration.
template <class T>
__global__ __launch_bounds__(256) void k_km_apply(int r, const double *__restrict__ sums, const int64_t *__restrict__ counts,
                                                  T *__restrict__ cent, int64_t *__restrict__ state, int K, int C,
                                                  double tol, int max_iter)
{
    __shared__ double sred[KM_TPB];
    if (threadIdx.x == 0) state[(int64_t)r * ST_WORDS + ST_RELOC] = 0;
    km_apply<T>(r, sums, counts, cent, state, K, C, tol, max_iter, sred);
}

// Relocation input: squared distance of every point of run r to its cluster's centre before this iteration's update.
template <class T>
__global__ __launch_bounds__(256) void k_km_reloc_dist(const T *__restrict__ Xc, int64_t n, int C, int K,
                                                       const T *__restrict__ cent, const int32_t *__restrict__ labels,
                                                       int r, double *__restrict__ dist)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int l = labels[(int64_t)r * n + p];
    const T *ce = cent + ((int64_t)r * K + l) * C;
    double d = 0.0;
    for (int c = 0; c < C; ++c) {
        const double t = (double)Xc[p * C + c] - (double)ce[c];
        d = d + t * t;
    }
    dist[p] = d;
}

// _is_same_clustering(labels_a, labels_b): the first point of every cluster of a, then whether every point of a
// cluster of a has the label b gives that first point.  Integer atomics only (min and or): order-free.
__global__ __launch_bounds__(256) void k_km_first(const int32_t *__restrict__ la, int64_t n, int *__restrict__ first)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) atomicMin(&first[la[p]], (int)p);
}
__global__ __launch_bounds__(256) void k_km_same(const int32_t *__restrict__ la, const int32_t *__restrict__ lb, int64_t n,
                                                 const int *__restrict__ first, int *__restrict__ differ)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n && lb[p] != lb[first[la[p]]]) atomicOr(differ, 1);
}

// numpy's RandomState.choice(n, p=w / w.sum()) for unit weights w of type T, given its one random_sample() draw
template <class T>
std::vector<int64_t> first_centres(int64_t n, const double *u0, int64_t stride, int R)
{
    const double p = (double)((T)1 / (T)n);
    std::vector<double> cdf((size_t)n);
    double s = 0.0;
    for (int64_t i = 0; i < n; ++i) cdf[(size_t)i] = s = s + p;
    const double last = cdf[(size_t)n - 1];
    for (double &v : cdf) v = v / last;
    std::vector<int64_t> out((size_t)R);
    for (int r = 0; r < R; ++r) {
        const double u = u0[(int64_t)r * stride];
        out[(size_t)r] = std::upper_bound(cdf.begin(), cdf.end(), u) - cdf.begin();
        if (out[(size_t)r] > n - 1) out[(size_t)r] = n - 1;
    }
    return out;
}

template <class T>
int kmeans_fit(sc_ctx *c, const T *X, int64_t n, int C, int K, int R, int max_iter, double tol, const T *x_mean,
               const double *uniforms, int32_t *labels_out, T *centers_out, double *inertia_out, int64_t *seeds_out,
               int32_t *n_iter_out, int32_t *strict_out, int32_t *distinct_out, int32_t *run_labels_dev = nullptr)
{
    hipStream_t s = c->stream;
    const int L = 2 + (int)std::log((double)K);
    const int64_t ustride = 1 + (int64_t)(K - 1) * L;
    const int64_t G = ceil_div64(n, KM_GRP);
    const int64_t KC = (int64_t)K * C;
    const int64_t tiles = ceil_div64(n, KM_TPB);
    // workgroups per run of the Lloyd pass: every workgroup has a tile; partial sums stay below 256 MiB
    const int64_t NB = std::max<int64_t>(1, std::min<int64_t>({tiles, 256, ((int64_t)1 << 25) / std::max<int64_t>(1, R * KC)}));
    const bool fast = C <= KM_FAST && K <= KM_FAST;

    DBuf m[20];
    enum { XC, XN, D2, S0, S1, CAND, CPART, CENTRE, SEEDS, POT, U, LAB, CENT, PART, CNT, CHG, INERT, SUMS, COUNTS, STATE };
    const size_t sz[20] = {sizeof(T) * (size_t)(n * C), sizeof(double) * (size_t)n, sizeof(T) * (size_t)(R * n),
                           sizeof(double) * (size_t)(R * G * KM_CH), sizeof(double) * (size_t)(R * G),
                           sizeof(int64_t) * (size_t)(R * KM_LMAX), sizeof(double) * (size_t)(R * KM_LMAX * G),
                           sizeof(int64_t) * (size_t)R, sizeof(int64_t) * (size_t)(R * K), sizeof(double) * (size_t)R,
                           sizeof(double) * (size_t)(R * ustride), sizeof(int32_t) * (size_t)(R * n),
                           sizeof(T) * (size_t)(R * KC), sizeof(double) * (size_t)(R * NB * KC),
                           sizeof(int64_t) * (size_t)(R * NB * K), sizeof(int64_t) * (size_t)(R * NB),
                           sizeof(double) * (size_t)(R * NB), sizeof(double) * (size_t)(R * KC),
                           sizeof(int64_t) * (size_t)(R * K), sizeof(int64_t) * (size_t)(R * ST_WORDS)};
    for (int i = 0; i < 20; ++i) SC_TRY(m[i].ensure(std::max<size_t>(sz[i], 64), &c->mem));

    // ---- centring; first centres from the runs' random_sample draws --------------------------------
    DBuf xin, xmean;
    SC_TRY(xin.ensure(sizeof(T) * (size_t)(n * C), &c->mem));
    SC_TRY(xmean.ensure(sizeof(T) * (size_t)C, &c->mem));
    SC_HIP(hipMemcpyAsync(xin.p, X, sizeof(T) * (size_t)(n * C), hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(xmean.p, x_mean, sizeof(T) * (size_t)C, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(m[U].p, uniforms, sz[U], hipMemcpyHostToDevice, s));
    std::vector<int64_t> c0 = first_centres<T>(n, uniforms, ustride, R);
    std::vector<int64_t> seeds0((size_t)(R * K), -1);
    for (int r = 0; r < R; ++r) seeds0[(size_t)r * K] = c0[(size_t)r];
    SC_HIP(hipMemcpyAsync(m[CENTRE].p, c0.data(), sz[CENTRE], hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(m[SEEDS].p, seeds0.data(), sz[SEEDS], hipMemcpyHostToDevice, s));
    T *Xc = m[XC].template as<T>();
    const double *xn = m[XN].template as<double>();
    {
        KernelTimerScope ts(c, SC_K_KMEANS_SEED);
        hipLaunchKernelGGL(k_km_center<T>, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, s, xin.template as<T>(),
                           xmean.template as<T>(), n, C, Xc, m[XN].template as<double>());
        // ---- k-means++ seeding, all runs per launch ------------------------------------------------
        for (int round = 1; round < K; ++round) {
            hipLaunchKernelGGL(k_seed_scan<T>, dim3((unsigned)G, (unsigned)R), dim3(KM_CH), 0, s, Xc, xn, n, C,
                               m[D2].template as<T>(), m[CENTRE].template as<int64_t>(), round == 1 ? 1 : 0, m[S0].template as<double>(),
                               m[S1].template as<double>());
            hipLaunchKernelGGL(k_seed_search<T>, dim3((unsigned)R), dim3(KM_CH), 0, s, m[S0].template as<double>(),
                               m[S1].template as<double>(), m[D2].template as<T>(), n, G,
                               m[U].template as<double>() + 1 + (int64_t)(round - 1) * L, ustride, L, m[CAND].template as<int64_t>(),
                               m[POT].template as<double>());
            hipLaunchKernelGGL(k_seed_cand<T>, dim3((unsigned)G, (unsigned)R), dim3(KM_CH), 0, s, Xc, xn, n, C,
                               m[D2].template as<T>(), m[CAND].template as<int64_t>(), L, m[CPART].template as<double>());
            hipLaunchKernelGGL(k_seed_best<T>, dim3((unsigned)R), dim3(KM_CH), 0, s, m[CPART].template as<double>(), G, L,
                               m[CAND].template as<int64_t>(), m[CENTRE].template as<int64_t>(), m[SEEDS].template as<int64_t>(), K, round);
        }
        const int64_t w = std::max<int64_t>(n, std::max<int64_t>(KC, ST_WORDS));
        hipLaunchKernelGGL(k_km_init<T>, dim3((unsigned)ceil_div64(w, 256), (unsigned)R), dim3(256), 0, s, Xc, n, C, K,
                           m[SEEDS].template as<int64_t>(), m[CENT].template as<T>(), m[LAB].template as<int32_t>(),
                           m[STATE].template as<int64_t>());
    }
    SC_HIP(hipGetLastError());

    // ---- Lloyd iterations, all active runs per launch; one small read-back per iteration -----------------
    std::vector<int64_t> st((size_t)(R * ST_WORDS));
    auto estep = [&](int mode) {
        if (fast)
            hipLaunchKernelGGL((k_km_estep<T, true>), dim3((unsigned)NB, (unsigned)R), dim3(KM_TPB), 0, s, Xc, n, C, K,
                               m[CENT].template as<T>(), m[LAB].template as<int32_t>(), m[STATE].template as<int64_t>(), mode,
                               m[PART].template as<double>(), m[CNT].template as<int64_t>(), m[CHG].template as<int64_t>(),
                               m[INERT].template as<double>());
        else
            hipLaunchKernelGGL((k_km_estep<T, false>), dim3((unsigned)NB, (unsigned)R), dim3(KM_TPB), 0, s, Xc, n, C, K,
                               m[CENT].template as<T>(), m[LAB].template as<int32_t>(), m[STATE].template as<int64_t>(), mode,
                               m[PART].template as<double>(), m[CNT].template as<int64_t>(), m[CHG].template as<int64_t>(),
                               m[INERT].template as<double>());
    };
    std::vector<double> hsums, hdist;
    std::vector<int64_t> hcounts;
    std::vector<int32_t> hlab;
    DBuf ddist;
    for (int it = 0; it < max_iter; ++it) {
        {
            KernelTimerScope ts(c, SC_K_KMEANS_LLOYD);
            estep(0);
            hipLaunchKernelGGL(k_km_reduce<T>, dim3((unsigned)R), dim3(KM_TPB), 0, s, m[PART].template as<double>(),
                               m[CNT].template as<int64_t>(), m[CHG].template as<int64_t>(), NB, m[SUMS].template as<double>(),
                               m[COUNTS].template as<int64_t>(), m[CENT].template as<T>(), m[STATE].template as<int64_t>(), K, C, tol,
                               max_iter);
        }
        SC_HIP(hipGetLastError());
        SC_HIP(hipMemcpyAsync(st.data(), m[STATE].p, sz[STATE], hipMemcpyDeviceToHost, s));
        SC_HIP(hipStreamSynchronize(s));
        for (int r = 0; r < R; ++r) {
            if (!st[(size_t)r * ST_WORDS + ST_RELOC]) continue;
            // _relocate_empty_clusters_dense: the empty clusters in index order take the points farthest from their
            // (old) centres, farthest first; equal distances go to the lowest point index (sklearn: unspecified)
            hsums.resize((size_t)KC);
            hcounts.resize((size_t)K);
            hlab.resize((size_t)n);
            hdist.resize((size_t)n);
            SC_TRY(ddist.ensure(sizeof(double) * (size_t)n, &c->mem));
            hipLaunchKernelGGL(k_km_reloc_dist<T>, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, s, Xc, n, C, K,
                               m[CENT].template as<T>(), m[LAB].template as<int32_t>(), r, ddist.template as<double>());
            SC_HIP(hipGetLastError());
            SC_HIP(hipMemcpyAsync(hsums.data(), m[SUMS].template as<double>() + (int64_t)r * KC, sizeof(double) * (size_t)KC,
                                  hipMemcpyDeviceToHost, s));
            SC_HIP(hipMemcpyAsync(hcounts.data(), m[COUNTS].template as<int64_t>() + (int64_t)r * K, sizeof(int64_t) * (size_t)K,
                                  hipMemcpyDeviceToHost, s));
            SC_HIP(hipMemcpyAsync(hlab.data(), m[LAB].template as<int32_t>() + (int64_t)r * n, sizeof(int32_t) * (size_t)n,
                                  hipMemcpyDeviceToHost, s));
            SC_HIP(hipMemcpyAsync(hdist.data(), ddist.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
            SC_HIP(hipStreamSynchronize(s));
            std::vector<int> empties;
            for (int k = 0; k < K; ++k)
                if (hcounts[(size_t)k] == 0) empties.push_back(k);
            std::vector<int64_t> order((size_t)n);
            std::iota(order.begin(), order.end(), (int64_t)0);
            const size_t ne = empties.size();
            std::partial_sort(order.begin(), order.begin() + (ptrdiff_t)ne, order.end(), [&](int64_t a, int64_t b2) {
                return hdist[(size_t)a] > hdist[(size_t)b2] || (hdist[(size_t)a] == hdist[(size_t)b2] && a < b2);
            });
            for (size_t e = 0; e < ne; ++e) {
                const int nk = empties[e];
                const int64_t f = order[e];
                const int ok = hlab[(size_t)f];
                for (int cc = 0; cc < C; ++cc) {
                    const double xv = (double)(T)(X[f * C + cc] - x_mean[cc]);
                    hsums[(size_t)ok * C + cc] -= xv;
                    hsums[(size_t)nk * C + cc] = xv;
                }
                hcounts[(size_t)nk] = 1;
                hcounts[(size_t)ok] -= 1;
            }
            SC_HIP(hipMemcpyAsync(m[SUMS].template as<double>() + (int64_t)r * KC, hsums.data(), sizeof(double) * (size_t)KC,
                                  hipMemcpyHostToDevice, s));
            SC_HIP(hipMemcpyAsync(m[COUNTS].template as<int64_t>() + (int64_t)r * K, hcounts.data(), sizeof(int64_t) * (size_t)K,
                                  hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_km_apply<T>, dim3(1), dim3(KM_TPB), 0, s, r, m[SUMS].template as<double>(),
                               m[COUNTS].template as<int64_t>(), m[CENT].template as<T>(), m[STATE].template as<int64_t>(), K, C, tol,
                               max_iter);
            SC_HIP(hipGetLastError());
            SC_HIP(hipMemcpyAsync(st.data() + (size_t)r * ST_WORDS, m[STATE].template as<int64_t>() + (int64_t)r * ST_WORDS,
                                  sizeof(int64_t) * ST_WORDS, hipMemcpyDeviceToHost, s));
            SC_HIP(hipStreamSynchronize(s));
        }
        bool any = false;
        for (int r = 0; r < R; ++r) any = any || st[(size_t)r * ST_WORDS + ST_ACTIVE];
        if (!any) break;
    }

    // ---- final E-step of the runs that did not converge strictly, inertia of every run --------------------------
    std::vector<double> inert((size_t)(R * NB));
    {
        KernelTimerScope ts(c, SC_K_KMEANS_LLOYD);
        estep(1);
    }
    SC_HIP(hipGetLastError());
    if (run_labels_dev) {   // sc_kmeans_run_labels: every run's labels stay on the device; no best run is chosen
        SC_HIP(hipMemcpyAsync(run_labels_dev, m[LAB].p, sz[LAB], hipMemcpyDeviceToDevice, s));
        SC_HIP(hipStreamSynchronize(s));
        return SC_OK;
    }
    SC_HIP(hipMemcpyAsync(inert.data(), m[INERT].p, sz[INERT], hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(st.data(), m[STATE].p, sz[STATE], hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(seeds_out, m[SEEDS].p, sz[SEEDS], hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    std::vector<double> inertia((size_t)R);
    for (int r = 0; r < R; ++r) {
        double t = 0.0;
        for (int64_t b = 0; b < NB; ++b) t = t + inert[(size_t)(r * NB + b)];
        inertia[(size_t)r] = t;
    }

    // ---- best run: a later run replaces the best only if its inertia is lower and its partition differs ----------
    int best = 0;
    DBuf dfirst;
    SC_TRY(dfirst.ensure(sizeof(int) * (size_t)(K + 1), &c->mem));
    for (int r = 1; r < R; ++r) {
        if (!(inertia[(size_t)r] < inertia[(size_t)best])) continue;
        const int32_t *la = m[LAB].template as<int32_t>() + (int64_t)r * n, *lb = m[LAB].template as<int32_t>() + (int64_t)best * n;
        SC_HIP(hipMemsetAsync(dfirst.p, 0x7f, sizeof(int) * (size_t)K, s));
        SC_HIP(hipMemsetAsync(dfirst.template as<int>() + K, 0, sizeof(int), s));
        hipLaunchKernelGGL(k_km_first, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, s, la, n, dfirst.template as<int>());
        hipLaunchKernelGGL(k_km_same, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, s, la, lb, n, dfirst.template as<int>(),
                           dfirst.template as<int>() + K);
        SC_HIP(hipGetLastError());
        int differ = 0;
        SC_HIP(hipMemcpyAsync(&differ, dfirst.template as<int>() + K, sizeof(int), hipMemcpyDeviceToHost, s));
        SC_HIP(hipStreamSynchronize(s));
        if (differ) best = r;
    }
    SC_HIP(hipMemcpyAsync(labels_out, m[LAB].template as<int32_t>() + (int64_t)best * n, sizeof(int32_t) * (size_t)n,
                          hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(centers_out, m[CENT].template as<T>() + (int64_t)best * KC, sizeof(T) * (size_t)KC,
                          hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    for (int64_t i = 0; i < KC; ++i) centers_out[i] = centers_out[i] + x_mean[i % C];   // best_centers += X_mean
    *inertia_out = inertia[(size_t)best];
    *n_iter_out = (int32_t)st[(size_t)best * ST_WORDS + ST_ITER];
    *strict_out = (int32_t)st[(size_t)best * ST_WORDS + ST_STRICT];
    std::vector<char> seen((size_t)K, 0);
    int32_t distinct = 0;
    for (int64_t i = 0; i < n; ++i)
        if (!seen[(size_t)labels_out[i]]) { seen[(size_t)labels_out[i]] = 1; ++distinct; }
    *distinct_out = distinct;
    return SC_OK;
}

}  // namespace

int sc_kmeans_run_labels(sc_ctx *c, const void *X, int dtype, int64_t n, int32_t C, int32_t K, int32_t n_init,
                         int32_t max_iter, double tol, const void *x_mean, const double *uniforms, int32_t *labels_dev)
{
    if (dtype == SC_F32)
        return kmeans_fit<float>(c, (const float *)X, n, C, K, n_init, max_iter, tol, (const float *)x_mean, uniforms,
                                 nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, labels_dev);
    return kmeans_fit<double>(c, (const double *)X, n, C, K, n_init, max_iter, tol, (const double *)x_mean, uniforms,
                              nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, labels_dev);
}

extern "C" int sc_kmeans_fit(sc_ctx *c, const void *X, int dtype, int64_t n, int32_t C, int32_t K, int32_t n_init,
                             int32_t max_iter, double tol, const void *x_mean, const double *uniforms,
                             int32_t *labels_out, void *centers_out, double *inertia_out, int64_t *seeds_out,
                             int32_t *n_iter_out, int32_t *strict_out, int32_t *distinct_out)
{
    SC_REQUIRE(c && X && x_mean && uniforms && labels_out && centers_out && inertia_out && seeds_out && n_iter_out &&
                   strict_out && distinct_out,
               SC_ERR_INVALID, "sc_kmeans_fit: null pointer");
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "sc_kmeans_fit: dtype must be SC_F32 or SC_F64");
    SC_REQUIRE(C >= 1, SC_ERR_INVALID, "sc_kmeans_fit: C must be >= 1, got %d", C);
    SC_REQUIRE(K >= 2 && (int64_t)K <= n, SC_ERR_INVALID, "sc_kmeans_fit: need 2 <= K <= n (K = %d, n = %lld)", K,
               (long long)n);
    SC_REQUIRE(n <= INT32_MAX, SC_ERR_INVALID, "sc_kmeans_fit: n = %lld exceeds 2^31 - 1", (long long)n);
    SC_REQUIRE(n_init >= 1 && max_iter >= 1, SC_ERR_INVALID, "sc_kmeans_fit: n_init and max_iter must be >= 1");
    SC_REQUIRE(std::isfinite(tol) && tol >= 0.0, SC_ERR_INVALID, "sc_kmeans_fit: tol must be finite and >= 0");
    SC_HIP(hipSetDevice(c->device));
    if (dtype == SC_F32)
        return kmeans_fit<float>(c, (const float *)X, n, C, K, n_init, max_iter, tol, (const float *)x_mean, uniforms,
                                 labels_out, (float *)centers_out, inertia_out, seeds_out, n_iter_out, strict_out,
                                 distinct_out);
    return kmeans_fit<double>(c, (const double *)X, n, C, K, n_init, max_iter, tol, (const double *)x_mean, uniforms,
                              labels_out, (double *)centers_out, inertia_out, seeds_out, n_iter_out, strict_out,
                              distinct_out);
}
