// sc_threshold.hip -- classify_by_threshold (CL:419-894, TH:27-344): metagene scores, the KS cutoff and the
// one-dimensional Gaussian mixture of sklearn 1.7.2.
//
// One summation order for every floating-point sum of this file ("block order", restated by
// tests/threshold_restated.py): workgroup b owns the TH_BLK = 2048 consecutive points from 2048 b; its thread t adds
// the points 2048 b + 256 j + t, j = 0 .. 7, in that order; the 256 thread values are added as the fixed tree
// value[t] += value[t + h], h = 128, 64, .. 1; a second launch adds the workgroups in index order.  No floating-point
// atomics anywhere (integer counts use integer atomics: order-free), so every result is a function of the arguments.
//
// GMM: all n_init runs advance together.  One launch per EM iteration reads each score once and serves every run that
// is still active: log-responsibilities under the run's current parameters, the lower-bound sum and the next M-step's
// sums; one small launch forms the new parameters and applies sklearn's stopping rule per run.  fp64 throughout.
// The variance is ONE pass around the current mean c: sum r (x - m)^2 = B - 2 (m - c) A + (m - c)^2 S0 with
// A = sum r (x - c), B = sum r (x - c)^2 -- sklearn takes a second pass around the new mean m.  The initialisation
// (one-hot responsibilities of the k-means labels) does take the second pass: there c = m and the formula is B alone.
#include <cfloat>
#include <cmath>
#include <vector>

#include "sc_sortscan.h"

namespace {

typedef unsigned long long u64;

constexpr int TH_TPB = 256;               // threads of a workgroup
constexpr int TH_PT = 8;                  // points per thread
constexpr int TH_BLK = TH_TPB * TH_PT;    // points per workgroup
constexpr int TH_FMAX = 64;               // features of a metagene
constexpr int GMM_KMAX = 8;               // components
constexpr int GMM_NV = 1 + 4 * GMM_KMAX;  // partial values per (run, workgroup): L | per component S0, S1, A, B
constexpr double LOG_2PI = 1.8378770664093453;   // numpy's log(2 pi)

// the fixed tree over the 256 thread values of N quantities at once; the sums are valid in thread 0
template <int N>
__device__ __forceinline__ void th_tree(double (&v)[N], double (*s)[TH_TPB])
{
    const int t = threadIdx.x;
    __syncthreads();   // the previous use of s is over
#pragma unroll
    for (int q = 0; q < N; ++q) s[q][t] = v[q];
    __syncthreads();
    if (t < 128) {
#pragma unroll
        for (int q = 0; q < N; ++q) s[q][t] = s[q][t] + s[q][t + 128];
    }
    __syncthreads();
    if (t < 64) {
#pragma unroll
        for (int q = 0; q < N; ++q) {
            double a = s[q][t] + s[q][t + 64];
            // lanes t < h hold the tree's values; what the other lanes compute is never read
            for (int h = 32; h >= 1; h >>= 1) a = a + __shfl_down(a, h, 64);
            v[q] = a;
        }
    }
}

// out[v] = partials [b][v] of NB workgroups added in workgroup order.  One thread per value.
__global__ __launch_bounds__(64) void k_th_final(const double *__restrict__ part, int64_t NB, int nv, double *__restrict__ out)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    double s = 0.0;
    for (int64_t b = 0; b < NB; ++b) s = s + part[b * nv + v];
    out[v] = s;
}

// ---- T1: metagene ------------------------------------------------------------------------------------------------
// numpy's pairwise sum of a contiguous row of f < 128 terms; get(i) is term i
template <class A, class G>
__device__ __forceinline__ A np_row_sum(int f, G get)
{
    if (f < 8) {
        A res = (A)0;
        for (int i = 0; i < f; ++i) res = res + get(i);
        return res;
    }
    A r0 = get(0), r1 = get(1), r2 = get(2), r3 = get(3), r4 = get(4), r5 = get(5), r6 = get(6), r7 = get(7);
    int i = 8;
    for (; i < f - (f % 8); i += 8) {
        r0 = r0 + get(i + 0); r1 = r1 + get(i + 1); r2 = r2 + get(i + 2); r3 = r3 + get(i + 3);
        r4 = r4 + get(i + 4); r5 = r5 + get(i + 5); r6 = r6 + get(i + 6); r7 = r7 + get(i + 7);
    }
    A res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < f; ++i) res = res + get(i);
    return res;
}

// element of rank `want` of the row (ties by index): O(f^2) comparisons, no local array
template <class T>
__device__ __forceinline__ T row_select(const T *__restrict__ x, int f, int want)
{
    for (int i = 0; i < f; ++i) {
        int rank = 0;
        for (int j = 0; j < f; ++j) rank += (x[j] < x[i]) || (x[j] == x[i] && j < i);
        if (rank == want) return x[i];
    }
    return x[0];
}

enum { MG_SHIFTED = 0, MG_GEOMETRIC, MG_ARITHMETIC, MG_MEDIAN, MG_MINIMUM };

// part[b][3] = sum | min | max of the workgroup's valid scores; counts[3] += valid | below 1e-6 | rows with a negative
template <class T>
__global__ __launch_bounds__(256) void k_metagene(const T *__restrict__ X, int64_t n, int f, int method, double pseudo,
                                                  uint8_t *__restrict__ valid, T *__restrict__ score,
                                                  double *__restrict__ part, u64 *__restrict__ counts)
{
    __shared__ double s[3][TH_TPB];
    __shared__ u64 scnt[3];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x;
    if (t < 3) scnt[t] = 0;
    __syncthreads();
    double v[3] = {0.0, INFINITY, -INFINITY};
    unsigned c_valid = 0, c_below = 0, c_neg = 0;
    const T zero_thr = (T)1e-6;
    for (int j = 0; j < TH_PT; ++j) {
        const int64_t i = b * TH_BLK + (int64_t)j * TH_TPB + t;
        if (i >= n) break;
        const T *x = X + i * f;
        bool ok = true, neg = false;
        for (int k = 0; k < f; ++k) {
            ok = ok && isfinite((double)x[k]);
            neg = neg || x[k] < (T)0;
        }
        T sc = (T)NAN;
        if (ok) {
            if (method == MG_SHIFTED) {
                const double m = np_row_sum<double>(f, [&](int k) { return log((double)x[k] + pseudo); }) / (double)f;
                sc = (T)(exp(m) - pseudo);
            } else if (method == MG_GEOMETRIC) {
                const double m = np_row_sum<double>(f, [&](int k) { return log((double)x[k] + 1e-10); }) / (double)f;
                sc = (T)exp(m);
            } else if (method == MG_ARITHMETIC) {
                sc = (T)((double)np_row_sum<T>(f, [&](int k) { return x[k]; }) / (double)f);
            } else if (method == MG_MEDIAN) {
                if (f & 1) sc = row_select(x, f, f / 2);
                else sc = (row_select(x, f, f / 2 - 1) + row_select(x, f, f / 2)) / (T)2;
            } else {
                sc = x[0];
                for (int k = 1; k < f; ++k) sc = x[k] < sc ? x[k] : sc;
            }
            ++c_valid;
            c_below += sc < zero_thr;
            c_neg += neg;
            const double d = (double)sc;
            v[0] = v[0] + d;
            v[1] = d < v[1] ? d : v[1];
            v[2] = d > v[2] ? d : v[2];
        }
        valid[i] = ok ? 1 : 0;
        score[i] = sc;
    }
    // sum: the fixed tree; min / max: order-free, reduced by thread 0
    double sum1[1] = {v[0]};
    th_tree<1>(sum1, s);
    __syncthreads();
    s[1][t] = v[1];
    s[2][t] = v[2];
    if (c_valid) atomicAdd(&scnt[0], (u64)c_valid);
    if (c_below) atomicAdd(&scnt[1], (u64)c_below);
    if (c_neg) atomicAdd(&scnt[2], (u64)c_neg);
    __syncthreads();
    if (t == 0) {
        double mn = INFINITY, mx = -INFINITY;
        for (int k = 0; k < TH_TPB; ++k) {
            mn = s[1][k] < mn ? s[1][k] : mn;
            mx = s[2][k] > mx ? s[2][k] : mx;
        }
        part[b * 3 + 0] = sum1[0];
        part[b * 3 + 1] = mn;
        part[b * 3 + 2] = mx;
        for (int k = 0; k < 3; ++k)
            if (scnt[k]) atomicAdd(&counts[k], scnt[k]);
    }
}

// stats[3] = sum in workgroup order | min | max
__global__ void k_metagene_final(const double *__restrict__ part, int64_t NB, double *__restrict__ stats)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int64_t b = 0; b < NB; ++b) {
        s = s + part[b * 3];
        mn = part[b * 3 + 1] < mn ? part[b * 3 + 1] : mn;
        mx = part[b * 3 + 2] > mx ? part[b * 3 + 2] : mx;
    }
    stats[0] = s;
    stats[1] = mn;
    stats[2] = mx;
}

// ---- T2: KS --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 ordered_bits(double d)
{
    const u64 u = (u64)__double_as_longlong(d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double from_ordered_bits(u64 k)
{
    const u64 u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)u);
}

template <class T>
__global__ __launch_bounds__(256) void k_ks_keys(const T *__restrict__ x, int64_t n, u64 *__restrict__ keys, uint32_t *__restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    keys[i] = ordered_bits((double)x[i]);
    idx[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void k_ks_unkey(const u64 *__restrict__ keys, int64_t n, double *__restrict__ sorted)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sorted[i] = from_ordered_bits(keys[i]);
}

// part[b] = sum over the workgroup's points i < m of x_i (sq = 0) or (x_i - centre)^2 (sq = 1), block order
__global__ __launch_bounds__(256) void k_th_sum(const double *__restrict__ x, int64_t m, int sq, double centre,
                                                double *__restrict__ part)
{
    __shared__ double s[1][TH_TPB];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x;
    double v[1] = {0.0};
    for (int j = 0; j < TH_PT; ++j) {
        const int64_t i = b * TH_BLK + (int64_t)j * TH_TPB + t;
        if (i >= m) break;
        const double d = sq ? x[i] - centre : x[i];
        v[0] = v[0] + (sq ? d * d : d);
    }
    th_tree<1>(v, s);
    if (t == 0) part[b] = v[0];
}

__global__ __launch_bounds__(64) void k_gather(const double *__restrict__ sorted, const int64_t *__restrict__ ranks, int nr,
                                               double *__restrict__ out)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nr) out[k] = sorted[ranks[k]];
}

// scipy's ndtr
__device__ __forceinline__ double th_ndtr(double a)
{
    const double x = a * 0.70710678118654752440;
    const double z = fabs(x);
    if (z < 1.0) return 0.5 + 0.5 * erf(x);
    const double y = 0.5 * erfc(z);
    return x > 0.0 ? 1.0 - y : y;
}

// best (D, index) of the workgroup: the larger D, the lower index among equal D
__global__ __launch_bounds__(256) void k_ks_argmax(const double *__restrict__ sorted, int64_t n, double mean, double sd,
                                                   double *__restrict__ bval, int64_t *__restrict__ bidx)
{
    __shared__ double sv[TH_TPB];
    __shared__ int64_t si[TH_TPB];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x;
    double best = -INFINITY;
    int64_t bi = INT64_MAX;
    for (int j = 0; j < TH_PT; ++j) {
        const int64_t i = b * TH_BLK + (int64_t)j * TH_TPB + t;
        if (i >= n) break;
        const double D = (double)(i + 1) / (double)n - th_ndtr((sorted[i] - mean) / sd);
        if (D > best || (D == best && i < bi)) { best = D; bi = i; }
    }
    sv[t] = best;
    si[t] = bi;
    __syncthreads();
    for (int h = TH_TPB / 2; h >= 1; h >>= 1) {
        if (t < h && (sv[t + h] > sv[t] || (sv[t + h] == sv[t] && si[t + h] < si[t]))) {
            sv[t] = sv[t + h];
            si[t] = si[t + h];
        }
        __syncthreads();
    }
    if (t == 0) { bval[b] = sv[0]; bidx[b] = si[0]; }
}

// out[0] = D, out[1] = score, iout[0] = index of the first largest D over the workgroups' bests
__global__ void k_ks_argmax_final(const double *__restrict__ bval, const int64_t *__restrict__ bidx, int64_t NB,
                                  const double *__restrict__ sorted, double *__restrict__ out, int64_t *__restrict__ iout)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double best = -INFINITY;
    int64_t bi = INT64_MAX;
    for (int64_t b = 0; b < NB; ++b)
        if (bidx[b] != INT64_MAX && (bval[b] > best || (bval[b] == best && bidx[b] < bi))) { best = bval[b]; bi = bidx[b]; }
    if (bi == INT64_MAX) bi = 0;   // every D is NaN: numpy's argmax answers with the first NaN, which is index 0 here
    out[0] = best;
    out[1] = sorted[bi];
    iout[0] = bi;
}

template <class T>
__global__ __launch_bounds__(256) void k_ks_classify(const T *__restrict__ x, int64_t n, double thr, double range,
                                                     double *__restrict__ dev, int32_t *__restrict__ lab, u64 *__restrict__ n_high)
{
    __shared__ unsigned cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const double s = (double)x[i];
        double d = (s - thr) / range;
        d = d < 0.0 ? 0.0 : (d > 1.0 ? 1.0 : d);
        dev[i] = d;
        const int l = s >= thr;
        lab[i] = l;
        if (l) atomicAdd(&cnt, 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0 && cnt) atomicAdd(n_high, (u64)cnt);
}

// ---- T3 / T4: Gaussian mixture ---------------------------------------------------------------------------------------
struct GmmRun {
    double w[GMM_KMAX], mu[GMM_KMAX], var[GMM_KMAX];      // weights_, means_, covariances_
    double p[GMM_KMAX], lp[GMM_KMAX], lw[GMM_KMAX];       // precisions_cholesky_, its log (log_det), log(weights_)
    double nk[GMM_KMAX];                                   // of the initialisation's first pass
    double lb;                                             // lower bound of the last iteration (-inf before the first)
    int32_t active, n_iter, converged, pad;
};

enum { GP_W = 0, GP_MU, GP_P, GP_LP, GP_LW, GP_ROWS };

// weighted log-probability of component k (rows of sp) and the log-sum-exp over the K components
__device__ __forceinline__ double gmm_wlp(double x, const double (*sp)[GMM_KMAX], int k)
{
    const double y = x * sp[GP_P][k] - sp[GP_MU][k] * sp[GP_P][k];
    return (-0.5 * (LOG_2PI + y * y) + sp[GP_LP][k]) + sp[GP_LW][k];
}
__device__ __forceinline__ double gmm_lse(double x, const double (*sp)[GMM_KMAX], int K)
{
    double m = -INFINITY;
    for (int k = 0; k < K; ++k) {
        const double a = gmm_wlp(x, sp, k);
        m = a > m ? a : m;
    }
    double s = 0.0;
    for (int k = 0; k < K; ++k) s = s + exp(gmm_wlp(x, sp, k) - m);
    return log(s) + m;
}

// One pass over the scores for every active run (grid NB, 256 threads).  INIT: responsibilities are the one-hot
// k-means labels of the run, the shift c is shift0 (first pass) or the run's mean (second pass).  Otherwise: the
// E-step under the run's parameters; c is the run's current mean.  part[r][b][GMM_NV] = L | per k: S0, S1, A, B.
template <class T, bool INIT>
__global__ __launch_bounds__(256) void k_gmm_pass(const T *__restrict__ X, int64_t n, int K, int R,
                                                  const GmmRun *__restrict__ runs, const int32_t *__restrict__ labels,
                                                  int use_mean_shift, double shift0, double *__restrict__ part)
{
    __shared__ double s[4][TH_TPB];
    __shared__ double sp[GP_ROWS][GMM_KMAX];
    const int t = threadIdx.x;
    const int64_t b = blockIdx.x, NB = gridDim.x;
    double x[TH_PT];
#pragma unroll
    for (int j = 0; j < TH_PT; ++j) {
        const int64_t i = b * TH_BLK + (int64_t)j * TH_TPB + t;
        x[j] = i < n ? (double)X[i] : 0.0;
    }
    for (int r = 0; r < R; ++r) {
        if (!runs[r].active) continue;   // uniform over the workgroup
        __syncthreads();
        if (t < K) {
            sp[GP_W][t] = runs[r].w[t];
            sp[GP_MU][t] = runs[r].mu[t];
            sp[GP_P][t] = runs[r].p[t];
            sp[GP_LP][t] = runs[r].lp[t];
            sp[GP_LW][t] = runs[r].lw[t];
        }
        __syncthreads();
        double *out = part + ((int64_t)r * NB + b) * GMM_NV;
        double lse[TH_PT];
        int lab[TH_PT];
        double L[1] = {0.0};
#pragma unroll
        for (int j = 0; j < TH_PT; ++j) {
            const int64_t i = b * TH_BLK + (int64_t)j * TH_TPB + t;
            lse[j] = 0.0;
            lab[j] = -1;
            if (i < n) {
                if (INIT) lab[j] = labels[(int64_t)r * n + i];
                else {
                    lse[j] = gmm_lse(x[j], sp, K);
                    L[0] = L[0] + lse[j];
                }
            }
        }
        if (!INIT) {
            th_tree<1>(L, s);
            if (t == 0) out[0] = L[0];
        }
        for (int k = 0; k < K; ++k) {
            const double c = (INIT && !use_mean_shift) ? shift0 : sp[GP_MU][k];
            double v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < TH_PT; ++j) {
                const int64_t i = b * TH_BLK + (int64_t)j * TH_TPB + t;
                if (i < n) {
                    const double rr = INIT ? (lab[j] == k ? 1.0 : 0.0) : exp(gmm_wlp(x[j], sp, k) - lse[j]);
                    const double d = x[j] - c;
                    v[0] = v[0] + rr;
                    v[1] = v[1] + rr * x[j];
                    v[2] = v[2] + rr * d;
                    v[3] = v[3] + rr * (d * d);
                }
            }
            th_tree<4>(v, s);
            if (t == 0) {
                out[1 + 4 * k + 0] = v[0];
                out[1 + 4 * k + 1] = v[1];
                out[1 + 4 * k + 2] = v[2];
                out[1 + 4 * k + 3] = v[3];
            }
        }
    }
}

// Per run (grid R, 64 threads): the workgroups' partials in workgroup order, then
//  mode 0 (initialisation, first pass): nk = S0 + 10 eps, mean = S1 / nk;
//  mode 1 (initialisation, second pass around that mean): variance = B / nk + reg, weights = nk / n;
//  mode 2 (an EM iteration): the M-step of the file header, weights = nk / sum nk, and sklearn's stopping rule.
__global__ __launch_bounds__(64) void k_gmm_stage2(const double *__restrict__ part, int64_t NB, int K, int64_t n, int mode,
                                                   double reg, double tol, int max_iter, GmmRun *__restrict__ runs)
{
    __shared__ double sums[GMM_NV];
    const int r = blockIdx.x, t = threadIdx.x;
    GmmRun *g = runs + r;
    if (!g->active) return;
    const int nv = 1 + 4 * K;
    if (t < nv) {
        double s = 0.0;
        for (int64_t b = 0; b < NB; ++b) s = s + part[((int64_t)r * NB + b) * GMM_NV + t];
        sums[t] = s;
    }
    __syncthreads();
    if (t != 0) return;
    const double eps10 = 10.0 * DBL_EPSILON;
    if (mode == 0) {
        for (int k = 0; k < K; ++k) {
            g->nk[k] = sums[1 + 4 * k] + eps10;
            g->mu[k] = sums[1 + 4 * k + 1] / g->nk[k];
        }
        return;
    }
    double nk[GMM_KMAX], tot = 0.0;
    for (int k = 0; k < K; ++k) {
        const double S0 = sums[1 + 4 * k], S1 = sums[1 + 4 * k + 1], A = sums[1 + 4 * k + 2], B = sums[1 + 4 * k + 3];
        if (mode == 1) {
            nk[k] = g->nk[k];
            g->var[k] = B / nk[k] + reg;
        } else {
            nk[k] = S0 + eps10;
            const double m = S1 / nk[k];
            const double d = m - g->mu[k];
            g->var[k] = ((B - (2.0 * d) * A) + (d * d) * S0) / nk[k] + reg;
            g->mu[k] = m;
        }
        tot = tot + nk[k];
    }
    for (int k = 0; k < K; ++k) {
        g->w[k] = mode == 1 ? nk[k] / (double)n : nk[k] / tot;
        g->p[k] = 1.0 / sqrt(g->var[k]);
        g->lp[k] = log(g->p[k]);
        g->lw[k] = log(g->w[k]);
    }
    if (mode == 2) {
        const double lb = sums[0] / (double)n;
        const double change = lb - g->lb;
        g->lb = lb;
        g->n_iter += 1;
        if (fabs(change) < tol) {
            g->converged = 1;
            g->active = 0;
        } else if (g->n_iter >= max_iter) {
            g->active = 0;
        }
    }
}

// par[GP_ROWS][GMM_KMAX] as k_gmm_pass's sp; prob = the responsibilities of the components high[0 .. nh) added in order
template <class T>
__global__ __launch_bounds__(256) void k_gmm_posterior(const T *__restrict__ X, int64_t n, int K, const double *__restrict__ par,
                                                       const int32_t *__restrict__ high, int nh, double cutoff,
                                                       double *__restrict__ prob, int32_t *__restrict__ lab,
                                                       u64 *__restrict__ n_high)
{
    __shared__ double sp[GP_ROWS][GMM_KMAX];
    __shared__ int sh[GMM_KMAX];
    __shared__ unsigned cnt;
    const int t = threadIdx.x;
    if (t < GP_ROWS * GMM_KMAX) sp[t / GMM_KMAX][t % GMM_KMAX] = par[t];
    if (t < nh) sh[t] = high[t];
    if (t == 0) cnt = 0;
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + t;
    if (i < n) {
        const double x = (double)X[i];
        const double lse = gmm_lse(x, sp, K);
        double pr = 0.0;
        for (int h = 0; h < nh; ++h) pr = pr + exp(gmm_wlp(x, sp, sh[h]) - lse);
        prob[i] = pr;
        const int l = pr > cutoff;
        lab[i] = l;
        if (l) atomicAdd(&cnt, 1u);
    }
    __syncthreads();
    if (t == 0 && cnt) atomicAdd(n_high, (u64)cnt);
}

inline size_t esize(int dtype) { return dtype == SC_F32 ? sizeof(float) : sizeof(double); }

int gmm_pass(sc_ctx *c, int dtype, bool init, const void *X, int64_t n, int K, int R, const GmmRun *runs,
             const int32_t *labels, int use_mean_shift, double shift0, double *part)
{
    const dim3 grid((unsigned)ceil_div64(n, TH_BLK)), block(TH_TPB);
    if (dtype == SC_F32) {
        if (init) hipLaunchKernelGGL((k_gmm_pass<float, true>), grid, block, 0, c->stream, (const float *)X, n, K, R, runs, labels, use_mean_shift, shift0, part);
        else hipLaunchKernelGGL((k_gmm_pass<float, false>), grid, block, 0, c->stream, (const float *)X, n, K, R, runs, labels, use_mean_shift, shift0, part);
    } else {
        if (init) hipLaunchKernelGGL((k_gmm_pass<double, true>), grid, block, 0, c->stream, (const double *)X, n, K, R, runs, labels, use_mean_shift, shift0, part);
        else hipLaunchKernelGGL((k_gmm_pass<double, false>), grid, block, 0, c->stream, (const double *)X, n, K, R, runs, labels, use_mean_shift, shift0, part);
    }
    SC_HIP(hipGetLastError());
    return SC_OK;
}

}  // namespace

extern "C" int sc_metagene_score(sc_ctx *c, const void *features, int dtype, int64_t n, int32_t n_features, int32_t method,
                                 double pseudocount, uint8_t *valid_out, void *score_out, double *stats_out,
                                 int64_t *counts_out)
{
    SC_REQUIRE(c && features && valid_out && score_out && stats_out && counts_out, SC_ERR_INVALID,
               "sc_metagene_score: null pointer");
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "sc_metagene_score: dtype must be SC_F32 or SC_F64");
    SC_REQUIRE(n >= 1 && n <= INT32_MAX, SC_ERR_INVALID, "sc_metagene_score: need 1 <= n <= 2^31 - 1, got %lld", (long long)n);
    SC_REQUIRE(n_features >= 1 && n_features <= TH_FMAX, SC_ERR_INVALID,
               "sc_metagene_score: need 1 <= n_features <= %d, got %d", TH_FMAX, n_features);
    SC_REQUIRE(method >= MG_SHIFTED && method <= MG_MINIMUM, SC_ERR_INVALID, "sc_metagene_score: unknown method %d", method);
    SC_REQUIRE(std::isfinite(pseudocount), SC_ERR_INVALID, "sc_metagene_score: pseudocount must be finite");
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t es = esize(dtype);
    const int64_t NB = ceil_div64(n, TH_BLK);
    DBuf m[6];
    enum { X, VALID, SCORE, PART, STATS, COUNTS };
    SC_TRY(m[X].ensure(es * (size_t)(n * n_features), &c->mem));
    SC_TRY(m[VALID].ensure((size_t)n, &c->mem));
    SC_TRY(m[SCORE].ensure(es * (size_t)n, &c->mem));
    SC_TRY(m[PART].ensure(sizeof(double) * 3 * (size_t)NB, &c->mem));
    SC_TRY(m[STATS].ensure(sizeof(double) * 3, &c->mem));
    SC_TRY(m[COUNTS].ensure(sizeof(u64) * 3, &c->mem));
    SC_HIP(hipMemcpyAsync(m[X].p, features, es * (size_t)(n * n_features), hipMemcpyHostToDevice, s));
    SC_HIP(hipMemsetAsync(m[COUNTS].p, 0, sizeof(u64) * 3, s));
    {
        KernelTimerScope ts(c, SC_K_THRESH_SCORE);
        if (dtype == SC_F32)
            hipLaunchKernelGGL(k_metagene<float>, dim3((unsigned)NB), dim3(TH_TPB), 0, s, m[X].as<float>(), n, (int)n_features,
                               (int)method, pseudocount, m[VALID].as<uint8_t>(), m[SCORE].as<float>(),
                               m[PART].as<double>(), m[COUNTS].as<u64>());
        else
            hipLaunchKernelGGL(k_metagene<double>, dim3((unsigned)NB), dim3(TH_TPB), 0, s, m[X].as<double>(), n, (int)n_features,
                               (int)method, pseudocount, m[VALID].as<uint8_t>(), m[SCORE].as<double>(),
                               m[PART].as<double>(), m[COUNTS].as<u64>());
        hipLaunchKernelGGL(k_metagene_final, dim3(1), dim3(64), 0, s, m[PART].as<double>(), NB, m[STATS].as<double>());
    }
    SC_HIP(hipGetLastError());
    double st[3];
    u64 cnt[3];
    SC_HIP(hipMemcpyAsync(valid_out, m[VALID].p, (size_t)n, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(score_out, m[SCORE].p, es * (size_t)n, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(st, m[STATS].p, sizeof(st), hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(cnt, m[COUNTS].p, sizeof(cnt), hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    stats_out[0] = st[1];
    stats_out[1] = st[2];
    stats_out[2] = cnt[0] ? st[0] / (double)cnt[0] : NAN;
    for (int k = 0; k < 3; ++k) counts_out[k] = (int64_t)cnt[k];
    return SC_OK;
}

extern "C" int sc_ks_prepare(sc_ctx *c, const void *scores, int dtype, int64_t n, double background_quantile,
                             const int64_t *ranks, int32_t n_ranks, double *rank_out, double *bg_out, double *sorted_out)
{
    SC_REQUIRE(c && scores && bg_out, SC_ERR_INVALID, "sc_ks_prepare: null pointer");
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "sc_ks_prepare: dtype must be SC_F32 or SC_F64");
    SC_REQUIRE(n >= 10 && n <= INT32_MAX, SC_ERR_INVALID, "sc_ks_prepare: need 10 <= n <= 2^31 - 1, got %lld", (long long)n);
    SC_REQUIRE(background_quantile > 0.0 && background_quantile < 1.0, SC_ERR_INVALID,
               "sc_ks_prepare: background_quantile must be in (0, 1)");
    SC_REQUIRE(n_ranks >= 0 && n_ranks <= 64 && (n_ranks == 0 || (ranks && rank_out)), SC_ERR_INVALID,
               "sc_ks_prepare: at most 64 order statistics, with their arrays");
    for (int k = 0; k < n_ranks; ++k)
        SC_REQUIRE(ranks[k] >= 0 && ranks[k] < n, SC_ERR_INVALID, "sc_ks_prepare: rank %lld outside [0, n)", (long long)ranks[k]);
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t es = esize(dtype);
    int64_t m_bg = (int64_t)((double)n * background_quantile);
    if (m_bg < 10) m_bg = 10;
    if (m_bg > n) m_bg = n;
    const int64_t NB = ceil_div64(m_bg, TH_BLK);
    c->th_n = 0;
    DBuf m[9];
    enum { X, K1, K2, I1, I2, PART, RED, RANKS, RVAL };
    SC_TRY(m[X].ensure(es * (size_t)n, &c->mem));
    SC_TRY(m[K1].ensure(sizeof(u64) * (size_t)n, &c->mem));
    SC_TRY(m[K2].ensure(sizeof(u64) * (size_t)n, &c->mem));
    SC_TRY(m[I1].ensure(sizeof(uint32_t) * (size_t)n, &c->mem));
    SC_TRY(m[I2].ensure(sizeof(uint32_t) * (size_t)n, &c->mem));
    SC_TRY(m[PART].ensure(sizeof(double) * (size_t)NB, &c->mem));
    SC_TRY(m[RED].ensure(sizeof(double) * 2, &c->mem));
    SC_TRY(m[RANKS].ensure(sizeof(int64_t) * 64, &c->mem));
    SC_TRY(m[RVAL].ensure(sizeof(double) * 64, &c->mem));
    SC_TRY(c->th_sorted.ensure(sizeof(double) * (size_t)n, &c->mem));
    SC_HIP(hipMemcpyAsync(m[X].p, scores, es * (size_t)n, hipMemcpyHostToDevice, s));
    const dim3 flat((unsigned)ceil_div64(n, 256)), tpb(256);
    double *sorted = c->th_sorted.as<double>();
    double sum = 0.0, ss = 0.0;
    {
        KernelTimerScope ts(c, SC_K_THRESH_SORT);
        if (dtype == SC_F32) hipLaunchKernelGGL(k_ks_keys<float>, flat, tpb, 0, s, m[X].as<float>(), n, m[K1].as<u64>(), m[I1].as<uint32_t>());
        else hipLaunchKernelGGL(k_ks_keys<double>, flat, tpb, 0, s, m[X].as<double>(), n, m[K1].as<u64>(), m[I1].as<uint32_t>());
        SC_TRY(sc_sort_pairs(c, c->rs_tmp, s, m[K1].as<u64>(), m[K2].as<u64>(), m[I1].as<uint32_t>(), m[I2].as<uint32_t>(), n, 64));
        hipLaunchKernelGGL(k_ks_unkey, flat, tpb, 0, s, m[K2].as<u64>(), n, sorted);
        // background moments: the mean, then the squared deviations around it (two passes, as numpy's std)
        hipLaunchKernelGGL(k_th_sum, dim3((unsigned)NB), tpb, 0, s, sorted, m_bg, 0, 0.0, m[PART].as<double>());
        hipLaunchKernelGGL(k_th_final, dim3(1), dim3(64), 0, s, m[PART].as<double>(), NB, 1, m[RED].as<double>());
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(&sum, m[RED].p, sizeof(double), hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    const double mean = sum / (double)m_bg;
    {
        KernelTimerScope ts(c, SC_K_THRESH_SORT);
        hipLaunchKernelGGL(k_th_sum, dim3((unsigned)NB), tpb, 0, s, sorted, m_bg, 1, mean, m[PART].as<double>());
        hipLaunchKernelGGL(k_th_final, dim3(1), dim3(64), 0, s, m[PART].as<double>(), NB, 1, m[RED].as<double>() + 1);
        if (n_ranks > 0) {
            SC_HIP(hipMemcpyAsync(m[RANKS].p, ranks, sizeof(int64_t) * (size_t)n_ranks, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(k_gather, dim3(1), dim3(64), 0, s, sorted, m[RANKS].as<int64_t>(), (int)n_ranks, m[RVAL].as<double>());
        }
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(&ss, m[RED].as<double>() + 1, sizeof(double), hipMemcpyDeviceToHost, s));
    if (n_ranks > 0) SC_HIP(hipMemcpyAsync(rank_out, m[RVAL].p, sizeof(double) * (size_t)n_ranks, hipMemcpyDeviceToHost, s));
    if (sorted_out) SC_HIP(hipMemcpyAsync(sorted_out, sorted, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    bg_out[0] = mean;
    bg_out[1] = std::sqrt(ss / (double)m_bg);
    c->th_n = n;
    return SC_OK;
}

extern "C" int sc_ks_argmax(sc_ctx *c, double bg_mean, double bg_std, int64_t *index_out, double *score_out, double *d_out)
{
    SC_REQUIRE(c && index_out && score_out && d_out, SC_ERR_INVALID, "sc_ks_argmax: null pointer");
    SC_REQUIRE(c->th_n > 0, SC_ERR_STATE, "sc_ks_argmax: no sorted scores (call sc_ks_prepare first)");
    SC_REQUIRE(std::isfinite(bg_mean) && std::isfinite(bg_std) && bg_std > 0.0, SC_ERR_INVALID,
               "sc_ks_argmax: the background mean must be finite and its standard deviation finite and > 0");
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int64_t n = c->th_n, NB = ceil_div64(n, TH_BLK);
    DBuf m[4];
    enum { BVAL, BIDX, OUT, IOUT };
    SC_TRY(m[BVAL].ensure(sizeof(double) * (size_t)NB, &c->mem));
    SC_TRY(m[BIDX].ensure(sizeof(int64_t) * (size_t)NB, &c->mem));
    SC_TRY(m[OUT].ensure(sizeof(double) * 2, &c->mem));
    SC_TRY(m[IOUT].ensure(sizeof(int64_t), &c->mem));
    {
        KernelTimerScope ts(c, SC_K_THRESH_KS);
        hipLaunchKernelGGL(k_ks_argmax, dim3((unsigned)NB), dim3(TH_TPB), 0, s, c->th_sorted.as<double>(), n, bg_mean, bg_std,
                           m[BVAL].as<double>(), m[BIDX].as<int64_t>());
        hipLaunchKernelGGL(k_ks_argmax_final, dim3(1), dim3(64), 0, s, m[BVAL].as<double>(), m[BIDX].as<int64_t>(), NB,
                           c->th_sorted.as<double>(), m[OUT].as<double>(), m[IOUT].as<int64_t>());
    }
    SC_HIP(hipGetLastError());
    double out[2];
    SC_HIP(hipMemcpyAsync(out, m[OUT].p, sizeof(out), hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(index_out, m[IOUT].p, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    *d_out = out[0];
    *score_out = out[1];
    return SC_OK;
}

extern "C" int sc_ks_classify(sc_ctx *c, const void *scores, int dtype, int64_t n, double threshold, double max_score,
                              double *deviation_out, int32_t *labels_out, int64_t *n_high_out)
{
    SC_REQUIRE(c && scores && deviation_out && labels_out && n_high_out, SC_ERR_INVALID, "sc_ks_classify: null pointer");
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "sc_ks_classify: dtype must be SC_F32 or SC_F64");
    SC_REQUIRE(n >= 1 && n <= INT32_MAX, SC_ERR_INVALID, "sc_ks_classify: need 1 <= n <= 2^31 - 1, got %lld", (long long)n);
    SC_REQUIRE(std::isfinite(threshold) && std::isfinite(max_score), SC_ERR_INVALID,
               "sc_ks_classify: threshold and max_score must be finite");
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t es = esize(dtype);
    double range = max_score - threshold;
    if (range < 1e-10) range = 1e-10;
    DBuf m[4];
    enum { X, DEV, LAB, CNT };
    SC_TRY(m[X].ensure(es * (size_t)n, &c->mem));
    SC_TRY(m[DEV].ensure(sizeof(double) * (size_t)n, &c->mem));
    SC_TRY(m[LAB].ensure(sizeof(int32_t) * (size_t)n, &c->mem));
    SC_TRY(m[CNT].ensure(sizeof(u64), &c->mem));
    SC_HIP(hipMemcpyAsync(m[X].p, scores, es * (size_t)n, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemsetAsync(m[CNT].p, 0, sizeof(u64), s));
    const dim3 flat((unsigned)ceil_div64(n, 256)), tpb(256);
    {
        KernelTimerScope ts(c, SC_K_THRESH_KS);
        if (dtype == SC_F32)
            hipLaunchKernelGGL(k_ks_classify<float>, flat, tpb, 0, s, m[X].as<float>(), n, threshold, range, m[DEV].as<double>(),
                               m[LAB].as<int32_t>(), m[CNT].as<u64>());
        else
            hipLaunchKernelGGL(k_ks_classify<double>, flat, tpb, 0, s, m[X].as<double>(), n, threshold, range, m[DEV].as<double>(),
                               m[LAB].as<int32_t>(), m[CNT].as<u64>());
    }
    SC_HIP(hipGetLastError());
    u64 cnt = 0;
    SC_HIP(hipMemcpyAsync(deviation_out, m[DEV].p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(labels_out, m[LAB].p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(&cnt, m[CNT].p, sizeof(u64), hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    *n_high_out = (int64_t)cnt;
    return SC_OK;
}

extern "C" int sc_gmm_fit(sc_ctx *c, const void *scores, int dtype, int64_t n, int32_t K, int32_t n_init, int32_t km_max_iter,
                          double km_tol, const void *x_mean, const double *uniforms, int32_t max_iter, double tol,
                          double reg_covar, int32_t *km_labels_out, double *weights_out, double *means_out,
                          double *variances_out, double *lower_bound_out, int32_t *n_iter_out, int32_t *converged_out,
                          int32_t *best_out)
{
    SC_REQUIRE(c && scores && x_mean && uniforms && weights_out && means_out && variances_out && lower_bound_out &&
                   n_iter_out && converged_out && best_out,
               SC_ERR_INVALID, "sc_gmm_fit: null pointer");
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "sc_gmm_fit: dtype must be SC_F32 or SC_F64");
    SC_REQUIRE(K >= 2 && K <= GMM_KMAX && (int64_t)K <= n, SC_ERR_INVALID,
               "sc_gmm_fit: need 2 <= K <= min(%d, n) (K = %d, n = %lld)", GMM_KMAX, K, (long long)n);
    SC_REQUIRE(n <= INT32_MAX, SC_ERR_INVALID, "sc_gmm_fit: n = %lld exceeds 2^31 - 1", (long long)n);
    SC_REQUIRE(n_init >= 1 && n_init <= 1024 && km_max_iter >= 1 && max_iter >= 1, SC_ERR_INVALID,
               "sc_gmm_fit: need 1 <= n_init <= 1024, km_max_iter >= 1 and max_iter >= 1");
    SC_REQUIRE(std::isfinite(km_tol) && km_tol >= 0.0 && std::isfinite(tol) && tol >= 0.0 && std::isfinite(reg_covar) &&
                   reg_covar >= 0.0,
               SC_ERR_INVALID, "sc_gmm_fit: km_tol, tol and reg_covar must be finite and >= 0");
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t es = esize(dtype);
    const int R = n_init;
    const int64_t NB = ceil_div64(n, TH_BLK);
    DBuf m[4];
    enum { X, LAB, PART, RUNS };
    SC_TRY(m[X].ensure(es * (size_t)n, &c->mem));
    SC_TRY(m[LAB].ensure(sizeof(int32_t) * (size_t)R * (size_t)n, &c->mem));
    SC_TRY(m[PART].ensure(sizeof(double) * (size_t)R * (size_t)NB * GMM_NV, &c->mem));
    SC_TRY(m[RUNS].ensure(sizeof(GmmRun) * (size_t)R, &c->mem));

    // ---- every run's k-means labels (sc_kmeans.hip) --------------------------------------------------------------
    SC_TRY(sc_kmeans_run_labels(c, scores, dtype, n, 1, K, R, km_max_iter, km_tol, x_mean, uniforms, m[LAB].as<int32_t>()));
    if (km_labels_out)
        SC_HIP(hipMemcpyAsync(km_labels_out, m[LAB].p, sizeof(int32_t) * (size_t)R * (size_t)n, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(m[X].p, scores, es * (size_t)n, hipMemcpyHostToDevice, s));

    // ---- initialisation: means, then variances around them ---------------------------------------------------------
    std::vector<GmmRun> runs((size_t)R);
    for (GmmRun &g : runs) {
        g = GmmRun();
        g.lb = -INFINITY;
        g.active = 1;
    }
    SC_HIP(hipMemcpyAsync(m[RUNS].p, runs.data(), sizeof(GmmRun) * (size_t)R, hipMemcpyHostToDevice, s));
    const double shift0 = dtype == SC_F32 ? (double)*(const float *)x_mean : *(const double *)x_mean;
    GmmRun *druns = m[RUNS].as<GmmRun>();
    double *part = m[PART].as<double>();
    auto stage2 = [&](int mode) {
        hipLaunchKernelGGL(k_gmm_stage2, dim3((unsigned)R), dim3(64), 0, s, part, NB, (int)K, n, mode, reg_covar, tol, (int)max_iter, druns);
    };
    {
        KernelTimerScope ts(c, SC_K_GMM_EM);
        SC_TRY(gmm_pass(c, dtype, true, m[X].p, n, K, R, druns, m[LAB].as<int32_t>(), 0, shift0, part));
        stage2(0);
        SC_TRY(gmm_pass(c, dtype, true, m[X].p, n, K, R, druns, m[LAB].as<int32_t>(), 1, shift0, part));
        stage2(1);
    }
    SC_HIP(hipGetLastError());

    // ---- EM, all active runs per launch; one small read-back per iteration --------------------------------------------
    for (int it = 0; it < max_iter; ++it) {
        {
            KernelTimerScope ts(c, SC_K_GMM_EM);
            SC_TRY(gmm_pass(c, dtype, false, m[X].p, n, K, R, druns, nullptr, 1, 0.0, part));
            stage2(2);
        }
        SC_HIP(hipGetLastError());
        SC_HIP(hipMemcpyAsync(runs.data(), druns, sizeof(GmmRun) * (size_t)R, hipMemcpyDeviceToHost, s));
        SC_HIP(hipStreamSynchronize(s));
        bool any = false;
        for (const GmmRun &g : runs) any = any || g.active;
        if (!any) break;
    }
    SC_HIP(hipStreamSynchronize(s));   // km_labels_out

    int best = 0;
    for (int r = 0; r < R; ++r) {
        const GmmRun &g = runs[(size_t)r];
        for (int k = 0; k < K; ++k) {
            weights_out[(size_t)r * K + k] = g.w[k];
            means_out[(size_t)r * K + k] = g.mu[k];
            variances_out[(size_t)r * K + k] = g.var[k];
        }
        lower_bound_out[r] = g.lb;
        n_iter_out[r] = g.n_iter;
        converged_out[r] = g.converged;
        if (g.lb > runs[(size_t)best].lb) best = r;   // strictly larger: the first of equal runs stays
    }
    *best_out = best;
    return SC_OK;
}

extern "C" int sc_gmm_posterior(sc_ctx *c, const void *scores, int dtype, int64_t n, int32_t K, const double *weights,
                                const double *means, const double *variances, const int32_t *high, int32_t n_high,
                                double cutoff, double *prob_out, int32_t *labels_out, int64_t *n_high_cells_out)
{
    SC_REQUIRE(c && scores && weights && means && variances && high && prob_out && labels_out && n_high_cells_out,
               SC_ERR_INVALID, "sc_gmm_posterior: null pointer");
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "sc_gmm_posterior: dtype must be SC_F32 or SC_F64");
    SC_REQUIRE(n >= 1 && n <= INT32_MAX, SC_ERR_INVALID, "sc_gmm_posterior: need 1 <= n <= 2^31 - 1, got %lld", (long long)n);
    SC_REQUIRE(K >= 1 && K <= GMM_KMAX, SC_ERR_INVALID, "sc_gmm_posterior: need 1 <= K <= %d, got %d", GMM_KMAX, K);
    SC_REQUIRE(n_high >= 1 && n_high <= K, SC_ERR_INVALID, "sc_gmm_posterior: need 1 <= n_high <= K, got %d", n_high);
    for (int h = 0; h < n_high; ++h)
        SC_REQUIRE(high[h] >= 0 && high[h] < K, SC_ERR_INVALID, "sc_gmm_posterior: component %d outside [0, K)", high[h]);
    double par[GP_ROWS][GMM_KMAX] = {};
    for (int k = 0; k < K; ++k) {
        SC_REQUIRE(weights[k] > 0.0 && variances[k] > 0.0 && std::isfinite(means[k]) && std::isfinite(weights[k]) &&
                       std::isfinite(variances[k]),
                   SC_ERR_INVALID, "sc_gmm_posterior: component %d needs a finite mean and finite positive weight and variance", k);
        par[GP_W][k] = weights[k];
        par[GP_MU][k] = means[k];
        par[GP_P][k] = 1.0 / std::sqrt(variances[k]);
        par[GP_LP][k] = std::log(par[GP_P][k]);
        par[GP_LW][k] = std::log(weights[k]);
    }
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t es = esize(dtype);
    DBuf m[6];
    enum { X, PAR, HIGH, PROB, LAB, CNT };
    SC_TRY(m[X].ensure(es * (size_t)n, &c->mem));
    SC_TRY(m[PAR].ensure(sizeof(par), &c->mem));
    SC_TRY(m[HIGH].ensure(sizeof(int32_t) * GMM_KMAX, &c->mem));
    SC_TRY(m[PROB].ensure(sizeof(double) * (size_t)n, &c->mem));
    SC_TRY(m[LAB].ensure(sizeof(int32_t) * (size_t)n, &c->mem));
    SC_TRY(m[CNT].ensure(sizeof(u64), &c->mem));
    SC_HIP(hipMemcpyAsync(m[X].p, scores, es * (size_t)n, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(m[PAR].p, par, sizeof(par), hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(m[HIGH].p, high, sizeof(int32_t) * (size_t)n_high, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemsetAsync(m[CNT].p, 0, sizeof(u64), s));
    const dim3 flat((unsigned)ceil_div64(n, 256)), tpb(256);
    {
        KernelTimerScope ts(c, SC_K_GMM_POST);
        if (dtype == SC_F32)
            hipLaunchKernelGGL(k_gmm_posterior<float>, flat, tpb, 0, s, m[X].as<float>(), n, (int)K, m[PAR].as<double>(),
                               m[HIGH].as<int32_t>(), (int)n_high, cutoff, m[PROB].as<double>(), m[LAB].as<int32_t>(),
                               m[CNT].as<u64>());
        else
            hipLaunchKernelGGL(k_gmm_posterior<double>, flat, tpb, 0, s, m[X].as<double>(), n, (int)K, m[PAR].as<double>(),
                               m[HIGH].as<int32_t>(), (int)n_high, cutoff, m[PROB].as<double>(), m[LAB].as<int32_t>(),
                               m[CNT].as<u64>());
    }
    SC_HIP(hipGetLastError());
    u64 cnt = 0;
    SC_HIP(hipMemcpyAsync(prob_out, m[PROB].p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(labels_out, m[LAB].p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(&cnt, m[CNT].p, sizeof(u64), hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    *n_high_cells_out = (int64_t)cnt;
    return SC_OK;
}
