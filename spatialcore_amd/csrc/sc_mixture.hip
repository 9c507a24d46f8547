// sc_mixture.hip -- sc_mixture_fit / sc_mixture_predict: multivariate Gaussian mixtures ("full" and "diag" covariances) by
// EM, sklearn 1.7.2's GaussianMixture(init_params="kmeans") step for step (restated by
// tests/mixture_restated.py).  fp64 throughout, no floating-point atomics; every sum has one fixed order that depends on
// the shape (n, D, K) alone, so a result is a function of the inputs, bit for bit.
//
//  - start: run r takes the labels of sc_kmeans_run_labels (sc_kmeans.hip: KMeans(K, n_init=1) on ONE shared stream of
//    draws), one-hot responsibilities, then the M-step.  K = 1 needs no k-means: every responsibility is 1.
//  - M-step: the cells are cut into slices of S rows, S = mix_slice_rows(n, D, K).  Pass 1 (k_mix_sums): per (slice, k)
//    sum r and sum r x, rows in ascending order; k_mix_means adds the slices in ascending order, nk = sum + 10 * 2^-52,
//    mean = sum / nk, weight = nk / sum_k nk (k ascending).  Pass 2 around the NEW mean: "full" -- k_mix_cov, one workgroup
//    per (64 x 64 block of the upper triangle, slice, k), 32 rows at a time in two LDS panels A = r (x - mu) and B = x - mu,
//    v_mfma_f64_16x16x4_f64 with the k-steps in ascending row order; k_mix_cov_reduce adds the slices in ascending order,
//    divides by nk, adds reg_covar on the diagonal and mirrors.  "diag" -- k_mix_sums again, sum r (x - mu)^2, and k_mix_var_reduce.
//  - precisions (k_mix_prec_full / _diag, one workgroup per component, in global memory): Cholesky cov = L L^T by plain column steps
//    (right-looking), P = L^-T by forward substitution (one thread per row of P, ascending), log det = sum_j log P_jj
//    (j ascending), b = mu^T P (ascending), log w.  A pivot that is not > 0 (or not finite) sets a flag the host reads:
//    SC_ERR_ILLDEFINED.  "diag": P = 1 / sqrt(var).
//  - E-step: "full" -- k_mix_logp_full, 64 rows staged in LDS, wavefront w owns the 16-column tiles w, w + 4, ... of
//    Y = X P_k (P_k upper triangular: only the k-steps up to the tile's last column), four row tiles per B operand;
//    q = sum_j (Y_j - b_j)^2: per lane its tiles ascending, then the 16 lanes of a row by a xor tree (1, 2, 4, 8), then the
//    four wavefronts in order.  "diag" -- k_mix_logp_diag, 16 lanes per row, lane l the columns l, l + 16, ..., the same
//    tree.  log p = (-(D log 2 pi + q) / 2 + log det) + log w.  k_mix_normalize: max, log sum exp (k ascending, compensated),
//    responsibilities exp(log p - max) / sum, the first largest as label, and the 256-row block sums of the log-likelihood, which k_mix_total
//    adds in two levels (256 runs of consecutive blocks, each ascending, then the runs ascending).
//  - loop: sklearn's.  prev = -inf; E, M, lb = mean log-likelihood of that E-step, converged when |lb - prev| < tol.  A
//    later run replaces the best only on a strictly larger lb.  Labels and responsibilities come from one more E-step under
//    the best run's parameters, by the very kernels sc_mixture_predict runs.
#include <cmath>
#include <cstring>
#include <vector>

#include "sc_ctx.h"

namespace {

constexpr int MIX_DMAX = 256;
constexpr int MIX_KMAX = 64;
constexpr int MIX_RMAX = 10;
constexpr int64_t MIX_SLICE_ROWS = 1024;                 // the shortest M-step slice
constexpr int64_t MIX_PARTIAL_BYTES = (int64_t)1 << 28;  // budget of the covariance partials: 256 MiB
constexpr int MIX_BLK = 64;                              // columns per covariance block: 4 x 4 MFMA tiles, 2 x 2 per wavefront
constexpr int MIX_CHUNK = 32;                            // rows staged at a time
constexpr int MIX_LD = MIX_BLK + 16;                     // LDS row stride (doubles) of a covariance panel
constexpr int MIX_EROWS = 64;                            // rows per E-step workgroup
constexpr int MIX_TPB = 256;
constexpr double MIX_LOG_2PI = 1.8378770664093453;       // log(2 pi)

typedef double v4f64 __attribute__((ext_vector_type(4)));

struct MixScalars {   // read back once per iteration
    double loglik_sum;
    int32_t ill;      // 1 + the first component whose covariance is not positive definite
    int32_t pad;
};

int64_t mix_slice_rows(int64_t n, int D, int K, bool full)
{
    const int64_t nb = (D + MIX_BLK - 1) / MIX_BLK, nq = nb * (nb + 1) / 2;
    const int64_t per_slice = full ? (int64_t)K * nq * MIX_BLK * MIX_BLK * 8 : (int64_t)K * D * 8;
    const int64_t smax = std::max<int64_t>(1, std::min<int64_t>(MIX_PARTIAL_BYTES / per_slice, 4096));
    return std::max<int64_t>(MIX_SLICE_ROWS, align_up64(ceil_div64(n, smax), MIX_CHUNK));
}

__global__ __launch_bounds__(256) void k_mix_onehot(const int32_t *__restrict__ lab, int64_t n, int K, double *__restrict__ resp)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n * K) return;
    resp[q] = (!lab || lab[q / K] == (int32_t)(q % K)) ? 1.0 : 0.0;
}

// ---- M-step, pass 1.  grid (slices, K), thread d < D: sum r x_d over the slice's rows in ascending order; pass = 0: x,
// pass 1: (x - mu)^2 ("diag" variances) ----
__global__ __launch_bounds__(256) void k_mix_sums(const double *__restrict__ X, const double *__restrict__ resp, int64_t n, int D, int K,
                                                  int64_t slice_rows, const double *__restrict__ mu, int pass,
                                                  double *__restrict__ psum, double *__restrict__ pnk)
{
    const int d = threadIdx.x, k = blockIdx.y;
    const int64_t s0 = (int64_t)blockIdx.x * slice_rows;
    const int64_t s1 = s0 + slice_rows < n ? s0 + slice_rows : n;
    if (d >= D) return;
    const double m = pass ? mu[k * D + d] : 0.0;
    double acc = 0.0, nk = 0.0;
    for (int64_t i = s0; i < s1; ++i) {
        const double r = resp[i * K + k];
        const double t = X[i * D + d] - m;
        acc = acc + r * (pass ? t * t : t);
        nk = nk + r;
    }
    psum[((int64_t)blockIdx.x * K + k) * D + d] = acc;
    if (!pass && d == 0) pnk[(int64_t)blockIdx.x * K + k] = nk;
}

// one workgroup: nk, means and weights from the slice sums (ascending slices, then ascending k for the total)
__global__ __launch_bounds__(256) void k_mix_means(const double *__restrict__ psum, const double *__restrict__ pnk, int slices, int D, int K,
                                                   double *__restrict__ nk, double *__restrict__ mu, double *__restrict__ w)
{
    __shared__ double snk[MIX_KMAX];
    const int t = threadIdx.x;
    if (t < K) {
        double s = 0.0;
        for (int sl = 0; sl < slices; ++sl) s = s + pnk[(int64_t)sl * K + t];
        s = s + 10.0 * 2.220446049250313e-16;
        snk[t] = s;
        nk[t] = s;
    }
    __syncthreads();
    for (int e = t; e < K * D; e += MIX_TPB) {
        double s = 0.0;
        for (int sl = 0; sl < slices; ++sl) s = s + psum[(int64_t)sl * K * D + e];
        mu[e] = s / snk[e / D];
    }
    if (t < K) {
        double tot = 0.0;
        for (int k = 0; k < K; ++k) tot = tot + snk[k];
        w[t] = snk[t] / tot;
    }
}

// "diag": var = slice sums (ascending) / nk + reg_covar
__global__ __launch_bounds__(256) void k_mix_var_reduce(const double *__restrict__ psum, int slices, int D, int K, const double *__restrict__ nk,
                                                        double reg, double *__restrict__ cov)
{
    const int e = blockIdx.x * MIX_TPB + threadIdx.x;
    if (e >= K * D) return;
    double s = 0.0;
    for (int sl = 0; sl < slices; ++sl) s = s + psum[(int64_t)sl * K * D + e];
    cov[e] = s / nk[e / D] + reg;
}

// ---- M-step, pass 2, "full".  grid (upper blocks, slices, K).  Operand maps of v_mfma_f64_16x16x4_f64 as k_pca_gram:
// A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], D[row = (lane >> 4) + 4 v][col = lane & 15]; here k is a
// staged row, A[i][k] = r (x - mu) at column i of block a, B[k][j] = (x - mu) at column j of block b.  Wavefront w owns the
// 32 x 32 quarter (w >> 1, w & 1); on a diagonal block the quarter below the diagonal is left out ----
__global__ __launch_bounds__(256) void k_mix_cov(const double *__restrict__ X, const double *__restrict__ resp, int64_t n, int D, int K,
                                                 int64_t slice_rows, const double *__restrict__ mu, const int2 *__restrict__ blocks,
                                                 double *__restrict__ partial)
{
    __shared__ double P[2 * MIX_CHUNK * MIX_LD];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int2 blk = blocks[blockIdx.x];
    const int k = blockIdx.z, nq = gridDim.x;
    const int wi = wave >> 1, wj = wave & 1;
    const bool idle = blk.x == blk.y && wi > wj;
    const int ca0 = blk.x * MIX_BLK, cb0 = blk.y * MIX_BLK;
    const int boff = MIX_CHUNK * MIX_LD;
    const int64_t s0 = (int64_t)blockIdx.y * slice_rows;
    const int64_t s1 = s0 + slice_rows < n ? s0 + slice_rows : n;
    const double *m = mu + (int64_t)k * D;
    v4f64 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = v4f64{0.0, 0.0, 0.0, 0.0};
    for (int64_t r0 = s0; r0 < s1; r0 += MIX_CHUNK) {
        for (int q = t; q < MIX_CHUNK * MIX_BLK; q += MIX_TPB) {
            const int lr = q / MIX_BLK, cc = q % MIX_BLK;
            const int64_t row = r0 + lr;
            double a = 0.0, b = 0.0;
            if (row < s1) {
                const double r = resp[row * K + k];
                if (ca0 + cc < D) a = r * (X[row * D + ca0 + cc] - m[ca0 + cc]);
                if (cb0 + cc < D) b = X[row * D + cb0 + cc] - m[cb0 + cc];
            }
            P[lr * MIX_LD + cc] = a;
            P[boff + lr * MIX_LD + cc] = b;
        }
        __syncthreads();
        if (!idle) {
            for (int k0 = 0; k0 < MIX_CHUNK; k0 += 4) {
                const int rowoff = (k0 + (lane >> 4)) * MIX_LD + (lane & 15);
                double a[2], b[2];
#pragma unroll
                for (int x = 0; x < 2; ++x) a[x] = P[rowoff + (wi * 2 + x) * 16];
#pragma unroll
                for (int y = 0; y < 2; ++y) b[y] = P[boff + rowoff + (wj * 2 + y) * 16];
#pragma unroll
                for (int x = 0; x < 2; ++x)
#pragma unroll
                    for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[x], b[y], acc[x][y], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    if (idle) return;
    double *out = partial + (((int64_t)blockIdx.y * K + k) * nq + blockIdx.x) * (MIX_BLK * MIX_BLK);
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                out[((wi * 2 + x) * 16 + (lane >> 4) + 4 * v) * MIX_BLK + (wj * 2 + y) * 16 + (lane & 15)] = acc[x][y][v];
}

// cov[k][i][j] = cov[k][j][i] = slice sums (ascending) / nk + reg_covar (i == j), i <= j.  grid (ceil(D D / 256), K)
__global__ __launch_bounds__(256) void k_mix_cov_reduce(const double *__restrict__ partial, int slices, int D, int K, int nb,
                                                        const double *__restrict__ nk, double reg, double *__restrict__ cov)
{
    const int e = blockIdx.x * MIX_TPB + threadIdx.x, k = blockIdx.y;
    if (e >= D * D) return;
    const int i = e / D, j = e % D;
    if (i > j) return;
    const int bi = i / MIX_BLK, bj = j / MIX_BLK, nq = nb * (nb + 1) / 2;
    const int q = bi * nb - bi * (bi - 1) / 2 + (bj - bi);
    const int off = (i % MIX_BLK) * MIX_BLK + j % MIX_BLK;
    double s = 0.0;
    for (int sl = 0; sl < slices; ++sl) s = s + partial[(((int64_t)sl * K + k) * nq + q) * (MIX_BLK * MIX_BLK) + off];
    double v = s / nk[k];
    if (i == j) v = v + reg;
    cov[((int64_t)k * D + i) * D + j] = v;
    cov[((int64_t)k * D + j) * D + i] = v;
}

// ---- precisions.  grid K, 256 threads.  L (scratch, D x D per component) and the padded P[k][Dp][Dp] (zero outside the
// upper triangle of the leading D x D), b[k][Dp], logdet[k], logw[k] ----
__global__ __launch_bounds__(256) void k_mix_prec_full(const double *__restrict__ cov, const double *__restrict__ mu, const double *__restrict__ w,
                                                       int D, int Dp, double *__restrict__ Lall, double *__restrict__ Pall,
                                                       double *__restrict__ ball, double *__restrict__ logdet, double *__restrict__ logw,
                                                       MixScalars *__restrict__ sc)
{
    __shared__ int bad;
    const int k = blockIdx.x, t = threadIdx.x;
    double *L = Lall + (int64_t)k * D * D;
    double *P = Pall + (int64_t)k * Dp * Dp;
    double *b = ball + (int64_t)k * Dp;
    const double *A = cov + (int64_t)k * D * D;
    if (t == 0) bad = 0;
    for (int e = t; e < D * D; e += MIX_TPB) L[e] = A[e];
    for (int e = t; e < Dp * Dp; e += MIX_TPB) P[e] = 0.0;
    for (int e = t; e < Dp; e += MIX_TPB) b[e] = 0.0;
    __syncthreads();
    // right-looking Cholesky on the lower triangle: column j, then the trailing update
    for (int j = 0; j < D; ++j) {
        if (t == 0) {
            const double p = L[j * D + j];
            if (!(p > 0.0) || !(p < INFINITY)) bad = 1;
            L[j * D + j] = sqrt(p);
        }
        __syncthreads();
        if (bad) break;
        const double ljj = L[j * D + j];
        for (int i = j + 1 + t; i < D; i += MIX_TPB) L[i * D + j] = L[i * D + j] / ljj;
        __syncthreads();
        const int m = D - j - 1;   // trailing rows / columns j + 1 ..
        for (int e = t; e < m * m; e += MIX_TPB) {
            const int i = j + 1 + e / m, c = j + 1 + e % m;
            if (c <= i) L[i * D + c] = L[i * D + c] - L[i * D + j] * L[c * D + j];
        }
        __syncthreads();
    }
    if (bad) {
        if (t == 0) atomicCAS(&sc->ill, 0, k + 1);
        if (t == 0) atomicMin(&sc->ill, k + 1);
        return;
    }
    // row c of P = column c of L^-1: y_c = 1 / L_cc, y_i = -(sum_{m = c}^{i - 1} L_im y_m) / L_ii
    for (int c = t; c < D; c += MIX_TPB) {
        double *y = P + (int64_t)c * Dp;
        y[c] = 1.0 / L[c * D + c];
        for (int i = c + 1; i < D; ++i) {
            double s = 0.0;
            for (int m = c; m < i; ++m) s = s + L[i * D + m] * y[m];
            y[i] = -s / L[i * D + i];
        }
    }
    __syncthreads();
    for (int j = t; j < D; j += MIX_TPB) {
        double s = 0.0;
        for (int m = 0; m <= j; ++m) s = s + mu[k * D + m] * P[(int64_t)m * Dp + j];
        b[j] = s;
    }
    if (t == 0) {
        double s = 0.0;
        for (int j = 0; j < D; ++j) s = s + log(P[(int64_t)j * Dp + j]);
        logdet[k] = s;
        logw[k] = log(w[k]);
    }
}

// "diag": P[k][d] = 1 / sqrt(var); grid K
__global__ __launch_bounds__(256) void k_mix_prec_diag(const double *__restrict__ cov, const double *__restrict__ w, int D, double *__restrict__ Pall,
                                                       double *__restrict__ logdet, double *__restrict__ logw, MixScalars *__restrict__ sc)
{
    __shared__ int bad;
    const int k = blockIdx.x, t = threadIdx.x;
    if (t == 0) bad = 0;
    __syncthreads();
    for (int d = t; d < D; d += MIX_TPB) {
        const double v = cov[k * D + d];
        if (!(v > 0.0) || !(v < INFINITY)) bad = 1;
        Pall[k * D + d] = 1.0 / sqrt(v);
    }
    __syncthreads();
    if (t == 0) {
        if (bad) {
            atomicCAS(&sc->ill, 0, k + 1);
            atomicMin(&sc->ill, k + 1);
            return;
        }
        double s = 0.0;
        for (int d = 0; d < D; ++d) s = s + log(Pall[k * D + d]);
        logdet[k] = s;
        logw[k] = log(w[k]);
    }
}

__device__ __forceinline__ double mix_tree16(double v)
{
    v = v + __shfl_xor(v, 1);
    v = v + __shfl_xor(v, 2);
    v = v + __shfl_xor(v, 4);
    v = v + __shfl_xor(v, 8);
    return v;
}

// ---- E-step, "full": weighted log-probabilities.  grid ceil(n / 64), 256 threads, dynamic LDS: Xs[64][Dp + 1] and
// qs[4][64].  A[i][k] = Xs[row tile * 16 + i][k0 + k], B[k][j] = P_k[k0 + k][tile * 16 + j] ----
__global__ __launch_bounds__(256) void k_mix_logp_full(const double *__restrict__ X, int64_t n, int D, int Dp, int K,
                                                       const double *__restrict__ Pall, const double *__restrict__ ball,
                                                       const double *__restrict__ logdet, const double *__restrict__ logw,
                                                       double *__restrict__ out)
{
    extern __shared__ double mix_lds[];
    const int LD = Dp + 1;
    double *Xs = mix_lds, *qs = mix_lds + MIX_EROWS * LD;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, l15 = lane & 15, l4 = lane >> 4;
    const int64_t r0 = (int64_t)blockIdx.x * MIX_EROWS;
    for (int q = t; q < MIX_EROWS * Dp; q += MIX_TPB) {
        const int lr = q / Dp, cc = q % Dp;
        Xs[lr * LD + cc] = (r0 + lr < n && cc < D) ? X[(r0 + lr) * D + cc] : 0.0;
    }
    __syncthreads();
    const int nt = Dp / 16;
    for (int k = 0; k < K; ++k) {
        const double *P = Pall + (int64_t)k * Dp * Dp;
        const double *b = ball + (int64_t)k * Dp;
        double qp[4][4];
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int v = 0; v < 4; ++v) qp[rt][v] = 0.0;
        for (int jt = wave; jt < nt; jt += 4) {
            v4f64 acc[4];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt) acc[rt] = v4f64{0.0, 0.0, 0.0, 0.0};
            const int kend = (jt + 1) * 16;
            for (int k0 = 0; k0 < kend; k0 += 4) {
                const double bv = P[(int64_t)(k0 + l4) * Dp + jt * 16 + l15];
#pragma unroll
                for (int rt = 0; rt < 4; ++rt) {
                    const double av = Xs[(rt * 16 + l15) * LD + k0 + l4];
                    acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[rt], 0, 0, 0);
                }
            }
            const double bj = b[jt * 16 + l15];
#pragma unroll
            for (int rt = 0; rt < 4; ++rt)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const double y = acc[rt][v] - bj;
                    qp[rt][v] = qp[rt][v] + y * y;
                }
        }
#pragma unroll
        for (int rt = 0; rt < 4; ++rt)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const double s = mix_tree16(qp[rt][v]);
                if (l15 == 0) qs[wave * MIX_EROWS + rt * 16 + l4 + 4 * v] = s;
            }
        __syncthreads();
        if (t < MIX_EROWS && r0 + t < n) {
            const double q = ((qs[t] + qs[MIX_EROWS + t]) + qs[2 * MIX_EROWS + t]) + qs[3 * MIX_EROWS + t];
            out[(r0 + t) * K + k] = (-0.5 * ((double)D * MIX_LOG_2PI + q) + logdet[k]) + logw[k];
        }
        __syncthreads();
    }
}

// ---- E-step, "diag": 16 lanes per row, lane l the columns l, l + 16, ... ascending, then the xor tree.  16 rows per
// workgroup ----
__global__ __launch_bounds__(256) void k_mix_logp_diag(const double *__restrict__ X, int64_t n, int D, int K, const double *__restrict__ mu,
                                                       const double *__restrict__ Pall, const double *__restrict__ logdet,
                                                       const double *__restrict__ logw, double *__restrict__ out)
{
    const int t = threadIdx.x, l = t & 15;
    const int64_t i = (int64_t)blockIdx.x * 16 + (t >> 4);
    const bool live = i < n;
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        if (live)
            for (int d = l; d < D; d += 16) {
                const double y = (X[i * D + d] - mu[k * D + d]) * Pall[k * D + d];
                s = s + y * y;
            }
        const double q = mix_tree16(s);
        if (live && l == 0) out[i * K + k] = (-0.5 * ((double)D * MIX_LOG_2PI + q) + logdet[k]) + logw[k];
    }
}

// per row: log sum exp, responsibilities in place, the first largest as label; per 256-row block the sum of the rows' log
// sum exp in row order
__global__ __launch_bounds__(256) void k_mix_normalize(double *__restrict__ resp, int64_t n, int K, int32_t *__restrict__ labels,
                                                       double *__restrict__ bpart)
{
    __shared__ double sred[MIX_TPB];
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * MIX_TPB + t;
    double lse = 0.0;
    if (i < n) {
        double *r = resp + i * K;
        double m = r[0];
        int bk = 0;
        for (int k = 1; k < K; ++k)
            if (r[k] > m) { m = r[k]; bk = k; }
        double s = 0.0, comp = 0.0;   // compensated (Kahan), k ascending: the sum is good to an ulp whatever K
        for (int k = 0; k < K; ++k) {
            const double e = exp(r[k] - m);
            r[k] = e;
            const double y = e - comp, t2 = s + y;
            comp = (t2 - s) - y;
            s = t2;
        }
        lse = m + log(s);
        for (int k = 0; k < K; ++k) r[k] = r[k] / s;   // exp(log p - lse) without lse's rounding: rows add up to 1
        if (labels) labels[i] = bk;
    }
    sred[t] = lse;
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int q = 0; q < MIX_TPB; ++q) s = s + sred[q];
        bpart[blockIdx.x] = s;
    }
}

// one workgroup: thread t adds the block sums t c .. (t + 1) c - 1 in ascending order, c = ceil(nbk / 256); thread 0 adds the 256
// thread sums in ascending order
__global__ __launch_bounds__(256) void k_mix_total(const double *__restrict__ bpart, int64_t nbk, MixScalars *__restrict__ sc)
{
    __shared__ double sred[MIX_TPB];
    const int t = threadIdx.x;
    const int64_t per = (nbk + MIX_TPB - 1) / MIX_TPB;
    const int64_t b1 = (t + 1) * per < nbk ? (t + 1) * per : nbk;
    double s = 0.0;
    for (int64_t b = t * per; b < b1; ++b) s = s + bpart[b];
    sred[t] = s;
    __syncthreads();
    if (t == 0) {
        double tot = 0.0;
        for (int q = 0; q < MIX_TPB; ++q) tot = tot + sred[q];
        sc->loglik_sum = tot;
    }
}

// the device state of one fit or predict call
struct MixWork {
    sc_ctx *c;
    int64_t n;
    int D, Dp, K, nb, nq, slices;
    bool full;
    int64_t slice_rows, nbk;
    size_t covsz, psz;   // doubles of one run's covariances / precisions
    DBuf X, resp, lab, psum, pnk, partial, blocks, nk, w, mu, cov, L, P, b, logdet, logw, bpart, sc;

    int init(sc_ctx *ctx, int64_t n_, int D_, int K_, bool full_)
    {
        c = ctx, n = n_, D = D_, K = K_, full = full_;
        Dp = (D + 15) / 16 * 16;
        nb = (D + MIX_BLK - 1) / MIX_BLK, nq = nb * (nb + 1) / 2;
        slice_rows = mix_slice_rows(n, D, K, full);
        slices = (int)ceil_div64(n, slice_rows);
        nbk = ceil_div64(n, MIX_TPB);
        covsz = full ? (size_t)K * D * D : (size_t)K * D;
        psz = full ? (size_t)K * Dp * Dp : (size_t)K * D;
        int64_t *mem = &c->mem;
        SC_TRY(X.ensure(sizeof(double) * (size_t)n * D, mem));
        SC_TRY(resp.ensure(sizeof(double) * (size_t)n * K, mem));
        SC_TRY(lab.ensure(sizeof(int32_t) * (size_t)n, mem));
        SC_TRY(psum.ensure(sizeof(double) * (size_t)slices * K * D, mem));
        SC_TRY(pnk.ensure(sizeof(double) * (size_t)slices * K, mem));
        SC_TRY(nk.ensure(sizeof(double) * (size_t)K, mem));
        SC_TRY(w.ensure(sizeof(double) * (size_t)K, mem));
        SC_TRY(mu.ensure(sizeof(double) * (size_t)K * D, mem));
        SC_TRY(cov.ensure(sizeof(double) * covsz, mem));
        SC_TRY(P.ensure(sizeof(double) * psz, mem));
        SC_TRY(b.ensure(sizeof(double) * (size_t)K * Dp, mem));
        SC_TRY(logdet.ensure(sizeof(double) * (size_t)K, mem));
        SC_TRY(logw.ensure(sizeof(double) * (size_t)K, mem));
        SC_TRY(bpart.ensure(sizeof(double) * (size_t)nbk, mem));
        SC_TRY(sc.ensure(sizeof(MixScalars), mem));
        if (full) {
            SC_TRY(L.ensure(sizeof(double) * (size_t)K * D * D, mem));
            SC_TRY(blocks.ensure(sizeof(int2) * (size_t)nq, mem));
            std::vector<int2> bl;
            for (int bi = 0; bi < nb; ++bi)
                for (int bj = bi; bj < nb; ++bj) bl.push_back(int2{bi, bj});
            SC_HIP(hipMemcpyAsync(blocks.p, bl.data(), sizeof(int2) * (size_t)nq, hipMemcpyHostToDevice, c->stream));
            SC_HIP(hipStreamSynchronize(c->stream));   // `bl` lives until here
            const size_t lds = sizeof(double) * ((size_t)MIX_EROWS * (Dp + 1) + 4 * MIX_EROWS);
            if (lds > 48 * 1024)
                SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mix_logp_full), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        }
        SC_HIP(hipMemsetAsync(sc.p, 0, sizeof(MixScalars), c->stream));
        return SC_OK;
    }

    // partials only while a fit runs
    int init_partials()
    {
        if (full) SC_TRY(partial.ensure(sizeof(double) * (size_t)slices * K * nq * MIX_BLK * MIX_BLK, &c->mem));
        return SC_OK;
    }

    void precisions()
    {
        hipStream_t s = c->stream;
        if (full)
            hipLaunchKernelGGL(k_mix_prec_full, dim3((unsigned)K), dim3(MIX_TPB), 0, s, cov.as<double>(), mu.as<double>(), w.as<double>(), D, Dp,
                               L.as<double>(), P.as<double>(), b.as<double>(), logdet.as<double>(), logw.as<double>(), sc.as<MixScalars>());
        else
            hipLaunchKernelGGL(k_mix_prec_diag, dim3((unsigned)K), dim3(MIX_TPB), 0, s, cov.as<double>(), w.as<double>(), D, P.as<double>(),
                               logdet.as<double>(), logw.as<double>(), sc.as<MixScalars>());
    }

    void mstep(double reg)
    {
        hipStream_t s = c->stream;
        KernelTimerScope ts(c, SC_K_MIX_MSTEP);
        hipLaunchKernelGGL(k_mix_sums, dim3((unsigned)slices, (unsigned)K), dim3(MIX_TPB), 0, s, X.as<double>(), resp.as<double>(), n, D, K, slice_rows,
                           mu.as<double>(), 0, psum.as<double>(), pnk.as<double>());
        hipLaunchKernelGGL(k_mix_means, dim3(1), dim3(MIX_TPB), 0, s, psum.as<double>(), pnk.as<double>(), slices, D, K, nk.as<double>(),
                           mu.as<double>(), w.as<double>());
        if (full) {
            hipLaunchKernelGGL(k_mix_cov, dim3((unsigned)nq, (unsigned)slices, (unsigned)K), dim3(MIX_TPB), 0, s, X.as<double>(), resp.as<double>(), n,
                               D, K, slice_rows, mu.as<double>(), blocks.as<int2>(), partial.as<double>());
            hipLaunchKernelGGL(k_mix_cov_reduce, dim3((unsigned)ceil_div64((int64_t)D * D, MIX_TPB), (unsigned)K), dim3(MIX_TPB), 0, s,
                               partial.as<double>(), slices, D, K, nb, nk.as<double>(), reg, cov.as<double>());
        } else {
            hipLaunchKernelGGL(k_mix_sums, dim3((unsigned)slices, (unsigned)K), dim3(MIX_TPB), 0, s, X.as<double>(), resp.as<double>(), n, D, K,
                               slice_rows, mu.as<double>(), 1, psum.as<double>(), pnk.as<double>());
            hipLaunchKernelGGL(k_mix_var_reduce, dim3((unsigned)ceil_div64((int64_t)K * D, MIX_TPB)), dim3(MIX_TPB), 0, s, psum.as<double>(), slices, D,
                               K, nk.as<double>(), reg, cov.as<double>());
        }
        precisions();
    }

    void estep(int32_t *labels)
    {
        hipStream_t s = c->stream;
        KernelTimerScope ts(c, SC_K_MIX_ESTEP);
        if (full) {
            const size_t lds = sizeof(double) * ((size_t)MIX_EROWS * (Dp + 1) + 4 * MIX_EROWS);
            hipLaunchKernelGGL(k_mix_logp_full, dim3((unsigned)ceil_div64(n, MIX_EROWS)), dim3(MIX_TPB), lds, s, X.as<double>(), n, D, Dp, K,
                               P.as<double>(), b.as<double>(), logdet.as<double>(), logw.as<double>(), resp.as<double>());
        } else {
            hipLaunchKernelGGL(k_mix_logp_diag, dim3((unsigned)ceil_div64(n, 16)), dim3(MIX_TPB), 0, s, X.as<double>(), n, D, K, mu.as<double>(),
                               P.as<double>(), logdet.as<double>(), logw.as<double>(), resp.as<double>());
        }
        hipLaunchKernelGGL(k_mix_normalize, dim3((unsigned)nbk), dim3(MIX_TPB), 0, s, resp.as<double>(), n, K, labels, bpart.as<double>());
        hipLaunchKernelGGL(k_mix_total, dim3(1), dim3(MIX_TPB), 0, s, bpart.as<double>(), nbk, sc.as<MixScalars>());
    }

    int scalars(MixScalars *out)
    {
        SC_HIP(hipGetLastError());
        SC_HIP(hipMemcpyAsync(out, sc.p, sizeof(MixScalars), hipMemcpyDeviceToHost, c->stream));
        SC_HIP(hipStreamSynchronize(c->stream));
        return SC_OK;
    }

    int ill_defined(const char *who, int comp)
    {
        sc_set_error("%s: the covariance of component %d is not positive definite (ill-defined empirical covariance): "
                     "decrease the number of components or increase reg_covar", who, comp);
        return SC_ERR_ILLDEFINED;
    }
};

// the input as fp64: the caller's array itself when it is fp64, a widened copy (held by `keep`) when it is float32
const double *mix_as_f64(const void *X, int dtype, size_t count, std::vector<double> &keep)
{
    if (dtype != SC_F32) return (const double *)X;
    keep.resize(count);
    for (size_t i = 0; i < count; ++i) keep[i] = (double)((const float *)X)[i];
    return keep.data();
}

int mix_check_shape(const char *who, int dtype, int64_t n, int D, int K, int cov_type)
{
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "%s: dtype must be SC_F32 or SC_F64", who);
    SC_REQUIRE(n >= 1 && n <= INT32_MAX, SC_ERR_INVALID, "%s: need 1 <= n <= 2^31 - 1, got %lld", who, (long long)n);
    SC_REQUIRE(D >= 1 && D <= MIX_DMAX, SC_ERR_INVALID, "%s: need 1 <= D <= %d, got %d", who, MIX_DMAX, D);
    SC_REQUIRE(K >= 1 && K <= MIX_KMAX && (int64_t)K <= n, SC_ERR_INVALID, "%s: need 1 <= K <= min(%d, n) (K = %d, n = %lld)", who, MIX_KMAX,
               K, (long long)n);
    SC_REQUIRE(cov_type == SC_MIX_FULL || cov_type == SC_MIX_DIAG, SC_ERR_INVALID, "%s: cov_type must be SC_MIX_FULL or SC_MIX_DIAG, got %d", who,
               cov_type);
    return SC_OK;
}

int mix_check_finite(const char *who, const char *what, const double *v, size_t count)
{
    for (size_t i = 0; i < count; ++i)
        SC_REQUIRE(std::isfinite(v[i]), SC_ERR_INVALID, "%s: %s %lld is not finite", who, what, (long long)i);
    return SC_OK;
}

}  // namespace

extern "C" int sc_mixture_fit(sc_ctx *c, const void *X, int dtype, int64_t n, int32_t D, int32_t K, int32_t cov_type, int32_t n_init,
                              int32_t km_max_iter, double km_tol, const double *x_mean, const double *uniforms, int32_t max_iter, double tol,
                              double reg_covar, double *weights_out, double *means_out, double *covariances_out, double *lower_bound_out,
                              int32_t *n_iter_out, int32_t *converged_out, int32_t *best_out, int32_t *labels_out, double *proba_out,
                              double *loglik_out)
{
    const char *who = "sc_mixture_fit";
    SC_REQUIRE(c && X && weights_out && means_out && covariances_out && lower_bound_out && n_iter_out && converged_out && best_out && labels_out &&
                   loglik_out,
               SC_ERR_INVALID, "%s: null pointer", who);
    SC_TRY(mix_check_shape(who, dtype, n, D, K, cov_type));
    SC_REQUIRE(K == 1 || (x_mean && uniforms), SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(n_init >= 1 && n_init <= MIX_RMAX, SC_ERR_INVALID, "%s: need 1 <= n_init <= %d, got %d", who, MIX_RMAX, n_init);
    SC_REQUIRE(km_max_iter >= 1 && max_iter >= 1, SC_ERR_INVALID, "%s: km_max_iter and max_iter must be >= 1", who);
    SC_REQUIRE(std::isfinite(km_tol) && km_tol >= 0.0 && std::isfinite(tol) && tol >= 0.0 && std::isfinite(reg_covar) && reg_covar >= 0.0,
               SC_ERR_INVALID, "%s: km_tol, tol and reg_covar must be finite and >= 0", who);
    std::vector<double> widened;
    const size_t count = (size_t)n * D;
    const double *X64 = mix_as_f64(X, dtype, count, widened);
    SC_TRY(mix_check_finite(who, "value", X64, count));

    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const bool full = cov_type == SC_MIX_FULL;
    const int R = n_init;
    MixWork m;
    DBuf kmlab, bestpar;
    StreamWaitOnExit wait{c->stream};
    SC_TRY(m.init(c, n, D, K, full));
    SC_TRY(m.init_partials());
    if (K > 1) {
        SC_TRY(kmlab.ensure(sizeof(int32_t) * (size_t)R * (size_t)n, &c->mem));
        SC_TRY(sc_kmeans_run_labels(c, X64, SC_F64, n, D, K, R, km_max_iter, km_tol, x_mean, uniforms, kmlab.as<int32_t>()));
    }
    SC_HIP(hipMemcpyAsync(m.X.p, X64, sizeof(double) * count, hipMemcpyHostToDevice, s));
    // the best run's parameters: weights, means, covariances
    const size_t npar = (size_t)K + (size_t)K * D + m.covsz;
    SC_TRY(bestpar.ensure(sizeof(double) * npar, &c->mem));

    const dim3 flat((unsigned)ceil_div64(n * K, 256)), tpb(256);
    int best = -1;
    double best_lb = -INFINITY;
    MixScalars sc;
    for (int r = 0; r < R; ++r) {
        hipLaunchKernelGGL(k_mix_onehot, flat, tpb, 0, s, K > 1 ? kmlab.as<int32_t>() + (int64_t)r * n : (const int32_t *)nullptr, n, K,
                           m.resp.as<double>());
        m.mstep(reg_covar);
        SC_TRY(m.scalars(&sc));
        if (sc.ill) return m.ill_defined(who, sc.ill - 1);
        double prev = -INFINITY, lb = -INFINITY;
        int it = 0, conv = 0;
        for (it = 1; it <= max_iter; ++it) {
            m.estep(nullptr);
            m.mstep(reg_covar);
            SC_TRY(m.scalars(&sc));
            if (sc.ill) return m.ill_defined(who, sc.ill - 1);
            lb = sc.loglik_sum / (double)n;
            if (std::fabs(lb - prev) < tol) {
                conv = 1;
                break;
            }
            prev = lb;
        }
        if (it > max_iter) it = max_iter;
        lower_bound_out[r] = lb;
        n_iter_out[r] = it;
        converged_out[r] = conv;
        SC_HIP(hipMemcpyAsync(weights_out + (size_t)r * K, m.w.p, sizeof(double) * (size_t)K, hipMemcpyDeviceToHost, s));
        SC_HIP(hipMemcpyAsync(means_out + (size_t)r * K * D, m.mu.p, sizeof(double) * (size_t)K * D, hipMemcpyDeviceToHost, s));
        SC_HIP(hipMemcpyAsync(covariances_out + (size_t)r * m.covsz, m.cov.p, sizeof(double) * m.covsz, hipMemcpyDeviceToHost, s));
        if (best < 0 || lb > best_lb) {   // strictly larger: the first of equal runs stays
            best = r, best_lb = lb;
            double *bp = bestpar.as<double>();
            SC_HIP(hipMemcpyAsync(bp, m.w.p, sizeof(double) * (size_t)K, hipMemcpyDeviceToDevice, s));
            SC_HIP(hipMemcpyAsync(bp + K, m.mu.p, sizeof(double) * (size_t)K * D, hipMemcpyDeviceToDevice, s));
            SC_HIP(hipMemcpyAsync(bp + K + (size_t)K * D, m.cov.p, sizeof(double) * m.covsz, hipMemcpyDeviceToDevice, s));
        }
        SC_HIP(hipStreamSynchronize(s));
    }
    // ---- one more E-step under the best run's parameters: what sc_mixture_predict computes from the same bytes ----
    {
        const double *bp = bestpar.as<double>();
        SC_HIP(hipMemcpyAsync(m.w.p, bp, sizeof(double) * (size_t)K, hipMemcpyDeviceToDevice, s));
        SC_HIP(hipMemcpyAsync(m.mu.p, bp + K, sizeof(double) * (size_t)K * D, hipMemcpyDeviceToDevice, s));
        SC_HIP(hipMemcpyAsync(m.cov.p, bp + K + (size_t)K * D, sizeof(double) * m.covsz, hipMemcpyDeviceToDevice, s));
        {
            KernelTimerScope ts(c, SC_K_MIX_MSTEP);
            m.precisions();
        }
        m.estep(m.lab.as<int32_t>());
        SC_TRY(m.scalars(&sc));
        if (sc.ill) return m.ill_defined(who, sc.ill - 1);
    }
    SC_HIP(hipMemcpyAsync(labels_out, m.lab.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    if (proba_out) SC_HIP(hipMemcpyAsync(proba_out, m.resp.p, sizeof(double) * (size_t)n * K, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    *best_out = best;
    *loglik_out = sc.loglik_sum / (double)n;
    return SC_OK;
}

extern "C" int sc_mixture_predict(sc_ctx *c, const void *X, int dtype, int64_t n, int32_t D, int32_t K, int32_t cov_type, const double *weights,
                                  const double *means, const double *covariances, int32_t *labels_out, double *proba_out, double *loglik_out)
{
    const char *who = "sc_mixture_predict";
    SC_REQUIRE(c && X && weights && means && covariances && labels_out && loglik_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "%s: dtype must be SC_F32 or SC_F64", who);
    SC_REQUIRE(n >= 1 && n <= INT32_MAX, SC_ERR_INVALID, "%s: need 1 <= n <= 2^31 - 1, got %lld", who, (long long)n);
    SC_REQUIRE(D >= 1 && D <= MIX_DMAX, SC_ERR_INVALID, "%s: need 1 <= D <= %d, got %d", who, MIX_DMAX, D);
    SC_REQUIRE(K >= 1 && K <= MIX_KMAX, SC_ERR_INVALID, "%s: need 1 <= K <= %d, got %d", who, MIX_KMAX, K);
    SC_REQUIRE(cov_type == SC_MIX_FULL || cov_type == SC_MIX_DIAG, SC_ERR_INVALID, "%s: cov_type must be SC_MIX_FULL or SC_MIX_DIAG, got %d", who,
               cov_type);
    const bool full = cov_type == SC_MIX_FULL;
    const size_t covsz = full ? (size_t)K * D * D : (size_t)K * D;
    for (int k = 0; k < K; ++k)
        SC_REQUIRE(std::isfinite(weights[k]) && weights[k] > 0.0, SC_ERR_INVALID, "%s: weight %d must be finite and > 0", who, k);
    SC_TRY(mix_check_finite(who, "mean", means, (size_t)K * D));
    SC_TRY(mix_check_finite(who, "covariance", covariances, covsz));
    std::vector<double> widened;
    const size_t count = (size_t)n * D;
    const double *X64 = mix_as_f64(X, dtype, count, widened);
    SC_TRY(mix_check_finite(who, "value", X64, count));

    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    MixWork m;
    StreamWaitOnExit wait{c->stream};
    SC_TRY(m.init(c, n, D, K, full));
    SC_HIP(hipMemcpyAsync(m.X.p, X64, sizeof(double) * count, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(m.w.p, weights, sizeof(double) * (size_t)K, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(m.mu.p, means, sizeof(double) * (size_t)K * D, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(m.cov.p, covariances, sizeof(double) * covsz, hipMemcpyHostToDevice, s));
    {
        KernelTimerScope ts(c, SC_K_MIX_MSTEP);
        m.precisions();
    }
    m.estep(m.lab.as<int32_t>());
    MixScalars sc;
    SC_TRY(m.scalars(&sc));
    if (sc.ill) return m.ill_defined(who, sc.ill - 1);
    SC_HIP(hipMemcpyAsync(labels_out, m.lab.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    if (proba_out) SC_HIP(hipMemcpyAsync(proba_out, m.resp.p, sizeof(double) * (size_t)n * K, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    *loglik_out = sc.loglik_sum / (double)n;
    return SC_OK;
}

extern "C" int sc_mixture_slice_rows(int64_t n, int32_t D, int32_t K, int32_t cov_type, int64_t *rows_out)
{
    const char *who = "sc_mixture_slice_rows";
    SC_REQUIRE(rows_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(n >= 1 && n <= INT32_MAX, SC_ERR_INVALID, "%s: need 1 <= n <= 2^31 - 1, got %lld", who, (long long)n);
    SC_REQUIRE(D >= 1 && D <= MIX_DMAX, SC_ERR_INVALID, "%s: need 1 <= D <= %d, got %d", who, MIX_DMAX, D);
    SC_REQUIRE(K >= 1 && K <= MIX_KMAX, SC_ERR_INVALID, "%s: need 1 <= K <= %d, got %d", who, MIX_KMAX, K);
    SC_REQUIRE(cov_type == SC_MIX_FULL || cov_type == SC_MIX_DIAG, SC_ERR_INVALID, "%s: cov_type must be SC_MIX_FULL or SC_MIX_DIAG, got %d", who,
               cov_type);
    *rows_out = mix_slice_rows(n, D, K, cov_type == SC_MIX_FULL);
    return SC_OK;
}
