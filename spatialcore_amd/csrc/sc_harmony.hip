// sc_harmony.hip -- sc_harmony_*: Harmony batch correction of an n x d embedding (Korsunsky et al. 2019; DESIGN.md 4.6t;
// restated by tests/harmony_restated.py).  The state lives on the device between sc_harmony_begin and sc_harmony_end; the
// outer loop is the caller's (integration/harmony.py).
//
// Layout.  The cells are sorted once, on the host, by (block, batch, cell index), block = cell mod n_blocks.  A block is then
// a run of positions, a (block, batch) segment a run inside it, and a segment is cut into slices of hm_slice_cells(n) cells
// (a function of n alone).  A slice is the unit of every sum over cells: it belongs to one block and one batch, so a slice
// sum is K (or K x d) values, never K x B.  Z, Zc, Zcorr are [position][d]; dist, S, R are [k][position] (a thread owns a
// position, a wavefront reads 64 consecutive positions of one cluster).
//
// fp64 throughout, no floating-point atomics, plain launches on the context's stream; every result is a function of the
// arguments alone.  The one expression order (fma = fused, everything else rounds separately, -ffp-contract=off):
//    Zc_i      = z / sqrt(q), q = 0.0 + z_0 z_0 + z_1 z_1 + ...                          (k_hm_normalise; also of Zcorr)
//    dot_ik    = fma(Zc_i[d-1], Y_k[d-1], ... fma(Zc_i[0], Y_k[0], 0.0)),  dist_ik = 2.0 (1.0 - dot_ik)      (k_hm_dist)
//    S_ik      = exp((m_i - dist_ik) * (1.0 / sigma)), m_i = min_k dist_ik; begin: R_ik = S_ik * (1.0 / (0.0 + S_i0 + ..))
//    a slice's sum over its cells: thread t of the 128 adds the cells t, t + 128, .. in order; the 64 values of a wavefront
//                are added as the tree v[l] += v[l ^ 32], ^ 16, .. ^ 1; then wavefront 0 + wavefront 1       (hm_slice_sum4)
//    "the slices in order" of a sum over ALL slices: groups of 64 consecutive slices, each 0.0 + its slices in order
//                (k_hm_fold), then 0.0 + the groups in order
//    O[t][k][b] = 0.0 + the slice sums of segment (t, b) in slice order                                      (k_hm_tables)
//    O-_kb     = 0.0 + O[t'][k][b], t' != t ascending;  E-_kb = (0.0 + O-_k0 + O-_k1 + ..) Pr_b, Pr_b = n_b / n
//    pen_kb    = pow((E-_kb + 1.0) / (O-_kb + 1.0), theta);  u_ik = S_ik pen_kb(i);  R_ik = u_ik * (1.0 / (0.0 + u_i0 + ..))
//    objective = t1 + sigma t2 + (sigma theta) t3: t1 = sum R dist, t2 = sum R log R (R > 0), t3 = sum R log((O_kb + 1.0) /
//                (E_kb + 1.0)) with O = 0.0 + O[0] + O[1] + ..; per cell over k ascending, per slice as above, slices in order
//    Y_k       = v / sqrt(0.0 + v_0 v_0 + ..), v = the slice sums of R^T Zc in slice order; a slice sum's element is the fma
//                chain over the slice's cells in position order (k_hm_rtz).  A cluster without mass keeps its centre.
//    r_b       = the slice sums of R^T Z of batch b's slices in slice order, r_0 = 0.0 + r_0 + r_1 + ..       (k_hm_ridge)
//    w_0       = (r_0 - (0.0 + sum_b o_b r_b / (o_b + lamb))) / (s - (0.0 + sum_b o_b o_b / (o_b + lamb))), s = 0.0 + sum_b o_b
//                (a cluster without mass, s = 0: w_0 = 0)
//    W_kb      = (r_b - o_b w_0) / (o_b + lamb);  Zcorr_i = Z_i - fma chain over k ascending of R_ik W_kb(i)  (k_hm_apply)
//
// The three n x K x d contractions (k_hm_dist, k_hm_rtz, k_hm_apply) are one register-tiled loop (hm_mac: a thread owns
// 4 x 4 outputs, both operands staged in LDS with the summed index outermost) on the fp64 vector unit.
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "sc_ctx.h"

namespace {

constexpr int HM_DMAX = 64, HM_KMAX = 128, HM_BMAX = 64, HM_NBMAX = 1024;
constexpr int HM_TPB = 256;               // threads of a contraction workgroup
constexpr int HM_M = 128;                 // cells per contraction tile, threads of a per-cell workgroup, slice granule
constexpr int64_t HM_MAX_SLICES = 8192;   // the slice length doubles, triples, .. once n needs more slices than this
constexpr int HM_LDA = HM_M + 4;          // LDS row stride of a 128-wide operand: 16-byte aligned, rows 4 banks apart
constexpr int HM_LDD = HM_DMAX + 4;       // ... of a 64-wide one
constexpr int HM_CH_D = 16, HM_CH = 32;   // summed-index chunk: features (k_hm_dist), cells (k_hm_rtz), clusters (k_hm_apply)

constexpr int HM_KH = 64;                 // clusters per pass of k_hm_dist
constexpr int HM_GROUP = 64;              // slices per group of hm_fold
static_assert(HM_KH == HM_DMAX, "k_hm_dist's cluster panel has the stride of a feature panel");

inline int64_t hm_slice_cells(int64_t n) { return HM_M * ceil_div64(n, HM_M * HM_MAX_SLICES); }

struct HmSlice {
    int64_t p0;      // first position
    int32_t len;     // cells
    int32_t batch;
};

// acc[p][a][b] += sum over t < len (ascending) of As[t][4 mt + a] * Bs[t][4 nt + b] for the thread's tile p = (mt, nt)
template <int NP>
__device__ __forceinline__ void hm_mac(const double *As, int lda, const double *Bs, int ldb, int len, const int (&mt)[NP],
                                       const int (&nt)[NP], const bool (&on)[NP], double (&acc)[NP][4][4])
{
    for (int t = 0; t < len; ++t) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            if (!on[p]) continue;
            double a[4], b[4];
#pragma unroll
            for (int x = 0; x < 4; ++x) a[x] = As[t * lda + 4 * mt[p] + x];
#pragma unroll
            for (int y = 0; y < 4; ++y) b[y] = Bs[t * ldb + 4 * nt[p] + y];
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) acc[p][x][y] = fma(a[x], b[y], acc[p][x][y]);
        }
    }
}

// the thread's tiles: tile q = threadIdx.x + 256 p of an (mtiles x ntiles) grid, mt fastest
template <int NP>
__device__ __forceinline__ void hm_tiles(int mtiles, int ntiles, int (&mt)[NP], int (&nt)[NP], bool (&on)[NP], double (&acc)[NP][4][4])
{
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int q = threadIdx.x + HM_TPB * p;
        on[p] = q < mtiles * ntiles;
        mt[p] = on[p] ? q % mtiles : 0;
        nt[p] = on[p] ? q / mtiles : 0;
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) acc[p][x][y] = 0.0;
    }
}

// v[x] <- the sum of v[x] over the 128 threads of a per-cell workgroup, in the documented tree, four sums per barrier pair
__device__ __forceinline__ void hm_slice_sum4(double (&v)[4], double *pair)   // pair[8]
{
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) v[x] = v[x] + __shfl_xor(v[x], h, 64);
    __syncthreads();   // the previous use of `pair` is over
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int x = 0; x < 4; ++x) pair[(threadIdx.x >> 6) * 4 + x] = v[x];
    __syncthreads();
#pragma unroll
    for (int x = 0; x < 4; ++x) v[x] = pair[x] + pair[4 + x];
}

// out_i = in_i / |in_i|, one thread per position
__global__ __launch_bounds__(256) void k_hm_normalise(const double *in, int64_t n, int d, double *out)   // in place for Y
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    double q = 0.0;
    for (int j = 0; j < d; ++j) q = q + in[p * d + j] * in[p * d + j];
    const double r = sqrt(q);
    for (int j = 0; j < d; ++j) out[p * d + j] = in[p * d + j] / r;
}

// dist[k][p] = 2 (1 - Zc_p . Y_k): a workgroup owns 128 positions, 64 clusters at a time; the features are summed in chunks of 16
__global__ __launch_bounds__(HM_TPB) void k_hm_dist(const double *__restrict__ Zc, const double *__restrict__ Y, int64_t n, int d,
                                                    int K, double *__restrict__ dist)
{
    __shared__ __attribute__((aligned(16))) double As[HM_CH_D * HM_LDA], Bs[HM_CH_D * HM_LDD];
    const int64_t p0 = (int64_t)blockIdx.x * HM_M;
    const int cells = (int)(n - p0 < HM_M ? n - p0 : HM_M);
    for (int k0 = 0; k0 < K; k0 += HM_KH) {   // 64 clusters at a time: 32 accumulators per thread, three wavefronts per SIMD
        const int kh = K - k0 < HM_KH ? K - k0 : HM_KH;
        int mt[2], nt[2];
        bool on[2];
        double acc[2][4][4];
        hm_tiles<2>(HM_M / 4, (kh + 3) / 4, mt, nt, on, acc);
        for (int j0 = 0; j0 < d; j0 += HM_CH_D) {
            for (int e = threadIdx.x; e < HM_CH_D * HM_M; e += HM_TPB) {
                const int j = e % HM_CH_D, c = e / HM_CH_D;
                As[j * HM_LDA + c] = (c < cells && j0 + j < d) ? Zc[(p0 + c) * d + j0 + j] : 0.0;
            }
            for (int e = threadIdx.x; e < HM_CH_D * HM_KH; e += HM_TPB) {
                const int j = e % HM_CH_D, c = e / HM_CH_D;
                Bs[j * HM_LDD + c] = (c < kh && j0 + j < d) ? Y[(k0 + c) * d + j0 + j] : 0.0;
            }
            __syncthreads();
            hm_mac<2>(As, HM_LDA, Bs, HM_LDD, HM_CH_D, mt, nt, on, acc);
            __syncthreads();
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            if (!on[p]) continue;
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                const int k = 4 * nt[p] + y;
                if (k >= kh) continue;
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const int c = 4 * mt[p] + x;
                    if (c < cells) dist[(int64_t)(k0 + k) * n + p0 + c] = 2.0 * (1.0 - acc[p][x][y]);
                }
            }
        }
    }
}

// S from dist, one thread per position; init: R = S / sum S as well
__global__ __launch_bounds__(256) void k_hm_soft(const double *__restrict__ dist, int64_t n, int K, double inv_sigma, int init,
                                                 double *__restrict__ S, double *__restrict__ R)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    double m = dist[p];
    for (int k = 1; k < K; ++k) {
        const double v = dist[(int64_t)k * n + p];
        m = v < m ? v : m;
    }
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
        const double s = exp((m - dist[(int64_t)k * n + p]) * inv_sigma);
        S[(int64_t)k * n + p] = s;
        sum = sum + s;
    }
    if (!init) return;
    const double inv = 1.0 / sum;
    for (int k = 0; k < K; ++k) R[(int64_t)k * n + p] = S[(int64_t)k * n + p] * inv;
}

// one slice per workgroup of 128: opart[slice][k] = the slice's sum of R[k]
__global__ __launch_bounds__(HM_M) void k_hm_slice_mass(const HmSlice *__restrict__ slices, const double *__restrict__ R, int64_t n,
                                                        int K, double *__restrict__ opart)
{
    __shared__ double pair[8];
    const HmSlice sl = slices[blockIdx.x];
    for (int k0 = 0; k0 < K; k0 += 4) {
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        for (int c = threadIdx.x; c < sl.len; c += HM_M)
#pragma unroll
            for (int x = 0; x < 4; ++x)
                if (k0 + x < K) v[x] = v[x] + R[(int64_t)(k0 + x) * n + sl.p0 + c];
        hm_slice_sum4(v, pair);
        if (threadIdx.x == 0)
#pragma unroll
            for (int x = 0; x < 4; ++x)
                if (k0 + x < K) opart[(int64_t)blockIdx.x * K + k0 + x] = v[x];
    }
}

// the block step: slice first + blockIdx.x (the slices of one block).  R = S pen / sum_k S pen for the slice's cells, then
// the slice's new mass
__global__ __launch_bounds__(HM_M) void k_hm_block(const HmSlice *__restrict__ slices, int first, const double *__restrict__ S,
                                                   const double *__restrict__ pen, int64_t n, int K, int B, double *__restrict__ R,
                                                   double *__restrict__ inv_sum, double *__restrict__ opart)
{
    __shared__ double pair[8];
    __shared__ double pk[HM_KMAX];
    const int s = first + blockIdx.x;
    const HmSlice sl = slices[s];
    for (int k = threadIdx.x; k < K; k += HM_M) pk[k] = pen[k * B + sl.batch];
    __syncthreads();
    for (int c = threadIdx.x; c < sl.len; c += HM_M) {
        double sum = 0.0;
        for (int k = 0; k < K; ++k) sum = sum + S[(int64_t)k * n + sl.p0 + c] * pk[k];
        inv_sum[sl.p0 + c] = 1.0 / sum;
    }
    for (int k0 = 0; k0 < K; k0 += 4) {
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        for (int c = threadIdx.x; c < sl.len; c += HM_M) {
            const double inv = inv_sum[sl.p0 + c];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                if (k0 + x >= K) continue;
                const int64_t at = (int64_t)(k0 + x) * n + sl.p0 + c;
                const double r = (S[at] * pk[k0 + x]) * inv;
                R[at] = r;
                v[x] = v[x] + r;
            }
        }
        hm_slice_sum4(v, pair);
        if (threadIdx.x == 0)
#pragma unroll
            for (int x = 0; x < 4; ++x)
                if (k0 + x < K) opart[(int64_t)s * K + k0 + x] = v[x];
    }
}

// One workgroup of 64 per cluster k, thread b.  rebuild >= 0: O[rebuild][k][b] from its slices' sums.  Then next < nb: pen
// for block `next` from the other blocks' tables; next == nb: the round is over, otot = the sum of every table and lratio =
// log((O + 1) / (E + 1)).  A thread reads back only what it wrote itself.
__global__ __launch_bounds__(64) void k_hm_tables(const int32_t *__restrict__ seg_first, const double *__restrict__ opart,
                                                  const double *__restrict__ pr, int nb, int K, int B, int rebuild, int next,
                                                  double theta, double *__restrict__ oblk, double *__restrict__ pen,
                                                  double *__restrict__ otot, double *__restrict__ lratio)
{
    __shared__ double om[HM_BMAX];
    const int k = blockIdx.x, b = threadIdx.x, KB = K * B, e = k * B + b;
    if (rebuild >= 0 && b < B) {
        double s = 0.0;
#pragma unroll 8
        for (int q = seg_first[rebuild * B + b]; q < seg_first[rebuild * B + b + 1]; ++q) s = s + opart[(int64_t)q * K + k];
        oblk[(int64_t)rebuild * KB + e] = s;
    }
    if (next < 0) return;
    if (b < B) {
        double s = 0.0;
        for (int t = 0; t < nb; ++t)
            if (t != next) s = s + oblk[(int64_t)t * KB + e];
        om[b] = s;
    }
    __syncthreads();
    if (b >= B) return;
    double row = 0.0;
    for (int x = 0; x < B; ++x) row = row + om[x];
    const double E = row * pr[b];
    if (next < nb) pen[e] = pow((E + 1.0) / (om[b] + 1.0), theta);
    else {
        otot[e] = om[b];
        lratio[e] = log((om[b] + 1.0) / (E + 1.0));
    }
}

// one slice per workgroup of 128: objpart[slice][3] = the slice's sums of R dist, R log R, R lratio
__global__ __launch_bounds__(HM_M) void k_hm_objective(const HmSlice *__restrict__ slices, const double *__restrict__ R,
                                                       const double *__restrict__ dist, const double *__restrict__ lratio,
                                                       int64_t n, int K, int B, double *__restrict__ objpart)
{
    __shared__ double pair[8];
    __shared__ double lk[HM_KMAX];
    const HmSlice sl = slices[blockIdx.x];
    for (int k = threadIdx.x; k < K; k += HM_M) lk[k] = lratio[k * B + sl.batch];
    __syncthreads();
    double t[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = threadIdx.x; c < sl.len; c += HM_M) {
        double a = 0.0, b = 0.0, g = 0.0;
        for (int k = 0; k < K; ++k) {
            const int64_t at = (int64_t)k * n + sl.p0 + c;
            const double r = R[at];
            a = a + r * dist[at];
            b = b + (r > 0.0 ? r * log(r) : 0.0);
            g = g + r * lk[k];
        }
        t[0] = t[0] + a;
        t[1] = t[1] + b;
        t[2] = t[2] + g;
    }
    hm_slice_sum4(t, pair);
    if (threadIdx.x == 0)
        for (int x = 0; x < 3; ++x) objpart[(int64_t)blockIdx.x * 3 + x] = t[x];
}

// out[g][e] = 0.0 + part[s][e] over the slices s of group g, [64 g, 64 g + 64), in slice order.  grid (groups, ceil(E / 256))
__global__ __launch_bounds__(256) void k_hm_fold(const double *__restrict__ part, int n_slices, int E, double *__restrict__ out)
{
    const int e = blockIdx.y * 256 + threadIdx.x, g = blockIdx.x;
    if (e >= E) return;
    const int q1 = (g + 1) * HM_GROUP < n_slices ? (g + 1) * HM_GROUP : n_slices;
    double s = 0.0;
#pragma unroll 8
    for (int q = g * HM_GROUP; q < q1; ++q) s = s + part[(int64_t)q * E + e];
    out[(int64_t)g * E + e] = s;
}

// one workgroup: the three terms over the slice groups in group order, then the objective
__global__ __launch_bounds__(64) void k_hm_objective_sum(const double *__restrict__ objpart, int n_groups, double sigma, double theta,
                                                         double *__restrict__ out)
{
    __shared__ double t[3];
    if (threadIdx.x < 3) {
        double s = 0.0;
        for (int q = 0; q < n_groups; ++q) s = s + objpart[(int64_t)q * 3 + threadIdx.x];
        t[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) out[0] = t[0] + sigma * t[1] + (sigma * theta) * t[2];
}

// part[slice][k][j] = sum over the slice's cells of R[k][p] X[p][j]: the cells are summed in chunks of 32
__global__ __launch_bounds__(HM_TPB) void k_hm_rtz(const HmSlice *__restrict__ slices, const double *__restrict__ R,
                                                   const double *__restrict__ X, int64_t n, int d, int K, double *__restrict__ part)
{
    __shared__ __attribute__((aligned(16))) double As[HM_CH * HM_LDA], Bs[HM_CH * HM_LDD];
    const HmSlice sl = slices[blockIdx.x];
    int mt[2], nt[2];
    bool on[2];
    double acc[2][4][4];
    hm_tiles<2>((K + 3) / 4, (d + 3) / 4, mt, nt, on, acc);
    for (int c0 = 0; c0 < sl.len; c0 += HM_CH) {
        for (int e = threadIdx.x; e < HM_CH * HM_KMAX; e += HM_TPB) {
            const int c = e % HM_CH, k = e / HM_CH;
            As[c * HM_LDA + k] = (k < K && c0 + c < sl.len) ? R[(int64_t)k * n + sl.p0 + c0 + c] : 0.0;
        }
        for (int e = threadIdx.x; e < HM_CH * HM_DMAX; e += HM_TPB) {
            const int j = e % HM_DMAX, c = e / HM_DMAX;
            Bs[c * HM_LDD + j] = (j < d && c0 + c < sl.len) ? X[(sl.p0 + c0 + c) * d + j] : 0.0;
        }
        __syncthreads();
        hm_mac<2>(As, HM_LDA, Bs, HM_LDD, HM_CH, mt, nt, on, acc);
        __syncthreads();
    }
    double *out = part + (int64_t)blockIdx.x * K * d;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        if (!on[p]) continue;
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                const int k = 4 * mt[p] + x, j = 4 * nt[p] + y;
                if (k < K && j < d) out[k * d + j] = acc[p][x][y];
            }
    }
}

// one workgroup of 64 per cluster: Y_k = the normalised sum of the slice groups' part[.][k], groups in order
__global__ __launch_bounds__(64) void k_hm_centres(const double *__restrict__ part, int n_groups, int d, int K, double *__restrict__ Y)
{
    __shared__ double v[HM_DMAX];
    __shared__ double norm;
    const int k = blockIdx.x, j = threadIdx.x;
    if (j < d) {
        double s = 0.0;
        for (int q = 0; q < n_groups; ++q) s = s + part[((int64_t)q * K + k) * d + j];
        v[j] = s;
    }
    __syncthreads();
    if (j == 0) {
        double q = 0.0;
        for (int x = 0; x < d; ++x) q = q + v[x] * v[x];
        norm = sqrt(q);
    }
    __syncthreads();
    if (j < d && norm > 0.0) Y[k * d + j] = v[j] / norm;
}

// one workgroup of 64 per cluster: r_b from the slices' part[.][k] (of R^T Z), then the arrowhead system in closed form
__global__ __launch_bounds__(64) void k_hm_ridge(const int32_t *__restrict__ seg_first, const double *__restrict__ part,
                                                 const double *__restrict__ otot, int nb, int d, int K, int B, double lamb,
                                                 double *__restrict__ rb, double *__restrict__ W)
{
    const int k = blockIdx.x, j = threadIdx.x;
    if (j >= d) return;
    double r0 = 0.0, t = 0.0, s = 0.0, u = 0.0;
    for (int b = 0; b < B; ++b) {
        double r = 0.0;
        for (int blk = 0; blk < nb; ++blk)
#pragma unroll 8
            for (int q = seg_first[blk * B + b]; q < seg_first[blk * B + b + 1]; ++q) r = r + part[((int64_t)q * K + k) * d + j];
        rb[((int64_t)k * B + b) * d + j] = r;
        const double o = otot[k * B + b];
        r0 = r0 + r;
        t = t + o * r / (o + lamb);
        s = s + o;
        u = u + o * o / (o + lamb);
    }
    const double w0 = s - u > 0.0 ? (r0 - t) / (s - u) : 0.0;   // a cluster without mass corrects nothing
    for (int b = 0; b < B; ++b) {
        const double o = otot[k * B + b];
        W[((int64_t)k * B + b) * d + j] = (rb[((int64_t)k * B + b) * d + j] - o * w0) / (o + lamb);
    }
}

// Zcorr[p] = Z[p] - sum_k R[k][p] W[k][batch]: a workgroup owns a slice, 128 positions at a time; the clusters in chunks of 32
__global__ __launch_bounds__(HM_TPB) void k_hm_apply(const HmSlice *__restrict__ slices, const double *__restrict__ R,
                                                     const double *__restrict__ W, const double *__restrict__ Z, int64_t n, int d,
                                                     int K, int B, double *__restrict__ Zcorr)
{
    __shared__ __attribute__((aligned(16))) double As[HM_CH * HM_LDA], Bs[HM_CH * HM_LDD];
    const HmSlice sl = slices[blockIdx.x];
    for (int m0 = 0; m0 < sl.len; m0 += HM_M) {
        const int cells = sl.len - m0 < HM_M ? sl.len - m0 : HM_M;
        const int64_t p0 = sl.p0 + m0;
        int mt[2], nt[2];
        bool on[2];
        double acc[2][4][4];
        hm_tiles<2>(HM_M / 4, (d + 3) / 4, mt, nt, on, acc);
        for (int k0 = 0; k0 < K; k0 += HM_CH) {
            for (int e = threadIdx.x; e < HM_CH * HM_M; e += HM_TPB) {
                const int c = e % HM_M, k = e / HM_M;
                As[k * HM_LDA + c] = (c < cells && k0 + k < K) ? R[(int64_t)(k0 + k) * n + p0 + c] : 0.0;
            }
            for (int e = threadIdx.x; e < HM_CH * HM_DMAX; e += HM_TPB) {
                const int j = e % HM_DMAX, k = e / HM_DMAX;
                Bs[k * HM_LDD + j] = (j < d && k0 + k < K) ? W[((int64_t)(k0 + k) * B + sl.batch) * d + j] : 0.0;
            }
            __syncthreads();
            hm_mac<2>(As, HM_LDA, Bs, HM_LDD, HM_CH, mt, nt, on, acc);
            __syncthreads();
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            if (!on[p]) continue;
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
                for (int y = 0; y < 4; ++y) {
                    const int c = 4 * mt[p] + x, j = 4 * nt[p] + y;
                    if (c < cells && j < d) Zcorr[(p0 + c) * d + j] = Z[(p0 + c) * d + j] - acc[p][x][y];
                }
        }
    }
}

template <class V>
int hm_check_rows(const char *who, const char *what, const V *X, int64_t rows, int d)
{
    for (int64_t i = 0; i < rows; ++i) {
        bool any = false;
        for (int j = 0; j < d; ++j) {
            const double v = (double)X[i * d + j];
            SC_REQUIRE(std::isfinite(v), SC_ERR_INVALID, "%s: %s[%lld][%d] is not finite", who, what, (long long)i, j);
            any = any || v != 0.0;
        }
        SC_REQUIRE(any, SC_ERR_INVALID, "%s: row %lld of %s is all zero", who, (long long)i, what);
    }
    return SC_OK;
}

}  // namespace

// the problem resident between sc_harmony_begin and sc_harmony_end
struct HarmonyState : Resident {
    int64_t n = 0;
    int d = 0, K = 0, B = 0, nb = 0, n_slices = 0, n_groups = 0;   // groups of 64 consecutive slices (k_hm_fold)
    double sigma = 0.0, theta = 0.0, lamb = 0.0;
    std::vector<int64_t> order;             // position -> cell
    std::vector<int32_t> blk_first;         // [nb + 1] first slice of every block
    DBuf Z, Zc, Zcorr, dist, S, R, Y, inv_sum, slices, seg_first, pr, opart, oblk, pen, otot, lratio, objpart, obj, part, fold, rb, W;
};
static HarmonyState *hm_state(const sc_ctx *c) { return resident<HarmonyState>(c->harmony); }

namespace {

// the end-of-round tables and the objective into obj[slot]
void hm_enqueue_objective(sc_ctx *c, HarmonyState &s, int rebuild, int slot)
{
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(k_hm_tables, dim3((unsigned)s.K), dim3(64), 0, st, s.seg_first.as<int32_t>(), s.opart.as<double>(), s.pr.as<double>(), s.nb, s.K,
                       s.B, rebuild, s.nb, s.theta, s.oblk.as<double>(), s.pen.as<double>(), s.otot.as<double>(), s.lratio.as<double>());
    hipLaunchKernelGGL(k_hm_objective, dim3((unsigned)s.n_slices), dim3(HM_M), 0, st, s.slices.as<HmSlice>(), s.R.as<double>(),
                       s.dist.as<double>(), s.lratio.as<double>(), s.n, s.K, s.B, s.objpart.as<double>());
    hipLaunchKernelGGL(k_hm_fold, dim3((unsigned)s.n_groups, 1), dim3(256), 0, st, s.objpart.as<double>(), s.n_slices, 3, s.fold.as<double>());
    hipLaunchKernelGGL(k_hm_objective_sum, dim3(1), dim3(64), 0, st, s.fold.as<double>(), s.n_groups, s.sigma, s.theta,
                       s.obj.as<double>() + slot);
}

void hm_enqueue_dist(sc_ctx *c, HarmonyState &s, int init)
{
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(k_hm_dist, dim3((unsigned)ceil_div64(s.n, HM_M)), dim3(HM_TPB), 0, st, s.Zc.as<double>(), s.Y.as<double>(), s.n, s.d,
                       s.K, s.dist.as<double>());
    hipLaunchKernelGGL(k_hm_soft, dim3((unsigned)ceil_div64(s.n, 256)), dim3(256), 0, st, s.dist.as<double>(), s.n, s.K, 1.0 / s.sigma, init,
                       s.S.as<double>(), s.R.as<double>());
}

// one clustering round: 9 + 2 n_blocks launches
void hm_enqueue_round(sc_ctx *c, HarmonyState &s, int slot)
{
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(k_hm_rtz, dim3((unsigned)s.n_slices), dim3(HM_TPB), 0, st, s.slices.as<HmSlice>(), s.R.as<double>(), s.Zc.as<double>(),
                       s.n, s.d, s.K, s.part.as<double>());
    hipLaunchKernelGGL(k_hm_fold, dim3((unsigned)s.n_groups, (unsigned)((s.K * s.d + 255) / 256)), dim3(256), 0, st, s.part.as<double>(), s.n_slices,
                       s.K * s.d, s.fold.as<double>());
    hipLaunchKernelGGL(k_hm_centres, dim3((unsigned)s.K), dim3(64), 0, st, s.fold.as<double>(), s.n_groups, s.d, s.K, s.Y.as<double>());
    hm_enqueue_dist(c, s, 0);
    for (int t = 0; t < s.nb; ++t) {
        hipLaunchKernelGGL(k_hm_tables, dim3((unsigned)s.K), dim3(64), 0, st, s.seg_first.as<int32_t>(), s.opart.as<double>(), s.pr.as<double>(), s.nb,
                           s.K, s.B, t - 1, t, s.theta, s.oblk.as<double>(), s.pen.as<double>(), s.otot.as<double>(), s.lratio.as<double>());
        hipLaunchKernelGGL(k_hm_block, dim3((unsigned)(s.blk_first[t + 1] - s.blk_first[t])), dim3(HM_M), 0, st, s.slices.as<HmSlice>(),
                           s.blk_first[t], s.S.as<double>(), s.pen.as<double>(), s.n, s.K, s.B, s.R.as<double>(), s.inv_sum.as<double>(),
                           s.opart.as<double>());
    }
    hm_enqueue_objective(c, s, s.nb - 1, slot);
}

}  // namespace

extern "C" int sc_harmony_begin(sc_ctx *c, const void *Z, int dtype, int64_t n, int32_t d, const int32_t *batch, int32_t n_batches,
                                const double *Y, int32_t K, int32_t n_blocks, double sigma, double theta, double lamb,
                                double *objective_out)
{
    const char *who = "sc_harmony_begin";
    SC_REQUIRE(c && Z && batch && Y && objective_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "%s: dtype must be SC_F32 or SC_F64", who);
    SC_REQUIRE(n >= 2 && n <= INT32_MAX, SC_ERR_INVALID, "%s: need 2 <= n <= 2^31 - 1, got %lld", who, (long long)n);
    SC_REQUIRE(d >= 1 && d <= HM_DMAX, SC_ERR_INVALID, "%s: need 1 <= d <= %d, got %d", who, HM_DMAX, d);
    SC_REQUIRE(K >= 2 && K <= HM_KMAX && K <= n, SC_ERR_INVALID, "%s: need 2 <= K <= min(%d, n), got %d", who, HM_KMAX, K);
    SC_REQUIRE(n_batches >= 2 && n_batches <= HM_BMAX, SC_ERR_INVALID, "%s: need 2 <= n_batches <= %d, got %d", who, HM_BMAX, n_batches);
    SC_REQUIRE(n_blocks >= 1 && n_blocks <= HM_NBMAX && n_blocks <= n, SC_ERR_INVALID, "%s: need 1 <= n_blocks <= min(%d, n), got %d", who,
               HM_NBMAX, n_blocks);
    SC_REQUIRE(sigma > 0.0 && std::isfinite(sigma), SC_ERR_INVALID, "%s: sigma must be finite and > 0", who);
    SC_REQUIRE(theta >= 0.0 && std::isfinite(theta), SC_ERR_INVALID, "%s: theta must be finite and >= 0", who);
    SC_REQUIRE(lamb > 0.0 && std::isfinite(lamb), SC_ERR_INVALID, "%s: lamb must be finite and > 0", who);
    const int B = n_batches, nb = n_blocks;
    std::vector<int64_t> batch_n(B, 0);
    for (int64_t i = 0; i < n; ++i) {
        SC_REQUIRE(batch[i] >= 0 && batch[i] < B, SC_ERR_INVALID, "%s: batch[%lld] = %d is outside [0, %d)", who, (long long)i, batch[i], B);
        ++batch_n[batch[i]];
    }
    for (int b = 0; b < B; ++b) SC_REQUIRE(batch_n[b] >= 1, SC_ERR_INVALID, "%s: batch %d has no cell", who, b);
    SC_TRY(dtype == SC_F32 ? hm_check_rows(who, "Z", (const float *)Z, n, d) : hm_check_rows(who, "Z", (const double *)Z, n, d));
    SC_TRY(hm_check_rows(who, "Y", Y, K, d));

    // the sort by (block, batch, cell) as a counting sort, and the slices of every segment
    std::vector<int64_t> seg_n((size_t)nb * B + 1, 0);
    for (int64_t i = 0; i < n; ++i) ++seg_n[(size_t)(i % nb) * B + batch[i] + 1];
    for (size_t q = 1; q < seg_n.size(); ++q) seg_n[q] += seg_n[q - 1];   // now: first position of every segment
    std::vector<int64_t> order((size_t)n);
    {
        std::vector<int64_t> cursor(seg_n.begin(), seg_n.end() - 1);
        for (int64_t i = 0; i < n; ++i) order[(size_t)cursor[(size_t)(i % nb) * B + batch[i]]++] = i;
    }
    const int64_t slice_cells = hm_slice_cells(n);
    std::vector<HmSlice> slices;
    std::vector<int32_t> seg_first((size_t)nb * B + 1, 0), blk_first((size_t)nb + 1, 0);
    for (int t = 0; t < nb; ++t) {
        blk_first[t] = (int32_t)slices.size();
        for (int b = 0; b < B; ++b) {
            seg_first[(size_t)t * B + b] = (int32_t)slices.size();
            const int64_t e = seg_n[(size_t)t * B + b + 1];
            for (int64_t p = seg_n[(size_t)t * B + b]; p < e; p += slice_cells)
                slices.push_back(HmSlice{p, (int32_t)(e - p < slice_cells ? e - p : slice_cells), b});
        }
    }
    seg_first[(size_t)nb * B] = blk_first[nb] = (int32_t)slices.size();
    std::vector<double> zs((size_t)n * d), pr(B);
    for (int64_t p = 0; p < n; ++p)
        for (int j = 0; j < d; ++j)
            zs[(size_t)p * d + j] = dtype == SC_F32 ? (double)((const float *)Z)[order[p] * d + j] : ((const double *)Z)[order[p] * d + j];
    for (int b = 0; b < B; ++b) pr[b] = (double)batch_n[b] / (double)n;

    SC_HIP(hipSetDevice(c->device));
    sc_resident_drop(c, c->harmony);
    c->harmony.reset(new HarmonyState());
    HarmonyState &s = *hm_state(c);
    s.n = n, s.d = d, s.K = K, s.B = B, s.nb = nb, s.n_slices = (int)slices.size();
    s.n_groups = (s.n_slices + HM_GROUP - 1) / HM_GROUP;
    s.sigma = sigma, s.theta = theta, s.lamb = lamb;
    s.order = std::move(order);
    s.blk_first = std::move(blk_first);
    const size_t nd = sizeof(double) * (size_t)n * d, nk = sizeof(double) * (size_t)n * K, kb = sizeof(double) * (size_t)K * B;
    struct { DBuf *b; size_t bytes; } want[] = {
        {&s.Z, nd}, {&s.Zc, nd}, {&s.Zcorr, nd}, {&s.dist, nk}, {&s.S, nk}, {&s.R, nk}, {&s.Y, sizeof(double) * (size_t)K * d},
        {&s.inv_sum, sizeof(double) * (size_t)n}, {&s.slices, sizeof(HmSlice) * slices.size()}, {&s.seg_first, sizeof(int32_t) * seg_first.size()},
        {&s.pr, sizeof(double) * (size_t)B}, {&s.opart, sizeof(double) * slices.size() * K}, {&s.oblk, kb * (size_t)nb}, {&s.pen, kb},
        {&s.otot, kb}, {&s.lratio, kb}, {&s.objpart, sizeof(double) * slices.size() * 3}, {&s.obj, sizeof(double) * 4096},
        {&s.part, sizeof(double) * slices.size() * K * d}, {&s.fold, sizeof(double) * (size_t)s.n_groups * (K * d > 3 ? K * d : 3)}, {&s.rb, kb * (size_t)d}, {&s.W, kb * (size_t)d}};
    for (auto &w : want) {
        const int rc = w.b->ensure(w.bytes, &c->mem);
        if (rc != SC_OK) {
            sc_resident_drop(c, c->harmony);
            return rc;
        }
    }
    hipStream_t st = c->stream;
    bool ok = hipMemcpyAsync(s.Z.p, zs.data(), nd, hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(s.Zcorr.p, zs.data(), nd, hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(s.Y.p, Y, sizeof(double) * (size_t)K * d, hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(s.slices.p, slices.data(), sizeof(HmSlice) * slices.size(), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(s.seg_first.p, seg_first.data(), sizeof(int32_t) * seg_first.size(), hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemcpyAsync(s.pr.p, pr.data(), sizeof(double) * (size_t)B, hipMemcpyHostToDevice, st) == hipSuccess;
    ok = ok && hipMemsetAsync(s.W.p, 0, kb * (size_t)d, st) == hipSuccess && hipMemsetAsync(s.rb.p, 0, kb * (size_t)d, st) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(k_hm_normalise, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, st, s.Z.as<double>(), n, d, s.Zc.as<double>());
        hipLaunchKernelGGL(k_hm_normalise, dim3((unsigned)ceil_div64(K, 256)), dim3(256), 0, st, s.Y.as<double>(), (int64_t)K, d, s.Y.as<double>());
        hm_enqueue_dist(c, s, 1);
        hipLaunchKernelGGL(k_hm_slice_mass, dim3((unsigned)s.n_slices), dim3(HM_M), 0, st, s.slices.as<HmSlice>(), s.R.as<double>(), n, K,
                           s.opart.as<double>());
        for (int t = 0; t < nb; ++t)
            hipLaunchKernelGGL(k_hm_tables, dim3((unsigned)s.K), dim3(64), 0, st, s.seg_first.as<int32_t>(), s.opart.as<double>(), s.pr.as<double>(), nb, K, B,
                               t, -1, theta, s.oblk.as<double>(), s.pen.as<double>(), s.otot.as<double>(), s.lratio.as<double>());
        hm_enqueue_objective(c, s, -1, 0);
        ok = hipGetLastError() == hipSuccess;
        ok = ok && hipMemcpyAsync(objective_out, s.obj.p, sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess;
    }
    if (!ok || hipStreamSynchronize(st) != hipSuccess) {   // the host arrays are free again
        sc_set_error("%s: failed on the device: %s", who, hipGetErrorString(hipGetLastError()));
        sc_resident_drop(c, c->harmony);
        return SC_ERR_HIP;
    }
    return SC_OK;
}

extern "C" int sc_harmony_cluster(sc_ctx *c, int32_t max_iter, double epsilon, int32_t *rounds_out, double *objectives_out)
{
    const char *who = "sc_harmony_cluster";
    SC_REQUIRE(c && rounds_out && objectives_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(max_iter >= 1 && max_iter <= 4096, SC_ERR_INVALID, "%s: need 1 <= max_iter <= 4096, got %d", who, max_iter);
    SC_REQUIRE(!std::isnan(epsilon), SC_ERR_INVALID, "%s: epsilon is NaN", who);
    SC_REQUIRE(c->harmony, SC_ERR_STATE, "%s: no problem is resident (sc_harmony_begin)", who);
    HarmonyState &s = *hm_state(c);
    SC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    int done = 0;
    if (epsilon < 0.0) {   // the full count: nothing comes back before the end
        for (int r = 0; r < max_iter; ++r) hm_enqueue_round(c, s, r);
        SC_HIP(hipGetLastError());
        SC_HIP(hipMemcpyAsync(objectives_out, s.obj.p, sizeof(double) * (size_t)max_iter, hipMemcpyDeviceToHost, st));
        SC_HIP(hipStreamSynchronize(st));
        done = max_iter;
    } else {
        for (int r = 0; r < max_iter; ++r) {
            hm_enqueue_round(c, s, r);
            SC_HIP(hipGetLastError());
            SC_HIP(hipMemcpyAsync(objectives_out + r, s.obj.as<double>() + r, sizeof(double), hipMemcpyDeviceToHost, st));
            SC_HIP(hipStreamSynchronize(st));
            done = r + 1;
            if (r > 3) {   // harmonypy's rule: windows of 3 rounds, one round apart
                const double *o = objectives_out;
                const double older = o[r - 1] + o[r - 2] + o[r - 3], newer = o[r] + o[r - 1] + o[r - 2];
                if (fabs(older - newer) / fabs(older) < epsilon) break;
            }
        }
    }
    *rounds_out = done;
    return SC_OK;
}

extern "C" int sc_harmony_correct(sc_ctx *c)
{
    const char *who = "sc_harmony_correct";
    SC_REQUIRE(c, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(c->harmony, SC_ERR_STATE, "%s: no problem is resident (sc_harmony_begin)", who);
    HarmonyState &s = *hm_state(c);
    SC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // otot = the sum of the tables as they stand (after begin and after every round k_hm_tables left exactly that)
    hipLaunchKernelGGL(k_hm_rtz, dim3((unsigned)s.n_slices), dim3(HM_TPB), 0, st, s.slices.as<HmSlice>(), s.R.as<double>(), s.Z.as<double>(), s.n,
                       s.d, s.K, s.part.as<double>());
    hipLaunchKernelGGL(k_hm_ridge, dim3((unsigned)s.K), dim3(64), 0, st, s.seg_first.as<int32_t>(), s.part.as<double>(), s.otot.as<double>(), s.nb,
                       s.d, s.K, s.B, s.lamb, s.rb.as<double>(), s.W.as<double>());
    hipLaunchKernelGGL(k_hm_apply, dim3((unsigned)s.n_slices), dim3(HM_TPB), 0, st, s.slices.as<HmSlice>(), s.R.as<double>(), s.W.as<double>(),
                       s.Z.as<double>(), s.n, s.d, s.K, s.B, s.Zcorr.as<double>());
    hipLaunchKernelGGL(k_hm_normalise, dim3((unsigned)ceil_div64(s.n, 256)), dim3(256), 0, st, s.Zcorr.as<double>(), s.n, s.d, s.Zc.as<double>());
    SC_HIP(hipGetLastError());
    SC_HIP(hipStreamSynchronize(st));
    return SC_OK;
}

extern "C" int sc_harmony_get(sc_ctx *c, int32_t what, void *out)
{
    const char *who = "sc_harmony_get";
    SC_REQUIRE(c && out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(what >= SC_HARMONY_ZCORR && what <= SC_HARMONY_DIST, SC_ERR_INVALID, "%s: unknown array %d", who, what);
    SC_REQUIRE(c->harmony, SC_ERR_STATE, "%s: no problem is resident (sc_harmony_begin)", who);
    HarmonyState &s = *hm_state(c);
    const int64_t n = s.n;
    const int d = s.d, K = s.K, B = s.B;
    if (what == SC_HARMONY_ORDER) {
        memcpy(out, s.order.data(), sizeof(int64_t) * (size_t)n);
        return SC_OK;
    }
    SC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const DBuf *src = nullptr;
    size_t count = 0;
    switch (what) {
    case SC_HARMONY_ZCORR: src = &s.Zcorr, count = (size_t)n * d; break;
    case SC_HARMONY_ZC: src = &s.Zc, count = (size_t)n * d; break;
    case SC_HARMONY_R: src = &s.R, count = (size_t)n * K; break;
    case SC_HARMONY_DIST: src = &s.dist, count = (size_t)n * K; break;
    case SC_HARMONY_Y: src = &s.Y, count = (size_t)K * d; break;
    case SC_HARMONY_O: src = &s.oblk, count = (size_t)s.nb * K * B; break;
    default: src = &s.W, count = (size_t)K * B * d; break;
    }
    double *dst = (double *)out;
    if (what == SC_HARMONY_Y || what == SC_HARMONY_O || what == SC_HARMONY_W) {
        SC_HIP(hipMemcpyAsync(dst, src->p, sizeof(double) * count, hipMemcpyDeviceToHost, st));
        SC_HIP(hipStreamSynchronize(st));
        return SC_OK;
    }
    std::vector<double> tmp(count);   // per position: back to the caller's cell order (and to [cell][k])
    SC_HIP(hipMemcpyAsync(tmp.data(), src->p, sizeof(double) * count, hipMemcpyDeviceToHost, st));
    SC_HIP(hipStreamSynchronize(st));
    if (what == SC_HARMONY_R || what == SC_HARMONY_DIST) {
        for (int k = 0; k < K; ++k)
            for (int64_t p = 0; p < n; ++p) dst[s.order[p] * K + k] = tmp[(size_t)k * n + p];
    } else {
        for (int64_t p = 0; p < n; ++p) memcpy(dst + s.order[p] * d, tmp.data() + (size_t)p * d, sizeof(double) * (size_t)d);
    }
    return SC_OK;
}

extern "C" int sc_harmony_end(sc_ctx *c)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "sc_harmony_end: null pointer");
    if (!c->harmony) return SC_OK;
    SC_HIP(hipSetDevice(c->device));
    sc_resident_drop(c, c->harmony);
    return SC_OK;
}
