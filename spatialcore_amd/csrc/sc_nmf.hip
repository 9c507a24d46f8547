// sc_nmf.hip -- sc_nmf_fit: sklearn 1.7.2 NMF(solver="mu") on a sparse cells x genes matrix, Frobenius and
// Kullback-Leibler losses (decomposition/_nmf.py: _fit_multiplicative_update with gamma = 1, no regularisation).
// DESIGN.md 4.6l; restated in the same order by tests/nmf_restated.py.
//
// fp64 throughout, -ffp-contract=off, no floating-point atomics: the factors involve + x / only and are a function of
// the arguments alone.  ONE summation order per sum:
//  - over a row's stored entries, over a column chunk's stored entries, over genes and over components: index order
//    (a running sum that starts at 0);
//  - the K-term dot (W H)_ig of the Kullback-Leibler quotient and of the errors: the K products W_ik H_kg, padded with
//    zeros to Kp = K rounded up to a power of two, added as the adjacent-pair tree (lane l takes lane l ^ 1, then
//    l ^ 2, ...: every lane of the group ends with the same bits, since a + b = b + a);
//  - over a gene column's stored entries: chunks of COL_CHUNK = 512 entries (rows ascending), each in index order
//    from 0, the chunk sums added in chunk order;
//  - over cells (W^T W, colsum(W), the per-cell error terms): chunks of NMF_CELL_CHUNK = 1024 cells, each in index
//    order from 0, the chunk sums added in chunk order;
//  - sum x^2 and sum x over the stored entries: on the host, in index order.
// None of this depends on the grid or on how many workgroups are resident.
//
// sc_nmf_fit_graph (graph-regularised NMF, Cai et al. 2011; restated by
// tests/spatial_nmf_restated.py) is the same loop with the Frobenius loss, H updated, and a Laplacian term in the W pass:
//  - d_i = sum_e a_e (once, in set-up) and g_ik = sum_e a_e Wold[j_e][k]: the graph row's stored entries in index order
//    from 0 (lane_group_walk with the neighbour's W row as the operand row);
//  - num = nx + lambda g, den = dx + (lambda d_i) w, nx and dx the plain pass's; den == 0 -> EPS; Wnew = w (num / den);
//  - every row reads the W of the previous iteration (Jacobi), so the pass reads one W buffer and writes the other; the
//    plain pass reads and writes the same one, which is correct only because its rows are independent;
//  - penalty: r_i = sum_e a_e T_k((w_ik - w_jk)^2), T the adjacent-pair tree over the Kp lanes (dead lanes hold 0), the
//    cells added in chunks of 1024 as the row errors are; tr(W^T L W) = R / 2; F = D + (lambda (R / 2)) / 2;
//  - with lambda = 0 every added term is + 0 x finite: the factors are sc_nmf_fit's byte for byte.
//
// Lanes = components: a group of Kp lanes serves one row (W pass, error pass), one column chunk (H pass) or one gene
// (H finish); a workgroup of 256 threads holds 256 / Kp groups.
#include <cmath>
#include <vector>

#include "sc_colsort.h"
#include "sc_csr_input.h"
#include "sc_ctx.h"
#include "sc_lane_group.h"

namespace {

constexpr int NMF_TPB = 256;
constexpr int NMF_KMAX = 64;
constexpr int NMF_CELL_CHUNK = 1024;   // cells per partial of the sums over cells
constexpr int NMF_TILE = 64;           // cells of W staged in LDS at a time by k_nmf_cellsums
constexpr double NMF_EPS = 1.1920928955078125e-07;   // 2^-23: sklearn's EPSILON (float32 eps)
constexpr double NMF_TINY = 2.220446049250313e-16;   // 2^-52: the Kullback-Leibler floor of H
enum { NMF_KL = 1, NMF_FRO = 2 };

// ---- set-up ------------------------------------------------------------------------------------------------------
// (the column-sorted copy and its chunk table: sc_colsort.h)
// per stored entry: its fp64 value
template <class T>
__global__ __launch_bounds__(256) void k_nmf_values(const T *__restrict__ data, int64_t nnz, double *__restrict__ val)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    val[p] = (double)data[p];
}
__global__ __launch_bounds__(256) void k_nmf_transpose(const double *__restrict__ H, int K, int G, double *__restrict__ Ht)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)K * G) return;
    const int g = (int)(t / K), k = (int)(t % K);
    Ht[t] = H[(int64_t)k * G + g];
}

// deg[i] = the graph row's stored weights in index order from 0 (one thread per row)
__global__ __launch_bounds__(256) void k_nmf_degree(const int64_t *__restrict__ gptr, const double *__restrict__ gval, int64_t n,
                                                    double *__restrict__ deg)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double d = 0.0;
    for (int64_t p = gptr[i]; p < gptr[i + 1]; ++p) d = d + gval[p];
    deg[i] = d;
}

// ---- per iteration -----------------------------------------------------------------------------------------------
// grid K, 64 threads: HHt[k][k'] = sum_g H[k][g] H[k'][g] and Hsum[k] = sum_g H[k][g], genes in index order (reads H^T)
__global__ __launch_bounds__(64) void k_nmf_hprep(const double *__restrict__ Ht, int K, int G, double *__restrict__ HHt,
                                                  double *__restrict__ Hsum)
{
    const int k = blockIdx.x, k2 = threadIdx.x;
    if (k2 >= K) return;
    double s = 0.0, r = 0.0;
    for (int g = 0; g < G; ++g) {
        const double a = Ht[(int64_t)g * K + k];
        s = s + a * Ht[(int64_t)g * K + k2];
        r = r + a;
    }
    HHt[k * K + k2] = s;
    if (k2 == 0) Hsum[k] = r;
}

// W pass: one group per row.  Frobenius: W_ik <- W_ik ((X H^T)_ik / (W (H H^T))_ik); Kullback-Leibler: W_ik <- W_ik
// ((Q H^T)_ik / rowsum(H)_k), q = x / max((W H)_ig, EPS) at the row's stored entries.  A denominator of 0 becomes EPS.
// GRAPH (Frobenius only): num + lambda (A Wold)_ik over lambda d_i w added to the denominator; the neighbours' rows are
// read from Wold, so Wnew must be another buffer.  Without GRAPH the graph arguments are unused and Wold == Wnew (a row
// is read by its own group before that group writes it, and by nobody else): hence no __restrict__ on the two.
// Dynamic LDS: Frobenius K * K (H H^T) + 256 (the workgroup's W rows) doubles.
template <int LOSS, bool GRAPH>
__global__ __launch_bounds__(256) void k_nmf_w(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                               const double *__restrict__ val, int64_t n, int K, int kp,
                                               const double *__restrict__ Ht, const double *__restrict__ HHt,
                                               const double *__restrict__ Hsum, const int64_t *__restrict__ gptr,
                                               const int32_t *__restrict__ gidx, const double *__restrict__ gval,
                                               const double *__restrict__ deg, double lambda, const double *Wold, double *Wnew)
{
    static_assert(!GRAPH || LOSS == NMF_FRO, "the graph term is a multiplicative update for the Frobenius loss only");
    extern __shared__ double nmf_lds[];
    const int t = threadIdx.x, grp = t / kp, k = t % kp;
    const int64_t i = (int64_t)blockIdx.x * (NMF_TPB / kp) + grp;
    const bool live = i < n && k < K;
    const double w = live ? Wold[i * K + k] : 0.0;
    if (LOSS == NMF_FRO) {
        for (int q = t; q < K * K; q += NMF_TPB) nmf_lds[q] = HHt[q];
        nmf_lds[K * K + t] = w;
        __syncthreads();
    }
    double num = 0.0, gw = 0.0;
    if (i < n) {   // uniform over the group, whose lanes walk the row together
        auto add = [&](double x, double h) {
            if (LOSS == NMF_FRO) {
                num = num + x * h;
            } else {
                double d = group_sum(w * h, kp);
                d = d < NMF_EPS ? NMF_EPS : d;
                num = num + (x / d) * h;
            }
        };
        auto row_of = [&](int32_t g) { return k < K ? Ht[(int64_t)g * K + k] : 0.0; };
        lane_group_walk(indices, val, indptr[i], indptr[i + 1], kp, k, row_of, add);   // four H^T rows in flight
        if (GRAPH) {
            auto gadd = [&](double a, double wj) { gw = gw + a * wj; };
            auto wrow_of = [&](int32_t j) { return k < K ? Wold[(int64_t)j * K + k] : 0.0; };
            lane_group_walk(gidx, gval, gptr[i], gptr[i + 1], kp, k, wrow_of, gadd);   // four neighbours' W rows in flight
        }
    }
    if (!live) return;
    double den;
    if (LOSS == NMF_FRO) {
        const double *wrow = nmf_lds + K * K + grp * kp;
        den = 0.0;
        for (int j = 0; j < K; ++j) den = den + wrow[j] * nmf_lds[j * K + k];
    } else {
        den = Hsum[k];
    }
    if (GRAPH) {
        num = num + lambda * gw;
        den = den + (lambda * deg[i]) * w;
    }
    if (den == 0.0) den = NMF_EPS;
    Wnew[i * K + k] = w * (num / den);
}

// Sums over cells, one workgroup per chunk of 1024 cells: part[chunk][P], P = K * K entries (k, k') of W^T W (Frobenius) or
// P = K entries of colsum(W) (Kullback-Leibler); cells in index order.  Thread t owns the entries t, t + 256, ...
template <int LOSS>
__global__ __launch_bounds__(256) void k_nmf_cellsums(const double *__restrict__ W, int64_t n, int K, double *__restrict__ part)
{
    __shared__ double tile[NMF_TILE * NMF_KMAX];
    const int t = threadIdx.x;
    const int P = LOSS == NMF_FRO ? K * K : K;
    const int64_t c0 = (int64_t)blockIdx.x * NMF_CELL_CHUNK;
    const int64_t c1 = c0 + NMF_CELL_CHUNK < n ? c0 + NMF_CELL_CHUNK : n;
    double acc[NMF_KMAX * NMF_KMAX / NMF_TPB];
#pragma unroll
    for (int j = 0; j < NMF_KMAX * NMF_KMAX / NMF_TPB; ++j) acc[j] = 0.0;
    for (int64_t b = c0; b < c1; b += NMF_TILE) {
        const int cells = (int)(c1 - b < NMF_TILE ? c1 - b : NMF_TILE);
        __syncthreads();
        for (int q = t; q < cells * K; q += NMF_TPB) tile[q] = W[b * K + q];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NMF_KMAX * NMF_KMAX / NMF_TPB; ++j) {
            const int e = t + j * NMF_TPB;
            if (e < P) {
                const int ka = LOSS == NMF_FRO ? e / K : e, kb = LOSS == NMF_FRO ? e % K : 0;
                double a = acc[j];
                for (int cc = 0; cc < cells; ++cc)
                    a = LOSS == NMF_FRO ? a + tile[cc * K + ka] * tile[cc * K + kb] : a + tile[cc * K + ka];
                acc[j] = a;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NMF_KMAX * NMF_KMAX / NMF_TPB; ++j) {
        const int e = t + j * NMF_TPB;
        if (e < P) part[(int64_t)blockIdx.x * P + e] = acc[j];
    }
}

// H pass: one group per column chunk; part[chunk][k] = sum over the chunk's entries of W_ik x (Frobenius: W^T X) or
// W_ik q with q = x / max((W H)_ig, EPS) (Kullback-Leibler: W^T Q), W the updated one, H the current one
template <int LOSS>
__global__ __launch_bounds__(256) void k_nmf_h(const int64_t *__restrict__ colptr, const int32_t *__restrict__ crow,
                                               const double *__restrict__ cval, const int64_t *__restrict__ cptr,
                                               const int32_t *__restrict__ cgene, int64_t chunks, int K, int kp,
                                               const double *__restrict__ W, const double *__restrict__ Ht,
                                               double *__restrict__ part)
{
    const int t = threadIdx.x, grp = t / kp, k = t % kp;
    const int64_t c = (int64_t)blockIdx.x * (NMF_TPB / kp) + grp;
    if (c >= chunks) return;   // the whole group leaves
    const ColChunk ch = col_chunk(colptr, cptr, cgene, c);
    const double h = (LOSS == NMF_KL && k < K) ? Ht[(int64_t)ch.g * K + k] : 0.0;
    double acc = 0.0;
    auto add = [&](double x, double w) {
        if (LOSS == NMF_FRO) {
            acc = acc + w * x;
        } else {
            double d = group_sum(w * h, kp);
            d = d < NMF_EPS ? NMF_EPS : d;
            acc = acc + w * (x / d);
        }
    };
    auto row_of = [&](int32_t i) { return k < K ? W[(int64_t)i * K + k] : 0.0; };
    lane_group_walk(crow, cval, ch.p0, ch.p1, kp, k, row_of, add);   // four W rows in flight
    if (k < K) part[c * K + k] = acc;
}

// H finish: one group per gene.  Numerator = the gene's chunk sums in chunk order; Frobenius: H_kg <- H_kg (num /
// ((W^T W) H)_kg), 0 -> EPS; Kullback-Leibler: H_kg <- H_kg (num / colsum(W)_k), 0 -> 1, then values < 2^-52 become 0.
// Reads H (K x G), writes the other H buffer and its transpose.
template <int LOSS>
__global__ __launch_bounds__(256) void k_nmf_h_finish(const int64_t *__restrict__ cptr, const double *__restrict__ part, int G,
                                                      int K, int kp, const double *__restrict__ cellsum,
                                                      const double *__restrict__ H, double *__restrict__ Hn,
                                                      double *__restrict__ Htn)
{
    const int t = threadIdx.x, grp = t / kp, k = t % kp;
    const int64_t g = (int64_t)blockIdx.x * (NMF_TPB / kp) + grp;
    if (g >= G || k >= K) return;
    double num = 0.0;
    for (int64_t c = cptr[g]; c < cptr[g + 1]; ++c) num = num + part[c * K + k];
    double den;
    if (LOSS == NMF_FRO) {
        den = 0.0;
        for (int j = 0; j < K; ++j) den = den + cellsum[k * K + j] * H[(int64_t)j * G + g];
        if (den == 0.0) den = NMF_EPS;
    } else {
        den = cellsum[k];
        if (den == 0.0) den = 1.0;
    }
    double hn = H[(int64_t)k * G + g] * (num / den);
    if (LOSS == NMF_KL && hn < NMF_TINY) hn = 0.0;
    Hn[(int64_t)k * G + g] = hn;
    Htn[g * K + k] = hn;
}

// ---- error -------------------------------------------------------------------------------------------------------
// rowerr[i] = sum over the row's stored entries, in index order, of x (W H)_ig (Frobenius: the cross term) or, for x > EPS
// only, x log(x / max((W H)_ig, EPS)) (Kullback-Leibler)
template <int LOSS>
__global__ __launch_bounds__(256) void k_nmf_rowerr(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                    const double *__restrict__ val, int64_t n, int K, int kp,
                                                    const double *__restrict__ Ht, const double *__restrict__ W,
                                                    double *__restrict__ rowerr)
{
    const int t = threadIdx.x, grp = t / kp, k = t % kp;
    const int64_t i = (int64_t)blockIdx.x * (NMF_TPB / kp) + grp;
    if (i >= n) return;   // the whole group leaves
    const double w = k < K ? W[i * K + k] : 0.0;
    double s = 0.0;
    const int64_t p1 = indptr[i + 1];
    for (int64_t p = indptr[i]; p < p1; ++p) {
        const int32_t g = indices[p];
        const double x = val[p];
        const double h = k < K ? Ht[(int64_t)g * K + k] : 0.0;
        const double d = group_sum(w * h, kp);
        if (LOSS == NMF_FRO) {
            s = s + x * d;
        } else if (x > NMF_EPS) {
            s = s + x * log(x / (d < NMF_EPS ? NMF_EPS : d));
        }
    }
    if (k == 0) rowerr[i] = s;
}
// part[chunk] = the chunk's 1024 cells in index order (one thread per chunk)
__global__ __launch_bounds__(64) void k_nmf_rowerr_chunks(const double *__restrict__ rowerr, int64_t n, int64_t chunks,
                                                          double *__restrict__ part)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= chunks) return;
    const int64_t c0 = c * NMF_CELL_CHUNK;
    const int64_t c1 = c0 + NMF_CELL_CHUNK < n ? c0 + NMF_CELL_CHUNK : n;
    double s = 0.0;
    for (int64_t i = c0; i < c1; ++i) s = s + rowerr[i];
    part[c] = s;
}
// rowpen[i] = sum over the graph row's stored entries, in index order, of a (sum_k (w_ik - w_jk)^2), the K squares as the
// adjacent-pair tree (dead lanes hold 0 - 0)
__global__ __launch_bounds__(256) void k_nmf_penalty(const int64_t *__restrict__ gptr, const int32_t *__restrict__ gidx,
                                                     const double *__restrict__ gval, int64_t n, int K, int kp,
                                                     const double *__restrict__ W, double *__restrict__ rowpen)
{
    const int t = threadIdx.x, grp = t / kp, k = t % kp;
    const int64_t i = (int64_t)blockIdx.x * (NMF_TPB / kp) + grp;
    if (i >= n) return;   // the whole group leaves
    const double w = k < K ? W[i * K + k] : 0.0;
    double s = 0.0;
    const int64_t p1 = gptr[i + 1];
    for (int64_t p = gptr[i]; p < p1; ++p) {
        const int32_t j = gidx[p];
        const double a = gval[p];
        const double diff = w - (k < K ? W[(int64_t)j * K + k] : 0.0);
        s = s + a * group_sum(diff * diff, kp);
    }
    if (k == 0) rowpen[i] = s;
}
// D of the current factors.  Frobenius: D = ((sum x^2 + tr((W^T W)(H H^T))) - 2 cross) / 2; Kullback-Leibler: D = sum x
// log(x / WH) + (colsum(W) . rowsum(H) - sum x).  cellsum = W^T W or colsum(W), hsum = H H^T or rowsum(H).
template <int LOSS>
__device__ double nmf_divergence(const double *__restrict__ part, int64_t chunks, int K, const double *__restrict__ cellsum,
                                 const double *__restrict__ hsum, double xconst)
{
    double s = 0.0;
    for (int64_t c = 0; c < chunks; ++c) s = s + part[c];
    if (LOSS == NMF_FRO) {
        double tr = 0.0;
        for (int k = 0; k < K; ++k)
            for (int j = 0; j < K; ++j) tr = tr + cellsum[k * K + j] * hsum[j * K + k];
        return ((xconst + tr) - 2.0 * s) / 2.0;
    }
    double sw = 0.0;
    for (int k = 0; k < K; ++k) sw = sw + cellsum[k] * hsum[k];
    return s + (sw - xconst);
}
// *out = sqrt(2 max(D, 0)); one thread
template <int LOSS>
__global__ void k_nmf_err_final(const double *__restrict__ part, int64_t chunks, int K, const double *__restrict__ cellsum,
                                const double *__restrict__ hsum, double xconst, double *__restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double D = nmf_divergence<LOSS>(part, chunks, K, cellsum, hsum, xconst);
    *out = sqrt(2.0 * (D > 0.0 ? D : 0.0));
}
// The graph form's evaluation: out[0] = sqrt(2 max(D, 0)), out[1] = sqrt(2 max(F, 0)) with F = D + (lambda (R / 2)) / 2,
// out[2] = R / 2 = tr(W^T L W); R = the penalty's chunk sums in chunk order.  One thread.
__global__ void k_nmf_obj_final(const double *__restrict__ part, const double *__restrict__ penpart, int64_t chunks, int K,
                                const double *__restrict__ cellsum, const double *__restrict__ hsum, double xconst, double lambda,
                                double *__restrict__ out)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double D = nmf_divergence<NMF_FRO>(part, chunks, K, cellsum, hsum, xconst);
    double R = 0.0;
    for (int64_t c = 0; c < chunks; ++c) R = R + penpart[c];
    const double tr = R / 2.0;
    const double F = D + (lambda * tr) / 2.0;
    out[0] = sqrt(2.0 * (D > 0.0 ? D : 0.0));
    out[1] = sqrt(2.0 * (F > 0.0 ? F : 0.0));
    out[2] = tr;
}

struct NmfBufs {   // a call's own buffers
    sc_ctx *c;
    enum { W, W1, H0, H1, HT0, HT1, HHT, HSUM, CELLPART, CELLSUM, HPART, ROWERR, ERRPART, ERR, GPTR, GIDX, GVAL, DEG, ROWPEN, PENPART, COUNT };
    DBuf b[COUNT];   // W1 and GPTR ... PENPART: the graph form only
    CsrDevice x;  // the matrix in row order
    ColSort cs;   // the column-sorted copy and its chunk table
    explicit NmfBufs(sc_ctx *ctx) : c(ctx) {}
    int get(int which, size_t bytes) { return b[which].ensure(bytes ? bytes : 8, &c->mem); }
    template <class T> T *as(int which) const { return b[which].as<T>(); }
};

struct NmfState {
    sc_ctx *c;
    NmfBufs *m;
    int64_t n, chunks, cell_chunks;
    int G, K, kp, loss;
    int cur = 0;   // which of the two H / H^T buffers is current
    double xconst; // sum x^2 (Frobenius) or sum of the x > EPS (Kullback-Leibler)
    bool graph = false;   // sc_nmf_fit_graph: the W pass carries the graph term and writes the other W buffer
    double lambda = 0.0;
    int wcur = 0;         // which of the two W buffers is current (always 0 without the graph)
    unsigned groups_grid(int64_t items) const { return (unsigned)ceil_div64(items, NMF_TPB / kp); }
    double *W() const { return m->as<double>(wcur ? NmfBufs::W1 : NmfBufs::W); }
    double *Wother() const { return m->as<double>(wcur ? NmfBufs::W : NmfBufs::W1); }
    double *H() const { return m->as<double>(cur ? NmfBufs::H1 : NmfBufs::H0); }
    double *Ht() const { return m->as<double>(cur ? NmfBufs::HT1 : NmfBufs::HT0); }
    double *Hother() const { return m->as<double>(cur ? NmfBufs::H0 : NmfBufs::H1); }
    double *Htother() const { return m->as<double>(cur ? NmfBufs::HT0 : NmfBufs::HT1); }

    void hprep() const
    {
        hipLaunchKernelGGL(k_nmf_hprep, dim3((unsigned)K), dim3(64), 0, c->stream, Ht(), K, G, m->as<double>(NmfBufs::HHT),
                           m->as<double>(NmfBufs::HSUM));
    }
    void cellsums() const   // W^T W or colsum(W) of the current W into CELLSUM
    {
        const int P = loss == NMF_FRO ? K * K : K;
        double *part = m->as<double>(NmfBufs::CELLPART);
        if (loss == NMF_FRO) hipLaunchKernelGGL(k_nmf_cellsums<NMF_FRO>, dim3((unsigned)cell_chunks), dim3(NMF_TPB), 0, c->stream, W(), n, K, part);
        else hipLaunchKernelGGL(k_nmf_cellsums<NMF_KL>, dim3((unsigned)cell_chunks), dim3(NMF_TPB), 0, c->stream, W(), n, K, part);
        hipLaunchKernelGGL(k_chunk_add, dim3((unsigned)ceil_div64(P, NMF_TPB)), dim3(NMF_TPB), 0, c->stream, part, cell_chunks, P,
                           m->as<double>(NmfBufs::CELLSUM));
    }
    void w_pass()   // the graph form writes the other W buffer and flips the current W
    {
        const dim3 grid(groups_grid(n)), block(NMF_TPB);
        const int64_t *indptr = m->x.indptr.as<int64_t>();
        const int32_t *indices = m->x.indices.as<int32_t>();
        const double *val = m->x.val.as<double>(), *HHt = m->as<double>(NmfBufs::HHT), *Hsum = m->as<double>(NmfBufs::HSUM);
        const size_t fro_lds = sizeof(double) * (size_t)(K * K + NMF_TPB);
        if (graph) {
            hipLaunchKernelGGL((k_nmf_w<NMF_FRO, true>), grid, block, fro_lds, c->stream, indptr, indices, val, n, K, kp, Ht(), HHt, Hsum,
                               m->as<int64_t>(NmfBufs::GPTR), m->as<int32_t>(NmfBufs::GIDX), m->as<double>(NmfBufs::GVAL),
                               m->as<double>(NmfBufs::DEG), lambda, W(), Wother());
            wcur ^= 1;
        } else if (loss == NMF_FRO) {
            hipLaunchKernelGGL((k_nmf_w<NMF_FRO, false>), grid, block, fro_lds, c->stream, indptr, indices, val, n, K, kp, Ht(), HHt, Hsum,
                               nullptr, nullptr, nullptr, nullptr, 0.0, W(), W());
        } else {
            hipLaunchKernelGGL((k_nmf_w<NMF_KL, false>), grid, block, 0, c->stream, indptr, indices, val, n, K, kp, Ht(), HHt, Hsum,
                               nullptr, nullptr, nullptr, nullptr, 0.0, W(), W());
        }
    }
    void h_pass()   // needs cellsums() of the updated W; flips the current H
    {
        const dim3 block(NMF_TPB);
        const int64_t *colptr = m->cs.colptr.as<int64_t>(), *cptr = m->cs.cptr.as<int64_t>();
        const int32_t *crow = m->cs.crow.as<int32_t>(), *cgene = m->cs.cgene.as<int32_t>();
        const double *cval = m->cs.cval.as<double>(), *W = this->W(), *cs = m->as<double>(NmfBufs::CELLSUM);
        double *part = m->as<double>(NmfBufs::HPART);
        if (loss == NMF_FRO) {
            if (chunks) hipLaunchKernelGGL(k_nmf_h<NMF_FRO>, dim3(groups_grid(chunks)), block, 0, c->stream, colptr, crow, cval, cptr, cgene, chunks, K, kp, W, Ht(), part);
            hipLaunchKernelGGL(k_nmf_h_finish<NMF_FRO>, dim3(groups_grid(G)), block, 0, c->stream, cptr, part, G, K, kp, cs, H(), Hother(), Htother());
        } else {
            if (chunks) hipLaunchKernelGGL(k_nmf_h<NMF_KL>, dim3(groups_grid(chunks)), block, 0, c->stream, colptr, crow, cval, cptr, cgene, chunks, K, kp, W, Ht(), part);
            hipLaunchKernelGGL(k_nmf_h_finish<NMF_KL>, dim3(groups_grid(G)), block, 0, c->stream, cptr, part, G, K, kp, cs, H(), Hother(), Htother());
        }
        cur ^= 1;
    }
    // the error of the current (W, H): enqueues everything, waits, returns the value in out[0]; the graph form also
    // returns the objective sqrt(2 max(F, 0)) in out[1] and tr(W^T L W) in out[2]
    int error(double *out) const
    {
        {
            KernelTimerScope ts(c, SC_K_NMF_ERR);
            if (graph) {
                hipLaunchKernelGGL(k_nmf_penalty, dim3(groups_grid(n)), dim3(NMF_TPB), 0, c->stream, m->as<int64_t>(NmfBufs::GPTR),
                                   m->as<int32_t>(NmfBufs::GIDX), m->as<double>(NmfBufs::GVAL), n, K, kp, W(), m->as<double>(NmfBufs::ROWPEN));
                hipLaunchKernelGGL(k_nmf_rowerr_chunks, dim3((unsigned)ceil_div64(cell_chunks, 64)), dim3(64), 0, c->stream,
                                   m->as<double>(NmfBufs::ROWPEN), n, cell_chunks, m->as<double>(NmfBufs::PENPART));
            }
            hprep();
            cellsums();
            const dim3 grid(groups_grid(n)), block(NMF_TPB);
            const int64_t *indptr = m->x.indptr.as<int64_t>();
            const int32_t *indices = m->x.indices.as<int32_t>();
            const double *val = m->x.val.as<double>();
            double *rowerr = m->as<double>(NmfBufs::ROWERR), *part = m->as<double>(NmfBufs::ERRPART);
            const double *cs = m->as<double>(NmfBufs::CELLSUM);
            double *err = m->as<double>(NmfBufs::ERR);
            if (loss == NMF_FRO) hipLaunchKernelGGL(k_nmf_rowerr<NMF_FRO>, grid, block, 0, c->stream, indptr, indices, val, n, K, kp, Ht(), W(), rowerr);
            else hipLaunchKernelGGL(k_nmf_rowerr<NMF_KL>, grid, block, 0, c->stream, indptr, indices, val, n, K, kp, Ht(), W(), rowerr);
            hipLaunchKernelGGL(k_nmf_rowerr_chunks, dim3((unsigned)ceil_div64(cell_chunks, 64)), dim3(64), 0, c->stream, rowerr, n, cell_chunks, part);
            if (graph) hipLaunchKernelGGL(k_nmf_obj_final, dim3(1), dim3(64), 0, c->stream, part, m->as<double>(NmfBufs::PENPART), cell_chunks, K, cs, m->as<double>(NmfBufs::HHT), xconst, lambda, err);
            else if (loss == NMF_FRO) hipLaunchKernelGGL(k_nmf_err_final<NMF_FRO>, dim3(1), dim3(64), 0, c->stream, part, cell_chunks, K, cs, m->as<double>(NmfBufs::HHT), xconst, err);
            else hipLaunchKernelGGL(k_nmf_err_final<NMF_KL>, dim3(1), dim3(64), 0, c->stream, part, cell_chunks, K, cs, m->as<double>(NmfBufs::HSUM), xconst, err);
        }
        SC_HIP(hipGetLastError());
        SC_HIP(hipMemcpyAsync(out, m->as<double>(NmfBufs::ERR), sizeof(double) * (graph ? 3 : 1), hipMemcpyDeviceToHost, c->stream));
        SC_HIP(hipStreamSynchronize(c->stream));
        return SC_OK;
    }
};

// sum x^2 (Frobenius) or the sum of the x > EPS (Kullback-Leibler) over the stored entries, in index order
template <class T>
double nmf_xconst(const T *data, int64_t nnz, int loss)
{
    double s = 0.0;
    for (int64_t p = 0; p < nnz; ++p) {
        const double x = (double)data[p];
        if (loss == NMF_FRO) s = s + x * x;
        else if (x > NMF_EPS) s = s + x;
    }
    return s;
}

// The graph of sc_nmf_fit_graph as the caller holds it (nullptr gptr: the plain fit)
struct NmfGraph {
    const int64_t *gptr;
    const int32_t *gidx;
    const double *gval;
    int64_t entries;
    double lambda;
    double *obj_trace_out, *penalty_out;
};

// The gate of the graph, on the host: canonical n x n CSR without a diagonal, weights finite and > 0, every entry with a
// mirror of equal value (binary search in the mirror row).  The first offending entry is named.
int nmf_check_graph(const char *who, const int64_t *gptr, const int32_t *gidx, const double *gval, int64_t n, int64_t *entries)
{
    SC_TRY(csr_check_offsets(who, gptr, n, entries));
    SC_REQUIRE(*entries <= (int64_t)UINT32_MAX, SC_ERR_INVALID, "%s: need stored graph entries <= 2^32 - 1, got %lld", who,
               (long long)*entries);
    SC_REQUIRE(*entries == 0 || (gidx && gval), SC_ERR_INVALID, "%s: null pointer", who);
    SC_TRY(csr_check_columns(who, gptr, gidx, n, n, "n", [&](int64_t i, int64_t p) {
        SC_REQUIRE(gidx[p] != i, SC_ERR_INVALID, "%s: graph entry %lld is on the diagonal (row %lld)", who, (long long)p, (long long)i);
        SC_REQUIRE(std::isfinite(gval[p]) && gval[p] > 0.0, SC_ERR_INVALID, "%s: graph weight %lld (row %lld, column %d) must be finite and > 0",
                   who, (long long)p, (long long)i, gidx[p]);
        return SC_OK;
    }));
    // every row is canonical here, so a mirror is found by bisection
    for (int64_t i = 0; i < n; ++i)
        for (int64_t p = gptr[i]; p < gptr[i + 1]; ++p) {
            const int32_t j = gidx[p];
            int64_t lo = gptr[j], hi = gptr[j + 1];
            while (lo < hi) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (gidx[mid] < i) lo = mid + 1;
                else hi = mid;
            }
            SC_REQUIRE(lo < gptr[j + 1] && gidx[lo] == i, SC_ERR_INVALID, "%s: graph entry %lld (row %lld, column %d) has no mirror entry", who,
                       (long long)p, (long long)i, j);
            SC_REQUIRE(gval[lo] == gval[p], SC_ERR_INVALID, "%s: graph entry %lld (row %lld, column %d) and its mirror differ in weight", who,
                       (long long)p, (long long)i, j);
        }
    return SC_OK;
}

// Both entry points: the arguments have passed their gates.  gr == nullptr: sc_nmf_fit.
int nmf_run(sc_ctx *c, const char *who, const int64_t *indptr, const int32_t *indices, const void *data, int dtype, int64_t n,
            int32_t n_genes, int32_t K, int32_t loss, int32_t update_H, int32_t max_iter, double tol, double *W, double *H,
            double *err_trace_out, int32_t *n_checks_out, int32_t *n_iter_out, double *recon_err_out, int64_t nnz, const NmfGraph *gr)
{
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const int G = n_genes;
    const int kp = lanes_for(K, 1, NMF_KMAX);
    NmfBufs m(c);
    NmfState st{c, &m, n, 0, ceil_div64(n, NMF_CELL_CHUNK), G, (int)K, kp, (int)loss};
    st.xconst = dtype == SC_F32 ? nmf_xconst((const float *)data, nnz, loss) : nmf_xconst((const double *)data, nnz, loss);
    st.graph = gr != nullptr;
    st.lambda = gr ? gr->lambda : 0.0;
    const size_t nW = sizeof(double) * (size_t)n * K, nH = sizeof(double) * (size_t)K * G;
    const int P = K * K;

    // ---- upload, fp64 values, the column-sorted copy and its chunks -------------------------------------------------
    SC_TRY(m.x.upload(c, indptr, indices, data, dtype, n, nnz));
    SC_TRY(colsort_alloc(c, m.cs, nnz, G));
    SC_TRY(m.get(NmfBufs::W, nW));
    SC_TRY(m.get(NmfBufs::H0, nH));
    SC_TRY(m.get(NmfBufs::H1, nH));
    SC_TRY(m.get(NmfBufs::HT0, nH));
    SC_TRY(m.get(NmfBufs::HT1, nH));
    SC_TRY(m.get(NmfBufs::HHT, sizeof(double) * (size_t)P));
    SC_TRY(m.get(NmfBufs::HSUM, sizeof(double) * (size_t)K));
    SC_TRY(m.get(NmfBufs::CELLPART, sizeof(double) * (size_t)st.cell_chunks * P));
    SC_TRY(m.get(NmfBufs::CELLSUM, sizeof(double) * (size_t)P));
    SC_TRY(m.get(NmfBufs::ROWERR, sizeof(double) * (size_t)n));
    SC_TRY(m.get(NmfBufs::ERRPART, sizeof(double) * (size_t)st.cell_chunks));
    SC_TRY(m.get(NmfBufs::ERR, sizeof(double) * 3));
    if (gr) {
        SC_TRY(m.get(NmfBufs::W1, nW));
        SC_TRY(m.get(NmfBufs::GPTR, sizeof(int64_t) * (size_t)(n + 1)));
        SC_TRY(m.get(NmfBufs::GIDX, sizeof(int32_t) * (size_t)gr->entries));
        SC_TRY(m.get(NmfBufs::GVAL, sizeof(double) * (size_t)gr->entries));
        SC_TRY(m.get(NmfBufs::DEG, sizeof(double) * (size_t)n));
        SC_TRY(m.get(NmfBufs::ROWPEN, sizeof(double) * (size_t)n));
        SC_TRY(m.get(NmfBufs::PENPART, sizeof(double) * (size_t)st.cell_chunks));
        SC_HIP(hipMemcpyAsync(m.b[NmfBufs::GPTR].p, gr->gptr, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, s));
        if (gr->entries) {
            SC_HIP(hipMemcpyAsync(m.b[NmfBufs::GIDX].p, gr->gidx, sizeof(int32_t) * (size_t)gr->entries, hipMemcpyHostToDevice, s));
            SC_HIP(hipMemcpyAsync(m.b[NmfBufs::GVAL].p, gr->gval, sizeof(double) * (size_t)gr->entries, hipMemcpyHostToDevice, s));
        }
    }
    SC_HIP(hipMemcpyAsync(m.b[NmfBufs::W].p, W, nW, hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(m.b[NmfBufs::H0].p, H, nH, hipMemcpyHostToDevice, s));
    {
        KernelTimerScope ts(c, SC_K_NMF_SETUP);
        const dim3 per_entry((unsigned)ceil_div64(nnz, 256)), tpb(256);
        if (dtype == SC_F32) hipLaunchKernelGGL(k_nmf_values<float>, per_entry, tpb, 0, s, m.x.raw.as<float>(), nnz, m.x.val.as<double>());
        else hipLaunchKernelGGL(k_nmf_values<double>, per_entry, tpb, 0, s, m.x.raw.as<double>(), nnz, m.x.val.as<double>());
        SC_TRY(colsort_enqueue(c, m.cs, m.x.indptr.as<int64_t>(), m.x.indices.as<int32_t>(), m.x.val.as<double>(), n, G, nnz));
        hipLaunchKernelGGL(k_nmf_transpose, dim3((unsigned)ceil_div64((int64_t)K * G, 256)), tpb, 0, s, m.as<double>(NmfBufs::H0), (int)K, G,
                           m.as<double>(NmfBufs::HT0));
        if (gr)
            hipLaunchKernelGGL(k_nmf_degree, dim3((unsigned)ceil_div64(n, 256)), tpb, 0, s, m.as<int64_t>(NmfBufs::GPTR),
                               m.as<double>(NmfBufs::GVAL), n, m.as<double>(NmfBufs::DEG));
    }
    {
        KernelTimerScope ts(c, SC_K_NMF_SETUP);
        SC_TRY(colsort_finish(c, m.cs, G, nnz, who));
    }
    SC_HIP(hipGetLastError());
    st.chunks = m.cs.chunks;
    SC_TRY(m.get(NmfBufs::HPART, sizeof(double) * (size_t)m.cs.chunks * K));

    // ---- sklearn's loop: one scalar comes back per check, nothing else waits for the host -------------------------------
    // ev = {error, objective, penalty}; the stopping rule looks at the objective, which without the graph is the error.
    // The graph form evaluates at every tenth iteration whatever tol is (its trace is what shows the descent).
    const int crit = gr ? 1 : 0;
    double ev0[3] = {0.0, 0.0, 0.0}, ev[3] = {0.0, 0.0, 0.0};
    SC_TRY(st.error(ev0));
    int checks = 0;
    if (gr) gr->obj_trace_out[checks] = ev0[1];
    err_trace_out[checks++] = ev0[0];
    const double e0 = ev0[crit];
    double prev = e0;
    int n_iter = 0, last_checked = 0;
    for (int it = 1; it <= max_iter; ++it) {
        {
            KernelTimerScope ts(c, SC_K_NMF_W);
            if (update_H || it == 1) st.hprep();
            st.w_pass();
        }
        if (update_H) {
            KernelTimerScope ts(c, SC_K_NMF_H);
            st.cellsums();
            st.h_pass();
        }
        SC_HIP(hipGetLastError());
        n_iter = it;
        if ((gr || tol > 0.0) && it % 10 == 0) {
            SC_TRY(st.error(ev));
            if (gr) gr->obj_trace_out[checks] = ev[1];
            err_trace_out[checks++] = ev[0];
            last_checked = it;
            if (tol > 0.0) {
                if ((prev - ev[crit]) / e0 < tol) break;
                prev = ev[crit];
            }
        }
    }
    if (last_checked != n_iter) SC_TRY(st.error(ev));
    SC_HIP(hipMemcpyAsync(W, st.W(), nW, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(H, st.H(), nH, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    *n_checks_out = checks;
    *n_iter_out = n_iter;
    *recon_err_out = ev[0];
    if (gr) *gr->penalty_out = ev[2];
    return SC_OK;
}

// the gates both entry points share, up to and including the starting factors; *nnz = the stored entries of X
int nmf_check_common(const char *who, const int64_t *indptr, const int32_t *indices, const void *data, int dtype, int64_t n,
                     int32_t n_genes, int32_t K, const double *W, const double *H, int64_t *nnz)
{
    SC_TRY(csr_check_offsets(who, indptr, n, nnz));
    SC_REQUIRE(*nnz >= 1 && *nnz <= (int64_t)UINT32_MAX, SC_ERR_INVALID, "%s: need 1 <= stored entries <= 2^32 - 1, got %lld", who,
               (long long)*nnz);
    SC_REQUIRE(indices && data, SC_ERR_INVALID, "%s: null pointer", who);
    SC_TRY(csr_check_columns(who, indptr, indices, n, n_genes, "n_genes"));
    SC_TRY(csr_check_values(who, data, dtype, *nnz, true, ""));
    for (int64_t q = 0; q < n * K; ++q)
        SC_REQUIRE(std::isfinite(W[q]) && W[q] >= 0.0, SC_ERR_INVALID, "%s: W0 must be finite and >= 0", who);
    for (int64_t q = 0; q < (int64_t)K * n_genes; ++q)
        SC_REQUIRE(std::isfinite(H[q]) && H[q] >= 0.0, SC_ERR_INVALID, "%s: H0 must be finite and >= 0", who);
    return SC_OK;
}

}  // namespace

extern "C" int sc_nmf_fit(sc_ctx *c, const int64_t *indptr, const int32_t *indices, const void *data, int dtype, int64_t n,
                          int32_t n_genes, int32_t K, int32_t loss, int32_t update_H, int32_t max_iter, double tol, double *W,
                          double *H, double *err_trace_out, int32_t *n_checks_out, int32_t *n_iter_out, double *recon_err_out)
{
    SC_REQUIRE(c && indptr && W && H && err_trace_out && n_checks_out && n_iter_out && recon_err_out, SC_ERR_INVALID,
               "sc_nmf_fit: null pointer");
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "sc_nmf_fit: dtype must be SC_F32 or SC_F64");
    SC_REQUIRE(n >= 1 && n <= INT32_MAX, SC_ERR_INVALID, "sc_nmf_fit: need 1 <= n <= 2^31 - 1, got %lld", (long long)n);
    SC_REQUIRE(n_genes >= 1 && n_genes <= 32768, SC_ERR_INVALID, "sc_nmf_fit: need 1 <= n_genes <= 32768, got %d", n_genes);
    SC_REQUIRE(K >= 1 && K <= NMF_KMAX, SC_ERR_INVALID, "sc_nmf_fit: need 1 <= K <= %d, got %d", NMF_KMAX, K);
    SC_REQUIRE(loss == NMF_FRO || loss == NMF_KL, SC_ERR_INVALID,
               "sc_nmf_fit: loss must be 2 (frobenius) or 1 (kullback-leibler), got %d", loss);
    SC_REQUIRE(max_iter >= 1, SC_ERR_INVALID, "sc_nmf_fit: max_iter must be >= 1, got %d", max_iter);
    SC_REQUIRE(std::isfinite(tol) && tol >= 0.0, SC_ERR_INVALID, "sc_nmf_fit: tol must be finite and >= 0");
    int64_t nnz = 0;
    SC_TRY(nmf_check_common("sc_nmf_fit", indptr, indices, data, dtype, n, n_genes, K, W, H, &nnz));
    return nmf_run(c, "sc_nmf_fit", indptr, indices, data, dtype, n, n_genes, K, loss, update_H, max_iter, tol, W, H, err_trace_out,
                   n_checks_out, n_iter_out, recon_err_out, nnz, nullptr);
}

extern "C" int sc_nmf_fit_graph(sc_ctx *c, const int64_t *indptr, const int32_t *indices, const void *data, int dtype, int64_t n,
                                int32_t n_genes, int32_t K, const int64_t *gptr, const int32_t *gidx, const double *gval, double lambda,
                                int32_t max_iter, double tol, double *W, double *H, double *obj_trace_out, double *err_trace_out,
                                int32_t *n_checks_out, int32_t *n_iter_out, double *recon_err_out, double *penalty_out)
{
    const char *who = "sc_nmf_fit_graph";
    SC_REQUIRE(c && indptr && gptr && W && H && obj_trace_out && err_trace_out && n_checks_out && n_iter_out && recon_err_out && penalty_out,
               SC_ERR_INVALID, "sc_nmf_fit_graph: null pointer");
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "sc_nmf_fit_graph: dtype must be SC_F32 or SC_F64");
    SC_REQUIRE(n >= 1 && n <= INT32_MAX, SC_ERR_INVALID, "sc_nmf_fit_graph: need 1 <= n <= 2^31 - 1, got %lld", (long long)n);
    SC_REQUIRE(n_genes >= 1 && n_genes <= 32768, SC_ERR_INVALID, "sc_nmf_fit_graph: need 1 <= n_genes <= 32768, got %d", n_genes);
    SC_REQUIRE(K >= 1 && K <= NMF_KMAX, SC_ERR_INVALID, "sc_nmf_fit_graph: need 1 <= K <= %d, got %d", NMF_KMAX, K);
    SC_REQUIRE(std::isfinite(lambda) && lambda >= 0.0, SC_ERR_INVALID, "sc_nmf_fit_graph: lambda must be finite and >= 0");
    SC_REQUIRE(max_iter >= 1, SC_ERR_INVALID, "sc_nmf_fit_graph: max_iter must be >= 1, got %d", max_iter);
    SC_REQUIRE(std::isfinite(tol) && tol >= 0.0, SC_ERR_INVALID, "sc_nmf_fit_graph: tol must be finite and >= 0");
    int64_t nnz = 0, entries = 0;
    SC_TRY(nmf_check_common(who, indptr, indices, data, dtype, n, n_genes, K, W, H, &nnz));
    SC_TRY(nmf_check_graph(who, gptr, gidx, gval, n, &entries));
    const NmfGraph gr{gptr, gidx, gval, entries, lambda, obj_trace_out, penalty_out};
    return nmf_run(c, who, indptr, indices, data, dtype, n, n_genes, K, NMF_FRO, 1, max_iter, tol, W, H, err_trace_out, n_checks_out,
                   n_iter_out, recon_err_out, nnz, &gr);
}
