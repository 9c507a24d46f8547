// The label-permutation tests (extensions: the reference has neither).  gfx950 only.
//  * N4, neighbourhood enrichment: cell-type pair counts over the edges of the active graph.
//  * N6, cross-type Ripley's K: cell-type pair counts over the pairs of points within each of several radii.
// Both count pairs whose two ends are positions of a spatially sorted order of the cells, under the observed labels and
// under label permutations, with ONE counting kernel that differs only in how it indexes the histogram.  They share that
// kernel with its plan and host helpers, the relabel kernels, the label upload, the kernel that adds a batch of tables to
// the integer sums of the null, and the host driver of the counter-based batches (generation of batch b + 1 beside the
// counting of batch b); each keeps its own checks of the graph or the pair list.  Ripley's G (sc_ripley_g.hip) takes a
// minimum per cell, not a sum over pairs: it has its own lists and kernel and shares the helpers of sc_labelperm.h.
#include <math.h>
#include <stdlib.h>

#include <functional>
#include <hipcub/hipcub.hpp>
#include <vector>

#include "sc_labelperm.h"
#include "sc_search.h"

// ------------------------------------------------------------------------------------------------
// shared by both tests
// ------------------------------------------------------------------------------------------------

// labp[r] = lab[order[r]]: the observed label of the cell at position r of a spatially sorted order of the cells (the
// graph's processing order, or the bin order of the Ripley pair list).  The pair kernel then needs ONE byte per pair end
// from an n-byte array, and the two ends of a pair -- spatial neighbours -- sit at nearby positions.
__global__ __launch_bounds__(256) void k_lp_labels_by_position(const unsigned char *__restrict__ lab,
                                                               const int32_t *__restrict__ order, int64_t n,
                                                               unsigned char *__restrict__ labp)
{
    const int64_t r0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (r0 >= n) return;
    uint32_t v = 0;
    for (int k = 0; k < 4 && r0 + k < n; ++k) v |= (uint32_t)lab[order[r0 + k]] << (8 * k);
    if (r0 + 4 <= n) *reinterpret_cast<uint32_t *>(labp + r0) = v;
    else for (int k = 0; r0 + k < n; ++k) labp[r0 + k] = (unsigned char)(v >> (8 * k));
}

// lab16[g][rank[cell]] = the labels of `cell` under permutations 16 g .. 16 g + 15 (rows clamped to rows - 1); rank may be
// null: the identity
__global__ __launch_bounds__(256) void k_lp_relabel_words(const unsigned char *__restrict__ lab,
                                                          const int32_t *__restrict__ rank,
                                                          const int32_t *__restrict__ perm, int64_t pstride, int rows,
                                                          int64_t n, uint4 *__restrict__ lab16)
{
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= n) return;
    const int g = blockIdx.y;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        const int row = 16 * g + p < rows ? 16 * g + p : rows - 1;
        w[p >> 2] |= (uint32_t)lab[perm[(int64_t)row * pstride + cell]] << (8 * (p & 3));
    }
    lab16[(int64_t)g * n + (rank ? rank[cell] : cell)] = make_uint4(w[0], w[1], w[2], w[3]);
}

// The integer sums of the null over a batch of n_perm tables counts[p][cells], one thread per (type pair, radius) of
// cells = type pairs x n_radii, on the CUMULATIVE counts u_p = sum_{j' <= j} counts[p][pair][j'] (n_radii = 1: the counts
// themselves): sums[0] += sum_p (u_p - u_obs), sums[1] += sum_p (u_p - u_obs)^2, sums[2] += #{p : u_p >= u_obs} and, with
// n_rows = 4, sums[3] += #{p : u_p <= u_obs}.  Exact and order-free, so batches and ranks add theirs.
__global__ __launch_bounds__(256) void k_lp_sums(const unsigned long long *__restrict__ counts,
                                                 const unsigned long long *__restrict__ obs, int n_perm, int cells,
                                                 int n_radii, int n_rows, long long *__restrict__ sums)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= cells) return;
    const int j = k % n_radii, k0 = k - j;
    long long o = 0;
    for (int jj = 0; jj <= j; ++jj) o += (long long)obs[k0 + jj];
    long long s1 = 0, s2 = 0, ge = 0, le = 0;
    for (int p = 0; p < n_perm; ++p) {
        long long u = 0;
        for (int jj = 0; jj <= j; ++jj) u += (long long)counts[(int64_t)p * cells + k0 + jj];
        const long long d = u - o;
        s1 += d;
        s2 += d * d;
        ge += d >= 0 ? 1 : 0;
        le += d <= 0 ? 1 : 0;
    }
    sums[k] += s1;
    sums[cells + k] += s2;
    sums[2 * cells + k] += ge;
    if (n_rows > 3) sums[3 * cells + k] += le;
}

// ---- declared in sc_labelperm.h ----

int lp_upload_labels(sc_ctx *c, const int32_t *labels, int64_t n, int32_t n_types)
{
    std::vector<unsigned char> lab8((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        SC_REQUIRE(labels[i] >= 0 && labels[i] < n_types, SC_ERR_INVALID, "label %d of cell %lld out of range", labels[i],
                   (long long)i);
        lab8[(size_t)i] = (unsigned char)labels[i];
    }
    SC_TRY(c->scratch_idx.ensure((size_t)n + 16, &c->mem));
    SC_HIP(hipMemcpyAsync(c->scratch_idx.p, lab8.data(), (size_t)n, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}

void lp_labels_by_position(sc_ctx *c, const int32_t *order, int64_t n, unsigned char *labp)
{
    hipLaunchKernelGGL(k_lp_labels_by_position, dim3((unsigned)ceil_div64(n, 1024)), dim3(256), 0, c->stream,
                       c->scratch_idx.as<unsigned char>(), order, n, labp);
}

void lp_sums(sc_ctx *c, const unsigned long long *counts, const unsigned long long *obs, int rows, int cells, int n_radii,
             int n_rows, long long *sums)
{
    hipLaunchKernelGGL(k_lp_sums, dim3((unsigned)ceil_div64(cells, 256)), dim3(256), 0, c->stream, counts, obs, rows, cells,
                       n_radii, n_rows, sums);
}

void lp_relabel_words(sc_ctx *c, int64_t n, const int32_t *rank, const int32_t *table, int rows, uint4 *lab16)
{
    hipLaunchKernelGGL(k_lp_relabel_words, dim3((unsigned)ceil_div64(n, 256), (unsigned)((rows + 15) / 16)), dim3(256), 0,
                       c->stream, c->scratch_idx.as<unsigned char>(), rank, table, c->p_stride, rows, n, lab16);
}

int lp_counter_batches(sc_ctx *c, const char *who, uint64_t seed, int64_t n, int64_t p_first, int64_t n_perm, int64_t batch,
                       const std::function<void(int)> &relabel, const std::function<int(int)> &count,
                       const std::function<void(int)> &accumulate)
{
    if (n_perm > 0) SC_TRY(sc_perm_alloc(c, n, batch));
    SC_TRY(c->streams.ensure(SR_SWAP_A));
    const int64_t batches = n_perm > 0 ? ceil_div64(n_perm, batch) : 0;
    auto rows = [&](int64_t b) { return (int)(b * batch + batch < n_perm ? batch : n_perm - b * batch); };
    std::vector<hipEvent_t> ev((size_t)batches * 2, nullptr);   // per batch: generated, relabelled
    int rc = SC_OK;
    auto generate = [&](int64_t b) -> int {   // batch b's rows into the table, on the generator's stream
        SC_TRY(sc_perm_counter_rows(c, seed, n, p_first + b * batch, rows(b), c->stream3));
        SC_HIP(hipEventCreateWithFlags(&ev[(size_t)(2 * b)], hipEventDisableTiming));
        SC_HIP(hipEventRecord(ev[(size_t)(2 * b)], c->stream3));
        return SC_OK;
    };
    if (batches > 0) {
        SC_HIP(hipStreamSynchronize(c->stream));   // (the table may still be read by an earlier call's kernels)
        rc = generate(0);
    }
    for (int64_t b = 0; b < batches && rc == SC_OK; ++b) {
        if (hipStreamWaitEvent(c->stream, ev[(size_t)(2 * b)], 0) != hipSuccess) { rc = SC_ERR_HIP; break; }
        relabel(rows(b));
        if (hipEventCreateWithFlags(&ev[(size_t)(2 * b + 1)], hipEventDisableTiming) != hipSuccess ||
            hipEventRecord(ev[(size_t)(2 * b + 1)], c->stream) != hipSuccess ||
            hipStreamWaitEvent(c->stream3, ev[(size_t)(2 * b + 1)], 0) != hipSuccess) { rc = SC_ERR_HIP; break; }
        if (b + 1 < batches) rc = generate(b + 1);   // beside the counting of batch b
        if (rc == SC_OK) rc = count(rows(b));
        if (rc != SC_OK) break;
        accumulate(rows(b));
    }
    if (rc == SC_ERR_HIP) sc_set_error("%s: event plumbing failed", who);
    (void)hipStreamSynchronize(c->stream3);
    (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    if (rc != SC_OK) return rc;
    SC_HIP(hipGetLastError());
    if (n_perm > 0) c->p_count = 0;   // the table holds the last batch only: not a table later calls may rely on
    return SC_OK;
}

// ------------------------------------------------------------------------------------------------
// the pair-count kernel of both tests
// ------------------------------------------------------------------------------------------------
//
// The job: for every stored pair (row position, column position), add 1 to a per-permutation LDS histogram at an index
// made from the two labels.  NP permutations per pass over the pairs, each with its own histogram of uint32 in LDS, one
// atomicAdd per pair and permutation; flushed per pair block to uint64 global counters.  Integer atomics only:
// order-free, bit-identical run to run.  NP is the largest of 16, 8, 4, 2, 1 whose histograms fit the 64 KB a workgroup
// may hold (two such workgroups share a CU's 160 KB).

#define LP_PAIRS_PER_BLOCK 65536
#define LP_THREADS(TRI) ((TRI) ? 512 : 256)   // the ordered form measured faster at 256
#define LP_LDS_WORDS 16384   // 64 KB of uint32 per workgroup: the limit on the words of one histogram

// The NP label bytes of a position, rotated right by `rot` bytes: byte s of the result is the label under permutation
// (s + rot) % NP of the pass.  Built from word selects with static indices and v_alignbit_b32 with amounts 0 / 8 / 16 / 24
// (no per-lane indexing of a register array, which would go to scratch, and no per-lane 64-bit shift, see sc_ctx.h).
__device__ __forceinline__ uint4 lp_rotated(const uint4 &w, int rot)
{
    const bool s1 = (rot >> 2) & 1, s2 = (rot >> 3) & 1;
    const uint32_t a0 = s1 ? w.y : w.x, a1 = s1 ? w.z : w.y, a2 = s1 ? w.w : w.z, a3 = s1 ? w.x : w.w;
    const uint32_t b0 = s2 ? a2 : a0, b1 = s2 ? a3 : a1, b2 = s2 ? a0 : a2, b3 = s2 ? a1 : a3;
    const uint32_t k = 8u * ((uint32_t)rot & 3u);
    return make_uint4(__builtin_amdgcn_alignbit(b1, b0, k), __builtin_amdgcn_alignbit(b2, b1, k),
                      __builtin_amdgcn_alignbit(b3, b2, k), __builtin_amdgcn_alignbit(b0, b3, k));
}
__device__ __forceinline__ uint2 lp_rotated(const uint2 &w, int rot)
{
    const bool s1 = (rot >> 2) & 1;
    const uint32_t a0 = s1 ? w.y : w.x, a1 = s1 ? w.x : w.y;
    const uint32_t k = 8u * ((uint32_t)rot & 3u);
    return make_uint2(__builtin_amdgcn_alignbit(a1, a0, k), __builtin_amdgcn_alignbit(a0, a1, k));
}
__device__ __forceinline__ uint32_t lp_rotated(const uint32_t &w, int rot)
{
    return __builtin_amdgcn_alignbit(w, w, 8u * ((uint32_t)rot & 3u));
}
__device__ __forceinline__ uint16_t lp_rotated(const uint16_t &w, int rot)
{
    const uint32_t v = (uint32_t)w | ((uint32_t)w << 16);
    return (uint16_t)(v >> (8u * ((uint32_t)rot & 1u)));
}
__device__ __forceinline__ unsigned char lp_rotated(const unsigned char &w, int) { return w; }

// first histogram row of the unordered type pair (lo, hi), lo <= hi, of T types: rows (0,0) (0,1) .. (0,T-1) (1,1) ..
__host__ __device__ __forceinline__ int rip_tri(int lo, int hi, int T) { return ((lo * (2 * T + 1 - lo)) >> 1) + hi - lo; }

// counts[q NP + p][index] += #{pairs of the block with that index under permutation q NP + p}.  TRI = false, the ordered
// form of the enrichment test: index = la T + lb for the labels (la, lb) of the pair's (row, column); no bin is read.
// TRI = true, Ripley's K: index = tri(lo, hi) R + bin[e], the unordered type pair and the pair's radius bin.  Workgroup
// (q, pair block); consecutive workgroups are the passes of ONE pair block (its bytes come from L2 after the first).  The
// labels of a position are NP consecutive bytes at lab + group stride * (q NP / 16) + position * cell_bytes + (q NP) % 16:
// the 16-byte words of k_lp_relabel_words (cell_bytes = 16), or the byte row of k_lp_labels_by_position (NP = 1,
// cell_bytes = 1: the observed labels).  Lane l takes the permutations in the rotated order (s + l) % NP, so that the
// atomics of one step spread over NP histograms, whose odd stride starts each at a different bank: with ~20 skewed cell
// types most of a wavefront's 64 LDS atomics would otherwise hit a handful of addresses and serialise.
template <int NP, bool TRI>
__global__ __launch_bounds__(LP_THREADS(TRI)) void k_lp_pairs(const int32_t *__restrict__ prow, const int32_t *__restrict__ pcol,
                                                          const unsigned char *__restrict__ pbin, int64_t n_pairs,
                                                          const unsigned char *__restrict__ lab, int64_t gstride, int cell_bytes,
                                                          int n_types, int n_radii, int hstride, int rows,
                                                          unsigned long long *__restrict__ counts)
{
    typedef typename LpWord<NP>::type word_t;
    extern __shared__ unsigned int hist[];   // [NP][hstride]
    const int q = blockIdx.x;
    const int cells = TRI ? ((n_types * (n_types + 1)) >> 1) * n_radii : n_types * n_types;
    for (int k = threadIdx.x; k < NP * hstride; k += LP_THREADS(TRI)) hist[k] = 0;
    __syncthreads();
    const unsigned char *lp = lab + (int64_t)((q * NP) >> 4) * gstride + ((q * NP) & 15);
    const int rot = threadIdx.x & (NP - 1);
    const int two_t1 = 2 * n_types + 1;
    const int64_t e0 = (int64_t)blockIdx.y * LP_PAIRS_PER_BLOCK;
    const int64_t e1 = e0 + LP_PAIRS_PER_BLOCK < n_pairs ? e0 + LP_PAIRS_PER_BLOCK : n_pairs;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += LP_THREADS(TRI)) {
        const word_t a = *reinterpret_cast<const word_t *>(lp + (int64_t)prow[e] * cell_bytes);
        const word_t b = *reinterpret_cast<const word_t *>(lp + (int64_t)pcol[e] * cell_bytes);
        const int bin = TRI ? pbin[e] : 0;
        const word_t ra = lp_rotated(a, rot), rb = lp_rotated(b, rot);
#pragma unroll
        for (int s = 0; s < NP; ++s) {
            const int p = (s + rot) & (NP - 1);
            const int la = lp_label(ra, s), lb = lp_label(rb, s);
            if (TRI) {
                const int lo = la < lb ? la : lb, hi = la < lb ? lb : la;
                atomicAdd(&hist[p * hstride + (((lo * (two_t1 - lo)) >> 1) + hi - lo) * n_radii + bin], 1u);
            } else {
                atomicAdd(&hist[p * hstride + la * n_types + lb], 1u);
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < NP * cells; k += LP_THREADS(TRI)) {
        const int p = k / cells, cell = k - p * cells;
        const unsigned int v = hist[p * hstride + cell];
        if (v && q * NP + p < rows) atomicAdd(&counts[(int64_t)(q * NP + p) * cells + cell], (unsigned long long)v);
    }
}

namespace {

// the stored pairs of one test, their two ends as positions of a spatially sorted order of the cells
struct LpPairs {
    const int32_t *row, *col;      // [n] the positions of the two ends
    const unsigned char *bin;      // [n] the radius bin of a pair (TRI); nullptr: the ordered form
    int64_t n;
    const int32_t *order, *rank;   // [cells] position -> cell, cell -> position
};

struct LpPlan {
    int T = 0, R = 1, cells = 0;   // cells: words of one histogram (T T, or T (T + 1) / 2 * R)
    int np = 1, hstride = 0;       // permutations per pass over the pairs, histogram stride in words
    unsigned pblocks = 0;
};

LpPlan lp_plan(int T, int R, int64_t cells, int64_t n_pairs)
{
    LpPlan pl;
    pl.T = T;
    pl.R = R;
    pl.cells = (int)cells;
    // the largest NP whose NP histograms (stride odd: histogram p starts at a different bank) fit 64 KB
    int np = 16;
    while (np > 1 && (int64_t)np * (cells | 1) > LP_LDS_WORDS) np >>= 1;
    pl.np = np;
    pl.hstride = np > 1 ? (int)(cells | 1) : (int)cells;
    pl.pblocks = (unsigned)ceil_div64(n_pairs, LP_PAIRS_PER_BLOCK);
    return pl;
}

// out[rows][cells] += the pair counts under the labels at `lab`, np permutations per pass over the pairs
void lp_launch(sc_ctx *c, const LpPlan &pl, const LpPairs &pr, int np, int hstride, const unsigned char *lab, int64_t gstride,
               int cell_bytes, int rows, unsigned long long *out)
{
    if (pr.n <= 0) return;
    const dim3 grid((unsigned)((rows + np - 1) / np), pl.pblocks);
    const size_t lds = sizeof(unsigned int) * (size_t)np * hstride;
#define LP_LAUNCH(NP, TRI)                                                                                              \
    hipLaunchKernelGGL((k_lp_pairs<NP, TRI>), grid, dim3(LP_THREADS(TRI)), lds, c->stream, pr.row, pr.col, pr.bin, pr.n, lab, \
                       gstride, cell_bytes, pl.T, pl.R, hstride, rows, out)
#define LP_LAUNCH_NP(TRI)                                                                                               \
    switch (np) {                                                                                                       \
    case 16: LP_LAUNCH(16, TRI); break;                                                                                 \
    case 8: LP_LAUNCH(8, TRI); break;                                                                                   \
    case 4: LP_LAUNCH(4, TRI); break;                                                                                   \
    case 2: LP_LAUNCH(2, TRI); break;                                                                                   \
    default: LP_LAUNCH(1, TRI); break;                                                                                  \
    }
    if (pr.bin) LP_LAUNCH_NP(true)
    else LP_LAUNCH_NP(false)
#undef LP_LAUNCH_NP
#undef LP_LAUNCH
}

// the observed labels by position into labp, their pair counts into out (one "permutation" without a table)
void lp_observed(sc_ctx *c, const LpPlan &pl, const LpPairs &pr, int64_t n, unsigned char *labp, unsigned long long *out)
{
    lp_labels_by_position(c, pr.order, n, labp);
    lp_launch(c, pl, pr, 1, pl.cells, labp, 0, 1, 1, out);
}

// `rows` rows of the permutation table -> 16-byte label words at the cells' positions, in scratch_a ...
void lp_relabel_pair_words(sc_ctx *c, const LpPairs &pr, int64_t n, const int32_t *table, int rows)
{
    lp_relabel_words(c, n, pr.rank, table, rows, c->scratch_a.as<uint4>());
}

// ... -> out[rows][cells]
void lp_count_words(sc_ctx *c, const LpPlan &pl, const LpPairs &pr, int64_t n, int rows, unsigned long long *out)
{
    lp_launch(c, pl, pr, pl.np, pl.hstride, c->scratch_a.as<unsigned char>(), n * 16, 16, rows, out);
}

// The tables of rows perm_row0 .. perm_row0 + n_perm - 1 of the resident permutation table, then the observed one:
// host[n_perm + 1][cells].
int lp_count_tables(sc_ctx *c, const LpPlan &pl, const LpPairs &pr, int64_t n, int64_t n_perm, int64_t perm_row0,
                    unsigned long long *host)
{
    const size_t bytes = sizeof(unsigned long long) * (size_t)pl.cells * (size_t)(n_perm + 1);
    SC_TRY(c->scratch_b.ensure(bytes, &c->mem));
    // [16-byte label words of the table rows | observed labels by position]
    const size_t word_bytes = (size_t)n * 16 * (size_t)((n_perm + 15) / 16);
    SC_TRY(c->scratch_a.ensure(word_bytes + (size_t)align_up64(n, 16), &c->mem));
    unsigned long long *d_cnt = c->scratch_b.as<unsigned long long>();
    SC_HIP(hipMemsetAsync(d_cnt, 0, bytes, c->stream));
    if (n_perm > 0) {
        lp_relabel_pair_words(c, pr, n, c->perm.as<int32_t>() + perm_row0 * c->p_stride, (int)n_perm);
        lp_count_words(c, pl, pr, n, (int)n_perm, d_cnt);
    }
    lp_observed(c, pl, pr, n, c->scratch_a.as<unsigned char>() + word_bytes, d_cnt + (size_t)pl.cells * (size_t)n_perm);
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(host, d_cnt, bytes, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}

// The whole test of one rank's range of counter-based permutations in ONE call: the observed table, then the n_rows
// integer sums of k_lp_sums accumulated on the device over the batches of lp_counter_batches: host[1 + n_rows][cells].
int lp_counter_sums(sc_ctx *c, const char *who, const LpPlan &pl, const LpPairs &pr, int64_t n, uint64_t seed, int64_t p_first,
                    int64_t n_perm, int64_t batch, int n_rows, unsigned long long *host)
{
    const int cells = pl.cells;
    const size_t cnt_bytes = sizeof(unsigned long long) * (size_t)cells * (size_t)batch;
    const size_t res_bytes = sizeof(unsigned long long) * (size_t)cells * (size_t)(1 + n_rows);
    SC_TRY(c->scratch_b.ensure(cnt_bytes + res_bytes, &c->mem));   // counts | observed | sums
    const size_t word_bytes = (size_t)n * 16 * (size_t)((batch + 15) / 16), lab_bytes = (size_t)align_up64(n, 16);
    SC_TRY(c->scratch_a.ensure(word_bytes > lab_bytes ? word_bytes : lab_bytes, &c->mem));
    unsigned long long *d_cnt = c->scratch_b.as<unsigned long long>(), *d_obs = d_cnt + (size_t)cells * batch;
    long long *d_sums = reinterpret_cast<long long *>(d_obs + cells);
    SC_HIP(hipMemsetAsync(d_obs, 0, res_bytes, c->stream));
    lp_observed(c, pl, pr, n, c->scratch_a.as<unsigned char>(), d_obs);   // (the label words of batch 0 follow on the same stream)
    SC_HIP(hipGetLastError());
    SC_TRY(lp_counter_batches(
        c, who, seed, n, p_first, n_perm, batch, [&](int rows) { lp_relabel_pair_words(c, pr, n, c->perm.as<int32_t>(), rows); },
        [&](int rows) -> int {
            SC_HIP(hipMemsetAsync(d_cnt, 0, cnt_bytes, c->stream));
            lp_count_words(c, pl, pr, n, rows, d_cnt);
            return SC_OK;
        },
        [&](int rows) { lp_sums(c, d_cnt, d_obs, rows, cells, pl.R, n_rows, d_sums); }));
    SC_HIP(hipMemcpy(host, d_obs, res_bytes, hipMemcpyDeviceToHost));
    return SC_OK;
}

}   // namespace

// ------------------------------------------------------------------------------------------------
// N4 (extension, no reference counterpart): cell-type pair counts over the graph's edges under label
// permutations.  counts[p][a][b] = #{edges i -> j : lab[perm_p[i]] == a and lab[perm_p[j]] == b}
// (p == n_perm: identity, i.e. the observed counts): the ordered form of k_lp_pairs over the edges
// (row position, column position) of the graph's processing order.
// ------------------------------------------------------------------------------------------------

// what both entry points need of the active graph: the edges by position, and the histogram plan for n_types
static int enr_prepare(sc_ctx *c, int32_t n_types, LpPairs *pr, LpPlan *pl)
{
    SC_TRY(sc_graph_ensure_order(c));
    *pr = LpPairs{c->g_erow_r.as<int32_t>(), c->g_indices_r.as<int32_t>(), nullptr, c->g_nnz, c->g_order.as<int32_t>(),
                  c->g_rank.as<int32_t>()};
    *pl = lp_plan(n_types, 1, (int64_t)n_types * n_types, c->g_nnz);
    return SC_OK;
}

extern "C" int sc_enrichment_counts(sc_ctx *c, const int32_t *labels, int64_t n, int32_t n_types, int64_t n_perm,
                                    int64_t perm_row0, int64_t *counts_out)
{
    SC_REQUIRE(c && labels && counts_out, SC_ERR_INVALID, "sc_enrichment_counts: null pointer");
    SC_HIP(hipSetDevice(c->device));
    SC_REQUIRE(c->g_n > 0 && n == c->g_n, SC_ERR_STATE, "sc_enrichment_counts: graph missing or size mismatch");
    SC_REQUIRE(n_types >= 1 && n_types <= 96, SC_ERR_INVALID, "sc_enrichment_counts: n_types must be 1..96");
    SC_REQUIRE(n_perm + 1 <= 65535 && ceil_div64(c->g_nnz, LP_PAIRS_PER_BLOCK) <= 65535, SC_ERR_INVALID,
               "sc_enrichment_counts: at most 65534 permutations per call (got %lld) and 4.2e9 edges; call it per batch of the table",
               (long long)n_perm);
    SC_TRY(lp_counts_rows(c, "sc_enrichment_counts", n, n_perm, perm_row0));
    SC_TRY(lp_upload_labels(c, labels, n, n_types));
    LpPairs pr;
    LpPlan pl;
    SC_TRY(enr_prepare(c, n_types, &pr, &pl));
    return lp_count_tables(c, pl, pr, n, n_perm, perm_row0, reinterpret_cast<unsigned long long *>(counts_out));
}

extern "C" int sc_enrichment_counter(sc_ctx *c, const int32_t *labels, int64_t n, int32_t n_types, uint64_t seed,
                                     int64_t p_first, int64_t n_perm, int64_t batch, int64_t *observed_out, int64_t *sums_out)
{
    SC_REQUIRE(c && labels && observed_out && sums_out, SC_ERR_INVALID, "sc_enrichment_counter: null pointer");
    SC_HIP(hipSetDevice(c->device));
    SC_REQUIRE(c->g_n > 0 && n == c->g_n, SC_ERR_STATE, "sc_enrichment_counter: graph missing or size mismatch");
    SC_REQUIRE(n_types >= 1 && n_types <= 96, SC_ERR_INVALID, "sc_enrichment_counter: n_types must be 1..96");
    SC_TRY(lp_counter_sizes("sc_enrichment_counter", p_first, n_perm, &batch));
    SC_REQUIRE(ceil_div64(c->g_nnz, LP_PAIRS_PER_BLOCK) <= 65535, SC_ERR_INVALID, "sc_enrichment_counter: more than 4.2e9 edges");
    SC_TRY(lp_upload_labels(c, labels, n, n_types));
    LpPairs pr;
    LpPlan pl;
    SC_TRY(enr_prepare(c, n_types, &pr, &pl));
    const size_t tt = (size_t)pl.cells;
    std::vector<unsigned long long> host(tt * 4);   // observed | 3 sums
    SC_TRY(lp_counter_sums(c, "sc_enrichment_counter", pl, pr, n, seed, p_first, n_perm, batch, 3, host.data()));
    for (size_t k = 0; k < tt; ++k) observed_out[k] = (int64_t)host[k];
    for (size_t k = 0; k < 3 * tt; ++k) sums_out[k] = (int64_t)host[tt + k];
    return SC_OK;
}

// ------------------------------------------------------------------------------------------------
// N6: cross-type Ripley's K with a label-permutation null (the reference has no point-pattern statistic)
// ------------------------------------------------------------------------------------------------
//
// Definition (include/spatialcore_hip.h, "N6"): count[a][b][j] = number of ORDERED pairs (i, i'), i != i', of types
// (a, b) with fl(fl(dx dx) + fl(dy dy)) <= fl(r_j r_j) -- the closed ball of sc_radius_count_2d, cumulative in j.
//
// What the device stores and counts is half of that.  The distance rule is symmetric to the last bit (dx and -dx have
// the same square), so (i, i') is within r exactly when (i', i) is: the pair list holds every UNORDERED pair once
// (row position < column position in the bin-sorted order of the points) and the histogram is indexed by the unordered
// type pair (lo <= hi).  count[a][b] = u[min(a, b)][max(a, b)] for a != b and 2 u[a][a] on the diagonal: half the
// pairs, half the atomics and half the LDS of the ordered form, the same integers.
//
//  * pair build: two passes over the bin grid like k_radius (count, exclusive scan, fill), one thread per point; a
//    thread looks only at its own bin row from its own position on and at the rows above (positions grow with the bin
//    key).  Each pair carries ONE BYTE: the index of the smallest radius that contains it (d^2 against the R values
//    fl(r_j r_j) the host computed; no square root).
//  * counting: edge-parallel, NON-cumulative bins.  NP permutations per pass over the pairs, each with its own
//    histogram [T (T + 1) / 2][R] of uint32 in LDS, one atomicAdd per pair and permutation; flushed per pair block to
//    uint64 global counters.  Integer atomics only: order-free, bit-identical run to run.  NP is the largest of
//    16, 8, 4, 2, 1 whose histograms fit the 64 KB a workgroup may hold (two such workgroups share a CU's 160 KB).
//  * the cumulative sum over j and the expansion to the ordered T x T x R table happen once, at the end.

#define RIP_MAX_RADII 32

struct RipleyR2 { double v[RIP_MAX_RADII]; };

// FILL = false: counts[t] = pairs (t, s), s > t, within the largest radius; rank[cell at t] = t.
// FILL = true: the pairs themselves at indptr[t] .., with their radius bins.  t, s: positions in bin order.
template <bool FILL>
__global__ __launch_bounds__(256) void k_ripley_pairs(BinGrid g, int64_t n, RipleyR2 r2, int n_radii, int rings,
                                                      long long *__restrict__ counts,
                                                      const long long *__restrict__ indptr, int32_t *__restrict__ prow,
                                                      int32_t *__restrict__ pcol, unsigned char *__restrict__ pbin,
                                                      int32_t *__restrict__ rank)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double qx = g.sx[t], qy = g.sy[t];
    const double r2max = r2.v[n_radii - 1];
    long long cnt = 0;
    const long long base = FILL ? indptr[t] : 0;
    window_walk<true>(g, qx, qy, rings, (int)t, [&](int s) {
        const double d = BinGrid::dist2(qx, qy, g.sx[s], g.sy[s]);
        if (d <= r2max) {
            if (FILL) {
                int b = 0;
                for (int j = 0; j < n_radii - 1; ++j) b += d > r2.v[j] ? 1 : 0;
                prow[base + cnt] = (int32_t)t;
                pcol[base + cnt] = s;
                pbin[base + cnt] = (unsigned char)b;
            }
            ++cnt;
        }
    });
    if (!FILL) {
        counts[t] = cnt;
        rank[g.sid[t]] = (int32_t)t;
    }
}

extern "C" int sc_ripley_build(sc_ctx *c, const double *xy, int64_t n, const double *radii, int32_t n_radii,
                               int64_t *n_pairs_out)
{
    SC_REQUIRE(c && xy && radii && n_pairs_out, SC_ERR_INVALID, "sc_ripley_build: null pointer");
    SC_REQUIRE(n_radii >= 1 && n_radii <= RIP_MAX_RADII, SC_ERR_INVALID, "sc_ripley_build: 1..%d radii, got %d",
               RIP_MAX_RADII, (int)n_radii);
    RipleyR2 r2;
    for (int j = 0; j < RIP_MAX_RADII; ++j) r2.v[j] = 0.0;
    for (int j = 0; j < n_radii; ++j) {
        SC_REQUIRE(radii[j] > 0 && isfinite(radii[j]), SC_ERR_INVALID, "sc_ripley_build: radius %d must be > 0 and finite, got %g",
                   j, radii[j]);
        SC_REQUIRE(j == 0 || radii[j] > radii[j - 1], SC_ERR_INVALID,
                   "sc_ripley_build: radii must be strictly increasing (radius %d = %g after %g)", j, radii[j], radii[j - 1]);
        r2.v[j] = radii[j] * radii[j];   // fl(r r): the compiler may not contract it (-ffp-contract=off), nothing to contract
        SC_REQUIRE(isfinite(r2.v[j]), SC_ERR_INVALID, "sc_ripley_build: radius %d squared is not finite (%g)", j, radii[j]);
    }
    SC_HIP(hipSetDevice(c->device));
    const double rmax = radii[n_radii - 1];
    // bins no smaller than the largest radius, as the radius graph takes them
    SC_TRY(sc_bin_points(c, xy, n, 4.0, rmax));
    const int rings = sc_window_rings(c, rmax);
    const BinGrid g = sc_bin_grid(c);
    SC_TRY(c->rp_cnt.ensure(sizeof(long long) * (size_t)(n + 1), &c->mem));
    SC_TRY(c->rp_indptr.ensure(sizeof(long long) * (size_t)(n + 1), &c->mem));
    SC_TRY(c->rp_rank.ensure(sizeof(int32_t) * (size_t)n, &c->mem));
    long long *counts = c->rp_cnt.as<long long>();
    SC_HIP(hipMemsetAsync(counts, 0, sizeof(long long) * (size_t)(n + 1), c->stream));
    const dim3 grid((unsigned)ceil_div64(n, 256));
    hipLaunchKernelGGL(k_ripley_pairs<false>, grid, dim3(256), 0, c->stream, g, n, r2, (int)n_radii, rings, counts,
                       (const long long *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, (unsigned char *)nullptr,
                       c->rp_rank.as<int32_t>());
    SC_HIP(hipGetLastError());
    long long total = 0;
    SC_TRY(sc_counts_to_offsets(c, counts, c->rp_indptr.as<long long>(), n, &total));
    SC_HIP(hipStreamSynchronize(c->stream));
    SC_REQUIRE(ceil_div64(total, LP_PAIRS_PER_BLOCK) <= 65535, SC_ERR_INVALID,
               "sc_ripley_build: %lld unordered pairs within the largest radius, more than 4.2e9", total);
    const size_t cap = (size_t)(total > 0 ? total : 1);
    SC_TRY(c->rp_row.ensure(sizeof(int32_t) * cap, &c->mem));
    SC_TRY(c->rp_col.ensure(sizeof(int32_t) * cap, &c->mem));
    SC_TRY(c->rp_bin.ensure(cap, &c->mem));
    if (total > 0) {
        hipLaunchKernelGGL(k_ripley_pairs<true>, grid, dim3(256), 0, c->stream, g, n, r2, (int)n_radii, rings,
                           (long long *)nullptr, c->rp_indptr.as<long long>(), c->rp_row.as<int32_t>(),
                           c->rp_col.as<int32_t>(), c->rp_bin.as<unsigned char>(), (int32_t *)nullptr);
        SC_HIP(hipGetLastError());
        SC_HIP(hipStreamSynchronize(c->stream));
    }
    c->rp_n = n;
    c->rp_pairs = total;
    c->rp_radii = n_radii;
    c->rp_valid = true;
    *n_pairs_out = 2 * (int64_t)total;   // ordered pairs: nnz of the radius graph at the largest radius
    return SC_OK;
}

// ------------------------------------------------------------------------------------------------
// counting: the TRI form of k_lp_pairs over the pair list
// ------------------------------------------------------------------------------------------------

namespace {

// what both counting entry points check: the pair list, the labels (uploaded to scratch_idx), the shape
int rip_prepare(sc_ctx *c, const char *who, const int32_t *labels, int64_t n, int32_t n_types, LpPairs *pr, LpPlan *pl)
{
    SC_REQUIRE(n_types >= 1 && n_types <= 96, SC_ERR_INVALID, "%s: n_types must be 1..96, got %d", who, (int)n_types);
    SC_REQUIRE(c->rp_valid, SC_ERR_STATE,
               "%s: no pair list (call sc_ripley_build first; a neighbour search since then has replaced its bins)", who);
    SC_REQUIRE(n == c->rp_n, SC_ERR_STATE, "%s: %lld labels for a pair list of %lld cells", who, (long long)n,
               (long long)c->rp_n);
    const int64_t cells = (int64_t)n_types * (n_types + 1) / 2 * c->rp_radii;
    SC_REQUIRE(cells <= LP_LDS_WORDS, SC_ERR_INVALID,
               "%s: n_types (n_types + 1) / 2 * n_radii = %lld exceeds the limit of %d histogram words (64 KB of LDS); "
               "n_types = %d, n_radii = %d", who, (long long)cells, LP_LDS_WORDS, (int)n_types, c->rp_radii);
    SC_TRY(lp_upload_labels(c, labels, n, n_types));
    *pr = LpPairs{c->rp_row.as<int32_t>(), c->rp_col.as<int32_t>(), c->rp_bin.as<unsigned char>(), c->rp_pairs,
                  c->sid.as<int32_t>(), c->rp_rank.as<int32_t>()};
    *pl = lp_plan(n_types, c->rp_radii, cells, c->rp_pairs);
    return SC_OK;
}

// unordered table u[pair][j] -> ordered table out[a][b][j].  cumulate: u holds the non-cumulative counts of the kernel
// (k_lp_sums' rows are sums over the cumulative counts already: false).  `diag`: the factor of the diagonal, 2 for
// counts and deviation sums, 4 for squared deviations, 1 for exceedance counts
void rip_expand(const LpPlan &pl, const unsigned long long *u, bool cumulate, long long diag, int64_t *out)
{
    for (int a = 0; a < pl.T; ++a)
        for (int b = 0; b < pl.T; ++b) {
            const unsigned long long *src = u + (size_t)rip_tri(a < b ? a : b, a < b ? b : a, pl.T) * pl.R;
            int64_t *dst = out + ((size_t)a * pl.T + b) * pl.R;
            long long run = 0;
            for (int j = 0; j < pl.R; ++j) {
                run = cumulate ? run + (long long)src[j] : (long long)src[j];
                dst[j] = (int64_t)(run * (a == b ? diag : 1));
            }
        }
}

}   // namespace

extern "C" int sc_ripley_counts(sc_ctx *c, const int32_t *labels, int64_t n, int32_t n_types, int64_t n_perm,
                                int64_t perm_row0, int64_t *counts_out)
{
    SC_REQUIRE(c && labels && counts_out, SC_ERR_INVALID, "sc_ripley_counts: null pointer");
    SC_HIP(hipSetDevice(c->device));
    LpPairs pr;
    LpPlan pl;
    SC_TRY(rip_prepare(c, "sc_ripley_counts", labels, n, n_types, &pr, &pl));
    SC_TRY(lp_counts_rows(c, "sc_ripley_counts", n, n_perm, perm_row0));
    std::vector<unsigned long long> host((size_t)pl.cells * (size_t)(n_perm + 1));
    SC_TRY(lp_count_tables(c, pl, pr, n, n_perm, perm_row0, host.data()));
    const size_t ttr = (size_t)pl.T * pl.T * pl.R;
    for (int64_t p = 0; p <= n_perm; ++p) rip_expand(pl, host.data() + (size_t)p * pl.cells, true, 2, counts_out + (size_t)p * ttr);
    return SC_OK;
}

extern "C" int sc_ripley_counter(sc_ctx *c, const int32_t *labels, int64_t n, int32_t n_types, uint64_t seed, int64_t p_first,
                                 int64_t n_perm, int64_t batch, int64_t *observed_out, int64_t *sums_out)
{
    SC_REQUIRE(c && labels && observed_out && sums_out, SC_ERR_INVALID, "sc_ripley_counter: null pointer");
    SC_TRY(lp_counter_sizes("sc_ripley_counter", p_first, n_perm, &batch));
    SC_HIP(hipSetDevice(c->device));
    LpPairs pr;
    LpPlan pl;
    SC_TRY(rip_prepare(c, "sc_ripley_counter", labels, n, n_types, &pr, &pl));
    const size_t cells = (size_t)pl.cells, ttr = (size_t)pl.T * pl.T * pl.R;
    std::vector<unsigned long long> host(cells * 5);   // observed | 4 sums
    SC_TRY(lp_counter_sums(c, "sc_ripley_counter", pl, pr, n, seed, p_first, n_perm, batch, 4, host.data()));
    rip_expand(pl, host.data(), true, 2, observed_out);
    // the sums are those of the cumulative UNORDERED counts u; a diagonal ordered count is 2 u: deviations double,
    // their squares quadruple, the comparisons stay
    rip_expand(pl, host.data() + cells * 1, false, 2, sums_out);
    rip_expand(pl, host.data() + cells * 2, false, 4, sums_out + ttr);
    rip_expand(pl, host.data() + cells * 3, false, 1, sums_out + 2 * ttr);
    rip_expand(pl, host.data() + cells * 4, false, 1, sums_out + 3 * ttr);
    return SC_OK;
}
