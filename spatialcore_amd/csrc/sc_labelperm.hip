// The label-permutation tests (extensions: the reference has neither).  gfx950 only.
//  * N4, neighbourhood enrichment: cell-type pair counts over the edges of the active graph.
//  * N6, cross-type Ripley's K: cell-type pair counts over the pairs of points within each of several radii.
// Both count pairs whose two ends are positions of a spatially sorted order of the cells, under the observed labels and
// under label permutations, and differ only in the counting kernels.  They share the relabel kernels, the label upload,
// the kernel that adds a batch of tables to the integer sums of the null, and the host driver of the counter-based
// batches (generation of batch b + 1 beside the counting of batch b).
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

// labp[p][r] = lab[perm_p[order[r]]] (p == n_perm: the identity, i.e. the observed labels): the permuted label of
// the cell at position r of the graph's spatially sorted processing order.  The edge kernel then needs ONE byte per
// edge end from an n-byte array (instead of a 4-byte index gather followed by a byte gather), and the two ends of an
// edge -- spatial neighbours -- sit at nearby positions: the row's k + 1 bytes come from one or two cache lines.
__global__ __launch_bounds__(256) void k_enrich_relabel(const unsigned char *__restrict__ lab,
                                                        const int32_t *__restrict__ order,
                                                        const int32_t *__restrict__ perm, int64_t pstride, int n_perm,
                                                        int64_t n, int64_t lstride, unsigned char *__restrict__ labp)
{
    const int p = blockIdx.y;
    const int32_t *prow = p < n_perm ? perm + (int64_t)p * pstride : nullptr;
    const int64_t r0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (r0 >= n) return;
    unsigned char *dst = labp + (int64_t)p * lstride;
    uint32_t v = 0;
    for (int k = 0; k < 4 && r0 + k < n; ++k) {
        const int32_t cell = order[r0 + k];
        v |= (uint32_t)lab[prow ? prow[cell] : cell] << (8 * k);
    }
    if (r0 + 4 <= n) *reinterpret_cast<uint32_t *>(dst + r0) = v;
    else for (int k = 0; r0 + k < n; ++k) dst[r0 + k] = (unsigned char)(v >> (8 * k));
}

// lab16[g][rank[cell]] = the labels of `cell` under permutations 16 g .. 16 g + 15 (rows clamped to rows - 1); rank may be
// null: the identity
__global__ __launch_bounds__(256) void k_enrich_relabel16(const unsigned char *__restrict__ lab,
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

void lp_relabel_words(sc_ctx *c, int64_t n, const int32_t *rank, const int32_t *table, int rows, uint4 *lab16)
{
    hipLaunchKernelGGL(k_enrich_relabel16, dim3((unsigned)ceil_div64(n, 256), (unsigned)((rows + 15) / 16)), dim3(256), 0,
                       c->stream, c->scratch_idx.as<unsigned char>(), rank, table, c->p_stride, rows, n, lab16);
}

int lp_counter_batches(sc_ctx *c, const char *who, uint64_t seed, int64_t n, int64_t p_first, int64_t n_perm, int64_t batch,
                       const std::function<void(int)> &relabel, const std::function<int(int)> &count,
                       const std::function<void(int)> &accumulate)
{
    if (n_perm > 0) SC_TRY(sc_perm_alloc(c, n, batch));
    if (!c->stream3) SC_HIP(hipStreamCreateWithFlags(&c->stream3, hipStreamNonBlocking));
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
// N4 (extension, no reference counterpart): cell-type pair counts over the graph's edges under label
// permutations.  counts[p][a][b] = #{edges i -> j : lab[perm_p[i]] == a and lab[perm_p[j]] == b}
// (p == n_perm: identity, i.e. the observed counts).  One workgroup = one permutation x one cell
// range; the T x T histogram lives in LDS (integer atomics: deterministic), then is added to global.
// ------------------------------------------------------------------------------------------------

#define ENR_EDGES_PER_BLOCK 65536

// counts[p][a][b] += #{edges of the block : label(row) = a, label(column) = b}.  One thread per EDGE (coalesced reads of
// the two relabelled end positions; consecutive workgroups are the permutations of ONE edge block, which L2 serves),
// `copies` private T x T histograms per workgroup (lane l adds into copy l % copies, copy stride odd: with ~20 skewed
// cell types most of a wavefront's 64 LDS atomics would otherwise hit a handful of addresses and banks and serialise).
__global__ __launch_bounds__(256) void k_enrich(const int32_t *__restrict__ erow_r, const int32_t *__restrict__ ecol_r,
                                                int64_t nnz, const unsigned char *__restrict__ labp, int64_t lstride,
                                                int n_types, int copies, int cstride, unsigned long long *__restrict__ counts)
{
    extern __shared__ unsigned int hist[];
    const int p = blockIdx.x;
    const int tt = n_types * n_types;
    for (int k = threadIdx.x; k < cstride * copies; k += 256) hist[k] = 0;
    __syncthreads();
    const unsigned char *lp = labp + (int64_t)p * lstride;
    unsigned int *mine = hist + (threadIdx.x & (copies - 1)) * cstride;
    const int64_t e0 = (int64_t)blockIdx.y * ENR_EDGES_PER_BLOCK;
    const int64_t e1 = e0 + ENR_EDGES_PER_BLOCK < nnz ? e0 + ENR_EDGES_PER_BLOCK : nnz;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += 256)
        atomicAdd(&mine[(int)lp[erow_r[e]] * n_types + lp[ecol_r[e]]], 1u);
    __syncthreads();
    unsigned long long *out = counts + (int64_t)p * tt;
    for (int k = threadIdx.x; k < tt; k += 256) {
        unsigned int v = 0;
        for (int c = 0; c < copies; ++c) v += hist[c * cstride + k];
        if (v) atomicAdd(&out[k], (unsigned long long)v);
    }
}

extern "C" int sc_enrichment_counts(sc_ctx *c, const int32_t *labels, int64_t n, int32_t n_types, int64_t n_perm,
                                    int64_t perm_row0, int64_t *counts_out)
{
    SC_REQUIRE(c && labels && counts_out, SC_ERR_INVALID, "sc_enrichment_counts: null pointer");
    SC_HIP(hipSetDevice(c->device));
    if (n_perm > 0) SC_TRY(sc_perm_forward_ensure(c));
    SC_REQUIRE(c->g_n > 0 && n == c->g_n, SC_ERR_STATE, "sc_enrichment_counts: graph missing or size mismatch");
    SC_REQUIRE(n_types >= 1 && n_types <= 96, SC_ERR_INVALID, "sc_enrichment_counts: n_types must be 1..96");
    SC_REQUIRE(n_perm >= 0 && perm_row0 >= 0, SC_ERR_INVALID, "sc_enrichment_counts: negative size");
    SC_REQUIRE(n_perm + 1 <= 65535 && ceil_div64(c->g_nnz, ENR_EDGES_PER_BLOCK) <= 65535, SC_ERR_INVALID,
               "sc_enrichment_counts: at most 65534 permutations per call (got %lld) and 4.2e9 edges; call it per batch of the table",
               (long long)n_perm);
    if (n_perm > 0)
        SC_REQUIRE(c->p_n == n && perm_row0 + n_perm <= c->p_count, SC_ERR_STATE,
                   "sc_enrichment_counts: needs permutation rows [%lld, %lld)", (long long)perm_row0,
                   (long long)(perm_row0 + n_perm));
    SC_TRY(lp_upload_labels(c, labels, n, n_types));
    const size_t tt = (size_t)n_types * n_types;
    const size_t out_bytes = sizeof(unsigned long long) * tt * (size_t)(n_perm + 1);
    const int64_t lstride = align_up64(n, 16);
    SC_TRY(c->scratch_b.ensure(out_bytes, &c->mem));
    SC_TRY(c->scratch_a.ensure((size_t)lstride * (size_t)(n_perm + 1), &c->mem));   // permuted label vectors
    SC_HIP(hipMemsetAsync(c->scratch_b.p, 0, out_bytes, c->stream));
    SC_TRY(sc_graph_ensure_order(c));
    hipLaunchKernelGGL(k_enrich_relabel, dim3((unsigned)ceil_div64(n, 1024), (unsigned)(n_perm + 1)), dim3(256), 0, c->stream,
                       c->scratch_idx.as<unsigned char>(), c->g_order.as<int32_t>(),
                       c->perm.as<int32_t>() + perm_row0 * c->p_stride, c->p_stride, (int)n_perm, n, lstride,
                       c->scratch_a.as<unsigned char>());
    if (c->g_nnz > 0) {
        int copies = 16;
        const int cstride = (int)tt | 1;   // odd: copy c starts at a different LDS bank
        while (copies > 1 && (size_t)copies * cstride > 12288) copies >>= 1;   // <= 48 KB of LDS per workgroup
        dim3 grid((unsigned)(n_perm + 1), (unsigned)ceil_div64(c->g_nnz, ENR_EDGES_PER_BLOCK));
        hipLaunchKernelGGL(k_enrich, grid, dim3(256), sizeof(unsigned int) * cstride * copies, c->stream,
                           c->g_erow_r.as<int32_t>(), c->g_indices_r.as<int32_t>(), c->g_nnz, c->scratch_a.as<unsigned char>(),
                           lstride, (int)n_types, copies, cstride, c->scratch_b.as<unsigned long long>());
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(counts_out, c->scratch_b.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}

// ------------------------------------------------------------------------------------------------
// The whole label-permutation test of one rank's range of counter-based permutations in ONE call (r03): the sums the
// p-values and z-scores need are accumulated on the device, and the generation of batch b + 1 (stage B's swaps are
// latency-bound: 21 ms per 512 permutations of 1M cells) runs on a second stream beside the edge counting of batch b
// (37 ms per 512; lp_counter_batches).
// ------------------------------------------------------------------------------------------------

// ---- sixteen permutations per edge (r03) ------------------------------------------------------------------------------
// k_enrich re-reads the 8 bytes of every edge once per permutation (123 GB of L2 traffic per 512 permutations of a 30M-edge
// graph: what bounds it, 37 ms).  Here the permuted labels of SIXTEEN permutations of a cell are one 16-byte word (at the
// cell's position in the graph's processing order), so an edge's indices are read once per 16 permutations and its two
// label words bring 16 label pairs.  Each of the 16 permutations has its own T x T histogram in LDS; lane l handles them
// in the rotated order (s + l) % 16, so that a wavefront's 64 atomics of one step spread over 16 histograms (what
// k_enrich's 16 private copies did).
#define ENR16_MAX_TT 768   // 16 histograms of <= 768 bins: 48 KB of LDS (T <= 27)

__global__ __launch_bounds__(256) void k_enrich16(const int32_t *__restrict__ erow_r, const int32_t *__restrict__ ecol_r,
                                                  int64_t nnz, const uint4 *__restrict__ lab16, int64_t n, int n_types,
                                                  int hstride, int rows, unsigned long long *__restrict__ counts)
{
    extern __shared__ unsigned int hist[];   // [16][hstride]
    const int g = blockIdx.x;
    const int tt = n_types * n_types;
    for (int k = threadIdx.x; k < 16 * hstride; k += 256) hist[k] = 0;
    __syncthreads();
    const uint4 *lp = lab16 + (int64_t)g * n;
    const int rot = threadIdx.x & 15;
    const int64_t e0 = (int64_t)blockIdx.y * ENR_EDGES_PER_BLOCK;
    const int64_t e1 = e0 + ENR_EDGES_PER_BLOCK < nnz ? e0 + ENR_EDGES_PER_BLOCK : nnz;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
        const uint4 a = lp[erow_r[e]], b = lp[ecol_r[e]];
        const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int p = (s + rot) & 15;
            const uint32_t la = (aw[p >> 2] >> (8 * (p & 3))) & 0xffu, lb = (bw[p >> 2] >> (8 * (p & 3))) & 0xffu;
            atomicAdd(&hist[p * hstride + (int)la * n_types + (int)lb], 1u);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 16 * tt; k += 256) {
        const int p = k / tt, bin = k - p * tt;
        const unsigned int v = hist[p * hstride + bin];
        if (v && 16 * g + p < rows) atomicAdd(&counts[(int64_t)(16 * g + p) * tt + bin], (unsigned long long)v);
    }
}

extern "C" int sc_enrichment_counter(sc_ctx *c, const int32_t *labels, int64_t n, int32_t n_types, uint64_t seed,
                                     int64_t p_first, int64_t n_perm, int64_t batch, int64_t *observed_out, int64_t *sums_out)
{
    SC_REQUIRE(c && labels && observed_out && sums_out, SC_ERR_INVALID, "sc_enrichment_counter: null pointer");
    SC_HIP(hipSetDevice(c->device));
    SC_REQUIRE(c->g_n > 0 && n == c->g_n, SC_ERR_STATE, "sc_enrichment_counter: graph missing or size mismatch");
    SC_REQUIRE(n_types >= 1 && n_types <= 96, SC_ERR_INVALID, "sc_enrichment_counter: n_types must be 1..96");
    SC_REQUIRE(n_perm >= 0 && p_first >= 0 && batch >= 1 && batch <= 65534, SC_ERR_INVALID, "sc_enrichment_counter: bad sizes");
    SC_REQUIRE(ceil_div64(c->g_nnz, ENR_EDGES_PER_BLOCK) <= 65535, SC_ERR_INVALID, "sc_enrichment_counter: more than 4.2e9 edges");
    SC_TRY(lp_upload_labels(c, labels, n, n_types));
    if (batch > n_perm) batch = n_perm > 0 ? n_perm : 1;
    const int tt = n_types * n_types;
    const int64_t lstride = align_up64(n, 16);
    const size_t cnt_bytes = sizeof(unsigned long long) * (size_t)tt * (size_t)batch;
    SC_TRY(c->scratch_b.ensure(cnt_bytes + sizeof(unsigned long long) * (size_t)tt * 4, &c->mem));   // counts | observed | 3 sums
    SC_TRY(c->scratch_a.ensure((size_t)lstride * (size_t)align_up64(batch, 16), &c->mem));   // (also the 16-wide form: n x 16 B per 16 rows)
    unsigned long long *d_cnt = c->scratch_b.as<unsigned long long>(), *d_obs = d_cnt + (size_t)tt * batch;
    long long *d_sums = reinterpret_cast<long long *>(d_obs + tt);
    SC_TRY(sc_graph_ensure_order(c));
    SC_HIP(hipMemsetAsync(d_obs, 0, sizeof(unsigned long long) * (size_t)tt * 4, c->stream));
    int copies = 16;
    const int cstride = tt | 1;   // odd: copy c starts at a different LDS bank
    while (copies > 1 && (size_t)copies * cstride > 12288) copies >>= 1;   // <= 48 KB of LDS per workgroup
    const unsigned eblocks = (unsigned)ceil_div64(c->g_nnz, ENR_EDGES_PER_BLOCK);
    const bool wide = tt <= ENR16_MAX_TT;   // sixteen permutations per edge (k_enrich16)
    const int hstride = tt | 1;
    auto relabel = [&](int rows, const int32_t *table) {
        if (wide && table)
            lp_relabel_words(c, n, c->g_rank.as<int32_t>(), table, rows, c->scratch_a.as<uint4>());
        else
            hipLaunchKernelGGL(k_enrich_relabel, dim3((unsigned)ceil_div64(n, 1024), (unsigned)rows), dim3(256), 0, c->stream,
                               c->scratch_idx.as<unsigned char>(), c->g_order.as<int32_t>(), table, c->p_stride, table ? rows : 0, n,
                               lstride, c->scratch_a.as<unsigned char>());
    };
    auto edges = [&](int rows, unsigned long long *out, bool from_table) {
        if (c->g_nnz <= 0) return;
        if (wide && from_table)
            hipLaunchKernelGGL(k_enrich16, dim3((unsigned)((rows + 15) / 16), eblocks), dim3(256), sizeof(unsigned int) * 16 * hstride,
                               c->stream, c->g_erow_r.as<int32_t>(), c->g_indices_r.as<int32_t>(), c->g_nnz, c->scratch_a.as<uint4>(), n,
                               (int)n_types, hstride, rows, out);
        else
            hipLaunchKernelGGL(k_enrich, dim3((unsigned)rows, eblocks), dim3(256), sizeof(unsigned int) * cstride * copies, c->stream,
                               c->g_erow_r.as<int32_t>(), c->g_indices_r.as<int32_t>(), c->g_nnz, c->scratch_a.as<unsigned char>(),
                               lstride, (int)n_types, copies, cstride, out);
    };
    // observed labels: one "permutation" without a table
    relabel(1, nullptr);
    edges(1, d_obs, false);
    SC_HIP(hipGetLastError());
    SC_TRY(lp_counter_batches(
        c, "sc_enrichment_counter", seed, n, p_first, n_perm, batch, [&](int rows) { relabel(rows, c->perm.as<int32_t>()); },
        [&](int rows) -> int {
            SC_HIP(hipMemsetAsync(d_cnt, 0, cnt_bytes, c->stream));
            edges(rows, d_cnt, true);
            return SC_OK;
        },
        [&](int rows) {
            hipLaunchKernelGGL(k_lp_sums, dim3((unsigned)ceil_div64(tt, 256)), dim3(256), 0, c->stream, d_cnt, d_obs, rows, tt, 1, 3,
                               d_sums);
        }));
    std::vector<unsigned long long> host((size_t)tt * 4);
    SC_HIP(hipMemcpy(host.data(), d_obs, sizeof(unsigned long long) * (size_t)tt * 4, hipMemcpyDeviceToHost));
    for (int k = 0; k < tt; ++k) observed_out[k] = (int64_t)host[(size_t)k];
    for (int k = 0; k < 3 * tt; ++k) sums_out[k] = (int64_t)host[(size_t)tt + k];
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
#define RIP_PAIRS_PER_BLOCK 65536
#define RIP_THREADS 512
#define RIP_LDS_WORDS 16384   // 64 KB of uint32 per workgroup: the limit on T (T + 1) / 2 * R

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
    SC_REQUIRE(ceil_div64(total, RIP_PAIRS_PER_BLOCK) <= 65535, SC_ERR_INVALID,
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
// counting
// ------------------------------------------------------------------------------------------------

// first histogram row of the unordered type pair (lo, hi), lo <= hi, of T types: rows (0,0) (0,1) .. (0,T-1) (1,1) ..
__host__ __device__ __forceinline__ int rip_tri(int lo, int hi, int T) { return ((lo * (2 * T + 1 - lo)) >> 1) + hi - lo; }

template <int NP> struct RipWord;
template <> struct RipWord<16> { typedef uint4 type; };
template <> struct RipWord<8> { typedef uint2 type; };
template <> struct RipWord<4> { typedef uint32_t type; };
template <> struct RipWord<2> { typedef uint16_t type; };
template <> struct RipWord<1> { typedef unsigned char type; };

// The NP label bytes of a position, rotated right by `rot` bytes: byte s of the result is the label under permutation
// (s + rot) % NP of the pass.  Built from word selects with static indices and v_alignbit_b32 with amounts 0 / 8 / 16 / 24
// (no per-lane indexing of a register array, which would go to scratch, and no per-lane 64-bit shift, see sc_ctx.h).
template <int NP> struct RipLabels { uint32_t r[NP >= 4 ? NP / 4 : 1]; };

__device__ __forceinline__ RipLabels<16> rip_rotated(const uint4 &w, int rot)
{
    const bool s1 = (rot >> 2) & 1, s2 = (rot >> 3) & 1;
    const uint32_t a0 = s1 ? w.y : w.x, a1 = s1 ? w.z : w.y, a2 = s1 ? w.w : w.z, a3 = s1 ? w.x : w.w;
    const uint32_t b0 = s2 ? a2 : a0, b1 = s2 ? a3 : a1, b2 = s2 ? a0 : a2, b3 = s2 ? a1 : a3;
    const uint32_t k = 8u * ((uint32_t)rot & 3u);
    RipLabels<16> o = {{__builtin_amdgcn_alignbit(b1, b0, k), __builtin_amdgcn_alignbit(b2, b1, k),
                        __builtin_amdgcn_alignbit(b3, b2, k), __builtin_amdgcn_alignbit(b0, b3, k)}};
    return o;
}
__device__ __forceinline__ RipLabels<8> rip_rotated(const uint2 &w, int rot)
{
    const bool s1 = (rot >> 2) & 1;
    const uint32_t a0 = s1 ? w.y : w.x, a1 = s1 ? w.x : w.y;
    const uint32_t k = 8u * ((uint32_t)rot & 3u);
    RipLabels<8> o = {{__builtin_amdgcn_alignbit(a1, a0, k), __builtin_amdgcn_alignbit(a0, a1, k)}};
    return o;
}
__device__ __forceinline__ RipLabels<4> rip_rotated(const uint32_t &w, int rot)
{
    RipLabels<4> o = {{__builtin_amdgcn_alignbit(w, w, 8u * ((uint32_t)rot & 3u))}};
    return o;
}
__device__ __forceinline__ RipLabels<2> rip_rotated(const uint16_t &w, int rot)
{
    const uint32_t v = (uint32_t)w | ((uint32_t)w << 16);
    RipLabels<2> o = {{v >> (8u * ((uint32_t)rot & 1u))}};
    return o;
}
__device__ __forceinline__ RipLabels<1> rip_rotated(const unsigned char &w, int) { RipLabels<1> o = {{w}}; return o; }

// counts[q NP + p][tri(lo, hi) R + bin] += #{pairs of the block with that unordered type pair under permutation q NP + p
// and that radius bin}.  Workgroup (q, pair block); consecutive workgroups are the passes of ONE pair block (its 9 bytes
// per pair come from L2 after the first).  The labels of a position are NP consecutive bytes at lab + group stride *
// (q NP / 16) + position * cell_bytes + (q NP) % 16: the 16-byte words of k_enrich_relabel16 (cell_bytes = 16), or the
// byte rows of k_enrich_relabel (NP = 1, cell_bytes = 1: the observed labels).  Lane l takes the permutations in the
// rotated order (s + l) % NP, so that the atomics of one step spread over NP histograms (k_enrich16's scheme).
template <int NP>
__global__ __launch_bounds__(RIP_THREADS) void k_ripley(const int32_t *__restrict__ prow, const int32_t *__restrict__ pcol,
                                                         const unsigned char *__restrict__ pbin, int64_t n_pairs,
                                                         const unsigned char *__restrict__ lab, int64_t gstride, int cell_bytes,
                                                         int n_types, int n_radii, int hstride, int rows,
                                                         unsigned long long *__restrict__ counts)
{
    typedef typename RipWord<NP>::type word_t;
    extern __shared__ unsigned int hist[];   // [NP][hstride]
    const int q = blockIdx.x;
    const int cells = ((n_types * (n_types + 1)) >> 1) * n_radii;
    for (int k = threadIdx.x; k < NP * hstride; k += RIP_THREADS) hist[k] = 0;
    __syncthreads();
    const unsigned char *lp = lab + (int64_t)((q * NP) >> 4) * gstride + ((q * NP) & 15);
    const int rot = threadIdx.x & (NP - 1);
    const int two_t1 = 2 * n_types + 1;
    const int64_t e0 = (int64_t)blockIdx.y * RIP_PAIRS_PER_BLOCK;
    const int64_t e1 = e0 + RIP_PAIRS_PER_BLOCK < n_pairs ? e0 + RIP_PAIRS_PER_BLOCK : n_pairs;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += RIP_THREADS) {
        const word_t a = *reinterpret_cast<const word_t *>(lp + (int64_t)prow[e] * cell_bytes);
        const word_t b = *reinterpret_cast<const word_t *>(lp + (int64_t)pcol[e] * cell_bytes);
        const int bin = pbin[e];
        const RipLabels<NP> ra = rip_rotated(a, rot), rb = rip_rotated(b, rot);
#pragma unroll
        for (int s = 0; s < NP; ++s) {
            const int p = (s + rot) & (NP - 1);
            const int la = (int)((ra.r[s >> 2] >> (8 * (s & 3))) & 0xffu), lb = (int)((rb.r[s >> 2] >> (8 * (s & 3))) & 0xffu);
            const int lo = la < lb ? la : lb, hi = la < lb ? lb : la;
            atomicAdd(&hist[p * hstride + (((lo * (two_t1 - lo)) >> 1) + hi - lo) * n_radii + bin], 1u);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < NP * cells; k += RIP_THREADS) {
        const int p = k / cells, cell = k - p * cells;
        const unsigned int v = hist[p * hstride + cell];
        if (v && q * NP + p < rows) atomicAdd(&counts[(int64_t)(q * NP + p) * cells + cell], (unsigned long long)v);
    }
}

namespace {

struct RipPlan {
    int T = 0, R = 0, cells = 0;   // cells = T (T + 1) / 2 * R: words of one histogram
    int np = 1, hstride = 0;       // permutations per pass over the pairs, histogram stride in words
    unsigned pblocks = 0;
};

// what both counting entry points check: the pair list, the labels (uploaded to scratch_idx), the shape
int rip_prepare(sc_ctx *c, const char *who, const int32_t *labels, int64_t n, int32_t n_types, RipPlan *plan)
{
    SC_REQUIRE(n_types >= 1 && n_types <= 96, SC_ERR_INVALID, "%s: n_types must be 1..96, got %d", who, (int)n_types);
    SC_REQUIRE(c->rp_valid, SC_ERR_STATE,
               "%s: no pair list (call sc_ripley_build first; a neighbour search since then has replaced its bins)", who);
    SC_REQUIRE(n == c->rp_n, SC_ERR_STATE, "%s: %lld labels for a pair list of %lld cells", who, (long long)n,
               (long long)c->rp_n);
    const int64_t cells = (int64_t)n_types * (n_types + 1) / 2 * c->rp_radii;
    SC_REQUIRE(cells <= RIP_LDS_WORDS, SC_ERR_INVALID,
               "%s: n_types (n_types + 1) / 2 * n_radii = %lld exceeds the limit of %d histogram words (64 KB of LDS); "
               "n_types = %d, n_radii = %d", who, (long long)cells, RIP_LDS_WORDS, (int)n_types, c->rp_radii);
    SC_TRY(lp_upload_labels(c, labels, n, n_types));
    plan->T = n_types;
    plan->R = c->rp_radii;
    plan->cells = (int)cells;
    // the largest NP whose NP histograms (stride odd: histogram p starts at a different bank) fit 64 KB
    int np = 16;
    while (np > 1 && (int64_t)np * (cells | 1) > RIP_LDS_WORDS) np >>= 1;
    plan->np = np;
    plan->hstride = np > 1 ? (int)(cells | 1) : (int)cells;
    plan->pblocks = (unsigned)ceil_div64(c->rp_pairs, RIP_PAIRS_PER_BLOCK);
    return SC_OK;
}

// the observed labels by position (k_enrich_relabel's identity row) into labp, their pair counts into out
void rip_observed(sc_ctx *c, const RipPlan &pl, int64_t n, unsigned char *labp, unsigned long long *out)
{
    hipLaunchKernelGGL(k_enrich_relabel, dim3((unsigned)ceil_div64(n, 1024), 1u), dim3(256), 0, c->stream,
                       c->scratch_idx.as<unsigned char>(), c->sid.as<int32_t>(), (const int32_t *)nullptr, (int64_t)0, 0, n,
                       align_up64(n, 16), labp);
    if (c->rp_pairs > 0)
        hipLaunchKernelGGL(k_ripley<1>, dim3(1u, pl.pblocks), dim3(RIP_THREADS), sizeof(unsigned int) * (size_t)pl.cells, c->stream,
                           c->rp_row.as<int32_t>(), c->rp_col.as<int32_t>(), c->rp_bin.as<unsigned char>(), c->rp_pairs, labp,
                           (int64_t)0, 1, pl.T, pl.R, pl.cells, 1, out);
}

// `rows` rows of the permutation table -> 16-byte label words in scratch_a
void rip_relabel_words(sc_ctx *c, int64_t n, const int32_t *table, int rows)
{
    lp_relabel_words(c, n, c->rp_rank.as<int32_t>(), table, rows, c->scratch_a.as<uint4>());
}

// ... -> out[rows][cells], NP permutations per pass over the pairs
void rip_count_words(sc_ctx *c, const RipPlan &pl, int64_t n, int rows, unsigned long long *out)
{
    if (c->rp_pairs <= 0) return;
    const dim3 grid((unsigned)((rows + pl.np - 1) / pl.np), pl.pblocks);
    const size_t lds = sizeof(unsigned int) * (size_t)pl.np * pl.hstride;
#define RIP_LAUNCH(NP)                                                                                                  \
    hipLaunchKernelGGL(k_ripley<NP>, grid, dim3(RIP_THREADS), lds, c->stream, c->rp_row.as<int32_t>(), c->rp_col.as<int32_t>(), \
                       c->rp_bin.as<unsigned char>(), c->rp_pairs, c->scratch_a.as<unsigned char>(), (int64_t)n * 16, 16, pl.T, pl.R, \
                       pl.hstride, rows, out)
    switch (pl.np) {
    case 16: RIP_LAUNCH(16); break;
    case 8: RIP_LAUNCH(8); break;
    case 4: RIP_LAUNCH(4); break;
    case 2: RIP_LAUNCH(2); break;
    default: RIP_LAUNCH(1); break;
    }
#undef RIP_LAUNCH
}

// unordered table u[pair][j] -> ordered table out[a][b][j].  cumulate: u holds the non-cumulative counts of the kernel
// (k_lp_sums' rows are sums over the cumulative counts already: false).  `diag`: the factor of the diagonal, 2 for
// counts and deviation sums, 4 for squared deviations, 1 for exceedance counts
void rip_expand(const RipPlan &pl, const unsigned long long *u, bool cumulate, long long diag, int64_t *out)
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
    SC_REQUIRE(n_perm >= 0 && perm_row0 >= 0, SC_ERR_INVALID, "sc_ripley_counts: negative size");
    SC_REQUIRE(n_perm + 1 <= 65535, SC_ERR_INVALID,
               "sc_ripley_counts: at most 65534 permutations per call (got %lld); call it per batch of the table", (long long)n_perm);
    SC_HIP(hipSetDevice(c->device));
    RipPlan pl;
    SC_TRY(rip_prepare(c, "sc_ripley_counts", labels, n, n_types, &pl));
    if (n_perm > 0) {
        SC_TRY(sc_perm_forward_ensure(c));
        SC_REQUIRE(c->p_n == n && perm_row0 + n_perm <= c->p_count, SC_ERR_STATE,
                   "sc_ripley_counts: needs permutation rows [%lld, %lld)", (long long)perm_row0, (long long)(perm_row0 + n_perm));
    }
    const size_t words = (size_t)pl.cells * (size_t)(n_perm + 1);
    const int64_t lstride = align_up64(n, 16);
    SC_TRY(c->scratch_b.ensure(sizeof(unsigned long long) * words, &c->mem));
    // [16-byte label words of the table rows | observed labels by position]
    const size_t word_bytes = (size_t)n * 16 * (size_t)((n_perm + 15) / 16);
    SC_TRY(c->scratch_a.ensure(word_bytes + (size_t)lstride, &c->mem));
    unsigned long long *d_cnt = c->scratch_b.as<unsigned long long>();
    SC_HIP(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * words, c->stream));
    if (n_perm > 0) {
        rip_relabel_words(c, n, c->perm.as<int32_t>() + perm_row0 * c->p_stride, (int)n_perm);
        rip_count_words(c, pl, n, (int)n_perm, d_cnt);
    }
    rip_observed(c, pl, n, c->scratch_a.as<unsigned char>() + word_bytes, d_cnt + (size_t)pl.cells * (size_t)n_perm);
    SC_HIP(hipGetLastError());
    std::vector<unsigned long long> host(words);
    SC_HIP(hipMemcpyAsync(host.data(), d_cnt, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    const size_t ttr = (size_t)pl.T * pl.T * pl.R;
    for (int64_t p = 0; p <= n_perm; ++p) rip_expand(pl, host.data() + (size_t)p * pl.cells, true, 2, counts_out + (size_t)p * ttr);
    return SC_OK;
}

extern "C" int sc_ripley_counter(sc_ctx *c, const int32_t *labels, int64_t n, int32_t n_types, uint64_t seed, int64_t p_first,
                                 int64_t n_perm, int64_t batch, int64_t *observed_out, int64_t *sums_out)
{
    SC_REQUIRE(c && labels && observed_out && sums_out, SC_ERR_INVALID, "sc_ripley_counter: null pointer");
    SC_REQUIRE(n_perm >= 0 && p_first >= 0 && batch >= 1 && batch <= 65534, SC_ERR_INVALID, "sc_ripley_counter: bad sizes");
    SC_HIP(hipSetDevice(c->device));
    RipPlan pl;
    SC_TRY(rip_prepare(c, "sc_ripley_counter", labels, n, n_types, &pl));
    if (batch > n_perm) batch = n_perm > 0 ? n_perm : 1;
    const int cells = pl.cells;
    const int64_t lstride = align_up64(n, 16);
    const size_t cnt_bytes = sizeof(unsigned long long) * (size_t)cells * (size_t)batch;
    SC_TRY(c->scratch_b.ensure(cnt_bytes + sizeof(unsigned long long) * (size_t)cells * 5, &c->mem));   // counts | observed | 4 sums
    const size_t word_bytes = (size_t)n * 16 * (size_t)((batch + 15) / 16);
    SC_TRY(c->scratch_a.ensure(word_bytes > (size_t)lstride ? word_bytes : (size_t)lstride, &c->mem));
    unsigned long long *d_cnt = c->scratch_b.as<unsigned long long>(), *d_obs = d_cnt + (size_t)cells * batch;
    long long *d_sums = reinterpret_cast<long long *>(d_obs + cells);
    SC_HIP(hipMemsetAsync(d_obs, 0, sizeof(unsigned long long) * (size_t)cells * 5, c->stream));
    rip_observed(c, pl, n, c->scratch_a.as<unsigned char>(), d_obs);   // (the label words of batch 0 follow on the same stream)
    SC_HIP(hipGetLastError());
    SC_TRY(lp_counter_batches(
        c, "sc_ripley_counter", seed, n, p_first, n_perm, batch, [&](int rows) { rip_relabel_words(c, n, c->perm.as<int32_t>(), rows); },
        [&](int rows) -> int {
            SC_HIP(hipMemsetAsync(d_cnt, 0, cnt_bytes, c->stream));
            rip_count_words(c, pl, n, rows, d_cnt);
            return SC_OK;
        },
        [&](int rows) {
            hipLaunchKernelGGL(k_lp_sums, dim3((unsigned)ceil_div64(cells, 256)), dim3(256), 0, c->stream, d_cnt, d_obs, rows, cells,
                               pl.R, 4, d_sums);
        }));
    std::vector<unsigned long long> host((size_t)cells * 5);
    SC_HIP(hipMemcpy(host.data(), d_obs, sizeof(unsigned long long) * (size_t)cells * 5, hipMemcpyDeviceToHost));
    const size_t ttr = (size_t)pl.T * pl.T * pl.R;
    rip_expand(pl, host.data(), true, 2, observed_out);
    // the sums are those of the cumulative UNORDERED counts u; a diagonal ordered count is 2 u: deviations double,
    // their squares quadruple, the comparisons stay
    rip_expand(pl, host.data() + (size_t)cells * 1, false, 2, sums_out);
    rip_expand(pl, host.data() + (size_t)cells * 2, false, 4, sums_out + ttr);
    rip_expand(pl, host.data() + (size_t)cells * 3, false, 1, sums_out + 2 * ttr);
    rip_expand(pl, host.data() + (size_t)cells * 4, false, 1, sums_out + 3 * ttr);
    return SC_OK;
}
