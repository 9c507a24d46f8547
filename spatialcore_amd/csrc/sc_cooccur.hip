// Cell-type co-occurrence by distance (extension N9; squidpy's co_occurrence): the pair counts behind it, every pair of
// cells in one streaming all-pairs pass.  gfx950 only.
//
// Definition.  n points in 2-D (fp64), sorted by type with offsets type_off[T + 1], thresholds t_0 < t_1 < ... < t_R
// (fp64, finite, t_0 >= 0; 2 <= R + 1 <= 128), T2[j] = fl(t_j t_j) computed once on the host.
//  - For an ordered pair (i, i'), i != i': d2 = fl(fl(dx dx) + fl(dy dy)) -- BinGrid::dist2, the project's one distance.
//  - The pair's bin is the smallest j with d2 <= T2[j]: the closed-ball predicate of sc_radius_count_2d and
//    sc_ripley_build.  A pair with d2 > T2[R] is dropped.
//  - count[a][b][j] = ordered pairs of types (a, b) in bin j, int64.  Bin 0 holds the pairs within t_0, bins 1 .. R the
//    annuli (t_{j-1}, t_j].
//  Hence count[a][b][j] == count[b][a][j]; the prefix sum over j, summed over a and b, is the nnz of the radius graph
//  at t_j; coincident points (d2 == 0) land in bin 0; the table is identical from run to run and does not depend on
//  the order of the cells (integer adds only).
//
// Kernel.  The shape of k_pair_table (sc_search.hip): the points are cut into chunks of <= 256 that never straddle a
// type, one source point per lane in registers, the target type streamed through an LDS tile as double2.  Every
// UNORDERED pair is evaluated once: workgroup (chunk, target type b) runs only for b >= the chunk's type a, and in the
// block b == a a lane visits only the positions behind its own.  The host mirrors the table and doubles its diagonal.
//  - Bin search: T2, padded with +inf to P - 1 keys (P the power of two with P - 1 >= R + 1), lies in LDS as the
//    implicit search tree of a binary search (node i has the children 2 i and 2 i + 1; level l is the contiguous
//    range [2^l, 2^(l+1))): node = 2 node + (key[node] < d2), log2(P) times, ends on leaf P + #{j : T2[j] < d2}, which
//    is P + the smallest j with d2 <= T2[j] (R + 1 for a dropped pair).  Exact compares against T2, no branch, and the
//    nodes a wavefront reads at one level are neighbours in LDS.  CO_UNROLL pairs are searched side by side so that the
//    dependent LDS reads of one search overlap those of the others.
//  - Histogram: one per workgroup, uint32 hist[bin][32] -- lane l adds into column l % 32, so the 32 lanes that an LDS
//    instruction serves in one cycle hit 32 different banks whatever their bins are; the adds are LDS integer atomics
//    (lanes l and l + 32, and the four wavefronts, share a column).  It is emptied into one 64-bit register per bin at
//    every tile, and the workgroup leaves with 64-bit global integer atomics.  No floating-point atomics anywhere.
#include <math.h>

#include <vector>

#include "sc_search.h"

#define CO_TILE 1024        // target points per LDS tile
#define CO_COLS 32          // histogram columns per bin: one per LDS bank
#define CO_MAX_THR 128      // thresholds (bins) at most
#define CO_UNROLL 4         // pairs per lane searched side by side

__global__ __launch_bounds__(256) void k_cooccur(const double2 *__restrict__ xy, const int64_t *__restrict__ chunk_a0,
                                                 const int32_t *__restrict__ chunk_cnt,
                                                 const int32_t *__restrict__ chunk_type,
                                                 const int64_t *__restrict__ type_off, int n_types,
                                                 const double *__restrict__ tree, int levels, int n_thr,
                                                 unsigned long long *__restrict__ counts)
{
    __shared__ double2 tile[CO_TILE];
    __shared__ double key[2 * CO_MAX_THR];            // the search tree: key[1 .. P - 1]
    __shared__ uint32_t hist[CO_MAX_THR * CO_COLS];
    const int a = chunk_type[blockIdx.x], b = (int)blockIdx.y;
    if (b < a) return;                                 // the mirror image of workgroup (chunk of b, a)
    const int tid = (int)threadIdx.x;
    const int64_t a0 = chunk_a0[blockIdx.x], b1 = type_off[b + 1];
    const int64_t own = a0 + tid;
    // the first target position: the type's first one, or (own type) the one behind the chunk's first point
    const int64_t j_begin = a == b ? a0 + 1 : type_off[b];
    if (j_begin >= b1) return;
    const bool live = tid < chunk_cnt[blockIdx.x];
    const double2 src = live ? xy[own] : make_double2(0.0, 0.0);
    // the first target position this lane visits (own type: the one behind its own; a lane without a point: none)
    const int64_t visit_from = !live ? INT64_MAX : (a == b ? own + 1 : j_begin);
    const int P = 1 << levels;
    for (int i = tid; i < P; i += 256) key[i] = tree[i];
    for (int i = tid; i < n_thr * CO_COLS; i += 256) hist[i] = 0u;
    const uint32_t leaf8_end = 8u * (uint32_t)(P + n_thr);
    const uint32_t col_bytes = 4u * (uint32_t)(tid & (CO_COLS - 1)) - 4u * CO_COLS * (uint32_t)P;   // (mod 2^32: 16 * node8 >= 128 P)
    unsigned long long acc = 0;                        // thread t < n_thr owns bin t
    // bin t of the histogram into its owner's register, columns in the rotated order (t + s) % 32: the lanes of a
    // wavefront read 32 different banks
    auto flush = [&]() {
        if (tid < n_thr) {
            uint32_t s = 0;
            for (int q = 0; q < CO_COLS; ++q) {
                const int at = tid * CO_COLS + ((tid + q) & (CO_COLS - 1));
                s += hist[at];
                hist[at] = 0u;
            }
            acc += s;
        }
    };
    for (int64_t j0 = j_begin; j0 < b1; j0 += CO_TILE) {
        const int cnt = (int)(b1 - j0 < CO_TILE ? b1 - j0 : CO_TILE);
        const int cnt_up = (cnt + CO_UNROLL - 1) / CO_UNROLL * CO_UNROLL;
        __syncthreads();     // the tile before is read, its adds are in the histogram (first round: key and hist are written)
        // A uint32 counter cannot overflow: a column takes the adds of 8 lanes (l and l + 32 of four wavefronts), each at
        // most one per target point, and the histogram is emptied at every tile: at most 8 * CO_TILE = 8192 per counter,
        // and 32 * 8192 = 2^18 in the sum s of a bin's columns.
        flush();
        // a tile is padded to a multiple of CO_UNROLL with points at infinity: d2 = +inf, beyond every threshold
        for (int k = tid; k < cnt_up; k += 256) tile[k] = k < cnt ? xy[j0 + k] : make_double2(HUGE_VAL, HUGE_VAL);
        __syncthreads();
        const int64_t rel = visit_from - j0;
        const int first = rel <= 0 ? 0 : (rel >= CO_TILE ? CO_TILE : (int)rel);
        for (int k = 0; k < cnt_up; k += CO_UNROLL) {
            double d2[CO_UNROLL];
            uint32_t node8[CO_UNROLL];      // 8 * node: the node's byte offset in key[]
#pragma unroll
            for (int u = 0; u < CO_UNROLL; ++u) {
                const double2 q = tile[k + u];
                d2[u] = BinGrid::dist2(src.x, src.y, q.x, q.y);
                node8[u] = 8u;
            }
            for (int l = 0; l < levels; ++l) {
#pragma unroll
                for (int u = 0; u < CO_UNROLL; ++u) {
                    const double kv = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(key) + node8[u]);
                    node8[u] = 2u * node8[u] + (kv < d2[u] ? 8u : 0u);
                }
            }
            // leaf P + bin, bin < n_thr for a pair in range; its counter hist[bin][col] lies 16 * node8 - 128 * P + 4 * col bytes
            // into the histogram
#pragma unroll
            for (int u = 0; u < CO_UNROLL; ++u)
                if ((node8[u] < leaf8_end) & (k + u >= first))
                    atomicAdd(reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(hist) + (16u * node8[u] + col_bytes)), 1u);
        }
    }
    __syncthreads();
    flush();
    if (tid < n_thr && acc) atomicAdd(&counts[((int64_t)a * n_types + b) * n_thr + tid], acc);
}

extern "C" int sc_cooccurrence_2d(sc_ctx *c, const double *xy, const int64_t *type_off, int32_t n_types,
                                  const double *thresholds, int32_t n_thresholds, int64_t *counts_out)
{
    SC_REQUIRE(c && xy && type_off && thresholds && counts_out, SC_ERR_INVALID, "sc_cooccurrence_2d: null pointer");
    SC_REQUIRE(n_types >= 1 && n_types <= 65535, SC_ERR_INVALID, "sc_cooccurrence_2d: n_types=%d out of range (1..65535)",
               n_types);
    SC_REQUIRE(type_off[0] == 0, SC_ERR_INVALID, "sc_cooccurrence_2d: offsets must start at 0");
    for (int g = 0; g < n_types; ++g)
        SC_REQUIRE(type_off[g + 1] >= type_off[g], SC_ERR_INVALID, "sc_cooccurrence_2d: offsets not monotone at type %d", g);
    const int64_t n = type_off[n_types];
    SC_REQUIRE(n >= 1 && n <= 0x7fffffffLL, SC_ERR_INVALID, "sc_cooccurrence_2d: n=%lld out of range", (long long)n);
    SC_REQUIRE(n_thresholds >= 2 && n_thresholds <= CO_MAX_THR, SC_ERR_INVALID,
               "sc_cooccurrence_2d: n_thresholds=%d out of range (2..%d)", n_thresholds, CO_MAX_THR);
    for (int j = 0; j < n_thresholds; ++j) {
        const double t = thresholds[j];
        SC_REQUIRE(isfinite(t) && isfinite(t * t), SC_ERR_INVALID,
                   "sc_cooccurrence_2d: threshold %d = %g is not finite or has no finite square", j, t);
        SC_REQUIRE(t >= 0.0, SC_ERR_INVALID, "sc_cooccurrence_2d: threshold %d = %g is negative", j, t);
        SC_REQUIRE(j == 0 || t > thresholds[j - 1], SC_ERR_INVALID,
                   "sc_cooccurrence_2d: thresholds must be strictly increasing, got %g after %g", t, j ? thresholds[j - 1] : 0.0);
    }
    SC_TRY(require_finite_points("sc_cooccurrence_2d", "point", xy, n));
    SC_HIP(hipSetDevice(c->device));

    // the search tree over T2 = fl(t t), padded with +inf: node i of level l (i = 2^l + m) holds key (2 m + 1) P / 2^(l+1) - 1
    int levels = 1;
    while ((1 << levels) - 1 < n_thresholds) ++levels;
    const int P = 1 << levels;
    std::vector<double> tree((size_t)P, 0.0);
    for (int l = 0; l < levels; ++l)
        for (int m = 0; m < (1 << l); ++m) {
            const int j = (2 * m + 1) * (P >> (l + 1)) - 1;
            tree[(size_t)(1 << l) + m] = j < n_thresholds ? thresholds[j] * thresholds[j] : HUGE_VAL;
        }
    std::vector<int64_t> ch0;
    std::vector<int32_t> chn, chg;
    for (int g = 0; g < n_types; ++g)
        for (int64_t p = type_off[g]; p < type_off[g + 1]; p += 256) {
            ch0.push_back(p);
            chn.push_back((int32_t)(type_off[g + 1] - p < 256 ? type_off[g + 1] - p : 256));
            chg.push_back(g);
        }
    const size_t chunks = ch0.size();
    const size_t table = (size_t)n_types * (size_t)n_types * (size_t)n_thresholds;
    // scratch that no entry point keeps anything in: neither the bin grid, nor the active graph, nor the Ripley pair
    // list is touched
    SC_TRY(c->e_tmp_data.ensure(sizeof(double) * (2 * (size_t)n + (size_t)P), &c->mem));
    SC_TRY(c->e_tmp_indptr.ensure(sizeof(int64_t) * (chunks + (size_t)n_types + 1), &c->mem));
    SC_TRY(c->e_tmp_indices.ensure(sizeof(int32_t) * 2 * chunks, &c->mem));
    SC_TRY(c->scratch_out.ensure(sizeof(int64_t) * table, &c->mem));
    double *d_xy = c->e_tmp_data.as<double>(), *d_tree = d_xy + 2 * n;
    int64_t *d_ch0 = c->e_tmp_indptr.as<int64_t>(), *d_off = d_ch0 + chunks;
    int32_t *d_chn = c->e_tmp_indices.as<int32_t>(), *d_chg = d_chn + chunks;
    SC_HIP(hipMemcpyAsync(d_xy, xy, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(d_tree, tree.data(), sizeof(double) * (size_t)P, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(d_ch0, ch0.data(), sizeof(int64_t) * chunks, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(d_off, type_off, sizeof(int64_t) * (size_t)(n_types + 1), hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(d_chn, chn.data(), sizeof(int32_t) * chunks, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(d_chg, chg.data(), sizeof(int32_t) * chunks, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemsetAsync(c->scratch_out.p, 0, sizeof(int64_t) * table, c->stream));
    {
        KernelTimerScope ts(c, SC_K_COOCCUR);
        hipLaunchKernelGGL(k_cooccur, dim3((unsigned)chunks, (unsigned)n_types), dim3(256), 0, c->stream,
                           reinterpret_cast<const double2 *>(d_xy), d_ch0, d_chn, d_chg, d_off, (int)n_types, d_tree, levels,
                           (int)n_thresholds, c->scratch_out.as<unsigned long long>());
    }
    SC_HIP(hipGetLastError());
    // the device filled the blocks a <= b with every unordered pair once
    SC_HIP(hipMemcpyAsync(counts_out, c->scratch_out.p, sizeof(int64_t) * table, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    const size_t T = (size_t)n_types, R1 = (size_t)n_thresholds;
    for (size_t a = 0; a < T; ++a) {
        for (size_t j = 0; j < R1; ++j) counts_out[(a * T + a) * R1 + j] *= 2;
        for (size_t b = a + 1; b < T; ++b)
            for (size_t j = 0; j < R1; ++j) counts_out[(b * T + a) * R1 + j] = counts_out[(a * T + b) * R1 + j];
    }
    return SC_OK;
}
