// N11: cross-type nearest-neighbour G function with a label-permutation null (extension: the reference has no
// point-pattern statistic; spatstat's Gcross, squidpy's ripley(mode="G")).  gfx950 only.
//
// Definition (include/spatialcore_hip.h, "N11"): count[a][b][j] = number of cells i of type a with at least one OTHER
// cell i' != i of type b within fl(fl(dx dx) + fl(dy dy)) <= fl(r_j r_j) -- the closed ball of sc_radius_count_2d,
// cumulative in j, not symmetric in (a, b).  It is a minimum per cell (the radius index of the nearest b), not a sum
// over pairs, so the pair-count kernel of sc_labelperm.hip cannot produce it.
//
//  * list build: two passes over the bin grid like k_ripley_pairs (count, exclusive scan, fill), one thread per point
//    over its whole window (window_walk<false>, the point itself skipped by position): every ORDERED pair once, as a
//    row per position.  An entry is 5 bytes: the int32 position of the neighbour and ONE BYTE, the index of the smallest
//    radius that contains the pair; a row starts at an int64 offset.  The fill thread then puts its own row in
//    non-decreasing order of that byte (selection passes, one per radius index, over the part of the row not yet placed:
//    the order inside one radius index is free, the statistic cannot see it).
//  * counting: one thread per position and NP permutations per pass.  Because a row is ordered by radius index, the first
//    entry whose label is b IS the nearest b of the cell: the state per (cell, permutation) is one bitmask of the types
//    already seen, a new bit costs one LDS atomicAdd at hist[s][(a T + b) R + bin], and the walk ends once every
//    permutation's mask holds every type that occurs.  At most T atomics per cell and permutation, whatever the row
//    length.  Per-permutation uint32 histograms in LDS at an odd stride, flushed per cell block to uint64 global
//    counters: integer atomics only, order-free, bit-identical run to run.
//  * the cumulative sum over j happens once, at the end (k_lp_sums cumulates for itself).
#include <math.h>

#include <vector>

#include "sc_labelperm.h"
#include "sc_search.h"

#define RG_MAX_RADII 32
#define RG_MAX_TYPES 64          // one bit per type in two 32-bit mask words
#define RG_THREADS 512
#define RG_CELLS_PER_BLOCK 2048  // cells of one workgroup of k_rg_count: four per thread
#define RG_AHEAD 4               // row entries a thread of k_rg_count has in flight
#define RG_LDS_WORDS 16384       // 64 KB of uint32 per workgroup: the limit on the words of one histogram
#define RG_MAX_ENTRIES (65535LL * 65536LL)   // sc_ripley_build's limit on its stored pairs

struct RgR2 { double v[RG_MAX_RADII]; };

// FILL = false: counts[t] = positions s != t within the largest radius of position t; rank[cell at t] = t.
// FILL = true: the row of t at indptr[t] .., ordered by radius index.  t, s: positions in bin order.
template <bool FILL>
__global__ __launch_bounds__(256) void k_rg_list(BinGrid g, int64_t n, RgR2 r2, int n_radii, int rings,
                                                 long long *__restrict__ counts, const long long *__restrict__ indptr,
                                                 int32_t *col, unsigned char *bin, int32_t *__restrict__ rank)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double qx = g.sx[t], qy = g.sy[t];
    const double r2max = r2.v[n_radii - 1];
    long long cnt = 0;
    const long long base = FILL ? indptr[t] : 0;
    window_walk<false>(g, qx, qy, rings, (int)t, [&](int s) {
        if (s == (int)t) return;   // "other" is decided by index: a coincident cell counts
        const double d = BinGrid::dist2(qx, qy, g.sx[s], g.sy[s]);
        if (d <= r2max) {
            if (FILL) {
                int b = 0;
                for (int j = 0; j < n_radii - 1; ++j) b += d > r2.v[j] ? 1 : 0;
                col[base + cnt] = s;
                bin[base + cnt] = (unsigned char)b;
            }
            ++cnt;
        }
    });
    if (!FILL) {
        counts[t] = cnt;
        rank[g.sid[t]] = (int32_t)t;
        return;
    }
    // the thread's own row (its own stores, read back in program order) into non-decreasing radius index: pass j moves
    // the entries of index j to the front of what is left; everything in front of `cur` is placed
    const long long end = base + cnt;
    long long cur = base;
    for (int j = 0; j < n_radii - 1 && cur < end; ++j)
        for (long long e = cur; e < end; ++e)
            if (bin[e] == j) {
                if (e != cur) {
                    const int32_t c0 = col[cur];
                    const unsigned char b0 = bin[cur];
                    col[cur] = col[e];
                    bin[cur] = (unsigned char)j;
                    col[e] = c0;
                    bin[e] = b0;
                }
                ++cur;
            }
}

// counts[q NP + p][(a T + b) R + j] += #{cells of the block of label a under permutation q NP + p whose FIRST row entry of
// label b has radius index j}: the non-cumulative form of the table.  Workgroup blockIdx.x = cell block * groups + q:
// consecutive workgroups are the passes of ONE cell block (its rows come from L2 after the first).  The labels of a
// position are NP consecutive bytes at lab + group stride * (q NP / 16) + position * cell_bytes + (q NP) % 16: the 16-byte
// words of k_lp_relabel_words (cell_bytes = 16), or the byte row of k_lp_labels_by_position (NP = 1, cell_bytes = 1: the
// observed labels).  seen_lo / seen_hi: per unrolled permutation s the types the cell has met, bit (label & 31) of the
// word (label >> 5); WIDE = false (n_types <= 32) keeps one word.  Every index of the two arrays is a constant after
// unrolling (no per-lane indexing of a register array, which would go to scratch) and every shift is a 32-bit one with
// its amount in [0, 31] (no per-lane 64-bit shift, see sc_ctx.h).  full_lo / full_hi: the types that occur at all -- a
// permutation keeps them -- so a cell whose masks all equal them has nothing left to find.
template <int NP, bool WIDE>
__global__ __launch_bounds__(RG_THREADS) void k_rg_count(const long long *__restrict__ indptr, const int32_t *__restrict__ col,
                                                         const unsigned char *__restrict__ bin, int64_t n,
                                                         const unsigned char *__restrict__ lab, int64_t gstride, int cell_bytes,
                                                         int n_types, int n_radii, int hstride, int groups, int rows,
                                                         uint32_t full_lo, uint32_t full_hi,
                                                         unsigned long long *__restrict__ counts)
{
    typedef typename LpWord<NP>::type word_t;
    extern __shared__ unsigned int hist[];   // [NP][hstride]
    const int q = (int)(blockIdx.x % (unsigned)groups);
    const int64_t cb = (int64_t)(blockIdx.x / (unsigned)groups);
    const int cells = n_types * n_types * n_radii;
    for (int k = threadIdx.x; k < NP * hstride; k += RG_THREADS) hist[k] = 0;
    __syncthreads();
    const unsigned char *lp = lab + (int64_t)((q * NP) >> 4) * gstride + ((q * NP) & 15);
    const int64_t t0 = cb * RG_CELLS_PER_BLOCK;
    const int64_t t1 = t0 + RG_CELLS_PER_BLOCK < n ? t0 + RG_CELLS_PER_BLOCK : n;
    for (int64_t t = t0 + threadIdx.x; t < t1; t += RG_THREADS) {
        const word_t a = *reinterpret_cast<const word_t *>(lp + t * cell_bytes);
        uint32_t seen_lo[NP], seen_hi[NP];
#pragma unroll
        for (int s = 0; s < NP; ++s) seen_lo[s] = seen_hi[s] = 0u;
        const long long e1 = indptr[t + 1];
        // RG_AHEAD entries per step: their column loads, then their label gathers, are in flight together (with one entry
        // per step the walk ran at the latency of two dependent loads per entry).  Past the row's end the
        // last entry is taken again, which changes nothing: its type is in the mask already.
        for (long long e = indptr[t]; e < e1; e += RG_AHEAD) {
            word_t b[RG_AHEAD];
            int bj[RG_AHEAD];
#pragma unroll
            for (int u = 0; u < RG_AHEAD; ++u) {
                const long long eu = e + u < e1 ? e + u : e1 - 1;
                b[u] = *reinterpret_cast<const word_t *>(lp + (int64_t)col[eu] * cell_bytes);
                bj[u] = bin[eu];
            }
            uint32_t open = 0u;   // != 0: some permutation still misses a type
#pragma unroll
            for (int s = 0; s < NP; ++s) {
                const int la = lp_label(a, s);
#pragma unroll
                for (int u = 0; u < RG_AHEAD; ++u) {
                    const int lb = lp_label(b[u], s);
                    const uint32_t bit = 1u << (lb & 31);
                    const bool hi = WIDE && (lb & 32);
                    const uint32_t have = hi ? seen_hi[s] : seen_lo[s];
                    if (!(have & bit)) {
                        if (WIDE) seen_hi[s] |= hi ? bit : 0u;
                        seen_lo[s] |= hi ? 0u : bit;
                        atomicAdd(&hist[s * hstride + (la * n_types + lb) * n_radii + bj[u]], 1u);
                    }
                }
                open |= seen_lo[s] ^ full_lo;
                if (WIDE) open |= seen_hi[s] ^ full_hi;
            }
            if (!open) break;
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < NP * cells; k += RG_THREADS) {
        const int p = k / cells, cell = k - p * cells;
        const unsigned int v = hist[p * hstride + cell];
        if (v && q * NP + p < rows) atomicAdd(&counts[(int64_t)(q * NP + p) * cells + cell], (unsigned long long)v);
    }
}

extern "C" int sc_ripley_g_build(sc_ctx *c, const double *xy, int64_t n, const double *radii, int32_t n_radii,
                                 int64_t *n_entries_out)
{
    SC_REQUIRE(c && xy && radii && n_entries_out, SC_ERR_INVALID, "sc_ripley_g_build: null pointer");
    SC_REQUIRE(n_radii >= 1 && n_radii <= RG_MAX_RADII, SC_ERR_INVALID, "sc_ripley_g_build: 1..%d radii, got %d",
               RG_MAX_RADII, (int)n_radii);
    RgR2 r2;
    for (int j = 0; j < RG_MAX_RADII; ++j) r2.v[j] = 0.0;
    for (int j = 0; j < n_radii; ++j) {
        SC_REQUIRE(radii[j] > 0 && isfinite(radii[j]), SC_ERR_INVALID, "sc_ripley_g_build: radius %d must be > 0 and finite, got %g",
                   j, radii[j]);
        SC_REQUIRE(j == 0 || radii[j] > radii[j - 1], SC_ERR_INVALID,
                   "sc_ripley_g_build: radii must be strictly increasing (radius %d = %g after %g)", j, radii[j], radii[j - 1]);
        r2.v[j] = radii[j] * radii[j];   // fl(r r): nothing to contract (-ffp-contract=off)
        SC_REQUIRE(isfinite(r2.v[j]), SC_ERR_INVALID, "sc_ripley_g_build: radius %d squared is not finite (%g)", j, radii[j]);
    }
    SC_HIP(hipSetDevice(c->device));
    const double rmax = radii[n_radii - 1];
    // bins no smaller than the largest radius, as the radius graph and sc_ripley_build take them
    SC_TRY(sc_bin_points(c, xy, n, 4.0, rmax));
    const int rings = sc_window_rings(c, rmax);
    const BinGrid g = sc_bin_grid(c);
    SC_TRY(c->rg_cnt.ensure(sizeof(long long) * (size_t)(n + 1), &c->mem));
    SC_TRY(c->rg_indptr.ensure(sizeof(long long) * (size_t)(n + 1), &c->mem));
    SC_TRY(c->rg_rank.ensure(sizeof(int32_t) * (size_t)n, &c->mem));
    long long *counts = c->rg_cnt.as<long long>();
    SC_HIP(hipMemsetAsync(counts, 0, sizeof(long long) * (size_t)(n + 1), c->stream));
    const dim3 grid((unsigned)ceil_div64(n, 256));
    {
        KernelTimerScope ts(c, SC_K_RIPLEY_G_LIST);
        hipLaunchKernelGGL(k_rg_list<false>, grid, dim3(256), 0, c->stream, g, n, r2, (int)n_radii, rings, counts,
                           (const long long *)nullptr, (int32_t *)nullptr, (unsigned char *)nullptr, c->rg_rank.as<int32_t>());
    }
    SC_HIP(hipGetLastError());
    long long total = 0;
    SC_TRY(sc_counts_to_offsets(c, counts, c->rg_indptr.as<long long>(), n, &total));
    SC_HIP(hipStreamSynchronize(c->stream));
    SC_REQUIRE(total <= RG_MAX_ENTRIES, SC_ERR_INVALID,
               "sc_ripley_g_build: %lld ordered pairs within the largest radius, more than 4.2e9", total);
    const size_t cap = (size_t)(total > 0 ? total : 1);
    SC_TRY(c->rg_col.ensure(sizeof(int32_t) * cap, &c->mem));
    SC_TRY(c->rg_bin.ensure(cap, &c->mem));
    if (total > 0) {
        {
            KernelTimerScope ts(c, SC_K_RIPLEY_G_LIST);
            hipLaunchKernelGGL(k_rg_list<true>, grid, dim3(256), 0, c->stream, g, n, r2, (int)n_radii, rings, (long long *)nullptr,
                               c->rg_indptr.as<long long>(), c->rg_col.as<int32_t>(), c->rg_bin.as<unsigned char>(),
                               (int32_t *)nullptr);
        }
        SC_HIP(hipGetLastError());
        SC_HIP(hipStreamSynchronize(c->stream));
    }
    c->rg_n = n;
    c->rg_entries = total;
    c->rg_radii = n_radii;
    c->rg_valid = true;
    *n_entries_out = (int64_t)total;   // ordered pairs: nnz of the radius graph at the largest radius
    return SC_OK;
}

namespace {

struct RgPlan {
    int T = 0, R = 1, cells = 0;      // cells: words of one histogram, T T R
    int np = 1, hstride = 0;          // permutations per pass over the rows, histogram stride in words
    uint32_t full_lo = 0, full_hi = 0;   // the types that occur
    int64_t cblocks = 0;
};

// what both counting entry points check: the shape, the lists, the labels (uploaded to scratch_idx); max_rows: the most
// permutation rows one launch will take
int rg_prepare(sc_ctx *c, const char *who, const int32_t *labels, int64_t n, int32_t n_types, int64_t max_rows, RgPlan *pl)
{
    SC_REQUIRE(n_types >= 1, SC_ERR_INVALID, "%s: n_types must be >= 1, got %d", who, (int)n_types);
    SC_REQUIRE(n_types <= RG_MAX_TYPES, SC_ERR_INVALID,
               "%s: n_types = %d exceeds the limit of %d cell types (one bit per type in the mask of types a cell has met)", who,
               (int)n_types, RG_MAX_TYPES);
    SC_REQUIRE(c->rg_valid, SC_ERR_STATE,
               "%s: no list (call sc_ripley_g_build first; a neighbour search since then has replaced its bins)", who);
    SC_REQUIRE(n == c->rg_n, SC_ERR_STATE, "%s: %lld labels for lists of %lld cells", who, (long long)n, (long long)c->rg_n);
    const int64_t cells = (int64_t)n_types * n_types * c->rg_radii;
    SC_REQUIRE(cells <= RG_LDS_WORDS, SC_ERR_INVALID,
               "%s: n_types * n_types * n_radii = %lld exceeds the limit of %d histogram words (64 KB of LDS); "
               "n_types = %d, n_radii = %d", who, (long long)cells, RG_LDS_WORDS, (int)n_types, c->rg_radii);
    SC_TRY(lp_upload_labels(c, labels, n, n_types));
    pl->T = n_types;
    pl->R = c->rg_radii;
    pl->cells = (int)cells;
    // lp_plan's rule: the largest NP whose NP histograms (stride odd: histogram p starts at a different bank) fit 64 KB
    int np = 16;
    while (np > 1 && (int64_t)np * (cells | 1) > RG_LDS_WORDS) np >>= 1;
    pl->np = np;
    pl->hstride = np > 1 ? (int)(cells | 1) : (int)cells;
    uint64_t full = 0;
    for (int64_t i = 0; i < n; ++i) full |= 1ull << labels[i];
    pl->full_lo = (uint32_t)full;
    pl->full_hi = (uint32_t)(full >> 32);
    pl->cblocks = ceil_div64(n, RG_CELLS_PER_BLOCK);
    SC_REQUIRE(pl->cblocks * ceil_div64(max_rows > 0 ? max_rows : 1, np) <= 0x7fffffffLL, SC_ERR_INVALID,
               "%s: %lld cells x %lld permutations per launch exceed the grid; use smaller batches", who, (long long)n,
               (long long)max_rows);
    return SC_OK;
}

// out[rows][cells] += the first-contact counts under the labels at `lab`, np permutations per pass over the rows
void rg_launch(sc_ctx *c, const RgPlan &pl, int np, int hstride, const unsigned char *lab, int64_t gstride, int cell_bytes,
               int rows, unsigned long long *out)
{
    if (c->rg_entries <= 0) return;   // no cell has a neighbour: every count is 0
    const int groups = (rows + np - 1) / np;
    const dim3 grid((unsigned)(pl.cblocks * groups));
    const size_t lds = sizeof(unsigned int) * (size_t)np * hstride;
    KernelTimerScope ts(c, SC_K_RIPLEY_G_COUNT);
#define RG_LAUNCH(NP, WIDE)                                                                                              \
    hipLaunchKernelGGL((k_rg_count<NP, WIDE>), grid, dim3(RG_THREADS), lds, c->stream, c->rg_indptr.as<long long>(),     \
                       c->rg_col.as<int32_t>(), c->rg_bin.as<unsigned char>(), c->rg_n, lab, gstride, cell_bytes, pl.T, pl.R, \
                       hstride, groups, rows, pl.full_lo, pl.full_hi, out)
    if (pl.T > 32) {
        switch (np) {   // (T >= 33 has at least 1089 words: never 16 per pass)
        case 8: RG_LAUNCH(8, true); break;
        case 4: RG_LAUNCH(4, true); break;
        case 2: RG_LAUNCH(2, true); break;
        default: RG_LAUNCH(1, true); break;
        }
    } else {
        switch (np) {
        case 16: RG_LAUNCH(16, false); break;
        case 8: RG_LAUNCH(8, false); break;
        case 4: RG_LAUNCH(4, false); break;
        case 2: RG_LAUNCH(2, false); break;
        default: RG_LAUNCH(1, false); break;
        }
    }
#undef RG_LAUNCH
}

// the observed labels by position into labp, their counts into out (one "permutation" without a table)
void rg_observed(sc_ctx *c, const RgPlan &pl, int64_t n, unsigned char *labp, unsigned long long *out)
{
    lp_labels_by_position(c, c->sid.as<int32_t>(), n, labp);
    rg_launch(c, pl, 1, pl.cells, labp, 0, 1, 1, out);
}

// `rows` rows of the permutation table -> 16-byte label words at the cells' positions, in scratch_a ...
void rg_relabel(sc_ctx *c, int64_t n, const int32_t *table, int rows)
{
    KernelTimerScope ts(c, SC_K_RIPLEY_G_RELABEL);
    lp_relabel_words(c, n, c->rg_rank.as<int32_t>(), table, rows, c->scratch_a.as<uint4>());
}

// ... -> out[rows][cells]
void rg_count_words(sc_ctx *c, const RgPlan &pl, int64_t n, int rows, unsigned long long *out)
{
    rg_launch(c, pl, pl.np, pl.hstride, c->scratch_a.as<unsigned char>(), n * 16, 16, rows, out);
}

// the kernel's non-cumulative table u[a][b][j] -> the cumulative one
void rg_cumulate(const RgPlan &pl, const unsigned long long *u, int64_t *out)
{
    for (int k = 0; k < pl.T * pl.T; ++k) {
        long long run = 0;
        for (int j = 0; j < pl.R; ++j) out[(size_t)k * pl.R + j] = (int64_t)(run += (long long)u[(size_t)k * pl.R + j]);
    }
}

}   // namespace

extern "C" int sc_ripley_g_counts(sc_ctx *c, const int32_t *labels, int64_t n, int32_t n_types, int64_t n_perm,
                                  int64_t perm_row0, int64_t *counts_out)
{
    SC_REQUIRE(c && labels && counts_out, SC_ERR_INVALID, "sc_ripley_g_counts: null pointer");
    SC_HIP(hipSetDevice(c->device));
    RgPlan pl;
    SC_TRY(rg_prepare(c, "sc_ripley_g_counts", labels, n, n_types, n_perm, &pl));
    SC_TRY(lp_counts_rows(c, "sc_ripley_g_counts", n, n_perm, perm_row0));
    const size_t cells = (size_t)pl.cells;
    const size_t bytes = sizeof(unsigned long long) * cells * (size_t)(n_perm + 1);
    SC_TRY(c->scratch_b.ensure(bytes, &c->mem));
    // [16-byte label words of the table rows | observed labels by position]
    const size_t word_bytes = (size_t)n * 16 * (size_t)((n_perm + 15) / 16);
    SC_TRY(c->scratch_a.ensure(word_bytes + (size_t)align_up64(n, 16), &c->mem));
    unsigned long long *d_cnt = c->scratch_b.as<unsigned long long>();
    SC_HIP(hipMemsetAsync(d_cnt, 0, bytes, c->stream));
    if (n_perm > 0) {
        rg_relabel(c, n, c->perm.as<int32_t>() + perm_row0 * c->p_stride, (int)n_perm);
        rg_count_words(c, pl, n, (int)n_perm, d_cnt);
    }
    rg_observed(c, pl, n, c->scratch_a.as<unsigned char>() + word_bytes, d_cnt + cells * (size_t)n_perm);
    SC_HIP(hipGetLastError());
    std::vector<unsigned long long> host(cells * (size_t)(n_perm + 1));
    SC_HIP(hipMemcpyAsync(host.data(), d_cnt, bytes, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    for (int64_t p = 0; p <= n_perm; ++p) rg_cumulate(pl, host.data() + (size_t)p * cells, counts_out + (size_t)p * cells);
    return SC_OK;
}

extern "C" int sc_ripley_g_counter(sc_ctx *c, const int32_t *labels, int64_t n, int32_t n_types, uint64_t seed, int64_t p_first,
                                   int64_t n_perm, int64_t batch, int64_t *observed_out, int64_t *sums_out)
{
    SC_REQUIRE(c && labels && observed_out && sums_out, SC_ERR_INVALID, "sc_ripley_g_counter: null pointer");
    SC_TRY(lp_counter_sizes("sc_ripley_g_counter", p_first, n_perm, &batch));
    SC_HIP(hipSetDevice(c->device));
    RgPlan pl;
    SC_TRY(rg_prepare(c, "sc_ripley_g_counter", labels, n, n_types, batch, &pl));
    const int cells = pl.cells;
    const size_t cnt_bytes = sizeof(unsigned long long) * (size_t)cells * (size_t)batch;
    const size_t res_bytes = sizeof(unsigned long long) * (size_t)cells * 5;   // observed | 4 sums
    SC_TRY(c->scratch_b.ensure(cnt_bytes + res_bytes, &c->mem));
    const size_t word_bytes = (size_t)n * 16 * (size_t)((batch + 15) / 16), lab_bytes = (size_t)align_up64(n, 16);
    SC_TRY(c->scratch_a.ensure(word_bytes > lab_bytes ? word_bytes : lab_bytes, &c->mem));
    unsigned long long *d_cnt = c->scratch_b.as<unsigned long long>(), *d_obs = d_cnt + (size_t)cells * (size_t)batch;
    long long *d_sums = reinterpret_cast<long long *>(d_obs + cells);
    SC_HIP(hipMemsetAsync(d_obs, 0, res_bytes, c->stream));
    rg_observed(c, pl, n, c->scratch_a.as<unsigned char>(), d_obs);   // (the label words of batch 0 follow on the same stream)
    SC_HIP(hipGetLastError());
    SC_TRY(lp_counter_batches(
        c, "sc_ripley_g_counter", seed, n, p_first, n_perm, batch, [&](int rows) { rg_relabel(c, n, c->perm.as<int32_t>(), rows); },
        [&](int rows) -> int {
            SC_HIP(hipMemsetAsync(d_cnt, 0, cnt_bytes, c->stream));
            rg_count_words(c, pl, n, rows, d_cnt);
            return SC_OK;
        },
        [&](int rows) { lp_sums(c, d_cnt, d_obs, rows, cells, pl.R, 4, d_sums); }));
    std::vector<unsigned long long> host((size_t)cells * 5);
    SC_HIP(hipMemcpy(host.data(), d_obs, res_bytes, hipMemcpyDeviceToHost));
    rg_cumulate(pl, host.data(), observed_out);
    for (size_t k = 0; k < (size_t)cells * 4; ++k) sums_out[k] = (int64_t)host[(size_t)cells + k];
    return SC_OK;
}
