// Ligand-receptor permutation test over cluster pairs (extension N10; squidpy's ligrec, the CellPhoneDB test): expression
// summed by permuted cluster label, and the exact comparison of every (interaction, ordered cluster pair) with the
// observed table.  gfx950 only.
//
// Definition (include/spatialcore_hip.h, "N10").  Gene g of the loaded expression carries a shift s_g; a value x enters
// as the integer q = rint(x 2^s_g), |q| < 2^32.  S[c][g] = sum of q over the cells of cluster c (int64: n < 2^31),
// N[c][g] = #{cells of c with x > 0}, n_c = cells of c.  A label permutation keeps every n_c, so for interaction (L, R)
// and the ordered cluster pair (a, b), "permuted (mean_L,a + mean_R,b) / 2 >= observed" is
//     2^s_R n_b (S_p[a][L] - S[a][L]) + 2^s_L n_a (S_p[b][R] - S[b][R]) >= 0,
// evaluated in 128-bit integers after both powers of two are divided by the smaller one (|s_L - s_R| <= 30: every
// product stays below 2^64 2^31 2^30 = 2^125).  Integer adds and integer compares only: the tables and the counts are
// functions of the inputs alone, whatever the batching, the genes loaded together, the rank count or the run.
//
// k_ligrec_sums, the hot path.  A workgroup owns LIG_CELLS cells of one 16-gene tile and NP permutations.  The 16 lanes
// of a quarter-wavefront read one cell's 128-byte row of the fp64 tile, one gene each, LIG_ROWS rows ahead; a lane whose
// value is zero does nothing more (expression is mostly zeros).  The others quantise, read the cell's label word (NP label bytes: the 16-byte
// words of k_lp_relabel_words, one load per 16 permutations) and add q into the LDS table [NP][K][16] of int64 with one
// 64-bit LDS integer atomic per permutation.  The lanes of a wavefront are 4 cells x 16 genes, so two lanes meet on an
// address only when their cells share a label under that permutation.  The workgroup leaves with 64-bit global integer
// atomics into [p][K][genes].  NP = 16, 8 or 4 by K, so that the table stays within 64 KB and two workgroups share a
// compute unit's LDS (the rule of k_lp_pairs' plan).  The observed pass is the same kernel on the identity labels (NP = 1); it also
// counts N and flags the genes with a value that cannot be quantised.  No floating-point atomics, no matrix cores (a
// one-hot x X product would spend K times the arithmetic on zeros).
//
// k_ligrec_count: one thread per (interaction, a, b) evaluates the comparison over a batch's tables and adds to count_ge.
#include <math.h>

#include <vector>

#include "sc_labelperm.h"

#define LIG_CELLS 8192        // cells per workgroup of k_ligrec_sums
#define LIG_ROWS 8            // rows of a tile a lane has in flight in k_ligrec_sums
#define LIG_MAX_TYPES 96      // the label-permutation tests' limit (one label byte, LDS tables)
#define LIG_MAX_SPREAD 30     // |s_L - s_R| of an interaction at most: keeps the comparison inside 128 bits
#define LIG_MAX_SHIFT 1200    // |s_g| at most (fp64 exponents: 32 - e_g lies in [-992, 1106])

// sums[q NP + p][c][tile 16 + slot] += sum of q over the workgroup's cells with label c under permutation q NP + p of the
// pass.  Workgroup (cell block x pass q, tile): blockIdx.x = cell block * groups + q, the passes of one cell block side by
// side (the counters show every pass fetching its rows from the memory side all the same: DESIGN.md 4.6j).  The labels of a cell are NP consecutive bytes at lab + group
// stride * (q NP / 16) + cell * cell_bytes + (q NP) % 16: the 16-byte words of k_lp_relabel_words (cell_bytes = 16), or
// the label bytes themselves (OBS: NP = 1, cell_bytes = 1, one pass).  OBS also counts nnz[c][gene] = #{x > 0} and sets
// bad[gene] when a value is not finite or its rint(x 2^s) leaves (-2^32, 2^32); such a value is added nowhere.
template <int NP, bool OBS>
__global__ __launch_bounds__(256) void k_ligrec_sums(const double *__restrict__ X, int64_t n, const int32_t *__restrict__ shift,
                                                     const unsigned char *__restrict__ lab, int64_t gstride, int cell_bytes,
                                                     int n_types, int gp, int groups, int rows,
                                                     unsigned long long *__restrict__ sums, unsigned long long *__restrict__ nnz,
                                                     uint32_t *__restrict__ bad)
{
    typedef typename LpWord<NP>::type word_t;
    extern __shared__ unsigned long long tab[];   // [NP][n_types][16], then (OBS) uint32 nz[n_types][16]
    const int words = NP * n_types * SC_TILE;
    uint32_t *nz = reinterpret_cast<uint32_t *>(tab + words);
    const int tid = (int)threadIdx.x;
    for (int k = tid; k < words; k += 256) tab[k] = 0ull;
    if (OBS)
        for (int k = tid; k < n_types * SC_TILE; k += 256) nz[k] = 0u;
    __syncthreads();
    const int q = (int)(blockIdx.x % (unsigned)groups);
    const int64_t cb = (int64_t)(blockIdx.x / (unsigned)groups);
    const int64_t tile = blockIdx.y;
    const int slot = tid & 15, sub = tid >> 4;
    const int gene = (int)tile * SC_TILE + slot;
    const int s_g = shift[gene];
    const double *xt = X + tile * n * SC_TILE;
    const unsigned char *lp = lab + (int64_t)((q * NP) >> 4) * gstride + ((q * NP) & 15);
    const int64_t c0 = cb * LIG_CELLS;
    const int64_t c1 = c0 + LIG_CELLS < n ? c0 + LIG_CELLS : n;
    // one value of one cell: quantised and added under each of the NP labels of the cell
    auto add = [&](int64_t cell, double x) {
        const double y = rint(ldexp(x, s_g));
        if (!(fabs(y) < 4294967296.0)) {   // (NaN and +-inf land here too)
            if (OBS) atomicOr(&bad[gene], 1u);
            return;
        }
        const unsigned long long qv = (unsigned long long)(long long)y;
        const word_t w = *reinterpret_cast<const word_t *>(lp + cell * cell_bytes);
        if (OBS && x > 0.0) atomicAdd(&nz[lp_label(w, 0) * SC_TILE + slot], 1u);
        if (qv != 0ull) {
#pragma unroll
            for (int s = 0; s < NP; ++s) atomicAdd(&tab[(s * n_types + lp_label(w, s)) * SC_TILE + slot], qv);
        }
    };
    // LIG_ROWS rows per lane are loaded before the first is looked at: with one load in flight per lane the kernel ran at
    // the latency of the tile reads
    for (int64_t cell = c0 + sub; cell < c1; cell += 16 * LIG_ROWS) {
        double x[LIG_ROWS];
#pragma unroll
        for (int u = 0; u < LIG_ROWS; ++u) x[u] = cell + 16 * u < c1 ? xt[(cell + 16 * u) * SC_TILE + slot] : 0.0;
#pragma unroll
        for (int u = 0; u < LIG_ROWS; ++u)
            if (x[u] != 0.0) add(cell + 16 * u, x[u]);
    }
    __syncthreads();
    const int per = n_types * SC_TILE;
    for (int k = tid; k < words; k += 256) {
        const int p = k / per, rem = k - p * per;
        const unsigned long long v = tab[k];
        if (v && q * NP + p < rows)
            atomicAdd(&sums[((int64_t)(q * NP + p) * n_types + (rem >> 4)) * gp + tile * SC_TILE + (rem & 15)], v);
    }
    if (OBS)
        for (int k = tid; k < per; k += 256)
            if (nz[k]) atomicAdd(&nnz[(int64_t)(k >> 4) * gp + tile * SC_TILE + (k & 15)], (unsigned long long)nz[k]);
}

// count_ge[i][a][b] += #{p < rows : wl_i n_b (S_p[a][L_i] - S[a][L_i]) + wr_i n_a (S_p[b][R_i] - S[b][R_i]) >= 0}, with
// wl_i = 2^(s_R - m), wr_i = 2^(s_L - m), m = min(s_L, s_R), as the host computed them (no variable shift on the device).
// A difference of two sums lies within +-2^64 and a weight times a cluster size below 2^61: 128-bit products and sum.
__global__ __launch_bounds__(256) void k_ligrec_count(const long long *__restrict__ nul, const long long *__restrict__ obs,
                                                      int rows, int n_types, int gp, const int32_t *__restrict__ pair_l,
                                                      const int32_t *__restrict__ pair_r, const long long *__restrict__ wl,
                                                      const long long *__restrict__ wr, const long long *__restrict__ group_n,
                                                      int64_t cells, long long *__restrict__ count_ge)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= cells) return;
    const int kk = n_types * n_types;
    const int i = (int)(t / kk), ab = (int)(t - (int64_t)i * kk);
    const int a = ab / n_types, b = ab - a * n_types;
    const int64_t at_l = (int64_t)a * gp + pair_l[i], at_r = (int64_t)b * gp + pair_r[i];
    const long long coef_l = wl[i] * group_n[b], coef_r = wr[i] * group_n[a];
    const long long o_l = obs[at_l], o_r = obs[at_r];
    const int64_t pstride = (int64_t)n_types * gp;
    long long ge = 0;
    for (int p = 0; p < rows; ++p) {
        const __int128 d_l = (__int128)nul[p * pstride + at_l] - o_l, d_r = (__int128)nul[p * pstride + at_r] - o_r;
        ge += d_l * coef_l + d_r * coef_r >= 0 ? 1 : 0;
    }
    count_ge[t] += ge;
}

namespace {

struct LigPlan {
    int64_t n = 0, cells = 0;        // cells of the section; threads of k_ligrec_count = I K K
    int K = 0, G = 0, gp = 0, I = 0; // clusters, loaded genes, padded genes (tiles x 16), interactions
    int np = 16;                     // permutations per pass of k_ligrec_sums
    unsigned cblocks = 0;
    // scratch_out: count_ge | group_n | wl | wr | pair_l | pair_r | shift | bad      scratch_b: observed sums | nnz | batch tables
    long long *count_ge = nullptr, *group_n = nullptr, *wl = nullptr, *wr = nullptr;
    int32_t *pair_l = nullptr, *pair_r = nullptr, *shift = nullptr;
    uint32_t *bad = nullptr;
    size_t table() const { return (size_t)K * (size_t)gp; }   // words of one [K][gp] table
};

// what both entry points check and upload: the labels (scratch_idx), the per-gene shifts, the interactions with their
// weights, the cluster sizes; count_ge zeroed.  max_rows: the most permutation rows one launch will take
int lig_prepare(sc_ctx *c, const char *who, const int32_t *labels, int64_t n, int32_t n_types, const int32_t *shift,
                const int32_t *pair_l, const int32_t *pair_r, int64_t n_pairs, int64_t max_rows, int64_t *group_n_out,
                LigPlan *pl)
{
    SC_REQUIRE(n_types >= 1 && n_types <= LIG_MAX_TYPES, SC_ERR_INVALID, "%s: n_types must be 1..%d, got %d", who,
               LIG_MAX_TYPES, (int)n_types);
    SC_REQUIRE(c->e_n > 0, SC_ERR_STATE, "%s: no expression loaded (call sc_expr_set_* first)", who);
    SC_REQUIRE(n == c->e_n, SC_ERR_INVALID, "%s: %lld labels for %lld loaded cells", who, (long long)n, (long long)c->e_n);
    SC_REQUIRE(n_pairs >= 1 && n_pairs <= (1 << 24), SC_ERR_INVALID, "%s: n_pairs=%lld out of range (1..2^24)", who,
               (long long)n_pairs);
    const int64_t G = c->e_genes, tiles = c->e_tiles, gp = tiles * SC_TILE;
    SC_REQUIRE(tiles <= 65535, SC_ERR_INVALID, "%s: at most %d genes per call, %lld are loaded", who, 65535 * SC_TILE, (long long)G);
    for (int64_t g = 0; g < G; ++g)
        SC_REQUIRE(shift[g] >= -LIG_MAX_SHIFT && shift[g] <= LIG_MAX_SHIFT, SC_ERR_INVALID, "%s: shift %d of gene %lld outside +-%d",
                   who, shift[g], (long long)g, LIG_MAX_SHIFT);
    std::vector<long long> wl((size_t)n_pairs), wr((size_t)n_pairs);
    for (int64_t i = 0; i < n_pairs; ++i) {
        const int32_t l = pair_l[i], r = pair_r[i];
        SC_REQUIRE(l >= 0 && l < G && r >= 0 && r < G, SC_ERR_INVALID, "%s: interaction %lld = (%d, %d) outside the %lld loaded genes",
                   who, (long long)i, l, r, (long long)G);
        const int spread = shift[l] - shift[r];
        SC_REQUIRE(spread >= -LIG_MAX_SPREAD && spread <= LIG_MAX_SPREAD, SC_ERR_INVALID,
                   "%s: interaction %lld: the shifts of genes %d and %d (%d, %d) differ by more than %d", who, (long long)i, l, r,
                   shift[l], shift[r], LIG_MAX_SPREAD);
        wl[(size_t)i] = 1ll << (spread < 0 ? -spread : 0);   // 2^(s_R - min)
        wr[(size_t)i] = 1ll << (spread > 0 ? spread : 0);    // 2^(s_L - min)
    }
    const int np = n_types <= 32 ? 16 : n_types <= 64 ? 8 : 4;   // NP K 128 bytes <= 64 KB
    const int64_t cblocks = ceil_div64(n, LIG_CELLS);
    SC_REQUIRE(cblocks * ceil_div64(max_rows > 0 ? max_rows : 1, np) <= 0x7fffffffLL, SC_ERR_INVALID,
               "%s: %lld cells x %lld permutations per launch exceed the grid; use smaller batches", who, (long long)n,
               (long long)max_rows);
    SC_TRY(lp_upload_labels(c, labels, n, n_types));
    std::vector<long long> group_n((size_t)n_types, 0);
    for (int64_t i = 0; i < n; ++i) ++group_n[(size_t)labels[i]];
    for (int k = 0; k < n_types; ++k) group_n_out[k] = group_n[(size_t)k];
    std::vector<int32_t> shift_p((size_t)gp, 0);
    for (int64_t g = 0; g < G; ++g) shift_p[(size_t)g] = shift[g];

    pl->n = n;
    pl->K = n_types;
    pl->G = (int)G;
    pl->gp = (int)gp;
    pl->I = (int)n_pairs;
    pl->np = np;
    pl->cblocks = (unsigned)cblocks;
    pl->cells = n_pairs * n_types * n_types;
    const size_t I = (size_t)n_pairs;
    SC_TRY(c->scratch_out.ensure(sizeof(long long) * ((size_t)pl->cells + (size_t)n_types + 2 * I) +
                                 sizeof(int32_t) * (2 * I + 2 * (size_t)gp), &c->mem));
    pl->count_ge = c->scratch_out.as<long long>();
    pl->group_n = pl->count_ge + pl->cells;
    pl->wl = pl->group_n + n_types;
    pl->wr = pl->wl + I;
    pl->pair_l = reinterpret_cast<int32_t *>(pl->wr + I);
    pl->pair_r = pl->pair_l + I;
    pl->shift = pl->pair_r + I;
    pl->bad = reinterpret_cast<uint32_t *>(pl->shift + gp);
    SC_HIP(hipMemsetAsync(pl->count_ge, 0, sizeof(long long) * (size_t)pl->cells, c->stream));
    SC_HIP(hipMemsetAsync(pl->bad, 0, sizeof(uint32_t) * (size_t)gp, c->stream));
    SC_HIP(hipMemcpyAsync(pl->group_n, group_n.data(), sizeof(long long) * (size_t)n_types, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(pl->wl, wl.data(), sizeof(long long) * I, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(pl->wr, wr.data(), sizeof(long long) * I, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(pl->pair_l, pair_l, sizeof(int32_t) * I, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(pl->pair_r, pair_r, sizeof(int32_t) * I, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(pl->shift, shift_p.data(), sizeof(int32_t) * (size_t)gp, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));   // (the staging vectors end here)
    return SC_OK;
}

// The observed tables: d_obs[K][gp] and d_nnz[K][gp] on the device, sum_out / nnz_out [K][G] on the host.  A gene with a
// value that cannot be quantised ends the call.
int lig_observed(sc_ctx *c, const char *who, const LigPlan &pl, unsigned long long *d_obs, unsigned long long *d_nnz,
                 int64_t *sum_out, int64_t *nnz_out)
{
    const size_t tw = pl.table();
    SC_HIP(hipMemsetAsync(d_obs, 0, sizeof(unsigned long long) * 2 * tw, c->stream));   // (d_nnz follows d_obs)
    {
        KernelTimerScope ts(c, SC_K_LIGREC);
        hipLaunchKernelGGL((k_ligrec_sums<1, true>), dim3(pl.cblocks, (unsigned)(pl.gp / SC_TILE)), dim3(256),
                           sizeof(unsigned long long) * (size_t)pl.K * SC_TILE + sizeof(uint32_t) * (size_t)pl.K * SC_TILE, c->stream,
                           c->X.as<double>(), pl.n, pl.shift, c->scratch_idx.as<unsigned char>(), (int64_t)0, 1, pl.K, pl.gp, 1, 1,
                           d_obs, d_nnz, pl.bad);
    }
    SC_HIP(hipGetLastError());
    std::vector<long long> host(2 * tw);
    std::vector<uint32_t> bad((size_t)pl.gp);
    SC_HIP(hipMemcpyAsync(host.data(), d_obs, sizeof(long long) * 2 * tw, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipMemcpyAsync(bad.data(), pl.bad, sizeof(uint32_t) * (size_t)pl.gp, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    for (int g = 0; g < pl.G; ++g)
        SC_REQUIRE(!bad[(size_t)g], SC_ERR_INVALID,
                   "%s: gene %d has a value that is not finite or whose rint(x * 2^shift) leaves (-2^32, 2^32)", who, g);
    for (int k = 0; k < pl.K; ++k)
        for (int g = 0; g < pl.G; ++g) {
            sum_out[(size_t)k * pl.G + g] = (int64_t)host[(size_t)k * pl.gp + g];
            nnz_out[(size_t)k * pl.G + g] = (int64_t)host[tw + (size_t)k * pl.gp + g];
        }
    return SC_OK;
}

// the label words of `rows` rows of `table` -> scratch_a (cell order: this test has no graph)
void lig_relabel(sc_ctx *c, const LigPlan &pl, const int32_t *table, int rows)
{
    lp_relabel_words(c, pl.n, nullptr, table, rows, c->scratch_a.as<uint4>());
}

// ... -> d_tab[rows][K][gp], zeroed first
int lig_sums(sc_ctx *c, const LigPlan &pl, int rows, unsigned long long *d_tab)
{
    SC_HIP(hipMemsetAsync(d_tab, 0, sizeof(unsigned long long) * pl.table() * (size_t)rows, c->stream));
    const int groups = (rows + pl.np - 1) / pl.np;
    const dim3 grid(pl.cblocks * (unsigned)groups, (unsigned)(pl.gp / SC_TILE));
    const size_t lds = sizeof(unsigned long long) * (size_t)pl.np * pl.K * SC_TILE;
    KernelTimerScope ts(c, SC_K_LIGREC);
#define LIG_LAUNCH(NP)                                                                                                      \
    hipLaunchKernelGGL((k_ligrec_sums<NP, false>), grid, dim3(256), lds, c->stream, c->X.as<double>(), pl.n, pl.shift,      \
                       c->scratch_a.as<unsigned char>(), (int64_t)pl.n * 16, 16, pl.K, pl.gp, groups, rows, d_tab,          \
                       (unsigned long long *)nullptr, (uint32_t *)nullptr)
    switch (pl.np) {
    case 16: LIG_LAUNCH(16); break;
    case 8: LIG_LAUNCH(8); break;
    default: LIG_LAUNCH(4); break;
    }
#undef LIG_LAUNCH
    return SC_OK;
}

// ... compared with the observed table, into count_ge
void lig_count(sc_ctx *c, const LigPlan &pl, int rows, const unsigned long long *d_tab, const unsigned long long *d_obs)
{
    hipLaunchKernelGGL(k_ligrec_count, dim3((unsigned)ceil_div64(pl.cells, 256)), dim3(256), 0, c->stream,
                       reinterpret_cast<const long long *>(d_tab), reinterpret_cast<const long long *>(d_obs), rows, pl.K, pl.gp,
                       pl.pair_l, pl.pair_r, pl.wl, pl.wr, pl.group_n, pl.cells, pl.count_ge);
}

}   // namespace

extern "C" int sc_ligrec_counts(sc_ctx *c, const int32_t *labels, int64_t n, int32_t n_types, const int32_t *shift,
                                const int32_t *pair_l, const int32_t *pair_r, int64_t n_pairs, int64_t n_perm,
                                int64_t perm_row0, int64_t *sum_out, int64_t *nnz_out, int64_t *group_n_out,
                                int64_t *null_sums_out, int64_t *count_ge_out)
{
    SC_REQUIRE(c && labels && shift && pair_l && pair_r && sum_out && nnz_out && group_n_out && count_ge_out, SC_ERR_INVALID,
               "sc_ligrec_counts: null pointer");
    SC_HIP(hipSetDevice(c->device));
    LigPlan pl;
    SC_TRY(lig_prepare(c, "sc_ligrec_counts", labels, n, n_types, shift, pair_l, pair_r, n_pairs, n_perm, group_n_out, &pl));
    SC_TRY(lp_counts_rows(c, "sc_ligrec_counts", n, n_perm, perm_row0));
    const size_t tw = pl.table();
    SC_TRY(c->scratch_b.ensure(sizeof(unsigned long long) * tw * (size_t)(n_perm + 2), &c->mem));
    unsigned long long *d_obs = c->scratch_b.as<unsigned long long>(), *d_nnz = d_obs + tw, *d_tab = d_nnz + tw;
    SC_TRY(lig_observed(c, "sc_ligrec_counts", pl, d_obs, d_nnz, sum_out, nnz_out));
    if (n_perm > 0) {
        SC_TRY(c->scratch_a.ensure((size_t)n * 16 * (size_t)((n_perm + 15) / 16), &c->mem));
        lig_relabel(c, pl, c->perm.as<int32_t>() + perm_row0 * c->p_stride, (int)n_perm);
        SC_TRY(lig_sums(c, pl, (int)n_perm, d_tab));
        lig_count(c, pl, (int)n_perm, d_tab, d_obs);
        SC_HIP(hipGetLastError());
    }
    SC_HIP(hipMemcpyAsync(count_ge_out, pl.count_ge, sizeof(int64_t) * (size_t)pl.cells, hipMemcpyDeviceToHost, c->stream));
    std::vector<long long> host;
    if (null_sums_out && n_perm > 0) {
        host.resize(tw * (size_t)n_perm);
        SC_HIP(hipMemcpyAsync(host.data(), d_tab, sizeof(long long) * host.size(), hipMemcpyDeviceToHost, c->stream));
    }
    SC_HIP(hipStreamSynchronize(c->stream));
    for (size_t pk = 0; pk < host.size() / (size_t)pl.gp; ++pk)   // rows (p, cluster): padded genes dropped
        for (int g = 0; g < pl.G; ++g) null_sums_out[pk * (size_t)pl.G + g] = (int64_t)host[pk * (size_t)pl.gp + g];
    return SC_OK;
}

extern "C" int sc_ligrec_counter(sc_ctx *c, const int32_t *labels, int64_t n, int32_t n_types, const int32_t *shift,
                                 const int32_t *pair_l, const int32_t *pair_r, int64_t n_pairs, uint64_t seed, int64_t p_first,
                                 int64_t n_perm, int64_t batch, int64_t *sum_out, int64_t *nnz_out, int64_t *group_n_out,
                                 int64_t *count_ge_out)
{
    SC_REQUIRE(c && labels && shift && pair_l && pair_r && sum_out && nnz_out && group_n_out && count_ge_out, SC_ERR_INVALID,
               "sc_ligrec_counter: null pointer");
    SC_TRY(lp_counter_sizes("sc_ligrec_counter", p_first, n_perm, &batch));
    SC_HIP(hipSetDevice(c->device));
    LigPlan pl;
    SC_TRY(lig_prepare(c, "sc_ligrec_counter", labels, n, n_types, shift, pair_l, pair_r, n_pairs, batch, group_n_out, &pl));
    const size_t tw = pl.table();
    SC_TRY(c->scratch_b.ensure(sizeof(unsigned long long) * tw * (size_t)(batch + 2), &c->mem));
    SC_TRY(c->scratch_a.ensure((size_t)n * 16 * (size_t)((batch + 15) / 16), &c->mem));
    unsigned long long *d_obs = c->scratch_b.as<unsigned long long>(), *d_nnz = d_obs + tw, *d_tab = d_nnz + tw;
    SC_TRY(lig_observed(c, "sc_ligrec_counter", pl, d_obs, d_nnz, sum_out, nnz_out));
    SC_TRY(lp_counter_batches(
        c, "sc_ligrec_counter", seed, n, p_first, n_perm, batch, [&](int rows) { lig_relabel(c, pl, c->perm.as<int32_t>(), rows); },
        [&](int rows) -> int { return lig_sums(c, pl, rows, d_tab); }, [&](int rows) { lig_count(c, pl, rows, d_tab, d_obs); }));
    SC_HIP(hipMemcpy(count_ge_out, pl.count_ge, sizeof(int64_t) * (size_t)pl.cells, hipMemcpyDeviceToHost));
    return SC_OK;
}
