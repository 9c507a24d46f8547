// Cross-type Ripley's K with a label-permutation null (extension: the reference has no point-pattern statistic).
// gfx950 only.
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
#include <math.h>

#include <hipcub/hipcub.hpp>
#include <vector>

#include "sc_ctx.h"
#include "sc_enrich.h"

#define RIP_MAX_RADII 32
#define RIP_PAIRS_PER_BLOCK 65536
#define RIP_THREADS 512
#define RIP_LDS_WORDS 16384   // 64 KB of uint32 per workgroup: the limit on T (T + 1) / 2 * R

struct RipleyR2 { double v[RIP_MAX_RADII]; };

// FILL = false: counts[t] = pairs (t, s), s > t, within the largest radius; rank[cell at t] = t.
// FILL = true: the pairs themselves at indptr[t] .., with their radius bins.  t, s: positions in bin order.
template <bool FILL>
__global__ __launch_bounds__(256) void k_ripley_pairs(const double *__restrict__ sx, const double *__restrict__ sy,
                                                      const int32_t *__restrict__ sid, const int32_t *__restrict__ bin_start,
                                                      int64_t n, RipleyR2 r2, int n_radii, int rings, double x0, double y0,
                                                      double h, int nbx, int nby, long long *__restrict__ counts,
                                                      const long long *__restrict__ indptr, int32_t *__restrict__ prow,
                                                      int32_t *__restrict__ pcol, unsigned char *__restrict__ pbin,
                                                      int32_t *__restrict__ rank)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double qx = sx[t], qy = sy[t];
    const double r2max = r2.v[n_radii - 1];
    const double inv_h = 1.0 / h;
    const int bx = bin_coord(qx, x0, inv_h, nbx), by = bin_coord(qy, y0, inv_h, nby);
    const int yhi = by + rings >= nby ? nby - 1 : by + rings;
    const int xlo = bx - rings < 0 ? 0 : bx - rings, xhi = bx + rings >= nbx ? nbx - 1 : bx + rings;
    long long cnt = 0;
    const long long base = FILL ? indptr[t] : 0;
    for (int yy = by; yy <= yhi; ++yy) {
        int s0 = bin_start[yy * nbx + xlo];
        const int s1 = bin_start[yy * nbx + xhi + 1];
        if (s0 <= t) s0 = (int)t + 1;   // (own row only: the rows above start behind t)
        for (int s = s0; s < s1; ++s) {
            const double dx = qx - sx[s], dy = qy - sy[s];
            const double d = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
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
        }
    }
    if (!FILL) {
        counts[t] = cnt;
        rank[sid[t]] = (int32_t)t;
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
    c->radius = -1.0;   // (a pending sc_radius_count_2d / _fill_2d pair loses its bins)
    // bins no smaller than the largest radius, as the radius graph takes them
    SC_TRY(sc_bin_points(c, xy, n, 4.0, rmax));
    int rings = (int)ceil(rmax / c->gh * (1.0 + 1e-9));
    if (rings < 1) rings = 1;
    SC_TRY(c->rp_cnt.ensure(sizeof(long long) * (size_t)(n + 1), &c->mem));
    SC_TRY(c->rp_indptr.ensure(sizeof(long long) * (size_t)(n + 1), &c->mem));
    SC_TRY(c->rp_rank.ensure(sizeof(int32_t) * (size_t)n, &c->mem));
    long long *counts = c->rp_cnt.as<long long>();
    SC_HIP(hipMemsetAsync(counts, 0, sizeof(long long) * (size_t)(n + 1), c->stream));
    const dim3 grid((unsigned)ceil_div64(n, 256));
    hipLaunchKernelGGL(k_ripley_pairs<false>, grid, dim3(256), 0, c->stream, c->sx.as<double>(), c->sy.as<double>(),
                       c->sid.as<int32_t>(), c->bin_start.as<int32_t>(), n, r2, (int)n_radii, rings, c->gx0, c->gy0, c->gh,
                       c->nbx, c->nby, counts, (const long long *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr,
                       (unsigned char *)nullptr, c->rp_rank.as<int32_t>());
    SC_HIP(hipGetLastError());
    size_t tmp_bytes = 0;
    SC_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, counts, c->rp_indptr.as<long long>(), (int)(n + 1), c->stream));
    SC_TRY(c->cub_tmp.ensure(tmp_bytes, &c->mem));
    SC_HIP(hipcub::DeviceScan::ExclusiveSum(c->cub_tmp.p, tmp_bytes, counts, c->rp_indptr.as<long long>(), (int)(n + 1),
                                            c->stream));
    long long total = 0;
    SC_HIP(hipMemcpyAsync(&total, c->rp_indptr.as<long long>() + n, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    SC_REQUIRE(ceil_div64(total, RIP_PAIRS_PER_BLOCK) <= 65535, SC_ERR_INVALID,
               "sc_ripley_build: %lld unordered pairs within the largest radius, more than 4.2e9", total);
    const size_t cap = (size_t)(total > 0 ? total : 1);
    SC_TRY(c->rp_row.ensure(sizeof(int32_t) * cap, &c->mem));
    SC_TRY(c->rp_col.ensure(sizeof(int32_t) * cap, &c->mem));
    SC_TRY(c->rp_bin.ensure(cap, &c->mem));
    if (total > 0) {
        hipLaunchKernelGGL(k_ripley_pairs<true>, grid, dim3(256), 0, c->stream, c->sx.as<double>(), c->sy.as<double>(),
                           c->sid.as<int32_t>(), c->bin_start.as<int32_t>(), n, r2, (int)n_radii, rings, c->gx0, c->gy0, c->gh,
                           c->nbx, c->nby, (long long *)nullptr, c->rp_indptr.as<long long>(), c->rp_row.as<int32_t>(),
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

// The enrichment's k_enrich_sums on the CUMULATIVE unordered counts, with the <= exceedance row.  One thread per
// (unordered type pair, radius): u_p = sum_{j' <= j} counts[p][pair][j'],
// sums[0] += sum_p (u_p - u_obs), sums[1] += sum_p (u_p - u_obs)^2, sums[2] += #{p : u_p >= u_obs}, sums[3] += #{p : u_p <= u_obs}
__global__ __launch_bounds__(256) void k_ripley_sums(const unsigned long long *__restrict__ counts,
                                                     const unsigned long long *__restrict__ obs, int n_perm, int cells,
                                                     int n_radii, long long *__restrict__ sums)
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
    sums[3 * cells + k] += le;
}

namespace {

struct RipPlan {
    int T = 0, R = 0, cells = 0;   // cells = T (T + 1) / 2 * R: words of one histogram
    int np = 1, hstride = 0;       // permutations per pass over the pairs, histogram stride in words
    unsigned pblocks = 0;
};

// what both counting entry points check: the pair list, the labels, the shape
int rip_prepare(sc_ctx *c, const char *who, const int32_t *labels, int64_t n, int32_t n_types, RipPlan *plan,
                std::vector<unsigned char> *lab8)
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
    lab8->resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        SC_REQUIRE(labels[i] >= 0 && labels[i] < n_types, SC_ERR_INVALID, "label %d of cell %lld out of range", labels[i],
                   (long long)i);
        (*lab8)[(size_t)i] = (unsigned char)labels[i];
    }
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
                       c->lee_pairs.as<unsigned char>(), c->sid.as<int32_t>(), (const int32_t *)nullptr, (int64_t)0, 0, n,
                       align_up64(n, 16), labp);
    if (c->rp_pairs > 0)
        hipLaunchKernelGGL(k_ripley<1>, dim3(1u, pl.pblocks), dim3(RIP_THREADS), sizeof(unsigned int) * (size_t)pl.cells, c->stream,
                           c->rp_row.as<int32_t>(), c->rp_col.as<int32_t>(), c->rp_bin.as<unsigned char>(), c->rp_pairs, labp,
                           (int64_t)0, 1, pl.T, pl.R, pl.cells, 1, out);
}

// `rows` rows of the permutation table -> 16-byte label words in lee_a
void rip_relabel_words(sc_ctx *c, int64_t n, const int32_t *table, int rows)
{
    hipLaunchKernelGGL(k_enrich_relabel16, dim3((unsigned)ceil_div64(n, 256), (unsigned)((rows + 15) / 16)), dim3(256), 0,
                       c->stream, c->lee_pairs.as<unsigned char>(), c->rp_rank.as<int32_t>(), table, c->p_stride, rows, n,
                       c->lee_a.as<uint4>());
}

// ... -> out[rows][cells], NP permutations per pass over the pairs
void rip_count_words(sc_ctx *c, const RipPlan &pl, int64_t n, int rows, unsigned long long *out)
{
    if (c->rp_pairs <= 0) return;
    const dim3 grid((unsigned)((rows + pl.np - 1) / pl.np), pl.pblocks);
    const size_t lds = sizeof(unsigned int) * (size_t)pl.np * pl.hstride;
#define RIP_LAUNCH(NP)                                                                                                  \
    hipLaunchKernelGGL(k_ripley<NP>, grid, dim3(RIP_THREADS), lds, c->stream, c->rp_row.as<int32_t>(), c->rp_col.as<int32_t>(), \
                       c->rp_bin.as<unsigned char>(), c->rp_pairs, c->lee_a.as<unsigned char>(), (int64_t)n * 16, 16, pl.T, pl.R, \
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
// (k_ripley_sums' rows are sums over the cumulative counts already: false).  `diag`: the factor of the diagonal, 2 for
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
    RipPlan pl;
    std::vector<unsigned char> lab8;
    SC_TRY(rip_prepare(c, "sc_ripley_counts", labels, n, n_types, &pl, &lab8));
    SC_HIP(hipSetDevice(c->device));
    if (n_perm > 0) {
        SC_TRY(sc_perm_forward_ensure(c));
        SC_REQUIRE(c->p_n == n && perm_row0 + n_perm <= c->p_count, SC_ERR_STATE,
                   "sc_ripley_counts: needs permutation rows [%lld, %lld)", (long long)perm_row0, (long long)(perm_row0 + n_perm));
    }
    const size_t words = (size_t)pl.cells * (size_t)(n_perm + 1);
    const int64_t lstride = align_up64(n, 16);
    SC_TRY(c->lee_pairs.ensure((size_t)n + 16, &c->mem));
    SC_TRY(c->lee_b.ensure(sizeof(unsigned long long) * words, &c->mem));
    // [16-byte label words of the table rows | observed labels by position]
    const size_t word_bytes = (size_t)n * 16 * (size_t)((n_perm + 15) / 16);
    SC_TRY(c->lee_a.ensure(word_bytes + (size_t)lstride, &c->mem));
    unsigned long long *d_cnt = c->lee_b.as<unsigned long long>();
    SC_HIP(hipMemcpyAsync(c->lee_pairs.p, lab8.data(), (size_t)n, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * words, c->stream));
    if (n_perm > 0) {
        rip_relabel_words(c, n, c->perm.as<int32_t>() + perm_row0 * c->p_stride, (int)n_perm);
        rip_count_words(c, pl, n, (int)n_perm, d_cnt);
    }
    rip_observed(c, pl, n, c->lee_a.as<unsigned char>() + word_bytes, d_cnt + (size_t)pl.cells * (size_t)n_perm);
    SC_HIP(hipGetLastError());
    std::vector<unsigned long long> host(words);
    SC_HIP(hipMemcpyAsync(host.data(), d_cnt, sizeof(unsigned long long) * words, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    const size_t ttr = (size_t)pl.T * pl.T * pl.R;
    for (int64_t p = 0; p <= n_perm; ++p) rip_expand(pl, host.data() + (size_t)p * pl.cells, true, 2, counts_out + (size_t)p * ttr);
    return SC_OK;
}

int sc_perm_counter_rows(sc_ctx *c, uint64_t seed, int64_t n, int64_t p_first, int64_t n_perm, hipStream_t s);   // sc_permgen.hip

extern "C" int sc_ripley_counter(sc_ctx *c, const int32_t *labels, int64_t n, int32_t n_types, uint64_t seed, int64_t p_first,
                                 int64_t n_perm, int64_t batch, int64_t *observed_out, int64_t *sums_out)
{
    SC_REQUIRE(c && labels && observed_out && sums_out, SC_ERR_INVALID, "sc_ripley_counter: null pointer");
    SC_REQUIRE(n_perm >= 0 && p_first >= 0 && batch >= 1 && batch <= 65534, SC_ERR_INVALID, "sc_ripley_counter: bad sizes");
    RipPlan pl;
    std::vector<unsigned char> lab8;
    SC_TRY(rip_prepare(c, "sc_ripley_counter", labels, n, n_types, &pl, &lab8));
    SC_HIP(hipSetDevice(c->device));
    if (batch > n_perm) batch = n_perm > 0 ? n_perm : 1;
    const int cells = pl.cells;
    const int64_t lstride = align_up64(n, 16);
    const size_t cnt_bytes = sizeof(unsigned long long) * (size_t)cells * (size_t)batch;
    SC_TRY(c->lee_pairs.ensure((size_t)n + 16, &c->mem));
    SC_TRY(c->lee_b.ensure(cnt_bytes + sizeof(unsigned long long) * (size_t)cells * 5, &c->mem));   // counts | observed | 4 sums
    const size_t word_bytes = (size_t)n * 16 * (size_t)((batch + 15) / 16);
    SC_TRY(c->lee_a.ensure(word_bytes > (size_t)lstride ? word_bytes : (size_t)lstride, &c->mem));
    unsigned long long *d_cnt = c->lee_b.as<unsigned long long>(), *d_obs = d_cnt + (size_t)cells * batch;
    long long *d_sums = reinterpret_cast<long long *>(d_obs + cells);
    if (n_perm > 0) SC_TRY(sc_perm_alloc(c, n, batch));
    if (!c->stream3) SC_HIP(hipStreamCreateWithFlags(&c->stream3, hipStreamNonBlocking));
    SC_HIP(hipMemcpyAsync(c->lee_pairs.p, lab8.data(), (size_t)n, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemsetAsync(d_obs, 0, sizeof(unsigned long long) * (size_t)cells * 5, c->stream));
    rip_observed(c, pl, n, c->lee_a.as<unsigned char>(), d_obs);   // (the label words of batch 0 follow on the same stream)
    SC_HIP(hipGetLastError());
    const int64_t batches = n_perm > 0 ? ceil_div64(n_perm, batch) : 0;
    std::vector<hipEvent_t> ev((size_t)batches * 2, nullptr);
    int rc = SC_OK;
    auto generate = [&](int64_t b) -> int {   // batch b's rows into the table, on the generator's stream
        const int64_t p0 = b * batch, cnt = p0 + batch < n_perm ? batch : n_perm - p0;
        SC_TRY(sc_perm_counter_rows(c, seed, n, p_first + p0, cnt, c->stream3));
        SC_HIP(hipEventCreateWithFlags(&ev[(size_t)(2 * b)], hipEventDisableTiming));
        SC_HIP(hipEventRecord(ev[(size_t)(2 * b)], c->stream3));
        return SC_OK;
    };
    if (batches > 0) {
        SC_HIP(hipStreamSynchronize(c->stream));   // (the table may still be read by an earlier call's kernels)
        rc = generate(0);
    }
    for (int64_t b = 0; b < batches && rc == SC_OK; ++b) {
        const int64_t p0 = b * batch;
        const int cnt = (int)(p0 + batch < n_perm ? batch : n_perm - p0);
        if (hipStreamWaitEvent(c->stream, ev[(size_t)(2 * b)], 0) != hipSuccess) { rc = SC_ERR_HIP; break; }
        if (hipMemsetAsync(d_cnt, 0, cnt_bytes, c->stream) != hipSuccess) { rc = SC_ERR_HIP; break; }
        // the label words are the only thing the counting reads: the table is free again behind the relabel kernel,
        // and batch b + 1 is generated beside the pair counting of batch b
        rip_relabel_words(c, n, c->perm.as<int32_t>(), cnt);
        if (hipEventCreateWithFlags(&ev[(size_t)(2 * b + 1)], hipEventDisableTiming) != hipSuccess ||
            hipEventRecord(ev[(size_t)(2 * b + 1)], c->stream) != hipSuccess ||
            hipStreamWaitEvent(c->stream3, ev[(size_t)(2 * b + 1)], 0) != hipSuccess) { rc = SC_ERR_HIP; break; }
        if (b + 1 < batches) rc = generate(b + 1);
        if (rc != SC_OK) break;
        rip_count_words(c, pl, n, cnt, d_cnt);
        hipLaunchKernelGGL(k_ripley_sums, dim3((unsigned)ceil_div64(cells, 256)), dim3(256), 0, c->stream, d_cnt, d_obs, cnt, cells,
                           pl.R, d_sums);
    }
    if (rc == SC_ERR_HIP) sc_set_error("sc_ripley_counter: event plumbing failed");
    (void)hipStreamSynchronize(c->stream3);
    (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : ev)
        if (e) (void)hipEventDestroy(e);
    if (rc != SC_OK) return rc;
    SC_HIP(hipGetLastError());
    if (n_perm > 0) c->p_count = 0;   // the table holds the last batch only: not a table later calls may rely on
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
