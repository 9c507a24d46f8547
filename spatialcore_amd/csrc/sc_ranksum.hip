// N8: Wilcoxon rank sums of the loaded genes per group of cells (include/spatialcore_hip.h), as exact integers.  gfx950 only.
//
// Only the non-zero values of the ranked cells are sorted; the zeros are one tie block whose rank is known in closed form.
//   count    one pass over the tiles in GROUP-SORTED cell order, cut into pieces of <= RS_PIECE cells of one group: per
//            (gene, piece) the non-zero count and the sum of the values, per gene the negative count and a non-finite flag.
//            One exclusive scan of the (gene, piece) counts is every pair's home in a gene-major compacted array.
//   scatter  the same walk writes (key, payload) of every non-zero; the order inside a (gene, piece) cell is arbitrary
//            (an LDS cursor) and nothing downstream depends on it: the integer sums are order-free.
//   sort     ONE device-wide radix sort of the batch (a segmented sort would hand each gene to a single workgroup).
//            float32-exact batches: key = gene << 32 | ordered float32 bits, payload = group (16 bits), one sort over
//            the bits in use.  Other batches: key = ordered fp64 bits, payload = gene << 12 | group; sorted by value,
//            then stably by gene through an index permutation.
//   runs     fixed chunks of the sorted array: tie runs [a, b) (a run may begin before its chunk and end after it: two
//            binary searches per chunk), 2 * rank = a + b + 1 (+ 2 n_zero for positive values) added into a (gene, group)
//            int64 table in LDS and flushed with integer atomics; the first element of a run adds t^3 - t to the gene's
//            128-bit tie sum.
//   final    per (gene, group): the pieces' counts and sums in piece order, and the zero block's share of the rank sum.
#include <hipcub/hipcub.hpp>

#include <vector>

#include "sc_sortscan.h"

#define RS_PIECE 256                         // ranked cells of one group per workgroup of the count / scatter walk
#define RS_CHUNK 2048                        // sorted pairs per workgroup of k_rs_runs: 256 threads x 8
#define RS_TABLE 4096                        // int64 entries of its LDS table = the n_groups envelope
#define RS_GROUP_BITS 12                     // ... in the 32-bit payload of the fp64 form
#define RS_PAIR_BUDGET ((int64_t)1 << 27)    // pairs per sort batch: ~20 bytes each with double buffering

typedef unsigned long long u64;

// order-preserving unsigned images of a float / double (no NaN reaches them); the top bit is set exactly for values > 0
__device__ __forceinline__ uint32_t rs_ord32(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ u64 rs_ord64(double d)
{
    const u64 u = (u64)__double_as_longlong(d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// ------------------------------------------------------------------------------------------------
// count / scatter: workgroup = (piece, tile); thread = (slot of the tile, one of 16 row lanes)
// ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_rs_count(const double *__restrict__ X, int64_t n, const int32_t *__restrict__ order,
                                                  const int64_t *__restrict__ pstart, int64_t P, double *__restrict__ psum,
                                                  long long *__restrict__ pnnz, u64 *__restrict__ gneg,
                                                  uint32_t *__restrict__ gflag)
{
    __shared__ double sh_s[256];
    __shared__ int sh_c[256], sh_n[256], sh_b[256];
    const int64_t p = blockIdx.x, tile = blockIdx.y;
    const int slot = threadIdx.x & 15, lane = threadIdx.x >> 4;
    const double *a = X + tile * n * SC_TILE;
    const int64_t r1 = pstart[p + 1];
    double s = 0.0;
    int cnt = 0, neg = 0, bad = 0;
    for (int64_t r = pstart[p] + lane; r < r1; r += 16) {
        const double v = a[(int64_t)order[r] * SC_TILE + slot];
        s += v;
        cnt += v != 0.0;
        neg += v < 0.0;
        bad |= !(fabs(v) <= 1.7976931348623157e308);
    }
    sh_s[threadIdx.x] = s;
    sh_c[threadIdx.x] = cnt;
    sh_n[threadIdx.x] = neg;
    sh_b[threadIdx.x] = bad;
    __syncthreads();
    for (int w = 128; w >= 16; w >>= 1) {   // the lanes' partials in one fixed tree
        if ((int)threadIdx.x < w) {
            sh_s[threadIdx.x] += sh_s[threadIdx.x + w];
            sh_c[threadIdx.x] += sh_c[threadIdx.x + w];
            sh_n[threadIdx.x] += sh_n[threadIdx.x + w];
            sh_b[threadIdx.x] |= sh_b[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x < 16) {
        const int64_t gene = tile * SC_TILE + threadIdx.x;
        psum[gene * P + p] = sh_s[threadIdx.x];
        pnnz[gene * P + p] = sh_c[threadIdx.x];
        if (sh_n[threadIdx.x]) atomicAdd(&gneg[gene], (u64)sh_n[threadIdx.x]);
        if (sh_b[threadIdx.x]) atomicOr(&gflag[gene], 1u);
    }
}

// goff[g] = first pair of gene g in the compacted array, g = 0 .. genes (poff is [gene][piece], one entry past the end)
__global__ void k_rs_gene_offsets(const long long *__restrict__ poff, int64_t P, int64_t genes, long long *__restrict__ goff)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g <= genes) goff[g] = poff[g * P];
}

template <bool K32>
__global__ __launch_bounds__(256) void k_rs_scatter(const double *__restrict__ X, int64_t n, const int32_t *__restrict__ order,
                                                    const int64_t *__restrict__ pstart, const int32_t *__restrict__ pgroup,
                                                    int64_t P, const long long *__restrict__ poff, int64_t tile0,
                                                    long long base, u64 *__restrict__ keys, uint16_t *__restrict__ pay16,
                                                    uint32_t *__restrict__ pay32)
{
    __shared__ uint32_t cur[16];
    const int64_t p = blockIdx.x, tile = tile0 + blockIdx.y;
    const int slot = threadIdx.x & 15, lane = threadIdx.x >> 4;
    if (threadIdx.x < 16) cur[threadIdx.x] = 0u;
    __syncthreads();
    const double *a = X + tile * n * SC_TILE;
    const uint32_t grp = (uint32_t)pgroup[p];
    const uint32_t gl = (uint32_t)(blockIdx.y * SC_TILE + slot);   // gene within the batch
    const long long home = poff[(tile * SC_TILE + slot) * P + p] - base;
    const int64_t r1 = pstart[p + 1];
    for (int64_t r = pstart[p] + lane; r < r1; r += 16) {
        const double v = a[(int64_t)order[r] * SC_TILE + slot];
        if (v != 0.0) {
            const long long pos = home + (long long)atomicAdd(&cur[slot], 1u);   // < the (gene, piece) count of k_rs_count
            if (K32) {
                keys[pos] = ((u64)gl << 32) | rs_ord32((float)v);
                pay16[pos] = (uint16_t)grp;
            } else {
                keys[pos] = rs_ord64(v);
                pay32[pos] = (gl << RS_GROUP_BITS) | grp;
            }
        }
    }
}

// fp64 form, between its two sorts: the gene of every value-sorted pair as the second key, its position as the payload
__global__ __launch_bounds__(256) void k_rs_gene_keys(const uint32_t *__restrict__ pay32, int64_t cnt, uint32_t *__restrict__ gkey,
                                                      uint32_t *__restrict__ idx)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    gkey[i] = pay32[i] >> RS_GROUP_BITS;
    idx[i] = (uint32_t)i;
}
__global__ __launch_bounds__(256) void k_rs_gather(const u64 *__restrict__ keys_in, const uint32_t *__restrict__ pay_in,
                                                   const uint32_t *__restrict__ idx, int64_t cnt, u64 *__restrict__ keys_out,
                                                   uint32_t *__restrict__ pay_out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cnt) return;
    const uint32_t j = idx[i];
    keys_out[i] = keys_in[j];
    pay_out[i] = pay_in[j];
}

// ------------------------------------------------------------------------------------------------
// runs
// ------------------------------------------------------------------------------------------------

// tie[0] = high word, tie[1] = low word; the add that wraps the low word sees it in its own return value and carries
__device__ __forceinline__ void rs_add128(u64 *tie, unsigned __int128 x)
{
    const u64 lo = (u64)x, hi = (u64)(x >> 64);
    const u64 old = atomicAdd(&tie[1], lo);
    const u64 carry = (u64)(old + lo < old);
    if (hi + carry) atomicAdd(&tie[0], hi + carry);
}

template <bool K32>
__global__ __launch_bounds__(256) void k_rs_runs(const u64 *__restrict__ keys, const uint16_t *__restrict__ pay16,
                                                 const uint32_t *__restrict__ pay32, int64_t cnt,
                                                 const long long *__restrict__ goff, int64_t gene0, long long base,
                                                 int32_t n_groups, int64_t n_ranked, u64 *__restrict__ rank2, u64 *__restrict__ tie)
{
    typedef hipcub::BlockScan<int, 256> Scan;
    __shared__ typename Scan::TempStorage scan_tmp;
    __shared__ u64 table[RS_TABLE];
    __shared__ int rs[RS_CHUNK + 1];        // first position (within the chunk) of every run that has one in the chunk
    __shared__ long long ext[2];            // where the first run of the chunk really begins, the last one really ends
    __shared__ uint32_t gspan[2];           // first and last gene (within the batch) of the chunk
    __shared__ uint32_t next_gene;          // table rounds: the first gene behind the round's window that has a pair in the chunk
    const int64_t c0 = (int64_t)blockIdx.x * RS_CHUNK;
    const int64_t c1 = c0 + RS_CHUNK < cnt ? c0 + RS_CHUNK : cnt;
    const int64_t i0 = c0 + (int64_t)threadIdx.x * 8;
    auto gene_at = [&](int64_t i) -> uint32_t { return K32 ? (uint32_t)(keys[i] >> 32) : (pay32[i] >> RS_GROUP_BITS); };

    u64 k[8];
    uint32_t gl[8], gr[8];
    int rid[8];
    bool head[8];
    u64 kp = 0;
    uint32_t gp = 0;
    if (i0 > c0 && i0 < c1) {
        kp = keys[i0 - 1];
        gp = gene_at(i0 - 1);
    }
    int heads = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int64_t i = i0 + e;
        head[e] = false;
        k[e] = 0;
        gl[e] = gr[e] = 0u;
        if (i < c1) {
            k[e] = keys[i];
            if (K32) {
                gl[e] = (uint32_t)(k[e] >> 32);
                gr[e] = pay16[i];
            } else {
                const uint32_t w = pay32[i];
                gl[e] = w >> RS_GROUP_BITS;
                gr[e] = w & ((1u << RS_GROUP_BITS) - 1u);
            }
            head[e] = i == c0 || k[e] != kp || gl[e] != gp;
            kp = k[e];
            gp = gl[e];
        }
        heads += head[e];
        rid[e] = heads;     // inclusive count within the thread, made global below
    }
    int before = 0, n_runs = 0;
    Scan(scan_tmp).ExclusiveSum(heads, before, n_runs);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        rid[e] += before - 1;
        if (head[e]) rs[rid[e]] = (int)(i0 + e - c0);
    }
    // the chunk's first run may begin before it and its last run may end after it, inside the gene's sorted segment
    if (threadIdx.x == 0) {
        const u64 kf = keys[c0];
        const uint32_t gf = gene_at(c0);
        long long lo = goff[gene0 + gf] - base, hi = c0;
        if (hi > lo && keys[hi - 1] == kf && gene_at(hi - 1) == gf) {
            --hi;                                   // keys[hi] == kf: the first such position in [lo, hi]
            while (lo < hi) {
                const long long mid = lo + (hi - lo) / 2;
                if (keys[mid] < kf) lo = mid + 1; else hi = mid;
            }
        }
        ext[0] = hi;
        gspan[0] = gf;
        rs[n_runs] = (int)(c1 - c0);
    }
    if (threadIdx.x == 64) {
        const u64 kl = keys[c1 - 1];
        const uint32_t gg = gene_at(c1 - 1);
        long long lo = c1, hi = goff[gene0 + gg + 1] - base;
        if (lo < hi && keys[lo] == kl && gene_at(lo) == gg) {
            ++lo;                                   // first position in [lo, hi] whose key is larger (hi = the segment's end)
            while (lo < hi) {
                const long long mid = lo + (hi - lo) / 2;
                if (keys[mid] <= kl) lo = mid + 1; else hi = mid;
            }
        } else {
            lo = c1;
        }
        ext[1] = lo;
        gspan[1] = gg;
    }
    __syncthreads();

    // every element's run [a, b) as positions among its gene's non-zeros, and twice its rank
    u64 val[8];
    unsigned __int128 acc = 0;
    uint32_t acc_gene = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        val[e] = 0;
        if (i0 + e >= c1) continue;
        const long long seg0 = goff[gene0 + gl[e]] - base, seg1 = goff[gene0 + gl[e] + 1] - base;
        const long long ra = rid[e] == 0 ? ext[0] : c0 + rs[rid[e]];
        const long long rb = rid[e] == n_runs - 1 ? ext[1] : c0 + rs[rid[e] + 1];
        const u64 n_zero = (u64)(n_ranked - (seg1 - seg0));
        val[e] = (u64)((ra - seg0) + (rb - seg0) + 1) + ((k[e] >> (K32 ? 31 : 63)) & 1ull ? 2ull * n_zero : 0ull);
        if (head[e] && ra >= c0) {                  // the run begins in this chunk: this element owns its tie term
            const u64 t = (u64)(rb - ra);
            if (t > 1) {
                if (acc != 0 && acc_gene != gl[e]) {
                    rs_add128(tie + 2 * (gene0 + acc_gene), acc);
                    acc = 0;
                }
                acc_gene = gl[e];
                acc += (unsigned __int128)t * t * t - t;
            }
        }
    }
    if (acc != 0) rs_add128(tie + 2 * (gene0 + acc_gene), acc);

    // (gene, group) sums through the LDS table, as many genes at a time as it holds; the next round begins at the next
    // gene that has a pair in the chunk, so genes without one cost nothing
    const uint32_t per = (uint32_t)(RS_TABLE / n_groups);
    for (uint32_t w0 = gspan[0];;) {
        const uint32_t genes_here = gspan[1] - w0 + 1u < per ? gspan[1] - w0 + 1u : per;
        const int entries = (int)genes_here * n_groups;
        if (threadIdx.x == 0) next_gene = 0xffffffffu;
        for (int t = threadIdx.x; t < entries; t += 256) table[t] = 0ull;
        __syncthreads();
        uint32_t later = 0xffffffffu;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (i0 + e >= c1 || gl[e] < w0) continue;
            if (gl[e] - w0 < genes_here) atomicAdd(&table[(gl[e] - w0) * n_groups + gr[e]], val[e]);
            else if (gl[e] < later) later = gl[e];
        }
        if (later != 0xffffffffu) atomicMin(&next_gene, later);
        __syncthreads();
        for (int t = threadIdx.x; t < entries; t += 256)
            if (table[t]) atomicAdd(&rank2[(gene0 + w0) * n_groups + t], table[t]);
        const uint32_t nxt = next_gene;
        __syncthreads();
        if (nxt == 0xffffffffu) break;
        w0 = nxt;
    }
}

// per (gene, group): counts and sums of the group's pieces in piece order; the zero block's share of the rank sum
__global__ __launch_bounds__(256) void k_rs_final(const double *__restrict__ psum, const long long *__restrict__ pnnz, int64_t P,
                                                  const int64_t *__restrict__ gpiece, const long long *__restrict__ goff,
                                                  const u64 *__restrict__ gneg, const int64_t *__restrict__ group_n,
                                                  int64_t genes, int32_t n_groups, int64_t n_ranked, u64 *__restrict__ rank2,
                                                  long long *__restrict__ nnz_out, double *__restrict__ sum_out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= genes * n_groups) return;
    const int64_t gene = t / n_groups;
    const int grp = (int)(t % n_groups);
    long long nz = 0;
    double s = 0.0;
    for (int64_t p = gpiece[grp]; p < gpiece[grp + 1]; ++p) {
        nz += pnnz[gene * P + p];
        s += psum[gene * P + p];
    }
    const u64 n_zero = (u64)(n_ranked - (goff[gene + 1] - goff[gene]));
    rank2[t] += (u64)(group_n[grp] - nz) * (2ull * gneg[gene] + n_zero + 1ull);
    nnz_out[t] = nz;
    sum_out[t] = s;
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------

extern "C" int sc_ranksum(sc_ctx *c, const int32_t *group_code, int64_t n, int32_t n_groups, int64_t *rank2_out,
                          uint64_t *tie_out, int64_t *nnz_out, double *sum_out, int64_t *n_neg_out, int64_t *group_n_out)
{
    SC_REQUIRE(c && group_code && rank2_out && tie_out && nnz_out && sum_out && n_neg_out && group_n_out, SC_ERR_INVALID,
               "sc_ranksum: null pointer");
    SC_REQUIRE(n_groups >= 1 && n_groups <= RS_TABLE, SC_ERR_INVALID, "sc_ranksum: n_groups=%d outside [1, %d]", n_groups,
               RS_TABLE);
    SC_REQUIRE(c->e_n > 0, SC_ERR_STATE, "sc_ranksum: no expression loaded (call sc_expr_set_* first)");
    SC_REQUIRE(n == c->e_n, SC_ERR_INVALID, "sc_ranksum: %lld group codes for %lld loaded cells", (long long)n,
               (long long)c->e_n);
    SC_HIP(hipSetDevice(c->device));
    const int64_t G = c->e_genes, T = c->e_tiles, Gp = T * SC_TILE;

    // ranked cells in group order (stable), cut into pieces of at most RS_PIECE cells of one group
    std::vector<int64_t> group_n((size_t)n_groups, 0);
    for (int64_t i = 0; i < n; ++i) {
        const int32_t g = group_code[i];
        SC_REQUIRE(g >= -1 && g < n_groups, SC_ERR_INVALID, "sc_ranksum: group code %d of cell %lld outside [-1, %d)", g,
                   (long long)i, n_groups);
        if (g >= 0) ++group_n[(size_t)g];
    }
    std::vector<int64_t> cursor((size_t)n_groups), gpiece((size_t)n_groups + 1), pstart;
    std::vector<int32_t> pgroup;
    int64_t N = 0;
    for (int32_t g = 0; g < n_groups; ++g) {
        cursor[(size_t)g] = N;
        gpiece[(size_t)g] = (int64_t)pgroup.size();
        for (int64_t s = 0; s < group_n[(size_t)g]; s += RS_PIECE) {
            pstart.push_back(N + s);
            pgroup.push_back(g);
        }
        N += group_n[(size_t)g];
    }
    const int64_t P = (int64_t)pgroup.size();
    gpiece[(size_t)n_groups] = P;
    pstart.push_back(N);
    std::vector<int32_t> order((size_t)N);
    for (int64_t i = 0; i < n; ++i)
        if (group_code[i] >= 0) order[(size_t)cursor[(size_t)group_code[i]]++] = (int32_t)i;

    for (int32_t g = 0; g < n_groups; ++g) group_n_out[g] = group_n[(size_t)g];
    const size_t cells = (size_t)G * (size_t)n_groups;
    if (N == 0) {   // nothing is ranked
        for (size_t t = 0; t < cells; ++t) {
            rank2_out[t] = 0;
            nnz_out[t] = 0;
            sum_out[t] = 0.0;
        }
        for (int64_t g = 0; g < G; ++g) tie_out[2 * g] = tie_out[2 * g + 1] = 0, n_neg_out[g] = 0;
        return SC_OK;
    }

    SC_TRY(c->rs_order.ensure(sizeof(int32_t) * (size_t)N, &c->mem));
    SC_TRY(c->rs_pstart.ensure(sizeof(int64_t) * (size_t)(P + 1), &c->mem));
    SC_TRY(c->rs_pgroup.ensure(sizeof(int32_t) * (size_t)P, &c->mem));
    SC_TRY(c->rs_gpiece.ensure(sizeof(int64_t) * (size_t)(n_groups + 1), &c->mem));
    SC_TRY(c->rs_groupn.ensure(sizeof(int64_t) * (size_t)n_groups, &c->mem));
    const size_t gp_entries = (size_t)Gp * (size_t)P;
    SC_TRY(c->rs_psum.ensure(sizeof(double) * gp_entries, &c->mem));
    SC_TRY(c->rs_pnnz.ensure(sizeof(long long) * (gp_entries + 1), &c->mem));
    SC_TRY(c->rs_poff.ensure(sizeof(long long) * (gp_entries + 1), &c->mem));
    SC_TRY(c->rs_goff.ensure(sizeof(long long) * (size_t)(Gp + 1), &c->mem));
    SC_TRY(c->rs_neg.ensure(sizeof(u64) * (size_t)Gp, &c->mem));
    SC_TRY(c->rs_flag.ensure(sizeof(uint32_t) * (size_t)Gp, &c->mem));
    SC_TRY(c->rs_rank2.ensure(sizeof(u64) * (size_t)Gp * (size_t)n_groups, &c->mem));
    SC_TRY(c->rs_tie.ensure(sizeof(u64) * 2 * (size_t)Gp, &c->mem));
    SC_TRY(c->rs_nnz.ensure(sizeof(long long) * cells, &c->mem));
    SC_TRY(c->rs_sum.ensure(sizeof(double) * cells, &c->mem));
    SC_HIP(hipMemcpyAsync(c->rs_order.p, order.data(), sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(c->rs_pstart.p, pstart.data(), sizeof(int64_t) * (size_t)(P + 1), hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(c->rs_pgroup.p, pgroup.data(), sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(c->rs_gpiece.p, gpiece.data(), sizeof(int64_t) * (size_t)(n_groups + 1), hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(c->rs_groupn.p, group_n.data(), sizeof(int64_t) * (size_t)n_groups, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemsetAsync(c->rs_pnnz.as<long long>() + gp_entries, 0, sizeof(long long), c->stream));
    SC_HIP(hipMemsetAsync(c->rs_neg.p, 0, sizeof(u64) * (size_t)Gp, c->stream));
    SC_HIP(hipMemsetAsync(c->rs_flag.p, 0, sizeof(uint32_t) * (size_t)Gp, c->stream));
    SC_HIP(hipMemsetAsync(c->rs_rank2.p, 0, sizeof(u64) * (size_t)Gp * (size_t)n_groups, c->stream));
    SC_HIP(hipMemsetAsync(c->rs_tie.p, 0, sizeof(u64) * 2 * (size_t)Gp, c->stream));

    std::vector<long long> goff((size_t)Gp + 1);
    std::vector<uint32_t> bad((size_t)Gp), cls((size_t)Gp);
    {
        KernelTimerScope ts(c, SC_K_RANK_EMIT);
        hipLaunchKernelGGL(k_rs_count, dim3((unsigned)P, (unsigned)T), dim3(256), 0, c->stream, c->X.as<double>(), n,
                           c->rs_order.as<int32_t>(), c->rs_pstart.as<int64_t>(), P, c->rs_psum.as<double>(),
                           c->rs_pnnz.as<long long>(), c->rs_neg.as<u64>(), c->rs_flag.as<uint32_t>());
        SC_HIP(hipGetLastError());
        SC_TRY(sc_exclusive_sum(c, c->rs_tmp, c->stream, c->rs_pnnz.as<long long>(), c->rs_poff.as<long long>(), (int64_t)gp_entries + 1));
        hipLaunchKernelGGL(k_rs_gene_offsets, dim3((unsigned)ceil_div64(Gp + 1, 256)), dim3(256), 0, c->stream,
                           c->rs_poff.as<long long>(), P, Gp, c->rs_goff.as<long long>());
        SC_HIP(hipGetLastError());
    }
    SC_TRY(expr_gene_stats(c));   // bit 2 of a gene's flags: some value is not a float32
    SC_HIP(hipMemcpyAsync(goff.data(), c->rs_goff.p, sizeof(long long) * (size_t)(Gp + 1), hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipMemcpyAsync(bad.data(), c->rs_flag.p, sizeof(uint32_t) * (size_t)Gp, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipMemcpyAsync(cls.data(), c->g_flags.p, sizeof(uint32_t) * (size_t)Gp, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    for (int64_t g = 0; g < G; ++g)
        SC_REQUIRE(!bad[(size_t)g], SC_ERR_INVALID, "sc_ranksum: gene %lld has a non-finite value", (long long)g);

    // batches of whole tiles whose pairs fit the budget (a single tile is taken whatever it holds)
    for (int64_t t0 = 0; t0 < T;) {
        int64_t t1 = t0 + 1;
        while (t1 < T && goff[(size_t)((t1 + 1) * SC_TILE)] - goff[(size_t)(t0 * SC_TILE)] <= RS_PAIR_BUDGET &&
               (t1 + 1 - t0) * SC_TILE <= ((int64_t)1 << (32 - RS_GROUP_BITS)))
            ++t1;
        const long long base = goff[(size_t)(t0 * SC_TILE)];
        const int64_t cnt = goff[(size_t)(t1 * SC_TILE)] - base;
        const int64_t gene0 = t0 * SC_TILE, genes_here = (t1 - t0) * SC_TILE;
        bool k32 = true;
        for (int64_t g = gene0; g < gene0 + genes_here; ++g) k32 = k32 && !(cls[(size_t)g] & 4u);
        t0 = t1;
        if (cnt == 0) continue;
        SC_REQUIRE(cnt < ((int64_t)1 << 32), SC_ERR_INVALID, "sc_ranksum: %lld non-zero values in 16 genes, at most 2^32 - 1",
                   (long long)cnt);
        SC_TRY(c->rs_keys.ensure(sizeof(u64) * (size_t)cnt, &c->mem));
        SC_TRY(c->rs_keys2.ensure(sizeof(u64) * (size_t)cnt, &c->mem));
        SC_TRY(c->rs_pay.ensure((k32 ? sizeof(uint16_t) : sizeof(uint32_t)) * (size_t)cnt, &c->mem));
        SC_TRY(c->rs_pay2.ensure((k32 ? sizeof(uint16_t) : sizeof(uint32_t)) * (size_t)cnt, &c->mem));
        const dim3 walk((unsigned)P, (unsigned)(t1 - (gene0 / SC_TILE)));
        const unsigned flat = (unsigned)ceil_div64(cnt, 256), chunks = (unsigned)ceil_div64(cnt, RS_CHUNK);
        {
            KernelTimerScope ts(c, SC_K_RANK_EMIT);
            auto scatter = k32 ? k_rs_scatter<true> : k_rs_scatter<false>;
            hipLaunchKernelGGL(scatter, walk, dim3(256), 0, c->stream, c->X.as<double>(), n, c->rs_order.as<int32_t>(),
                               c->rs_pstart.as<int64_t>(), c->rs_pgroup.as<int32_t>(), P, c->rs_poff.as<long long>(),
                               gene0 / SC_TILE, base, c->rs_keys.as<u64>(), c->rs_pay.as<uint16_t>(), c->rs_pay.as<uint32_t>());
            SC_HIP(hipGetLastError());
        }
        const u64 *keys = nullptr;
        if (k32) {
            KernelTimerScope ts(c, SC_K_RANK_SORT);
            SC_TRY(sc_sort_pairs(c, c->rs_tmp, c->stream, c->rs_keys.as<u64>(), c->rs_keys2.as<u64>(), c->rs_pay.as<uint16_t>(),
                                 c->rs_pay2.as<uint16_t>(), cnt, 32 + sc_bits_for(genes_here)));
            keys = c->rs_keys2.as<u64>();
        } else {
            KernelTimerScope ts(c, SC_K_RANK_SORT);
            SC_TRY(c->rs_gkey.ensure(sizeof(uint32_t) * (size_t)cnt, &c->mem));
            SC_TRY(c->rs_gkey2.ensure(sizeof(uint32_t) * (size_t)cnt, &c->mem));
            SC_TRY(c->rs_idx.ensure(sizeof(uint32_t) * (size_t)cnt, &c->mem));
            SC_TRY(c->rs_idx2.ensure(sizeof(uint32_t) * (size_t)cnt, &c->mem));
            SC_TRY(sc_sort_pairs(c, c->rs_tmp, c->stream, c->rs_keys.as<u64>(), c->rs_keys2.as<u64>(), c->rs_pay.as<uint32_t>(),
                                 c->rs_pay2.as<uint32_t>(), cnt, 64));
            hipLaunchKernelGGL(k_rs_gene_keys, dim3(flat), dim3(256), 0, c->stream, c->rs_pay2.as<uint32_t>(), cnt,
                               c->rs_gkey.as<uint32_t>(), c->rs_idx.as<uint32_t>());
            SC_HIP(hipGetLastError());
            SC_TRY(sc_sort_pairs(c, c->rs_tmp, c->stream, c->rs_gkey.as<uint32_t>(), c->rs_gkey2.as<uint32_t>(), c->rs_idx.as<uint32_t>(),
                                 c->rs_idx2.as<uint32_t>(), cnt, sc_bits_for(genes_here)));
            hipLaunchKernelGGL(k_rs_gather, dim3(flat), dim3(256), 0, c->stream, c->rs_keys2.as<u64>(), c->rs_pay2.as<uint32_t>(),
                               c->rs_idx2.as<uint32_t>(), cnt, c->rs_keys.as<u64>(), c->rs_pay.as<uint32_t>());
            SC_HIP(hipGetLastError());
            keys = c->rs_keys.as<u64>();
        }
        {
            KernelTimerScope ts(c, SC_K_RANK_RUNS);
            auto runs = k32 ? k_rs_runs<true> : k_rs_runs<false>;
            hipLaunchKernelGGL(runs, dim3(chunks), dim3(256), 0, c->stream, keys, c->rs_pay2.as<uint16_t>(),
                               c->rs_pay.as<uint32_t>(), cnt, c->rs_goff.as<long long>(), gene0, base, n_groups, N,
                               c->rs_rank2.as<u64>(), c->rs_tie.as<u64>());
            SC_HIP(hipGetLastError());
        }
    }
    hipLaunchKernelGGL(k_rs_final, dim3((unsigned)ceil_div64((int64_t)cells, 256)), dim3(256), 0, c->stream,
                       c->rs_psum.as<double>(), c->rs_pnnz.as<long long>(), P, c->rs_gpiece.as<int64_t>(),
                       c->rs_goff.as<long long>(), c->rs_neg.as<u64>(), c->rs_groupn.as<int64_t>(), G, n_groups, N,
                       c->rs_rank2.as<u64>(), c->rs_nnz.as<long long>(), c->rs_sum.as<double>());
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(rank2_out, c->rs_rank2.p, sizeof(int64_t) * cells, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipMemcpyAsync(tie_out, c->rs_tie.p, sizeof(uint64_t) * 2 * (size_t)G, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipMemcpyAsync(nnz_out, c->rs_nnz.p, sizeof(int64_t) * cells, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipMemcpyAsync(sum_out, c->rs_sum.p, sizeof(double) * cells, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipMemcpyAsync(n_neg_out, c->rs_neg.p, sizeof(int64_t) * (size_t)G, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}
