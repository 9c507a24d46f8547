// Global Moran's I with permutations: the scoring prelude, the scoring kernels, the finalisation.  gfx950 only.
// (Tiles: sc_expr.hip.  The permutation table is [perm][cell] int32 with a row stride that is a multiple of 32 elements,
// so that rows can be read as int4: sc_perm.hip.)
#include <math.h>
#include <stdlib.h>

#include <functional>
#include <vector>

#include "sc_permgen.h"

// ------------------------------------------------------------------------------------------------
// A5: the permutation kernel (the metric's dominant kernel)
//
//   partial[s][p][g] = sum_{i in split s} Z[i][g] * Lag[perm_p[i]][g]        (one 16-gene tile)
//
// Workgroup = 256 threads = 4 wavefronts; wavefront w of block (s, pt) owns permutations
// pt*32 + w*8 + (lane >> 3) and the gene pair (lane & 7): every lane keeps its two fp64
// accumulators in registers across the whole cell range, so there is no cross-lane reduction at
// all.  Per cell a wavefront issues ONE 16-byte-per-lane gather that pulls 8 full 128-byte Lag
// rows (8 permutations x 16 genes) and one broadcast read of the 128-byte Z row.
// ------------------------------------------------------------------------------------------------

#define MP_PERMS_PER_BLOCK 32

__global__ __launch_bounds__(256) void k_moran_perm(const double *__restrict__ Zt,
                                                    const double *__restrict__ Lt,
                                                    const int32_t *__restrict__ perm,
                                                    double *__restrict__ partial, int64_t n,
                                                    int64_t pstride, int n_perm, int64_t cells_per_split)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane >> 3, q = lane & 7;
    const int pbase = blockIdx.y * MP_PERMS_PER_BLOCK + wave * 8;
    if (pbase >= n_perm) return;  // whole wavefront idle (no barriers in this kernel)
    const int p = pbase + r;
    const int pc = p < n_perm ? p : n_perm - 1;
    const int64_t c0 = (int64_t)blockIdx.x * cells_per_split;
    int64_t c1 = c0 + cells_per_split;
    if (c1 > n) c1 = n;
    const int32_t *prow = perm + (int64_t)pc * pstride;
    const double2 *Z2 = reinterpret_cast<const double2 *>(Zt) + q;
    const double2 *L2 = reinterpret_cast<const double2 *>(Lt) + q;

    double a0x = 0.0, a0y = 0.0, a1x = 0.0, a1y = 0.0;
    int64_t i = c0;  // c0 is a multiple of 8 (cells_per_split is)
    for (; i + 8 <= c1; i += 8) {
        const int4 ia = *reinterpret_cast<const int4 *>(prow + i);
        const int4 ib = *reinterpret_cast<const int4 *>(prow + i + 4);
        const double2 l0 = L2[(int64_t)ia.x * 8];
        const double2 l1 = L2[(int64_t)ia.y * 8];
        const double2 l2 = L2[(int64_t)ia.z * 8];
        const double2 l3 = L2[(int64_t)ia.w * 8];
        const double2 l4 = L2[(int64_t)ib.x * 8];
        const double2 l5 = L2[(int64_t)ib.y * 8];
        const double2 l6 = L2[(int64_t)ib.z * 8];
        const double2 l7 = L2[(int64_t)ib.w * 8];
        const double2 z0 = Z2[(i + 0) * 8];
        const double2 z1 = Z2[(i + 1) * 8];
        const double2 z2 = Z2[(i + 2) * 8];
        const double2 z3 = Z2[(i + 3) * 8];
        const double2 z4 = Z2[(i + 4) * 8];
        const double2 z5 = Z2[(i + 5) * 8];
        const double2 z6 = Z2[(i + 6) * 8];
        const double2 z7 = Z2[(i + 7) * 8];
        a0x = fma(z0.x, l0.x, a0x); a0y = fma(z0.y, l0.y, a0y);
        a1x = fma(z1.x, l1.x, a1x); a1y = fma(z1.y, l1.y, a1y);
        a0x = fma(z2.x, l2.x, a0x); a0y = fma(z2.y, l2.y, a0y);
        a1x = fma(z3.x, l3.x, a1x); a1y = fma(z3.y, l3.y, a1y);
        a0x = fma(z4.x, l4.x, a0x); a0y = fma(z4.y, l4.y, a0y);
        a1x = fma(z5.x, l5.x, a1x); a1y = fma(z5.y, l5.y, a1y);
        a0x = fma(z6.x, l6.x, a0x); a0y = fma(z6.y, l6.y, a0y);
        a1x = fma(z7.x, l7.x, a1x); a1y = fma(z7.y, l7.y, a1y);
    }
    for (; i < c1; ++i) {
        const double2 l = L2[(int64_t)prow[i] * 8];
        const double2 z = Z2[i * 8];
        a0x = fma(z.x, l.x, a0x);
        a0y = fma(z.y, l.y, a0y);
    }
    if (p < n_perm) {
        double2 *out = reinterpret_cast<double2 *>(partial) +
                       ((int64_t)blockIdx.x * n_perm + p) * 8 + q;
        *out = make_double2(a0x + a1x, a0y + a1y);
    }
}

// sims[p0 + p][g0 + slot] = seff * (sum_s partial[s][p][slot] - corr)   (ascending s); raw = the sum itself
__global__ __launch_bounds__(256) void k_moran_finalize(const double *__restrict__ partial,
                                                        const double *__restrict__ seff, const double *__restrict__ corr,
                                                        double *__restrict__ sims, double *__restrict__ raw, int n_perm, int splits,
                                                        int64_t n_genes, int64_t g0, int64_t p0)
{
    int t = blockIdx.x * blockDim.x + threadIdx.x;
    int p = t >> 4, slot = t & 15;
    if (p >= n_perm || g0 + slot >= n_genes) return;
    double s = 0.0;
    for (int k = 0; k < splits; ++k) s += partial[((int64_t)k * n_perm + p) * SC_TILE + slot];
    raw[(p0 + p) * n_genes + g0 + slot] = s;
    sims[(p0 + p) * n_genes + g0 + slot] = seff[g0 + slot] * (s - corr[g0 + slot]);
}

// Per gene: how a sum over the cells becomes the statistic, and what the permutation count compares.
//   ordinary gene: sum = sum_j lag_j z_j;  seff = n / s0 / z2, corr = 0, I = seff * sum, count: sims >= I
//   lattice gene (integer counts, every graph weight = w): sum = T = sum_j S_j x_j, an exact integer (S = unweighted
//     neighbour sums); sum_j lag_j z_j = w (T - mean * sum_j S_j) in exact arithmetic, so seff = n / s0 / z2 * w,
//     corr = mean * sum_j S_j, I = seff * (T_obs - corr), and the count compares the integers: T_p >= T_obs
__global__ void k_moran_scale(const double *__restrict__ z2, const double *__restrict__ inum, const double *__restrict__ slag,
                              const double *__restrict__ mean, const double *__restrict__ lat, double *__restrict__ seff,
                              double *__restrict__ corr, double *__restrict__ thr, double *__restrict__ I, double n_over_s0,
                              double w, int64_t total)
{
    int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const bool l = lat[g] != 0.0;
    const double sc = l ? (n_over_s0 / z2[g]) * w : n_over_s0 / z2[g];
    const double co = l ? mean[g] * slag[g] : 0.0;
    const double v = sc * (inum[g] - co);
    seff[g] = sc;
    corr[g] = co;
    I[g] = v;
    thr[g] = l ? inum[g] : v;
}

// per gene: count(sims >= I) -- for lattice genes count(T_p >= T_obs), on the exact integer sums --, sum sims,
// sum sims^2 over permutations (block per gene, fixed tree).  A zero-variance gene (I = NaN) counts nothing.
__global__ __launch_bounds__(256) void k_moran_count(const double *__restrict__ sims, const double *__restrict__ raw,
                                                     const double *__restrict__ thr, const double *__restrict__ lat,
                                                     const double *__restrict__ z2, int n_perm,
                                                     int64_t n_genes, long long *__restrict__ count,
                                                     double *__restrict__ ssum, double *__restrict__ ssq)
{
    __shared__ double sh_a[256], sh_b[256];
    __shared__ int sh_c[256];
    int64_t g = blockIdx.x;
    const double t = thr[g];
    const bool l = lat[g] != 0.0, alive = z2[g] > 0.0;
    double a = 0.0, b = 0.0;
    int cnt = 0;
    for (int p = threadIdx.x; p < n_perm; p += 256) {
        double v = sims[(int64_t)p * n_genes + g];
        const double cv = l ? raw[(int64_t)p * n_genes + g] : v;
        cnt += (alive && cv >= t) ? 1 : 0;
        a += v;
        b += v * v;
    }
    sh_a[threadIdx.x] = a;
    sh_b[threadIdx.x] = b;
    sh_c[threadIdx.x] = cnt;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sh_a[threadIdx.x] += sh_a[threadIdx.x + s];
            sh_b[threadIdx.x] += sh_b[threadIdx.x + s];
            sh_c[threadIdx.x] += sh_c[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        count[g] = sh_c[0];
        ssum[g] = sh_a[0];
        ssq[g] = sh_b[0];
    }
}

// ------------------------------------------------------------------------------------------------
// A5: the permutation statistic, summed over the TARGET cell,
//
//   sims[p][g] = scale_g * sum_j lag_g[j] * z_g[inv_p[j]],   inv_p = perm_p^-1,   z = (double)x - centre_g
//
// The fp64 lag rows are the streamed, coalesced operand; the INVERSE permutation supplies the gather index; the
// gathered operand is a 128-byte row of the raw values in the narrowest type that holds EVERY loaded gene exactly:
//   * 128 uint8 genes  (BITS = 8)   every value an integer count in [0, 255] and every gene a lattice gene (below),
//   * 64 uint16 genes  (BITS = 16)  every value an integer count in [0, 65535],
//   * 32 float32 genes (BITS = 32)  every value a float32 (AnnData's usual dtype),
//   * 16 fp64 genes    (BITS = 64)  anything else: the rows of the Z tiles themselves.
// z is rebuilt in registers: (double)x - centre is the very subtraction k_center performs for the Z tiles, and every
// width adds the same products in the same order (cells ascending inside a split, splits ascending in the
// finalisation) -- A GENE'S STATISTICS DO NOT DEPEND ON THE WIDTH, i.e. not on the genes it is loaded with.
//
// Lattice genes (integer counts on a graph whose weights all equal w, e.g. kNN: w = 1 / k): lag_j = w S_j - mean with
// the integer neighbour sum S_j, so the part of the statistic that depends on the permutation is T_p = sum_j S_j x[inv_p[j]],
// an integer, and a permutation can TIE the observed value exactly (41 of 250 Poisson genes of the bench matrix have
// such a permutation among 1000).  Rounded lag / z operands decide those ties by summation-order noise -- the
// reference's numba loop as much as any kernel here.  They are therefore scored on the lattice itself: centre = 0,
// streamed operand = S (k_lag with unit weights).  Every product and partial sum is an integer below 2^53 (checked on
// the host: max degree * largest count * sum of counts), so the fp64 arithmetic is EXACT in any order, and the
// permutation count is #{T_p >= T_obs} on integers (k_moran_scale / k_moran_count turn T into I and sims).
// The uint8 kernel has no registers for 16 centres next to its 16 accumulators; it is used when every loaded gene is a
// lattice gene (centre 0); uint8-sized counts on a graph with unequal weights take the uint16 kernel.
//
// Row layout (all widths): the 8 lanes q that share a row own genes {16 t + 2 q, 16 t + 2 q + 1 : t < TG} of the
// group's TG 16-gene tiles (TG = 8 / 4 / 2 / 1), stored as the lane's 16 bytes [t][e]: a lane's lag operands are then TG
// 16-byte LDS reads that are contiguous across q (no bank conflicts), one per lag tile.
//
// What bounds the uint8 form (r02, 1M cells, 128 genes x 128 permutations, 3.56 ms on 248 CUs; measured with diagnostic
// builds that gave wrong sums on purpose -- they are in history, commit 2d8ee49): half the LDS reads of lag 3.40 ms, no
// int -> fp64 conversions 3.50, neither byte extraction nor conversion 3.44 -- neither LDS nor VALU issue; the gathered
// rows alone are 4.6 TB/s, with the lag rows and indices ~5.7 TB/s memory-side: the random 128-byte gather at what the
// fabric sustains.
// ------------------------------------------------------------------------------------------------

// centre[g] = lat[g] ? 0 : mean[g]
__global__ void k_moran_centres(const double *__restrict__ mean, const double *__restrict__ lat, double *__restrict__ centre,
                                int64_t total)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g < total) centre[g] = lat[g] != 0.0 ? 0.0 : mean[g];
}

// ------------------------------------------------------------------------------------------------
// The scoring kernel: PERSISTENT, one 16-wavefront workgroup per compute unit, wavefronts as independent workers.
//
// Work = tasks (gene group, cell split, group of 8 permutations); wavefront w of the grid takes tasks w, w + W,
// w + 2 W, ... (groups slowest: the chip works on one 128-MB narrow table at a time, which stays in the
// Infinity Cache).  Lane = (permutation r of the 8, q): it keeps 2 TG fp64 accumulators over the task's cell range --
// no cross-lane reduction, no workgroup barrier.  A task is software-pipelined in blocks of CB cells:
//   (1) the lag rows of block b + 1 are loaded cooperatively (one coalesced 16-byte load per lane and piece: every
//       lag row is fetched ONCE per wavefront, not once per permutation),
//   (2) all CB random row gathers of block b + 1 are issued (indices were loaded two blocks ahead),
//   (3) the indices of block b + 3 are loaded,
//   (4) [wait: only the loads of (2), (3) stay outstanding -- vmcnt retires in order]
//   (5) the lag rows of block b + 1 are parked in the wavefront's private LDS slice,
//   (6) block b is multiplied: gathered rows from registers, lag rows from LDS (a broadcast to the 8 permutations).
// CB kilobytes of random rows are in flight per wavefront while it computes.
//
// Why persistent and 1024 threads: with > 64 VGPRs per lane a second 16-wavefront workgroup cannot fit on a compute
// unit, so a grid of W workgroups occupies exactly W of the 256 compute units and leaves the others EMPTY for the
// permutation generator that runs beside it (sc_moran_seeded) -- without CU-masked or prioritised streams, which were
// found to corrupt concurrently running kernels on this platform (see moran_seeded_streams).
// Sums: per gene, cells ascending inside a split, splits ascending in k_moran_finalize_groups -- the same order for
// both source widths, so their results are bit-identical (and independent of the grid size).
// ------------------------------------------------------------------------------------------------

#define SCORE_WAVES 16
#define SCORE_PRIVATE_WAVES 8   // k_moran_score (r04): 512-thread workgroups -- under the 128-VGPR cap of a 1024-thread workgroup
                                // its private lag staging spilled 6-10 registers (28-44 B of scratch per lane); its wavefronts
                                // are independent workers, so two workgroups of 8 per compute unit are the same 16 workers

// L16 (BITS == 8 only, r04): the lag operand arrives as the 16-bit neighbour sums k_lag_u8 leaves -- Lag16[group][cell][t][q]
// = S of genes (16 t + 2 q, + 1) as two uint16 in one word, 256 bytes per cell and 128-gene group instead of 1 KB of fp64
// -- and becomes the same fp64 values when it is parked in LDS (integers: exact): a quarter of the streamed bytes.
__device__ __forceinline__ double2 lag16_to_double2(uint32_t v) { return make_double2((double)(v & 0xffffu), (double)(v >> 16)); }

// ---- what k_moran_score and k_moran_score_wg do alike, in their pipelined loops and in their ragged tails ----
// (A task's operands come in by reference, and each kernel binds them once per task in a one-line lambda: passed by
// value, or named at every call, hipcc orders the address arithmetic of several instantiations differently -- as it does
// with the per-task set-up, centres and cleared accumulators, in a function: that stays written out in both kernels.
// scripts/isa_diff.py compares the ISA.)

// The lane's 16 bytes (qoff = 16 q) of row i of a group's table Xg, at byte offset 128 i: a 32-bit offset from a
// wavefront-uniform base (n < 2^25 cells, else the host picks the BIG form), i.e. no 64-bit address arithmetic per gather
template <bool BIG>
__device__ __forceinline__ uint4 score_row(const char *const &Xg, const uint32_t &qoff, int32_t i)
{
    if constexpr (BIG) return *reinterpret_cast<const uint4 *>(Xg + ((uint64_t)(uint32_t)i * 128u + qoff));
    else return *reinterpret_cast<const uint4 *>(Xg + ((uint32_t)i * 128u + qoff));
}

// the index vectors of block b of the nblk blocks of a split that begins at cell c0 of the inverse row irow
template <int CB>
__device__ __forceinline__ void score_load_idx(int4 (&id)[CB / 4], const int32_t *const &irow, const int64_t &c0, int64_t b, const int64_t &nblk)
{
    const int64_t bb = b < nblk ? b : nblk - 1;   // past the end: a harmless reload of the last block
#pragma unroll
    for (int k = 0; k < CB / 4; ++k) id[k] = *reinterpret_cast<const int4 *>(irow + c0 + bb * CB + 4 * k);
}

template <int CB, bool BIG>
__device__ __forceinline__ void score_gather(uint4 (&x)[CB], const int4 (&id)[CB / 4], const char *const &Xg, const uint32_t &qoff)
{
#pragma unroll
    for (int k = 0; k < CB / 4; ++k) {
        x[4 * k + 0] = score_row<BIG>(Xg, qoff, id[k].x);
        x[4 * k + 1] = score_row<BIG>(Xg, qoff, id[k].y);
        x[4 * k + 2] = score_row<BIG>(Xg, qoff, id[k].z);
        x[4 * k + 3] = score_row<BIG>(Xg, qoff, id[k].w);
    }
}

// tile t of one gathered row (w: the lane's four words): the two values of the lane's gene pair, centred, times the lag pair l
template <int BITS, bool CENTER>
__device__ __forceinline__ void score_fma(const uint32_t (&w)[4], int t, double2 l, const double (&m)[2], double (&acc)[2])
{
    double v0, v1;
    if (BITS == 8) {
        const uint32_t h = w[t >> 1] >> (16 * (t & 1));
        v0 = (double)(h & 0xffu); v1 = (double)((h >> 8) & 0xffu);
    } else if (BITS == 16) { v0 = (double)(w[t] & 0xffffu); v1 = (double)(w[t] >> 16); }
    else if (BITS == 32) { v0 = (double)__uint_as_float(w[2 * t]); v1 = (double)__uint_as_float(w[2 * t + 1]); }
    else { v0 = __hiloint2double((int)w[1], (int)w[0]); v1 = __hiloint2double((int)w[3], (int)w[2]); }
    if constexpr (CENTER) { v0 -= m[0]; v1 -= m[1]; }
    acc[0] = fma(l.x, v0, acc[0]);
    acc[1] = fma(l.y, v1, acc[1]);
}

// ---- the byte-plane products of k_moran_score_wg<8, 4, false, true> ----
// Counts x <= 255 and neighbour sums S = lo + 256 hi <= 65535 are integers, so sum_j S_j x_j = sum lo x + 256 sum hi x, and
// each plane is a sum of byte products: v_dot4_u32_u8 takes four cells at a time once both operands hold one gene's bytes
// of the block's four cells in one word.  Exact, and the same doubles as the fp64 products give: a plane sum of a task is
// at most cells_per_split * 255 * 255 <= 65536 * 65025 = 4 261 478 400 < 2^32 (score_cells_per_split(n) <= 65536 for every
// n < 2^25 this form serves), and the recombined sum is below 65536 * 65535 * 255 < 2^53.

// o[i] = byte i of the words a, b, c, d of four rows (ascending): the transposed 4 x 4 byte square
__device__ __forceinline__ void score_transpose4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t (&o)[4])
{
    const uint32_t ab0 = __builtin_amdgcn_perm(b, a, 0x05010400u), ab1 = __builtin_amdgcn_perm(b, a, 0x07030602u);
    const uint32_t cd0 = __builtin_amdgcn_perm(d, c, 0x05010400u), cd1 = __builtin_amdgcn_perm(d, c, 0x07030602u);
    o[0] = __builtin_amdgcn_perm(cd0, ab0, 0x05040100u);
    o[1] = __builtin_amdgcn_perm(cd0, ab0, 0x07060302u);
    o[2] = __builtin_amdgcn_perm(cd1, ab1, 0x05040100u);
    o[3] = __builtin_amdgcn_perm(cd1, ab1, 0x07060302u);
}

// One block of four gathered rows times its plane image sp = &image[block][q]: piece sp[8 t] holds, for tile t, the words
// {lo, hi of gene 16 t + 2 q; lo, hi of gene 16 t + 2 q + 1}, byte i of a word = cell i of the block.  lo / hi[2 t + e]: the
// lane's plane sums of gene 16 t + 2 q + e.
__device__ __forceinline__ void score_dot_block(const uint4 (&x)[4], const uint4 *sp, uint32_t (&lo)[16], uint32_t (&hi)[16])
{
    const uint32_t w[4][4] = {{x[0].x, x[0].y, x[0].z, x[0].w}, {x[1].x, x[1].y, x[1].z, x[1].w},
                              {x[2].x, x[2].y, x[2].z, x[2].w}, {x[3].x, x[3].y, x[3].z, x[3].w}};
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // word k of the rows: tiles 2 k and 2 k + 1
        uint32_t o[4];
        score_transpose4(w[0][k], w[1][k], w[2][k], w[3][k], o);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint4 s = sp[(2 * k + h) * 8];
            const int g = 4 * k + 2 * h;
            lo[g] = __builtin_amdgcn_udot4(o[2 * h], s.x, lo[g], false);
            hi[g] = __builtin_amdgcn_udot4(o[2 * h], s.y, hi[g], false);
            lo[g + 1] = __builtin_amdgcn_udot4(o[2 * h + 1], s.z, lo[g + 1], false);
            hi[g + 1] = __builtin_amdgcn_udot4(o[2 * h + 1], s.w, hi[g + 1], false);
        }
    }
}

template <int BITS, int CB, bool BIG, bool L16 = false>
__global__ __launch_bounds__(SCORE_PRIVATE_WAVES * 64) void k_moran_score(
    const uint4 *__restrict__ narrow, const double *__restrict__ Lag, int64_t tile_elems, int tiles16,
    const double *__restrict__ mean, const int32_t *__restrict__ inv, double *__restrict__ partial, int64_t n,
    int64_t pstride, int n_perm, int64_t cells_per_split, int n_splits, int n_groups)
{
    static_assert((BITS == 8 || BITS == 16 || BITS == 32 || BITS == 64) && (CB == 4 || CB == 8), "source width / block size");
    static_assert(!L16 || BITS == 8, "16-bit lag rows belong to the uint8 source");
    constexpr int TG = BITS == 8 ? 8 : BITS == 16 ? 4 : BITS == 32 ? 2 : 1;   // 16-gene lag tiles per gene group
    // BITS == 8 (128 genes per row, 16 accumulators per lane): no room for 16 centres in registers -- only launched when
    // every gene of the batch is a lattice gene (centre 0, integer operands: exact).  BITS == 64 gathers rows of the Z
    // tiles, which are centred already.
    constexpr bool CENTER = BITS == 16 || BITS == 32;
    constexpr int ROW = TG * 8;                  // 16-byte pieces of a group's lag row (one cell)
    static_assert((CB * ROW) % 64 == 0, "a block's lag rows are loaded by whole wavefront instructions");
    constexpr int NI = CB / 4;                   // index vectors per block
    constexpr int NL = CB * ROW / 64;            // lag pieces per lane and block
    constexpr int CSTEP = 64 / ROW;              // cells covered by one cooperative lag load
    __shared__ double2 lds_lag[SCORE_PRIVATE_WAVES][2][CB * ROW];   // [wavefront][buffer][cell][ROW]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane >> 3, q = lane & 7;
    const int lcell0 = lane / ROW, ltile = (lane % ROW) >> 3;
    double2 *lw = &lds_lag[wave][0][0];
    const int pgroups = (n_perm + 7) >> 3;
    // (Measured and dropped in r02: giving each XCD -- blockIdx % 8 -- its own subset of the cell splits, so that a
    //  split's lag rows are fetched by one L2 only: same launch time, same PMC traffic.)
    const int64_t n_tasks = (int64_t)n_groups * n_splits * pgroups;
    const int64_t worker = (int64_t)blockIdx.x * SCORE_PRIVATE_WAVES + wave, workers = (int64_t)gridDim.x * SCORE_PRIVATE_WAVES;

    for (int64_t task = worker; task < n_tasks; task += workers) {
        const int pg = (int)(task % pgroups);
        const int64_t rest = task / pgroups;
        const int split = (int)(rest % n_splits), grp = (int)(rest / n_splits);
        const int p = pg * 8 + r;
        const int pc = p < n_perm ? p : n_perm - 1;
        const int64_t c0 = (int64_t)split * cells_per_split;
        int64_t c1 = c0 + cells_per_split;
        if (c1 > n) c1 = n;
        const int32_t *irow = inv + (int64_t)pc * pstride;
        const char *Xg = reinterpret_cast<const char *>(narrow + (int64_t)grp * n * 8);
        const uint32_t qoff = (uint32_t)q * 16u;
        const int tiles_left = tiles16 - TG * grp;                                 // lag tiles this group really has
        const double *lag_g = Lag + (int64_t)TG * grp * tile_elems;
        // (a padded last group re-reads its first tile for the missing ones; those sums are never used)
        const double2 *lsrc = reinterpret_cast<const double2 *>(lag_g + (int64_t)(ltile < tiles_left ? ltile : 0) * tile_elems) + (lane & 7);
        const uint32_t *lag16_g = reinterpret_cast<const uint32_t *>(Lag) + (int64_t)grp * n * ROW;   // L16: [cell][ROW] words
        const uint32_t *lsrc16 = lag16_g + (lane % ROW);
        double m[CENTER ? TG : 1][2], acc[TG][2];
#pragma unroll
        for (int t = 0; t < TG; ++t) {
            if constexpr (CENTER) {
                const double *mt = mean + (int64_t)(TG * grp + (t < tiles_left ? t : 0)) * SC_TILE + 2 * q;
                m[t][0] = mt[0]; m[t][1] = mt[1];
            }
            acc[t][0] = acc[t][1] = 0.0;
        }
        const int64_t nblk = (c1 - c0) / CB;

        int4 ida[NI], idb[NI];
        double2 lg0, lg1, lg2, lg3;   // lag pieces on their way to LDS (as many as NL)
        uint32_t lh0 = 0, lh1 = 0, lh2 = 0, lh3 = 0;   // ... as 16-bit pairs (L16)
        uint4 xa[CB], xb[CB];

        auto load_idx = [&](int4 (&id)[NI], int64_t b) { score_load_idx<CB>(id, irow, c0, b, nblk); };
        auto load_lag = [&](int64_t b) {
            const int64_t bb = b < nblk ? b : nblk - 1;
            const int64_t row0 = c0 + bb * CB + lcell0;
            if constexpr (L16) {
                lh0 = lsrc16[row0 * ROW];
                if constexpr (NL > 1) lh1 = lsrc16[(row0 + CSTEP) * ROW];
                if constexpr (NL > 2) { lh2 = lsrc16[(row0 + 2 * CSTEP) * ROW]; lh3 = lsrc16[(row0 + 3 * CSTEP) * ROW]; }
            } else {
                lg0 = lsrc[row0 * 8];
                if constexpr (NL > 1) lg1 = lsrc[(row0 + CSTEP) * 8];
                if constexpr (NL > 2) { lg2 = lsrc[(row0 + 2 * CSTEP) * 8]; lg3 = lsrc[(row0 + 3 * CSTEP) * 8]; }
            }
        };
        auto gather = [&](uint4 (&x)[CB], const int4 (&id)[NI]) { score_gather<CB, BIG>(x, id, Xg, qoff); };
        auto park_lag = [&](int buf) {
            double2 *dst = lw + buf * (CB * ROW) + lane;
            if constexpr (L16) {
                dst[0] = lag16_to_double2(lh0);
                if constexpr (NL > 1) dst[64] = lag16_to_double2(lh1);
                if constexpr (NL > 2) { dst[128] = lag16_to_double2(lh2); dst[192] = lag16_to_double2(lh3); }
            } else {
                dst[0] = lg0;
                if constexpr (NL > 1) dst[64] = lg1;
                if constexpr (NL > 2) { dst[128] = lg2; dst[192] = lg3; }
            }
        };
        auto mul_cell = [&](const uint4 &x, const double2 *lr) {
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int t = 0; t < TG; ++t) score_fma<BITS, CENTER>(w, t, lr[t * 8], m[CENTER ? t : 0], acc[t]);
        };
        auto multiply = [&](const uint4 (&x)[CB], int buf) {
            const double2 *lr = lw + buf * (CB * ROW) + q;
#pragma unroll
            for (int c = 0; c < CB; ++c) mul_cell(x[c], lr + c * ROW);
        };
        // one stage for block b: `cur` holds its gathered rows; `nxt` receives block b + 1; `id_next` holds the indices
        // of block b + 1 and is refilled with those of block b + 3 (its partner holds b + 2)
        auto stage = [&](const uint4 (&cur)[CB], uint4 (&nxt)[CB], int4 (&id_next)[NI], int64_t b) {
            load_lag(b + 1);
            __builtin_amdgcn_sched_barrier(0);   // issue order matters: vmcnt retires in order
            gather(nxt, id_next);
            __builtin_amdgcn_sched_barrier(0);
            load_idx(id_next, b + 3);
            __builtin_amdgcn_sched_barrier(0);
            park_lag((int)((b + 1) & 1));        // (the compiler's s_waitcnt here leaves the loads of (2), (3) outstanding)
            multiply(cur, (int)(b & 1));
            __builtin_amdgcn_sched_barrier(0);
        };

        if (nblk > 0) {
            load_idx(ida, 0);
            load_lag(0);
            gather(xa, ida);
            load_idx(idb, 1);
            load_idx(ida, 2);
            park_lag(0);
            int64_t b = 0;
            for (; b + 2 <= nblk; b += 2) {
                stage(xa, xb, idb, b);        // idb: block b + 1 -> refilled with b + 3
                stage(xb, xa, ida, b + 1);    // ida: block b + 2 -> refilled with b + 4
            }
            if (b < nblk) stage(xa, xb, idb, b);
        }
        for (int64_t j = c0 + nblk * CB; j < c1; ++j) {   // ragged tail of the split: straight from global memory
            const uint4 x = score_row<BIG>(Xg, qoff, irow[j]);
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int t = 0; t < TG; ++t) {
                double2 l;
                if constexpr (L16) l = lag16_to_double2(lag16_g[j * ROW + t * 8 + q]);
                else l = reinterpret_cast<const double2 *>(lag_g + (int64_t)(t < tiles_left ? t : 0) * tile_elems)[j * 8 + q];
                score_fma<BITS, CENTER>(w, t, l, m[CENTER ? t : 0], acc[t]);
            }
        }
        if (p < n_perm) {
            // partial[group][split][perm][16 t + 2 q + e]
            double2 *out = reinterpret_cast<double2 *>(partial) + (((int64_t)grp * n_splits + split) * n_perm + p) * ROW + q;
#pragma unroll
            for (int t = 0; t < TG; ++t) out[t * 8] = make_double2(acc[t][0], acc[t][1]);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The same scoring with the lag rows SHARED BY THE WORKGROUP (r03).
//
// What bounds k_moran_score (r03 measurement, bench size, all three narrow widths, alone and inside the pipeline): the
// bytes a compute unit pulls through its vector memory path, ~35 GB/s per CU -- gathered rows AND lag rows alike.  There
// every wavefront fetches the lag rows of its cells for itself: 1 KB of lag per 1 KB of gathered rows for the uint8
// source (8 lag tiles per 128-gene row), i.e. HALF of a compute unit's traffic is the same lag rows arriving 16 times.
// Here a task is (gene group, cell split, 128 permutations): the workgroup's 16 wavefronts score 8 permutations each
// over the SAME cells, and the lag rows of a super-block of SB = 16 cells are loaded ONCE per workgroup -- every thread
// one 16-byte piece, a single load instruction per wavefront and super-block -- into a double-buffered LDS tile
// (2 x 16 cells x ROW pieces: 32 KB for uint8), handed over by ONE workgroup barrier per 16 cells.  Bytes through the
// compute unit per gathered row: 128 + 4 + 128 TG / 16 instead of 128 + 4 + 128 TG.  Same products, same order of
// summation per (gene, permutation): bit-identical to k_moran_score.
// A super-block = 16 / CB stages of the software pipeline of k_moran_score (gather rows(b + 1), indices(b + 3), multiply
// block b); its first stage also issues the lag load of the NEXT super-block, its last stage parks it in the other LDS
// buffer and ends with the barrier.  The pipelined region has NO branch: hipcc's wait-count pass answers a divergent
// path with s_waitcnt vmcnt(0), which would drain the gathers in flight (measured in the ISA of two earlier forms: a
// loader-wavefront `if`, and a skip for wavefronts beyond the chunk's permutations INSIDE the loop).  Hence: narrower
// sources, whose 16 cells have fewer than 1024 pieces, load some pieces twice (same bytes to the same LDS address); and a
// wavefront beyond the chunk's permutations (a chunk shorter than 128) takes a loop of its own, chosen by a
// wavefront-uniform branch OUTSIDE the pipelined loop: it only carries its pieces of the lag rows into LDS and meets the
// same barriers.  What bounds the kernel is the bytes a compute unit pulls in, so a short chunk costs about its share of a
// full one while enough wavefronts are left to keep the memory path busy; the host sends chunks with fewer than
// SCORE_WG_MIN_PERMS permutations in their last task to k_moran_score instead.
// <8, 4, false, true> (uint8 rows, 16-bit lag): the same loop with integer products (score_dot_block).  The lag words are
// parked as two byte planes, transposed so that a word holds one gene's bytes of a block's four cells: 2 x 4 KB of LDS, 32
// ds_read_b128 per wavefront and super-block instead of 128, 32 v_perm_b32 + 32 v_dot4_u32_u8 per block and lane instead of
// 200 instructions of which 128 were fp64.  Its task sums are the same doubles (bound: above score_transpose4).
// ------------------------------------------------------------------------------------------------
#define SCORE_SB 16   // cells per lag super-block
#define SCORE_WG_MIN_PERMS 24   // permutations in a chunk's last (partial) task from which the workgroup form is used

template <int BITS, int CB, bool BIG, bool L16 = false>
__global__ __launch_bounds__(SCORE_WAVES * 64) void k_moran_score_wg(
    const uint4 *__restrict__ narrow, const double *__restrict__ Lag, int64_t tile_elems, int tiles16,
    const double *__restrict__ mean, const int32_t *__restrict__ inv, double *__restrict__ partial, int64_t n,
    int64_t pstride, int n_perm, int64_t cells_per_split, int n_splits, int n_groups)
{
    static_assert((BITS == 4 || BITS == 8 || BITS == 16 || BITS == 32 || BITS == 64) && (CB == 4 || CB == 8), "source width / block size");
    // BITS == 4 (r04): 256 nibble slots per row; TG = the lane's four 16-byte pieces of uint16 operands per cell (8 slots each)
    constexpr bool NIB = BITS == 4;
    constexpr int TG = BITS == 8 ? 8 : BITS == 16 ? 4 : BITS == 32 ? 2 : NIB ? 4 : 1;
    constexpr bool CENTER = BITS == 16 || BITS == 32;
    constexpr int ROW = TG * 8;
    constexpr int NI = CB / 4;
    constexpr int SPS = SCORE_SB / CB;            // pipeline stages per super-block
    constexpr int PIECES = SCORE_SB * ROW;        // 16-byte pieces of one super-block's lag rows (<= 1024)
    static_assert(PIECES <= SCORE_WAVES * 64 && (SCORE_WAVES * 64) % PIECES == 0, "every thread loads one piece");
    // PLANES: the uint8 source on 16-bit lag rows multiplies in integers, four cells per instruction (score_dot_block)
    constexpr bool PLANES = BITS == 8 && CB == 4 && !BIG && L16;
    __shared__ double2 lds_lag[2][PLANES ? SCORE_SB / 4 * ROW : PIECES];   // [buffer][cell][ROW]; PLANES: [buffer][block][ROW]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane >> 3, q = lane & 7;
    const int pid = (int)threadIdx.x % PIECES;    // this thread's piece of every super-block
    const int lcell = pid / ROW, ltile = (pid % ROW) >> 3;
    const int pchunks = (n_perm + 8 * SCORE_WAVES - 1) / (8 * SCORE_WAVES);
    const int64_t n_tasks = (int64_t)n_groups * n_splits * pchunks;

    for (int64_t task = blockIdx.x; task < n_tasks; task += gridDim.x) {
        const int pch = (int)(task % pchunks);
        const int64_t rest = task / pchunks;
        const int split = (int)(rest % n_splits), grp = (int)(rest / n_splits);
        const int pbase = (pch * SCORE_WAVES + (BITS != 64 ? __builtin_amdgcn_readfirstlane(wave) : wave)) * 8;
        const bool live = pbase < n_perm;          // wavefront-uniform (and known to the compiler as such)
        const int p = pbase + r;
        const int pc = p < n_perm ? p : n_perm - 1;
        const int64_t c0 = (int64_t)split * cells_per_split;
        int64_t c1 = c0 + cells_per_split;
        if (c1 > n) c1 = n;
        const int32_t *irow = inv + (int64_t)pc * pstride;
        const char *Xg = reinterpret_cast<const char *>(narrow + (int64_t)grp * n * 8);
        const uint32_t qoff = (uint32_t)q * 16u;
        const int tiles_left = tiles16 - TG * grp;
        const double *lag_g = Lag + (int64_t)TG * grp * tile_elems;
        // (a padded last group re-reads its first tile for the missing ones; those sums are never used)
        // (NIB: the operand rows are [group][cell][ROW pieces] -- 512 bytes of uint16 per cell --, moved as 16-byte pieces like lag tiles)
        const double2 *lsrc = NIB ? reinterpret_cast<const double2 *>(Lag) + (int64_t)grp * n * ROW + (pid % ROW)
                                  : reinterpret_cast<const double2 *>(lag_g + (int64_t)(ltile < tiles_left ? ltile : 0) * tile_elems) + (pid & 7);
        constexpr int LSTRIDE = NIB ? ROW : 8;      // pieces from one cell's row to the next
        const uint32_t *lag16_g = reinterpret_cast<const uint32_t *>(Lag) + (int64_t)grp * n * ROW;   // L16: [cell][ROW] words
        const uint32_t *lsrc16 = lag16_g + (pid % ROW);
        double m[CENTER ? TG : 1][2], acc[TG][2];
#pragma unroll
        for (int t = 0; t < TG; ++t) {
            if constexpr (CENTER) {
                const double *mt = mean + (int64_t)(TG * grp + (t < tiles_left ? t : 0)) * SC_TILE + 2 * q;
                m[t][0] = mt[0]; m[t][1] = mt[1];
            }
            acc[t][0] = acc[t][1] = 0.0;
        }
        uint32_t ai[NIB ? 32 : 1];   // NIB: integer sums of the lane's 32 slots
#pragma unroll
        for (int k2 = 0; k2 < (NIB ? 32 : 1); ++k2) ai[k2] = 0u;
        uint32_t plo[PLANES ? 16 : 1], phi[PLANES ? 16 : 1];   // PLANES: plane sums of the lane's 16 genes (score_dot_block)
#pragma unroll
        for (int k2 = 0; k2 < (PLANES ? 16 : 1); ++k2) plo[k2] = phi[k2] = 0u;
        const int64_t nsb = (c1 - c0) / SCORE_SB;   // whole super-blocks of the split (the rest: tail loop below)
        const int64_t nblk = nsb * SPS;

        double2 lg;
        uint32_t lh = 0;   // L16: the thread's piece as a pair of 16-bit sums
        uint4 xa[CB], xb[CB];
        auto park = [&](int buf) {
            if constexpr (PLANES) {
                // the image score_dot_block reads: this thread's word is (cell lcell, tile, q) = {lo, hi, lo, hi} of two genes;
                // its bytes go to byte lcell % 4 of the four words of piece [block lcell / 4][tile][q].  The eight pieces one
                // ds_read_b128 fetches (q = 0 .. 7, each broadcast to the 8 permutations) are contiguous: no bank conflict.
                unsigned char *dst = reinterpret_cast<unsigned char *>(&lds_lag[buf][(lcell >> 2) * ROW + (pid % ROW)]) + (lcell & 3);
                dst[0] = (unsigned char)lh; dst[4] = (unsigned char)(lh >> 8);
                dst[8] = (unsigned char)(lh >> 16); dst[12] = (unsigned char)(lh >> 24);
            } else
            if constexpr (L16) lds_lag[buf][pid] = lag16_to_double2(lh);
            else lds_lag[buf][pid] = lg;
        };

        auto load_idx = [&](int4 (&id)[NI], int64_t b) { score_load_idx<CB>(id, irow, c0, b, nblk); };
        auto load_lag = [&](int64_t sb) {
            const int64_t ss = sb < nsb ? sb : nsb - 1;
            if constexpr (L16) lh = lsrc16[(c0 + ss * SCORE_SB + lcell) * ROW];
            else lg = lsrc[(c0 + ss * SCORE_SB + lcell) * LSTRIDE];
        };
        auto gather = [&](uint4 (&x)[CB], const int4 (&id)[NI]) { score_gather<CB, BIG>(x, id, Xg, qoff); };
        auto mul_cell = [&](const uint4 &x, const double2 *lr) {
            const uint32_t w[4] = {x.x, x.y, x.z, x.w};
            if constexpr (NIB) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const uint4 sp = *reinterpret_cast<const uint4 *>(&lr[t * 8]);   // the 8 uint16 operands of slots 64 t + 8 q + e
                    const uint32_t sw[4] = {sp.x, sp.y, sp.z, sp.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        ai[t * 8 + e] += __umul24((w[t] >> (4 * e)) & 15u, (sw[e >> 1] >> (16 * (e & 1))) & 0xffffu);
                }
                return;
            }
#pragma unroll
            for (int t = 0; t < TG; ++t) score_fma<BITS, CENTER>(w, t, lr[t * 8], m[CENTER ? t : 0], acc[t]);
        };
        // one stage for block b = sb * SPS + k: `cur` holds its gathered rows; `nxt` receives block b + 1; `id_next` holds
        // the indices of block b + 1 and is refilled with those of block b + 1 + SPS, i.e. every index vector is consumed in
        // the NEXT trip of the super-block loop (consumed in the same trip, hipcc sinks the load down to its use -- seen in
        // the IR -- and the gather then waits vmcnt(0) for it)
        auto stage = [&](const uint4 (&cur)[CB], uint4 (&nxt)[CB], int4 (&id_next)[NI], int64_t sb, int k) {
            if (k == 0) load_lag(sb + 1);            // (k is a literal at every call site)
            __builtin_amdgcn_sched_barrier(0);       // issue order matters: vmcnt retires in order
            gather(nxt, id_next);
            __builtin_amdgcn_sched_barrier(0);
            load_idx(id_next, sb * SPS + k + 1 + SPS);
            __builtin_amdgcn_sched_barrier(0);
            const double2 *lr = &lds_lag[sb & 1][(PLANES ? k * ROW : k * CB * ROW) + q];
            if constexpr (PLANES) score_dot_block(cur, reinterpret_cast<const uint4 *>(lr), plo, phi);
#pragma unroll
            for (int c = 0; c < (PLANES ? 0 : CB); ++c) {
                mul_cell(cur[c], lr + c * ROW);
                if constexpr (NIB) __builtin_amdgcn_sched_barrier(0);   // (one cell's operand pieces at a time: hoisted together they spill)
            }
            __builtin_amdgcn_sched_barrier(0);
            if (k == SPS - 1) {
                park((int)((sb + 1) & 1));           // (that buffer was last read in super-block sb - 1, before its barrier)
                __syncthreads();
            }
        };

        if (BITS != 64 && nsb > 0 && !live) {
            // (the fp64-row form has no registers to spare for a second loop: its idle wavefronts score their clamped
            // permutation again, and the host keeps short chunks away from it)
            // a wavefront beyond the chunk's permutations only carries its pieces of the lag rows into LDS: the same
            // barriers as the scoring loop below, no gathers (the branch is wavefront-uniform and OUTSIDE that loop)
            load_lag(0);
            park(0);
            __syncthreads();
            for (int64_t sb = 0; sb < nsb; ++sb) {
                load_lag(sb + 1);
                park((int)((sb + 1) & 1));
                __syncthreads();
            }
        } else if (nsb > 0) {
            int4 id0[NI], id1[NI], id2[NI], id3[NI];   // indices of blocks b + 1 .. b + SPS at the top of a trip (id0 .. id1 when SPS == 2)
            load_lag(0);
            load_idx(id3, 0);
            gather(xa, id3);
            load_idx(id0, 1);
            load_idx(id1, 2);
            if constexpr (SPS == 4) { load_idx(id2, 3); load_idx(id3, 4); }
            park(0);
            __syncthreads();
            for (int64_t sb = 0; sb < nsb; ++sb) {
                stage(xa, xb, id0, sb, 0);
                stage(xb, xa, id1, sb, 1);
                if constexpr (SPS == 4) {
                    stage(xa, xb, id2, sb, 2);
                    stage(xb, xa, id3, sb, 3);
                }
            }
        }
        if (live) {
            if constexpr (PLANES) {
                // ragged tail of the split (< 16 cells) in plain integers (one cell per trip: vectorised by two, hipcc keeps a second
                // set of the 32 sums and spills)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
                for (int64_t j = c0 + nsb * SCORE_SB; j < c1; ++j) {
                    const uint4 x = score_row<BIG>(Xg, qoff, irow[j]);
                    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                    for (int t = 0; t < TG; ++t) {
                        const uint32_t s = lag16_g[j * ROW + t * 8 + q], h = w[t >> 1] >> (16 * (t & 1));
                        const uint32_t x0 = h & 0xffu, x1 = (h >> 8) & 0xffu;
                        plo[2 * t] += __umul24(x0, s & 0xffu); phi[2 * t] += __umul24(x0, (s >> 8) & 0xffu);
                        plo[2 * t + 1] += __umul24(x1, (s >> 16) & 0xffu); phi[2 * t + 1] += __umul24(x1, s >> 24);
                    }
                }
            } else
            for (int64_t j = c0 + nsb * SCORE_SB; j < c1; ++j) {   // ragged tail of the split (< 16 cells): straight from global memory
                const uint4 x = score_row<BIG>(Xg, qoff, irow[j]);
                const uint32_t w[4] = {x.x, x.y, x.z, x.w};
                if constexpr (NIB) {
                    const uint4 *srow = reinterpret_cast<const uint4 *>(Lag) + ((int64_t)grp * n + j) * ROW + q;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const uint4 sp = srow[t * 8];
                        const uint32_t sw[4] = {sp.x, sp.y, sp.z, sp.w};
#pragma unroll
                        for (int e = 0; e < 8; ++e)
                            ai[t * 8 + e] += __umul24((w[t] >> (4 * e)) & 15u, (sw[e >> 1] >> (16 * (e & 1))) & 0xffffu);
                    }
                    continue;
                }
#pragma unroll
                for (int t = 0; t < TG; ++t) {
                    double2 l;
                    if constexpr (L16) l = lag16_to_double2(lag16_g[j * ROW + t * 8 + q]);
                    else l = reinterpret_cast<const double2 *>(lag_g + (int64_t)(t < tiles_left ? t : 0) * tile_elems)[j * 8 + q];
                    score_fma<BITS, CENTER>(w, t, l, m[CENTER ? t : 0], acc[t]);
                }
            }
            if (p < n_perm) {
                if constexpr (NIB) {   // partial[group][split][perm][slot 64 t + 8 q + e]
                    double2 *out = reinterpret_cast<double2 *>(partial + ((((int64_t)grp * n_splits + split) * n_perm + p) * 256 + q * 8));
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int e2 = 0; e2 < 4; ++e2)
                            out[t * 32 + e2] = make_double2((double)ai[t * 8 + 2 * e2], (double)ai[t * 8 + 2 * e2 + 1]);
                } else {
                // partial[group][split][perm][16 t + 2 q + e]
                double2 *out = reinterpret_cast<double2 *>(partial) + (((int64_t)grp * n_splits + split) * n_perm + p) * ROW + q;
#pragma unroll
                for (int t = 0; t < TG; ++t) {
                    if constexpr (PLANES) out[t * 8] = make_double2((double)plo[2 * t] + 256.0 * (double)phi[2 * t],
                                                                    (double)plo[2 * t + 1] + 256.0 * (double)phi[2 * t + 1]);
                    else out[t * 8] = make_double2(acc[t][0], acc[t][1]);
                }
                }
            }
        }
    }
}

// sims[p0 + p][GP grp + slot] = seff * (sum_s partial[grp][s][p][slot] - corr) (ascending s), raw = the sum itself, for
// every gene group of a chunk in one launch (GP = genes per group: 128 / 64 / 32 / 16 by source width); seff, corr:
// k_moran_scale
template <int GP>
__global__ __launch_bounds__(256) void k_moran_finalize_groups(const double *__restrict__ partial,
                                                               const double *__restrict__ seff,
                                                               const double *__restrict__ corr,
                                                               double *__restrict__ sims, double *__restrict__ raw, int n_perm,
                                                               int splits, int64_t n_genes, int64_t p0)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int p = t / GP, slot = t % GP;
    const int64_t g = GP * (int64_t)blockIdx.y + slot;
    if (p >= n_perm || g >= n_genes) return;
    const double *pt = partial + (int64_t)blockIdx.y * splits * n_perm * GP;
    double s = 0.0;
    for (int k = 0; k < splits; ++k) s += pt[((int64_t)k * n_perm + p) * GP + slot];
    raw[(p0 + p) * n_genes + g] = s;
    sims[(p0 + p) * n_genes + g] = seff[g] * (s - corr[g]);
}

// cell range of one scoring task: a function of n ALONE (results must not depend on the chunking of the
// permutations or on the source width): >= 2048 cells, a multiple of 8, at most 512 splits
static int64_t score_cells_per_split(int64_t n)
{
    int64_t cps = align_up64(ceil_div64(n, 512), 8);
    return cps < 2048 ? 2048 : cps;
}

static int pick_splits(int64_t n, int n_perm_tiles, int64_t *cells_per_split)
{
    // aim for >= 2048 workgroups per launch (256 CUs x 8 resident), splits <= 256,
    // and a cell range that is a multiple of 8 and not shorter than 2048 cells
    int64_t want = ceil_div64(2048, n_perm_tiles > 0 ? n_perm_tiles : 1);
    if (want < 1) want = 1;
    if (want > 256) want = 256;
    int64_t cps = align_up64(ceil_div64(n, want), 8);
    if (cps < 2048) cps = 2048;
    *cells_per_split = cps;
    return (int)ceil_div64(n, cps);
}

static int moran_check(sc_ctx *c, int64_t n_perm, const double *I_out)
{
    SC_REQUIRE(c && I_out, SC_ERR_INVALID, "sc_moran: null pointer");
    SC_REQUIRE(n_perm >= 0 && n_perm <= (1 << 24), SC_ERR_INVALID, "sc_moran: n_perm=%lld out of range",
               (long long)n_perm);
    SC_HIP(hipSetDevice(c->device));
    SC_REQUIRE(c->e_n > 0, SC_ERR_STATE, "sc_moran: no expression loaded");
    SC_REQUIRE(c->g_n > 0, SC_ERR_STATE, "sc_moran: no graph set");
    SC_REQUIRE(c->g_n == c->e_n, SC_ERR_INVALID, "sc_moran: graph has %lld rows but expression has %lld cells",
               (long long)c->g_n, (long long)c->e_n);
    return SC_OK;
}

// The same lag from the float32 narrow rows (r04): a float32-source batch has its raw values as 32 genes per 128-byte row
// (k_pack_narrow<32>: the lane's 16 bytes = genes {16 t + 2 q, + 1} of the group's two tiles), so a neighbour costs one
// 16-byte piece per lane for FOUR genes instead of one per tile for two -- half the gathered bytes (what bounds k_lag is
// the rows through the CUs' vector memory path, section 4.2 of DESIGN.md).  z = (double)x - centre is rebuilt in
// registers, the very value the Z tile holds; products and sums rounded separately, edges in ascending order: Lag is
// k_lag's bit for bit.
__global__ __launch_bounds__(256) void k_lag_f32rows(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                     const double *__restrict__ w, const uint4 *__restrict__ narrow,
                                                     const double *__restrict__ centre, double *__restrict__ Lag, int64_t n,
                                                     int tiles16, const double *__restrict__ unit,
                                                     const int32_t *__restrict__ order)
{
    const int64_t per_xcd = (int64_t)(gridDim.x >> 3);                 // gridDim.x is a multiple of 8
    const int64_t blk = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
    const int64_t t = blk * blockDim.x + threadIdx.x;
    const int64_t pos = t >> 3;
    const int q = (int)(t & 7);
    if (pos >= n) return;
    const int64_t i = order ? order[pos] : pos;
    const int grp = blockIdx.y;                                        // 32 genes = tiles 2 grp, 2 grp + 1
    const int tiles_left = tiles16 - 2 * grp;
    const uint4 *Xg = narrow + (int64_t)grp * n * 8;
    double cen[4];
    bool un[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t g = (int64_t)(2 * grp + ((k >> 1) < tiles_left ? (k >> 1) : 0)) * SC_TILE + 2 * q + (k & 1);
        cen[k] = centre[g];
        un[k] = unit && unit[g] != 0.0;
    }
    const int64_t e0 = indptr[i], e1 = indptr[i + 1];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t e = e0; e < e1; ++e) {
        const uint4 v = Xg[(int64_t)indices[e] * 8 + q];
        const double ww = w[e];
        const double z[4] = {(double)__uint_as_float(v.x) - cen[0], (double)__uint_as_float(v.y) - cen[1],
                             (double)__uint_as_float(v.z) - cen[2], (double)__uint_as_float(v.w) - cen[3]};
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = __dadd_rn(s[k], __dmul_rn(un[k] ? 1.0 : ww, z[k]));
    }
    reinterpret_cast<double2 *>(Lag + (int64_t)(2 * grp) * n * SC_TILE)[i * 8 + q] = make_double2(s[0], s[1]);
    if (tiles_left > 1) reinterpret_cast<double2 *>(Lag + (int64_t)(2 * grp + 1) * n * SC_TILE)[i * 8 + q] = make_double2(s[2], s[3]);
}

// ------------------------------------------------------------------------------------------------
// The prelude of an all-lattice uint8 batch in one pass (r03).  For count data on a kNN graph the streamed operand of
// the scoring kernel is S = A x, the unweighted neighbour sums of the raw counts.  k_lag makes them from fp64 tiles: 15
// neighbours x 8 lanes x 16 B per cell and 16-gene tile = 61 GB through the CUs' texture path at bench size, 11.8 ms in
// the scoring's serial prelude.  The uint8 rows the scoring kernel gathers hold 128 genes per 128 bytes: summing THOSE is
// an eighth of the gathered bytes, the sums fit 16 bits (degree <= 257), and the two column sums the observed statistic
// needs (T_obs = sum_i x_i S_i, sum_i S_i: integers, exact in fp64 in any order) fall out of the same pass.  Cells are
// walked in the graph's processing order, one XCD per contiguous eighth.  Lag gets the same fp64 values k_lag writes
// for lattice genes (integers), so everything downstream is bit-identical.
// ------------------------------------------------------------------------------------------------
#define LAG8_CELLS_PER_BLOCK 4096

__global__ __launch_bounds__(256) void k_lag_u8(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                const uint4 *__restrict__ narrow, const int32_t *__restrict__ order, int64_t n,
                                                int tiles16, int64_t tile_elems, double *__restrict__ Lag,
                                                uint32_t *__restrict__ Lag16 /* non-null: the sums as 16-bit pairs instead */,
                                                double *__restrict__ partial /* [2][tile][chunk][16] */, int chunks)
{
    __shared__ double shT[128], shS[128];      // [tile of the group][slot]
    const int grp = blockIdx.y;
    const int64_t per_xcd = (int64_t)(gridDim.x >> 3);
    const int64_t chunk = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);   // gridDim.x is a multiple of 8
    const int q = threadIdx.x & 7, row = threadIdx.x >> 3;
    if (threadIdx.x < 128) { shT[threadIdx.x] = 0.0; shS[threadIdx.x] = 0.0; }
    __syncthreads();
    const uint4 *Xg = narrow + (int64_t)grp * n * 8;
    const int tiles_left = tiles16 - 8 * grp;
    double accT[16], accS[16];
#pragma unroll
    for (int b = 0; b < 16; ++b) accT[b] = accS[b] = 0.0;
    const int64_t p0 = chunk * LAG8_CELLS_PER_BLOCK;
    if (chunk < chunks) {
        for (int it = 0; it < LAG8_CELLS_PER_BLOCK / 32; ++it) {
            const int64_t pos = p0 + it * 32 + row;
            if (pos >= n) break;
            const int64_t cell = order ? order[pos] : pos;
            const uint4 own = Xg[cell * 8 + q];
            uint32_t lo[4] = {0u, 0u, 0u, 0u}, hi[4] = {0u, 0u, 0u, 0u};   // packed 16-bit sums of the even / odd bytes
            for (long long e = indptr[cell]; e < indptr[cell + 1]; ++e) {
                const uint4 v = Xg[(int64_t)indices[e] * 8 + q];
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) { lo[k] += w[k] & 0x00ff00ffu; hi[k] += (w[k] >> 8) & 0x00ff00ffu; }
            }
            const uint32_t xo[4] = {own.x, own.y, own.z, own.w};
            // byte b = 2 t + e of the lane's 16 bytes is gene 16 t + 2 q + e of the group: word t >> 1, byte 2 (t & 1) + e
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int k = t >> 1, sh = 16 * (t & 1);
                const double s0 = (double)((lo[k] >> sh) & 0xffffu), s1 = (double)((hi[k] >> sh) & 0xffffu);
                const double x0 = (double)((xo[k] >> sh) & 0xffu), x1 = (double)((xo[k] >> (sh + 8)) & 0xffu);
                if (Lag16) Lag16[((int64_t)grp * n + cell) * 64 + t * 8 + q] = ((lo[k] >> sh) & 0xffffu) | (((hi[k] >> sh) & 0xffffu) << 16);
                else if (t < tiles_left)
                    reinterpret_cast<double2 *>(Lag + (int64_t)(8 * grp + t) * tile_elems)[cell * 8 + q] = make_double2(s0, s1);
                accS[2 * t] += s0; accS[2 * t + 1] += s1;
                accT[2 * t] = fma(x0, s0, accT[2 * t]); accT[2 * t + 1] = fma(x1, s1, accT[2 * t + 1]);
            }
        }
    }
    // integers below 2^53: the order of these additions does not matter
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            atomicAdd(&shT[t * 16 + 2 * q + e], accT[2 * t + e]);
            atomicAdd(&shS[t * 16 + 2 * q + e], accS[2 * t + e]);
        }
    __syncthreads();
    if (threadIdx.x < 128 && chunk < chunks) {
        const int t = threadIdx.x >> 4, slot = threadIdx.x & 15;
        if (t < tiles_left) {
            const int64_t tile = 8 * grp + t;
            partial[((int64_t)tile * chunks + chunk) * SC_TILE + slot] = shT[threadIdx.x];
            partial[((int64_t)(tiles16 + tile) * chunks + chunk) * SC_TILE + slot] = shS[threadIdx.x];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// r04: the 4-BIT source.  Count data is mostly small counts: a gene whose largest count is below 16 needs a nibble per
// cell, and a gene with counts up to 255 is the sum of two such pseudo-genes, x = lo + 16 hi, whose statistics add exactly
// (integer lattice: T = sum_j S_j x[inv(j)] = T_lo + 16 T_hi).  256 nibble SLOTS fit the 128-byte row the scoring kernel
// gathers per (permutation, cell): slot s < G is the low nibble of gene s, slots G .. G + nw - 1 the high nibbles of the nw
// genes that have one.  Used when that takes FEWER rows than 128 genes per uint8 row (the bench's 500 genes, 75 of them
// with a count >= 16: 575 slots = 3 rows instead of 4 -- a quarter of the gathered bytes, which is what bounds the kernel).
// Row layout: lane q of the 8 that share a row holds, in word t (0 .. 3) nibble e (0 .. 7), slot 64 t + 8 q + e; the
// streamed operand is S (neighbour sums of the FULL gene, for both of its slots) as uint16 in slot order (512 bytes per
// cell and group), so the lane's operands are again 16-byte LDS pieces (t, q) that are contiguous across q; products
// (< 2^20) are added in int32 per task (15 x largest S x cells of a split < 2^31: checked on the host), then as doubles.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pack_nib(const double *__restrict__ X, uint4 *__restrict__ out, int64_t n, int64_t G,
                                                  int64_t NS, const int32_t *__restrict__ wide)
{
    const int64_t tt = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // (cell, q)
    if (tt >= n * 8) return;
    const int64_t cell = tt >> 3;
    const int q = (int)(tt & 7), grp = blockIdx.y;
    uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int64_t s0 = (int64_t)grp * 256 + t * 64 + q * 8;
        if (s0 >= NS) continue;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int64_t s = s0 + e;
            if (s >= NS) break;
            const int64_t g = s < G ? s : (int64_t)wide[s - G];
            const double x = X[(g >> 4) * n * SC_TILE + cell * SC_TILE + (g & 15)];
            const uint32_t v = (uint32_t)(x >= 0.0 && x <= 255.0 ? x : 0.0);
            o[t] |= (s < G ? (v & 15u) : (v >> 4)) << (4 * e);
        }
    }
    out[((int64_t)grp * n + cell) * 8 + q] = make_uint4(o[0], o[1], o[2], o[3]);
}

// neighbour sums of every slot (uint16, slot order), cells in the graph's processing order like k_lag_u8
__global__ __launch_bounds__(256) void k_lag_nib(const long long *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                 const uint4 *__restrict__ nib, const int32_t *__restrict__ order, int64_t n,
                                                 uint4 *__restrict__ S16, int chunks)
{
    const int grp = blockIdx.y;
    const int64_t per_xcd = (int64_t)(gridDim.x >> 3);
    const int64_t chunk = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);   // gridDim.x is a multiple of 8
    if (chunk >= chunks) return;
    const int q = threadIdx.x & 7, row = threadIdx.x >> 3;
    const uint4 *Xg = nib + (int64_t)grp * n * 8;
    const int64_t p0 = chunk * LAG8_CELLS_PER_BLOCK;
    for (int it = 0; it < LAG8_CELLS_PER_BLOCK / 32; ++it) {
        const int64_t pos = p0 + it * 32 + row;
        if (pos >= n) break;
        const int64_t cell = order ? order[pos] : pos;
        uint32_t acc[4][4];   // [word t][pair k]: 16-bit sums of nibbles e = 2 k (low half) and 2 k + 1 (high half)
        uint32_t ev[4] = {0u, 0u, 0u, 0u}, od[4] = {0u, 0u, 0u, 0u};   // byte sums of the even / odd nibbles (<= 16 neighbours x 15)
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[t][k] = 0u;
        int pending = 0;
        auto flush = [&]() {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[t][k] += ((ev[t] >> (8 * k)) & 0xffu) | (((od[t] >> (8 * k)) & 0xffu) << 16);
                ev[t] = od[t] = 0u;
            }
            pending = 0;
        };
        for (long long e = indptr[cell]; e < indptr[cell + 1]; ++e) {
            const uint4 v = Xg[(int64_t)indices[e] * 8 + q];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) { ev[t] += w[t] & 0x0f0f0f0fu; od[t] += (w[t] >> 4) & 0x0f0f0f0fu; }
            if (++pending == 16) flush();
        }
        flush();
        uint4 *dst = S16 + ((int64_t)grp * n + cell) * 32 + q;
#pragma unroll
        for (int t = 0; t < 4; ++t) dst[t * 8] = make_uint4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    }
}

// S of a gene with a high nibble = S_lo + 16 S_hi, for BOTH of its slots
__global__ __launch_bounds__(256) void k_nib_fixup(uint16_t *__restrict__ S16, int64_t n, int64_t G, int nw,
                                                   const int32_t *__restrict__ wide)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * nw) return;
    const int64_t cell = t / nw;
    const int j = (int)(t - cell * nw);
    const int64_t sl = wide[j], sh = G + j;
    uint16_t *a = S16 + ((sl >> 8) * n + cell) * 256 + (sl & 255), *b = S16 + ((sh >> 8) * n + cell) * 256 + (sh & 255);
    const uint32_t s = (uint32_t)*a + 16u * (uint32_t)*b;
    *a = (uint16_t)s;
    *b = (uint16_t)s;
}

// per slot and chunk of cells: sum nibble x S and sum S (integers, exact in fp64)
__global__ __launch_bounds__(256) void k_nib_colsum(const uint8_t *__restrict__ nib, const uint16_t *__restrict__ S16, int64_t n,
                                                    double *__restrict__ partT, double *__restrict__ partS, int chunks)
{
    const int grp = blockIdx.y, chunk = blockIdx.x, s = threadIdx.x;
    const int q = (s & 63) >> 3, t = s >> 6, e = s & 7;
    const int64_t c0 = (int64_t)chunk * LAG8_CELLS_PER_BLOCK, c1 = c0 + LAG8_CELLS_PER_BLOCK < n ? c0 + LAG8_CELLS_PER_BLOCK : n;
    unsigned long long T = 0, SS = 0;
    for (int64_t cell = c0; cell < c1; ++cell) {
        const uint32_t S = S16[((int64_t)grp * n + cell) * 256 + s];
        const uint32_t by = nib[((int64_t)grp * n + cell) * 128 + q * 16 + t * 4 + (e >> 1)];
        const uint32_t v = (e & 1) ? (by >> 4) : (by & 15u);
        T += (unsigned long long)v * S;
        SS += S;
    }
    partT[((int64_t)grp * chunks + chunk) * 256 + s] = (double)T;
    partS[((int64_t)grp * chunks + chunk) * 256 + s] = (double)SS;
}

// per gene: T_obs = sum x S = T[lo] + 16 T[hi], sum S (chunks in order)
__global__ void k_nib_colsum_final(const double *__restrict__ partT, const double *__restrict__ partS, int chunks, int64_t G,
                                   const int32_t *__restrict__ hi_slot, double *__restrict__ inum, double *__restrict__ slag)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    const int64_t sh = hi_slot[g];
    double T = 0.0, Th = 0.0, S = 0.0;
    for (int c = 0; c < chunks; ++c) {
        T += partT[((g >> 8) * chunks + c) * 256 + (g & 255)];
        S += partS[((g >> 8) * chunks + c) * 256 + (g & 255)];
        if (sh >= 0) Th += partT[((sh >> 8) * chunks + c) * 256 + (sh & 255)];
    }
    inum[g] = T + 16.0 * Th;
    slag[g] = S;
}

// sims / raw of the nibble form: the sums of a gene's slot(s) over the splits (ascending), T = T[lo] + 16 T[hi]
__global__ __launch_bounds__(256) void k_moran_finalize_nib(const double *__restrict__ partial, const double *__restrict__ seff,
                                                            const double *__restrict__ corr, const int32_t *__restrict__ hi_slot,
                                                            double *__restrict__ sims, double *__restrict__ raw, int n_perm,
                                                            int splits, int64_t n_genes, int64_t p0)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t p = t / n_genes, g = t - p * n_genes;
    if (p >= n_perm) return;
    const int64_t sh = hi_slot[g];
    double lo = 0.0, hi = 0.0;
    for (int k = 0; k < splits; ++k) {
        lo += partial[((((g >> 8) * splits + k) * n_perm) + p) * 256 + (g & 255)];
        if (sh >= 0) hi += partial[((((sh >> 8) * splits + k) * n_perm) + p) * 256 + (sh & 255)];
    }
    const double s = lo + 16.0 * hi;
    raw[(p0 + p) * n_genes + g] = s;
    sims[(p0 + p) * n_genes + g] = seff[g] * (s - corr[g]);
}

// ---- the ring of partial-sum slices (MoranRing, sc_ctx.h) ----
// Nothing reads sims before k_moran_count at the end of the job, so a chunk's finalise need not sit between two scoring
// launches on the context stream (bench size: eleven finalise launches of 0.2-1.25 ms, each re-reading up to 256 MB while
// the scoring's CUs wait, and a launch boundary more each).  With one slice per launch in flight the finalise runs on the
// side stream beside the NEXT scoring launch.  Its kernels and their order of summation are unchanged: every output is
// bit-identical to the in-line form.  What the step gains (it is bound by the generator until its last chunks, so only
// the launches behind those count): DESIGN.md sections 4.3 and 5.

// a new job: R slices of `slice` doubles, no launch yet
static int moran_ring_begin(sc_ctx *c, size_t slice)
{
    MoranRing &r = c->ring;
    SC_TRY(c->streams.ensure(SR_FINALISE));
    // (a job that ended in an error may have left finalise launches behind: they read what this job's set-up rewrites)
    if (r.launches > 0) SC_HIP(hipStreamSynchronize(c->stream_out));
    for (int k = 0; k < MORAN_RING; ++k) {
        if (!r.scored[k]) SC_HIP(hipEventCreateWithFlags(&r.scored[k], hipEventDisableTiming));
        if (!r.done[k]) SC_HIP(hipEventCreateWithFlags(&r.done[k], hipEventDisableTiming));
    }
    SC_TRY(c->partial.ensure(sizeof(double) * slice * MORAN_RING, &c->mem));
    r.slice = slice;
    r.launches = 0;
    return SC_OK;
}

// the slice of the job's next scoring launch; the context stream waits for the finalise that read it MORAN_RING
// launches ago (long done in practice: the finalise takes a tenth of a scoring launch)
static int moran_ring_slice(sc_ctx *c, double **slice)
{
    MoranRing &r = c->ring;
    const int k = (int)(r.launches % MORAN_RING);
    if (r.launches >= MORAN_RING) SC_HIP(hipStreamWaitEvent(c->stream, r.done[k], 0));
    *slice = c->partial.as<double>() + (size_t)k * r.slice;
    return SC_OK;
}

// behind the scoring launch: the side stream, ready for that launch's finalise
static int moran_ring_scored(sc_ctx *c)
{
    MoranRing &r = c->ring;
    const int k = (int)(r.launches % MORAN_RING);
    SC_HIP(hipEventRecord(r.scored[k], c->stream));
    SC_HIP(hipStreamWaitEvent(c->stream_out, r.scored[k], 0));
    return SC_OK;
}

// behind the finalise launch
static int moran_ring_finalised(sc_ctx *c)
{
    MoranRing &r = c->ring;
    SC_HIP(hipGetLastError());
    SC_HIP(hipEventRecord(r.done[r.launches % MORAN_RING], c->stream_out));
    r.launches += 1;
    return SC_OK;
}

// the context stream waits for every finalise of the job (the side stream runs them in order)
static int moran_ring_join(sc_ctx *c)
{
    MoranRing &r = c->ring;
    if (r.launches > 0) SC_HIP(hipStreamWaitEvent(c->stream, r.done[(r.launches - 1) % MORAN_RING], 0));
    return SC_OK;
}

// Everything the permutation kernels need, from the loaded tiles and the active graph:
//   value class + lattice decision per gene (one pass + one host sync), Z = X - centre, Lag = W Z (lattice genes: the
//   unweighted neighbour sums of the raw counts), I, the per-gene finalisation constants, the narrow copy of the batch.
// allow_lattice = false: ordinary arithmetic for every gene (tables that are not permutations: the identity
// sum_j x[idx[j]] = sum_j x[j] behind the lattice form does not hold for them).
// First half of moran_prepare: everything that needs neither a decision of the host nor the permutation count -- the
// weight sum, the graph moments (side stream), the gene moments and value classes -- is enqueued, with its small results
// on their way into pinned host memory, and nothing is waited for.  (r03 measured this half ENQUEUED AHEAD of the
// generator's launches for a resident expression -- the generator takes the host ~10 ms to enqueue -- : scoring started
// at 19 ms instead of 31, but the generator's own first launches queued behind these full-chip kernels, its chain
// started 4.5 ms later, and the step, which ends with the generator, was 1-2 ms LONGER.  Not kept; the split stays.)
static int moran_prepare_early(sc_ctx *c)
{
    const int64_t n = c->e_n, T = c->e_tiles;
    const int64_t Gpad = align_up64(T, 8) * SC_TILE;
    SC_REQUIRE(n > 0 && c->g_n == n, SC_ERR_STATE, "internal: early preparation without expression and graph");
    const bool need_s0 = !(c->s0_valid || c->s0_only_valid);
    const int blocks = need_s0 ? sc_graph_weight_sum_blocks(c) : 0;
    const size_t bytes = sizeof(double) * ((size_t)blocks + (size_t)(T * SC_TILE)) + sizeof(uint32_t) * 2 * (size_t)Gpad;
    if (bytes > c->prep_host_cap) {
        SC_HIP(hipStreamSynchronize(c->stream));   // (copies of an earlier, abandoned first half may still be writing the old buffer)
        if (c->prep_host) (void)hipHostFree(c->prep_host);
        c->prep_host = nullptr; c->prep_host_cap = 0;
        SC_HIP(hipHostMalloc(&c->prep_host, bytes, hipHostMallocDefault));
        c->prep_host_cap = bytes;
    }
    double *h_s0 = reinterpret_cast<double *>(c->prep_host), *h_xsum = h_s0 + blocks;
    uint32_t *h_flags = reinterpret_cast<uint32_t *>(h_xsum + T * SC_TILE), *h_xmax = h_flags + Gpad;
    c->prep_s0_blocks = blocks;
    if (need_s0) SC_TRY(sc_graph_weight_sum_launch(c, h_s0));
    SC_TRY(sc_graph_moments_begin(c));   // s1, s2 (p_norm, z-scores): on the side stream, out of this serial prelude
    SC_TRY(expr_moments(c));
    SC_TRY(expr_gene_stats(c));   // value classes
    SC_HIP(hipMemcpyAsync(h_flags, c->g_flags.p, sizeof(uint32_t) * (size_t)Gpad, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipMemcpyAsync(h_xmax, c->g_xmax.p, sizeof(uint32_t) * (size_t)Gpad, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipMemcpyAsync(h_xsum, c->g_xsum.p, sizeof(double) * (size_t)(T * SC_TILE), hipMemcpyDeviceToHost, c->stream));
    c->prep_early = true;
    return SC_OK;
}

static int moran_prepare(sc_ctx *c, int64_t n_perm, bool allow_lattice)
{
    const int64_t n = c->e_n, T = c->e_tiles, G = c->e_genes;
    const int64_t Tpad = align_up64(T, 8), Gpad = Tpad * SC_TILE;
    if (!c->prep_early) SC_TRY(moran_prepare_early(c));
    c->prep_early = false;
    SC_HIP(hipStreamSynchronize(c->stream));   // the ONE synchronisation of the preparation
    const double *h_s0 = reinterpret_cast<const double *>(c->prep_host), *xsum = h_s0 + c->prep_s0_blocks;
    const uint32_t *flags = reinterpret_cast<const uint32_t *>(xsum + T * SC_TILE), *xmax = flags + Gpad;
    if (c->prep_s0_blocks > 0) sc_graph_weight_sum_collect(c, h_s0, c->prep_s0_blocks);
    std::vector<double> lat((size_t)Gpad, 0.0);
    int bits = c->source_bits_min;
    bool lat_any = false, lat_all = true;
    // equal weights AND equal degrees: sum_i z_i lag[pi(i)] = w (T - mean sum S) drops the term -w mean sum_i z_i deg[pi(i)],
    // which vanishes only when deg is constant (r03 advisor finding: a binary adjacency with unequal rows took this path)
    const bool lattice_graph = allow_lattice && c->g_uniform_w > 0.0 && c->g_regular;
    for (int64_t g = 0; g < G; ++g) {
        const int cls = !(flags[(size_t)g] & 1u) ? 8 : !(flags[(size_t)g] & 2u) ? 16 : !(flags[(size_t)g] & 4u) ? 32 : 64;
        if (cls > bits) bits = cls;
        // every partial sum of T_p = sum_j S_j x[inv_p(j)] stays an integer below 2^53: T <= max_j S_j * sum x
        const bool l = lattice_graph && cls <= 16 &&
                       (double)c->g_deg_max * (double)xmax[(size_t)g] * xsum[(size_t)g] < 4.0e15;
        lat[(size_t)g] = l ? 1.0 : 0.0;
        lat_any |= l;
        lat_all &= l;
    }
    if (bits == 8 && !lat_all) bits = 16;      // the uint8 kernel does not centre
    if (n >= ((int64_t)1 << 25)) bits = 64;    // (rows beyond a 32-bit byte offset: the fp64-row kernel with 64-bit addresses)
    c->narrow_bits = bits;
    c->lat_any = lat_any;
    SC_HIP(hipMemcpyAsync(c->g_lat.p, lat.data(), sizeof(double) * (size_t)Gpad, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_moran_centres, dim3((unsigned)ceil_div64(T * SC_TILE, 256)), dim3(256), 0, c->stream,
                       c->g_mean.as<double>(), c->g_lat.as<double>(), c->g_meanc.as<double>(), T * SC_TILE);
    // ---- operands ----
    const size_t gb = (size_t)Gpad * sizeof(double);
    SC_TRY(c->g_slag.ensure(gb, &c->mem));
    SC_TRY(c->g_seff.ensure(gb, &c->mem));
    SC_TRY(c->g_corr.ensure(gb, &c->mem));
    SC_TRY(c->g_thr.ensure(gb, &c->mem));
    SC_TRY(c->g_I.ensure(gb, &c->mem));
    {   // fp64 tiles, or (uint8 batches) 256 bytes of 16-bit sums per cell and 128-gene group -- more than ONE fp64 tile
        const size_t tiles_b = (size_t)T * n * SC_TILE * sizeof(double), sums16_b = (size_t)ceil_div64(T, 8) * n * 256;
        SC_TRY(c->Lag.ensure(tiles_b > sums16_b ? tiles_b : sums16_b, &c->mem));
    }
    // an all-lattice uint8 batch (count data on a kNN graph): narrow copy first, then neighbour sums + both column sums
    // from the uint8 rows in one pass (k_lag_u8); no Z tiles at all (the lattice operand IS the raw value)
    const bool u8_prelude = n_perm > 0 && bits == 8 && lat_all && c->g_deg_max <= 257;
    // ... or as NIBBLE slots (r04, "the 4-bit source" above) when that takes fewer gathered rows per (permutation, cell)
    int64_t nw = 0;
    uint32_t xmax_all = 0;
    for (int64_t g = 0; g < G; ++g) {
        if (xmax[(size_t)g] >= 16u) ++nw;
        if (xmax[(size_t)g] > xmax_all) xmax_all = xmax[(size_t)g];
    }
    const int64_t nib_slots = G + nw, nib_groups = ceil_div64(nib_slots, 256);
    const bool nib = u8_prelude && c->source_bits_min <= 4 && nib_groups < ceil_div64(G, 128) &&
                     15.0 * (double)xmax_all * (double)c->g_deg_max * (double)score_cells_per_split(n) < 2.0e9;
    c->nib_groups = nib ? (int)nib_groups : 0;
    // ... with the neighbour sums kept as the 16-bit integers they are (r04): a quarter of the bytes k_lag_u8 writes in the
    // serial prelude and of the lag bytes every scoring launch streams
    const bool lag16 = u8_prelude && !nib;
    bool narrow_packed = false;   // the narrow copy of the batch exists already (built in front of the lag that reads it)
    c->lag_u16 = lag16;
    if (nib) {
        c->lm_valid = false;   // (Lag is about to be rewritten)
        bits = 4;
        c->narrow_bits = 4;
        c->lag_u16 = true;
        // slot map: [Gpad] slot of the gene's high nibble (-1: none) | [nw] the genes that have one, ascending
        std::vector<int32_t> map((size_t)Gpad + (size_t)(nw > 0 ? nw : 1), -1);
        for (int64_t g = 0, j = 0; g < G; ++g)
            if (xmax[(size_t)g] >= 16u) { map[(size_t)g] = (int32_t)(G + j); map[(size_t)Gpad + (size_t)j] = (int32_t)g; ++j; }
        SC_TRY(c->nib_map.ensure(sizeof(int32_t) * map.size(), &c->mem));
        SC_HIP(hipMemcpyAsync(c->nib_map.p, map.data(), sizeof(int32_t) * map.size(), hipMemcpyHostToDevice, c->stream));
        SC_HIP(hipStreamSynchronize(c->stream));   // (`map` is a local)
        const int32_t *hi_slot = c->nib_map.as<int32_t>(), *wide = hi_slot + Gpad;
        SC_TRY(c->X32.ensure(sizeof(uint4) * (size_t)nib_groups * n * 8, &c->mem));
        SC_TRY(c->Lag.ensure(sizeof(uint4) * (size_t)nib_groups * n * 32, &c->mem));
        hipLaunchKernelGGL(k_pack_nib, dim3((unsigned)ceil_div64(n * 8, 256), (unsigned)nib_groups), dim3(256), 0, c->stream,
                           c->X.as<double>(), c->X32.as<uint4>(), n, G, nib_slots, wide);
        const int chunks = (int)ceil_div64(n, LAG8_CELLS_PER_BLOCK);
        const int32_t *order = sc_processing_order(c, n);
        {
            KernelTimerScope ts(c, SC_K_LAG);
            hipLaunchKernelGGL(k_lag_nib, dim3((unsigned)align_up64(chunks, 8), (unsigned)nib_groups), dim3(256), 0, c->stream,
                               c->g_indptr.as<long long>(), c->g_indices.as<int32_t>(), c->X32.as<uint4>(), order, n,
                               c->Lag.as<uint4>(), chunks);
            if (nw > 0)
                hipLaunchKernelGGL(k_nib_fixup, dim3((unsigned)ceil_div64(n * nw, 256)), dim3(256), 0, c->stream,
                                   c->Lag.as<uint16_t>(), n, G, (int)nw, wide);
        }
        SC_TRY(c->red_tmp.ensure(sizeof(double) * 2 * (size_t)nib_groups * chunks * 256, &c->mem));
        double *partT = c->red_tmp.as<double>(), *partS = partT + (size_t)nib_groups * chunks * 256;
        hipLaunchKernelGGL(k_nib_colsum, dim3((unsigned)chunks, (unsigned)nib_groups), dim3(256), 0, c->stream,
                           c->X32.as<uint8_t>(), c->Lag.as<uint16_t>(), n, partT, partS, chunks);
        hipLaunchKernelGGL(k_nib_colsum_final, dim3((unsigned)ceil_div64(G, 256)), dim3(256), 0, c->stream, partT, partS, chunks, G,
                           hi_slot, c->g_Inum.as<double>(), c->g_slag.as<double>());
        SC_HIP(hipGetLastError());
    } else if (u8_prelude) {
        c->lm_valid = false;   // (Lag is about to be rewritten)
        SC_TRY(expr_pack_narrow(c, 8));
        const int chunks = (int)ceil_div64(n, LAG8_CELLS_PER_BLOCK);
        SC_TRY(c->red_tmp.ensure(sizeof(double) * 2 * (size_t)T * chunks * SC_TILE, &c->mem));
        const int32_t *order = sc_processing_order(c, n);
        {
            KernelTimerScope ts(c, SC_K_LAG);
            hipLaunchKernelGGL(k_lag_u8, dim3((unsigned)align_up64(chunks, 8), (unsigned)ceil_div64(T, 8)), dim3(256), 0, c->stream,
                               c->g_indptr.as<long long>(), c->g_indices.as<int32_t>(), c->X32.as<uint4>(), order, n, (int)T,
                               (int64_t)n * SC_TILE, c->Lag.as<double>(), lag16 ? c->Lag.as<uint32_t>() : nullptr,
                               c->red_tmp.as<double>(), chunks);
        }
        SC_HIP(hipGetLastError());
        SC_TRY(expr_colsum_chunks(c, c->red_tmp.as<double>(), chunks, c->g_Inum.as<double>()));
        SC_TRY(expr_colsum_chunks(c, c->red_tmp.as<double>() + (size_t)T * chunks * SC_TILE, chunks, c->g_slag.as<double>()));
    } else {
        SC_TRY(expr_write_z(c, c->g_meanc.as<double>()));
        const bool lag_from_rows = n_perm > 0 && bits == 32;
        if (lag_from_rows) {   // the float32 narrow copy first, then the lag from ITS rows (half the gathered bytes of the fp64 tiles)
            SC_TRY(expr_pack_narrow(c, 32));
            const int32_t *order = sc_processing_order(c, n);
            KernelTimerScope ts(c, SC_K_LAG);
            hipLaunchKernelGGL(k_lag_f32rows, dim3((unsigned)align_up64(ceil_div64(n * 8, 256), 8), (unsigned)ceil_div64(T, 2)),
                               dim3(256), 0, c->stream, c->g_indptr.as<int64_t>(), c->g_indices.as<int32_t>(),
                               c->g_data.as<double>(), c->X32.as<uint4>(), c->g_meanc.as<double>(), c->Lag.as<double>(), n, (int)T,
                               lat_any ? c->g_lat.as<double>() : nullptr, order);
            SC_HIP(hipGetLastError());
            narrow_packed = true;
        } else
        SC_TRY(sc_lag_tiles(c, c->g_indptr, c->g_indices, c->g_data, c->Z.as<double>(), c->Lag.as<double>(),
                            lat_any ? c->g_lat.as<double>() : nullptr));
        SC_TRY(expr_colsum(c, OP_MUL, c->Z.as<double>(), c->Lag.as<double>(), c->g_Inum.as<double>(), 1.0));
        if (lat_any) SC_TRY(expr_colsum(c, OP_ID, c->Lag.as<double>(), nullptr, c->g_slag.as<double>(), 1.0));
    }
    SC_TRY(c->sims.ensure(sizeof(double) * (size_t)(T * SC_TILE) * (size_t)(n_perm > 0 ? n_perm : 1), &c->mem));
    hipLaunchKernelGGL(k_moran_scale, dim3((unsigned)ceil_div64(T * SC_TILE, 256)), dim3(256), 0, c->stream,
                       c->g_z2.as<double>(), c->g_Inum.as<double>(), c->g_slag.as<double>(), c->g_mean.as<double>(),
                       c->g_lat.as<double>(), c->g_seff.as<double>(), c->g_corr.as<double>(), c->g_thr.as<double>(),
                       c->g_I.as<double>(), (double)n / c->s0, c->g_uniform_w, T * SC_TILE);
    SC_HIP(hipGetLastError());
    if (n_perm > 0) {
        // partial sums for one chunk of permutations (<= PERM_CHUNK), one slice of the ring: the persistent kernel keeps one row
        // per (128-gene-padded gene, split, permutation); the index-row kernel one per (16 genes, split, permutation)
        int64_t cps = 0;
        const int splits64 = pick_splits(n, 1, &cps);  // upper bound on the index-row kernel's split count
        const int64_t score_splits = ceil_div64(n, score_cells_per_split(n));
        size_t narrow_rows = (size_t)score_splits * (size_t)align_up64(T * SC_TILE, 128);
        if (nib && (size_t)score_splits * (size_t)nib_groups * 256 > narrow_rows) narrow_rows = (size_t)score_splits * (size_t)nib_groups * 256;
        const size_t wide_rows = (size_t)splits64 * SC_TILE;
        SC_TRY(moran_ring_begin(c, (size_t)n_perm * (narrow_rows > wide_rows ? narrow_rows : wide_rows)));
        // the gathered operand: the raw values in the narrowest type that holds every gene of the batch exactly
        if (bits < 64 && bits > 4 && !u8_prelude && !narrow_packed) SC_TRY(expr_pack_narrow(c, bits));
    }
    return SC_OK;
}

template <int BITS, int CB, bool BIG, bool L16 = false>
static void launch_score(sc_ctx *c, int wgs, const uint4 *rows, double *partial, int64_t p0, int cnt, int64_t cps, int splits, int groups)
{
    // the workgroup form scores 128 permutations per task; wavefronts beyond a short chunk's permutations only help with
    // the lag rows.  Below SCORE_WG_MIN_PERMS live permutations a compute unit has too few gathers in flight: such chunks
    // take the per-wavefront form -- same results
    const int last_task = cnt % (8 * SCORE_WAVES);
    if (BITS == 4 || last_task == 0 || last_task >= (BITS == 64 ? 6 * SCORE_WAVES : SCORE_WG_MIN_PERMS)) {
        const int64_t tasks = (int64_t)groups * splits * ((cnt + 8 * SCORE_WAVES - 1) / (8 * SCORE_WAVES));
        if (wgs > tasks) wgs = (int)tasks;
        // (r03 measured the grid rounded to whole rounds of tasks -- 1956 tasks are 13 rounds on 160 workgroups, 12 on 163,
        // and 151 suffice for 13: the launches were 3 % shorter with 163, the generator 4 % slower with 3 compute units
        // fewer, the step the same within its noise either way, and with 151 as well.  Not kept.)
        hipLaunchKernelGGL((k_moran_score_wg<BITS, CB, BIG, L16>), dim3((unsigned)wgs), dim3(SCORE_WAVES * 64), 0, c->stream, rows,
                           c->Lag.as<double>(), (int64_t)c->e_n * SC_TILE, (int)c->e_tiles, c->g_meanc.as<double>(),
                           c->inv.as<int32_t>() + p0 * c->p_stride, partial, c->e_n, c->p_stride, cnt, cps,
                           splits, groups);
        return;
    }
    if constexpr (BITS != 4)
    hipLaunchKernelGGL((k_moran_score<BITS, CB, BIG, L16>), dim3((unsigned)(wgs * (SCORE_WAVES / SCORE_PRIVATE_WAVES))),
                       dim3(SCORE_PRIVATE_WAVES * 64), 0, c->stream, rows,
                       c->Lag.as<double>(), (int64_t)c->e_n * SC_TILE, (int)c->e_tiles, c->g_meanc.as<double>(),
                       c->inv.as<int32_t>() + p0 * c->p_stride, partial, c->e_n, c->p_stride, cnt, cps,
                       splits, groups);
}

// score permutations [p0, p1) of the active table for every gene (on the context stream; the finalise beside it).
// bits: 8 / 16 / 32 / 64 = the persistent kernel gathers rows of that element width through the INVERSE permutation
// (needs inverse rows [p0, p1); invert_here launches that inversion first); 0 = the table's rows are arbitrary index
// maps: the index-row kernel over the fp64 tiles.
static int moran_perm_range(sc_ctx *c, int64_t p0, int64_t p1, int bits, bool invert_here)
{
    const int64_t n = c->e_n, G = c->e_genes, T = c->e_tiles;
    const size_t tile_elems = (size_t)n * SC_TILE;
    const int cnt = (int)(p1 - p0);
    if (cnt <= 0) return SC_OK;
    c->last_source_bits = bits ? bits : 64;
    if (bits) {
        const bool big = n >= ((int64_t)1 << 25);
        SC_REQUIRE(!big || bits == 64, SC_ERR_STATE, "internal: %lld cells need the 64-bit-address scoring kernel", (long long)n);
        if (invert_here) SC_TRY(invert_rows(c, p0, p1, c->stream));
        const int GP = bits == 4 ? 256 : bits == 8 ? 128 : bits == 16 ? 64 : bits == 32 ? 32 : 16;
        const int groups = bits == 4 ? c->nib_groups : (int)ceil_div64(T * SC_TILE, GP);
        const int64_t cps = score_cells_per_split(n);
        const int splits = (int)ceil_div64(n, cps);
        // one workgroup per compute unit: all of them, or all but those left to a generator that runs beside us
        if (c->n_cus <= 0) {
            hipDeviceProp_t prop;
            SC_HIP(hipGetDeviceProperties(&prop, c->device));
            c->n_cus = prop.multiProcessorCount;
        }
        int wgs = c->n_cus - (c->score_leave_cus > 0 && c->score_leave_cus < c->n_cus ? c->score_leave_cus : 0);
        const int64_t tasks = (int64_t)groups * splits * ((cnt + 7) / 8);
        if ((int64_t)wgs * SCORE_WAVES > tasks) wgs = (int)ceil_div64(tasks, SCORE_WAVES);
        double *partial = nullptr;
        SC_TRY(moran_ring_slice(c, &partial));
        {
            KernelTimerScope ts(c, SC_K_MORAN_PERM);   // (the scoring launch alone: neither the ring's wait nor the finalise)
            // (8 cells per stage were measured for the narrow sources too: under the 128-VGPR cap of the 1024-thread form they spill)
            if (bits == 4) launch_score<4, 4, false>(c, wgs, c->X32.as<uint4>(), partial, p0, cnt, cps, splits, groups);
            else if (bits == 8 && c->lag_u16) launch_score<8, 4, false, true>(c, wgs, c->X32.as<uint4>(), partial, p0, cnt, cps, splits, groups);
            else if (bits == 8) launch_score<8, 4, false>(c, wgs, c->X32.as<uint4>(), partial, p0, cnt, cps, splits, groups);
            else if (bits == 16) launch_score<16, 4, false>(c, wgs, c->X32.as<uint4>(), partial, p0, cnt, cps, splits, groups);
            else if (bits == 32) launch_score<32, 4, false>(c, wgs, c->X32.as<uint4>(), partial, p0, cnt, cps, splits, groups);
            else if (!big) launch_score<64, 8, false>(c, wgs, c->Z.as<uint4>(), partial, p0, cnt, cps, splits, groups);
            else launch_score<64, 8, true>(c, wgs, c->Z.as<uint4>(), partial, p0, cnt, cps, splits, groups);
        }
        SC_TRY(moran_ring_scored(c));
        if (bits == 4) {
            hipLaunchKernelGGL(k_moran_finalize_nib, dim3((unsigned)ceil_div64((int64_t)cnt * G, 256)), dim3(256), 0, c->stream_out,
                               partial, c->g_seff.as<double>(), c->g_corr.as<double>(), c->nib_map.as<int32_t>(),
                               c->sims.as<double>(), c->sims_raw.as<double>(), cnt, splits, G, p0);
            return moran_ring_finalised(c);
        }
        const dim3 fgrid((unsigned)ceil_div64((int64_t)cnt * GP, 256), (unsigned)groups);
        auto fin = bits == 8 ? k_moran_finalize_groups<128> : bits == 16 ? k_moran_finalize_groups<64>
                 : bits == 32 ? k_moran_finalize_groups<32> : k_moran_finalize_groups<16>;
        hipLaunchKernelGGL(fin, fgrid, dim3(256), 0, c->stream_out, partial, c->g_seff.as<double>(),
                           c->g_corr.as<double>(), c->sims.as<double>(), c->sims_raw.as<double>(), cnt, splits, G, p0);
        return moran_ring_finalised(c);
    }
    const int ptiles = (int)ceil_div64(cnt, MP_PERMS_PER_BLOCK);
    int64_t cps = 0;
    const int splits = pick_splits(n, ptiles, &cps);
    for (int64_t t = 0; t < T; ++t) {   // (every tile's launch takes the ring's next slice)
        double *partial = nullptr;
        SC_TRY(moran_ring_slice(c, &partial));
        {
            KernelTimerScope ts(c, SC_K_MORAN_PERM);
            hipLaunchKernelGGL(k_moran_perm, dim3((unsigned)splits, (unsigned)ptiles), dim3(256), 0, c->stream,
                               c->Z.as<double>() + t * tile_elems, c->Lag.as<double>() + t * tile_elems,
                               c->perm.as<int32_t>() + p0 * c->p_stride, partial, n, c->p_stride,
                               cnt, cps);
        }
        SC_TRY(moran_ring_scored(c));
        hipLaunchKernelGGL(k_moran_finalize, dim3((unsigned)ceil_div64((int64_t)cnt * SC_TILE, 256)), dim3(256), 0,
                           c->stream_out, partial, c->g_seff.as<double>(), c->g_corr.as<double>(),
                           c->sims.as<double>(), c->sims_raw.as<double>(), cnt, splits, G, t * SC_TILE, p0);
        SC_TRY(moran_ring_finalised(c));
    }
    return SC_OK;
}

static int moran_alloc_sims(sc_ctx *c, int64_t n_perm)
{
    const size_t bytes = sizeof(double) * (size_t)(c->e_tiles * SC_TILE) * (size_t)(n_perm > 0 ? n_perm : 1);
    SC_TRY(c->sims.ensure(bytes, &c->mem));
    SC_TRY(c->sims_raw.ensure(bytes, &c->mem));
    return SC_OK;
}

static int moran_finish(sc_ctx *c, int64_t n_perm, double *I_out, double *sims_out, int64_t *count_ge_out,
                        double *sim_sum_out, double *sim_sumsq_out)
{
    const int64_t G = c->e_genes;
    if (n_perm > 0) {
        SC_TRY(c->counts.ensure(sizeof(long long) * (size_t)G, &c->mem));
        SC_TRY(c->sim_sum.ensure(sizeof(double) * (size_t)G, &c->mem));
        SC_TRY(c->sim_sumsq.ensure(sizeof(double) * (size_t)G, &c->mem));
        SC_TRY(moran_ring_join(c));   // sims are complete behind the last finalise
        hipLaunchKernelGGL(k_moran_count, dim3((unsigned)G), dim3(256), 0, c->stream, c->sims.as<double>(),
                           c->sims_raw.as<double>(), c->g_thr.as<double>(), c->g_lat.as<double>(), c->g_z2.as<double>(),
                           (int)n_perm, G, c->counts.as<long long>(), c->sim_sum.as<double>(),
                           c->sim_sumsq.as<double>());
        SC_HIP(hipGetLastError());
        if (sims_out)
            SC_HIP(hipMemcpyAsync(sims_out, c->sims.p, sizeof(double) * (size_t)n_perm * (size_t)G,
                                  hipMemcpyDeviceToHost, c->stream));
        if (count_ge_out)
            SC_HIP(hipMemcpyAsync(count_ge_out, c->counts.p, sizeof(int64_t) * (size_t)G, hipMemcpyDeviceToHost,
                                  c->stream));
        if (sim_sum_out)
            SC_HIP(hipMemcpyAsync(sim_sum_out, c->sim_sum.p, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost,
                                  c->stream));
        if (sim_sumsq_out)
            SC_HIP(hipMemcpyAsync(sim_sumsq_out, c->sim_sumsq.p, sizeof(double) * (size_t)G,
                                  hipMemcpyDeviceToHost, c->stream));
    }
    SC_HIP(hipMemcpyAsync(I_out, c->g_I.p, sizeof(double) * (size_t)G, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    c->ring.launches = 0;   // (the side stream is idle: the context stream waited for its last launch)
    return SC_OK;
}

extern "C" int sc_moran(sc_ctx *c, int64_t n_perm, double *I_out, double *sims_out, int64_t *count_ge_out,
                        double *sim_sum_out, double *sim_sumsq_out)
{
    SC_TRY(moran_check(c, n_perm, I_out));
    if (n_perm > 0) {
        SC_REQUIRE(c->p_count >= n_perm, SC_ERR_STATE, "sc_moran: permutation table holds %lld rows, need %lld",
                   (long long)c->p_count, (long long)n_perm);
        SC_REQUIRE(c->p_n == c->e_n, SC_ERR_INVALID, "sc_moran: permutation length %lld != n_cells %lld",
                   (long long)c->p_n, (long long)c->e_n);
    }
    // A table left by sc_moran_seeded may exist only as inverse rows, which is all the scoring kernel reads: the
    // permutation rows themselves are materialised only when rows are needed whose inverse is not there yet.
    const bool inverse_suffices = n_perm > 0 && c->perm_bijective && c->inv_rows_valid >= n_perm;
    if (n_perm > 0 && !inverse_suffices) SC_TRY(sc_perm_forward_ensure(c));
    bool bijective = true;
    SC_TRY(sc_perm_table_is_bijective(c, n_perm, &bijective));
    SC_TRY(moran_prepare(c, n_perm < PERM_CHUNK ? n_perm : PERM_CHUNK, n_perm <= 0 || bijective));
    SC_TRY(moran_alloc_sims(c, n_perm));
    const int bits = bijective ? c->narrow_bits : 0;
    for (int64_t p0 = 0; p0 < n_perm; p0 += PERM_CHUNK) {
        const int64_t p1 = p0 + PERM_CHUNK < n_perm ? p0 + PERM_CHUNK : n_perm;
        SC_TRY(moran_perm_range(c, p0, p1, bits, bits != 0 && p1 > c->inv_rows_valid));
        if (bits != 0 && p1 > c->inv_rows_valid) c->inv_rows_valid = p1;
    }
    return moran_finish(c, n_perm, I_out, sims_out, count_ge_out, sim_sum_out, sim_sumsq_out);
}

// (what the number means and how it was chosen: the comment in front of moran_seeded_streams)
#define SCORE_RESERVED_CUS 128   // byte-plane scoring (two runs of 20 steps each, same box, ms per step): 96 -> 151.2 / 151.8,
                                 // 112 -> 149.7 / 149.2, 128 -> 143.8 / 143.5, 144 -> 143.9 / 143.8 (and 120 -> 146.1 / 146.3, 125 ->
                                 // 144.5 / 144.2, 136 -> 147.4 / 146.7).  At 112 the integer kernel's launches are a tenth shorter than the
                                 // fp64 kernel's (104 ms per step instead of 116) but the chain beside them slows from 123 to 129 ms and
                                 // the step stays where it was; with 16 more CUs the chain takes 105 ms, the launches 109 ms.
                                 // Swept again with the coalesced expansion (k_expand 10.8 instead of 17.7 ms of the generator's CUs
                                 // per step), same protocol: 112 -> 145.1 / 144.4, 120 -> 144.1 / 142.6, 128 -> 140.3 / 139.7 (chain
                                 // 126 / 120 / 101 ms): the cheaper expansion does not let the generator give CUs back, 128 stays
static int moran_seeded_once(sc_ctx *c, uint64_t *state6, int64_t n_perm, double *I_out, double *sims_out,
                             int64_t *count_ge_out, double *sim_sum_out, double *sim_sumsq_out, PermPipe *begun)
{
    SC_REQUIRE(state6, SC_ERR_INVALID, "sc_moran_seeded: null state");
    SC_TRY(moran_check(c, n_perm, I_out));
    SC_REQUIRE(n_perm >= 1, SC_ERR_INVALID, "sc_moran_seeded: n_perm must be >= 1 (use sc_moran for n_perm = 0)");
    const int64_t n = c->e_n;
    SC_TRY(moran_alloc_sims(c, n_perm));
    // every scoring kernel gathers through the inverse table only (the inverse of a Fisher-Yates result is the same
    // transpositions in ascending order: no permutation rows, no scatter pass)
    const bool inverse_only = permgen_can_swap_inverse(n);
    int bits = 64;
    // the set-up in two halves: what only enqueues, then -- with the generator topped up in between (pipe_consume) -- the
    // synchronisation, the host's decisions and the rest
    auto prepare_early = [&]() -> int { return moran_prepare_early(c); };
    auto prepare = [&]() -> int {
        SC_TRY(moran_prepare(c, n_perm < PERM_CHUNK ? n_perm : PERM_CHUNK, true));
        bits = c->narrow_bits;
        // CUs left to the generator, by source width (r04, bench size, ms per step at 64 / 80 / 96 / 112 CUs left): the uint8
        // step is balanced between generator and scoring (SCORE_RESERVED_CUS); uint16 243.0 / 246.8 / 238.5 / 239.2; float32,
        // whose step is scoring-bound, 389.3 / 390.4 / 398.1 / 408.6
        if (c->score_leave_cus > 8) c->score_leave_cus = bits == 8 ? SCORE_RESERVED_CUS : bits == 16 ? 96 : 64;
        return SC_OK;
    };
    auto score = [&](int64_t p0, int64_t p1) -> int {
        // The last chunk is scored after the generator has finished (its own swaps are the generator's last launches):
        // it takes the CUs the earlier launches left to the generator; the one before it runs beside the generator's
        // short last chunk only.  CUs left by the second-to-last / last chunk's launch, measured at bench size (ms per
        // step): 64,64 -> 211.5, 64,8 -> 209.9, 32,8 -> 207.1, 8,8 -> 207.9.
        const int keep = c->score_leave_cus;
        if (keep > 8) {
            const int tail_prev = keep < 32 ? keep : 32, tail_last = 8;
            if (p1 == n_perm) c->score_leave_cus = tail_last;
            // launches with fewer permutations than the tapering chunks' still to come use tail_prev
            else if (n_perm > 3 * PERM_CHUNK && n_perm - p1 < PIPE_TAIL_TOTAL) c->score_leave_cus = tail_prev;
        }
        const int rc = moran_perm_range(c, p0, p1, bits, false);
        c->score_leave_cus = keep;
        return rc;
    };
    if (begun) SC_TRY(pipe_consume(c, *begun, state6, prepare_early, prepare, score));   // the generator has been running since _begin
    else SC_TRY(sc_perm_pipeline(c, state6, n, n_perm, inverse_only ? 1 : 2, PIPE_AHEAD, prepare_early, prepare, score));
    return moran_finish(c, n_perm, I_out, sims_out, count_ge_out, sim_sum_out, sim_sumsq_out);
}

// SCORE_RESERVED_CUS: compute units the persistent scoring kernel leaves EMPTY for the generator that runs beside it.
//
// The scoring kernel would fill every compute unit with wavefronts that live for milliseconds, and the generator is
// a chain of sub-millisecond launches (most of them 1024-thread workgroups that need a nearly empty compute unit)
// that must not queue behind them.  r01 kept them apart with CU-masked and prioritised streams; r02 does it by the
// scoring kernel's own shape -- a grid of (CUs - reserved) one-per-CU workgroups (see k_moran_score) on plain streams,
// each stream on its own hardware queue (GPU_MAX_HW_QUEUES, see sc_api.hip).  Measured on one box, 1M cells x 500
// genes x 1000 permutations, uint16 source, event-ordered generator: reserved 16 -> 1406 genes/s, 32 -> 1716, 48 -> no
// better; with the runtime's default of 4 shared hardware queues 1174 (the chain's launches queue behind 25-ms scoring
// launches).  With the uint8 source and the flag-ordered generator (one chain launch per chunk; its gate / publish
// launches need free wavefront slots at once): 32 -> 2050, 40 / 48 -> 2177, 64 -> 2327, 72 -> 2332, 80 -> 2302,
// 96 -> 2347, 128 -> 2173 (scoring 125 ms on 224 CUs, 157 on 192, 190 on 128: the step is balanced around 64-96).
// r03, workgroup-shared lag rows (scoring a third faster, the step generator-bound): the chain itself slows down when
// the scoring kernel has more of the chip -- chain busy 170 / 144 / 136 / 134 / 132 ms per step with 48 / 64 / 96 / 128 /
// 160 CUs reserved (memory-system interference: the chain is one workgroup of dependent loads) -- and the step is
// 198 / 179 / 175 / 180 / 196 ms: 96 (with a 48-permutation last chunk).
static int moran_seeded_streams(sc_ctx *c, uint64_t *state6, int64_t n_perm, double *I_out, double *sims_out,
                                int64_t *count_ge_out, double *sim_sum_out, double *sim_sumsq_out, PermPipe *begun = nullptr)
{
    c->score_leave_cus = c && c->e_n > 0 && permgen_is_block_parallel(c, c->e_n) ? SCORE_RESERVED_CUS : 8;
    const int rc = moran_seeded_once(c, state6, n_perm, I_out, sims_out, count_ge_out, sim_sum_out, sim_sumsq_out, begun);
    c->score_leave_cus = 0;
    return rc;
}

extern "C" int sc_moran_seeded(sc_ctx *c, uint64_t *state6, int64_t n_perm, double *I_out, double *sims_out,
                               int64_t *count_ge_out, double *sim_sum_out, double *sim_sumsq_out)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "sc_moran_seeded: null context");
    // (nothing is returned before the job has passed its verification: nothing to undo before the sequential rerun, whose
    // call recomputes the CU reservation for the sequential scan)
    return permgen_rerun_on_failure(
        c, [&]() { return moran_seeded_streams(c, state6, n_perm, I_out, sims_out, count_ge_out, sim_sum_out, sim_sumsq_out); },
        nullptr);
}

// The same call in two halves, so that the generator -- the longest chain of the job, which needs nothing but n_cells and
// the seed's state -- runs while the caller is still building the graph and uploading the expression matrix
// (morans_i: kNN + the D2H of the neighbour lists for obsp + 40 ms of PCIe upload used to sit in front of it):
//   sc_moran_seeded_begin(ctx, state6, n_cells, n_perm)   enqueues the whole generator job and returns at once;
//   ... sc_knn_2d / sc_graph_* / sc_expr_set_* on the same context ...
//   sc_moran_seeded_finish(ctx, state6, outputs)          prepares the operands and scores chunk after chunk.
// Results and the final generator state are those of sc_moran_seeded.  A job that is begun and not finished is
// dropped by sc_moran_seeded_abort, by any call that replaces the permutation table, and with the context.
extern "C" int sc_moran_seeded_begin(sc_ctx *c, const uint64_t *state6, int64_t n_cells, int64_t n_perm, int64_t ahead_chunks)
{
    SC_REQUIRE(c && state6, SC_ERR_INVALID, "sc_moran_seeded_begin: null pointer");
    SC_REQUIRE(n_perm >= 1 && n_perm <= (1 << 24), SC_ERR_INVALID, "sc_moran_seeded_begin: n_perm=%lld out of range", (long long)n_perm);
    SC_HIP(hipSetDevice(c->device));
    sc_perm_pipe_abort(c);
    auto pp = std::make_unique<PermPipe>();
    // ahead_chunks: chunks of the generator enqueued before returning (a chunk is ~250 launches, ~3.5 ms of host time);
    // 0 = all of them (a caller with tens of milliseconds of host-blocking work in front of _finish: an upload), else at
    // least 2 (_finish enqueues the rest, two ahead of the scoring)
    const int64_t ahead_n = ahead_chunks <= 0 ? (int64_t)1 << 40 : (ahead_chunks < 2 ? 2 : ahead_chunks);
    // (r04 measured again, and dropped again: the first half of the scoring's preparation enqueued right behind the
    // generator's FIRST chunk for callers whose operands are resident -- scoring starts ~9 ms earlier, the step is 3.5 ms
    // LONGER (165.4 vs 161.9 ms, same box): the full-chip column-sum kernels delay the generator's first units, and the
    // scoring then only waits longer for its first chunks.)
    SC_TRY(pipe_begin(c, state6, n_cells, n_perm, permgen_can_swap_inverse(n_cells) ? 1 : 2, PIPE_AHEAD, *pp, ahead_n));
    c->pipe = std::move(pp);
    return SC_OK;
}

extern "C" int sc_moran_seeded_abort(sc_ctx *c)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "null context");
    SC_HIP(hipSetDevice(c->device));
    sc_perm_pipe_abort(c);
    return SC_OK;
}

extern "C" int sc_moran_seeded_finish(sc_ctx *c, uint64_t *state6, double *I_out, double *sims_out, int64_t *count_ge_out,
                                      double *sim_sum_out, double *sim_sumsq_out)
{
    SC_REQUIRE(c && state6, SC_ERR_INVALID, "sc_moran_seeded_finish: null pointer");
    SC_REQUIRE(c->pipe, SC_ERR_STATE, "sc_moran_seeded_finish: no job begun (sc_moran_seeded_begin)");
    SC_HIP(hipSetDevice(c->device));
    std::unique_ptr<PermPipe> pp = std::move(c->pipe);
    const int64_t n_perm = pp->n_perm;
    // first the begun job; if it fails its verification, nothing was returned: the job is dropped and rerun in one piece
    auto attempt = [&]() -> int {
        if (!pp) return moran_seeded_streams(c, state6, n_perm, I_out, sims_out, count_ge_out, sim_sum_out, sim_sumsq_out);
        SC_REQUIRE(pp->n == c->e_n, SC_ERR_INVALID, "sc_moran_seeded_finish: the job was begun for %lld cells, the expression has %lld",
                   (long long)pp->n, (long long)c->e_n);
        return moran_seeded_streams(c, state6, n_perm, I_out, sims_out, count_ge_out, sim_sum_out, sim_sumsq_out, pp.get());
    };
    auto drop = [&]() -> int {
        pipe_drain(c, *pp);
        for (int k = 0; k < 6; ++k) state6[k] = pp->state0[k];
        pp.reset();
        return SC_OK;
    };
    const int rc = permgen_rerun_on_failure(c, attempt, drop);
    if (pp) pipe_drain(c, *pp);   // (no-op after a completed consume; an error path may have left launches in flight)
    return rc;
}

