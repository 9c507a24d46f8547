// What the units of the numpy-exact permutation generator share (the units: sc_permgen.hip's header).  gfx950 only.
// A kernel is launched only from its own unit; other units call the host functions declared at the end.
#pragma once

#include "sc_ctx.h"

typedef unsigned __int128 u128;

#define PCG_MULT_HI 0x2360ed051fc65da4ULL
#define PCG_MULT_LO 0x4385df649fccf645ULL

struct Affine {  // x -> mult * x + plus  (mod 2^128)
    u128 mult, plus;
};

__host__ __device__ static inline u128 pcg_mult() { return ((u128)PCG_MULT_HI << 64) | PCG_MULT_LO; }

// the LCG step composed `delta` times
__host__ __device__ static inline Affine lcg_pow(u128 inc, uint64_t delta)
{
    u128 acc_m = 1, acc_p = 0, cur_m = pcg_mult(), cur_p = inc;
    while (delta > 0) {
        if (delta & 1) {
            acc_m *= cur_m;
            acc_p = acc_p * cur_m + cur_p;
        }
        cur_p = (cur_m + 1) * cur_p;
        cur_m *= cur_m;
        delta >>= 1;
    }
    Affine a;
    a.mult = acc_m;
    a.plus = acc_p;
    return a;
}

__host__ __device__ static inline uint64_t xsl_rr(u128 s)
{
    uint64_t hi = (uint64_t)(s >> 64), lo = (uint64_t)s;
    uint64_t x = hi ^ lo;
    unsigned r = (unsigned)(hi >> 58);
    return (x >> r) | (x << ((64 - r) & 63));
}

// The same rotation from 32-bit funnel shifts only (v_alignbit_b32) -- the form the DEVICE uses.
// r02 finding: with the plain form above, the compiler emits v_lshlrev_b64 / v_lshrrev_b64 with a per-lane shift
// amount, and k_raw_stream then wrote WRONG outputs for whole wavefronts (the left-shifted half of the rotation)
// whenever kernels of other hardware queues ran on the chip at the same time -- never when it ran alone:
// ~50 wavefronts per 1M x 1000 job inside the Moran pipeline, i.e. every r01 pipeline run at bench size drew some
// non-numpy permutations; also when a second process used the GPU.  Same job, same box, A/B by kernel variant
// (scripts/pipeline_soak.py, 3 repetitions each): 64-bit shifts 38k-139k wrong draws per job; with an added
// s_waitcnt after every store 1.5-2.1M; this form 0, and every statistic bit-equal to the host generator's.
// Evidence and decoding of the wrong words: profiles/r02_gpu_sharing_raw_stream_corruption.txt.
__device__ static inline uint64_t xsl_rr32(u128 s)
{
    const uint64_t hi = (uint64_t)(s >> 64), lo = (uint64_t)s;
    const uint64_t x = hi ^ lo;
    const uint32_t r = (uint32_t)(hi >> 58);
    uint32_t xl = (uint32_t)x, xh = (uint32_t)(x >> 32);
    if (r & 32) { const uint32_t t = xl; xl = xh; xh = t; }          // rotate by 32: swap the halves
    const uint32_t k = r & 31;
    const uint32_t ol = __builtin_amdgcn_alignbit(xh, xl, k);         // ({xh, xl} >> k) low word
    const uint32_t oh = __builtin_amdgcn_alignbit(xl, xh, k);
    return ((uint64_t)oh << 32) | ol;
}

// every bit below v's top bit set as well: the mask of numpy's bounded draw on [0, v] (the host's mask_of)
static inline uint32_t smear_mask(uint32_t v) { v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16; return v; }

// A0: the raw 32-bit stream, stored in the layout the scan reads.
//
// Stream draw r (r = 0: low half of 64-bit output 0, r = 1: its high half, ...) lives at
//   phys(r) = block(r) * SCAN_BLOCK + g * (4 * SCAN_THREADS) + tau * 4 + (r & 3),
//   tau = (r % SCAN_BLOCK) / SCAN_D, g = ((r % SCAN_D) / 4)
// i.e. inside every SCAN_BLOCK-draw block, scan thread tau's draws [D tau, D tau + D) are stored as D/4
// groups of 4, group g at block + g*4*SCAN_THREADS + 4*tau: the scan's g-th 16-byte load is contiguous
// across the workgroup's threads.  One generator thread produces one such 16-byte group (2 consecutive 64-bit
// outputs) per block for RAW_BLOCKS consecutive blocks, stepping its LCG state by the constant
// jump A^16384 between blocks.

#define SCAN_THREADS 1024
#define SCAN_D 16  // draws per thread and round (r01 sweep at 1M cells, sequential / block-parallel scan of 300
                   // permutations: 8 -> 145 / 83 ms, 12 -> 119 / 72, 16 -> 107 / 58, 20 -> 103 / 59, 24 -> 114 / 63, 32 -> 154 / 84)
#define SCAN_BLOCK (SCAN_THREADS * SCAN_D)
#define SCAN_GROUPS (SCAN_D / 4)
#if SCAN_D <= 32
typedef uint32_t bits_t;
#else
typedef uint64_t bits_t;
#endif
#define RAW_BLOCKS 8

#if defined(__HIPCC__)   // ---- the in-block rejection scan, shared by k_scan, k_phi_events, k_chain and k_block_exact ----
__device__ __forceinline__ uint32_t mask_of(uint32_t i) { return 0xffffffffu >> __clz((int)i); }  // i >= 1

// What one thread knows about its SCAN_D draws for a given entering count.
struct ScanRes {
    uint32_t c_used;  // entering count (accepted steps of this block in front of the thread) it was computed for
    uint32_t cnt;     // accepted draws
    bits_t bits;      // accept mask, bit s = draw s accepted
    uint32_t gap;     // fast path: the entering count may move by up to +-gap without flipping any decision
                      //   (min over draws of: threshold - value if accepted, value - threshold - 1 if rejected)
    uint32_t i0;      // threshold of the first draw
    uint32_t mask;    // fast path: the one mask used
    uint32_t fast;    // computed on the fast path
    uint32_t end;     // 1 + local index of the draw that completed the job's last step (0: none)
};

// Sequential pass of one thread over its draws, entering with c accepted steps in front of it.
__device__ __forceinline__ void scan_thread(const uint32_t (&u)[SCAN_D], uint32_t c_in,
                                            uint32_t rem_block, uint32_t M, uint32_t top_mask, uint32_t limit,
                                            ScanRes &r)
{
    uint32_t c = c_in, rem = rem_block;
    if (c >= rem) { c = (c - rem) % M; rem = M; }
    const uint32_t i0 = rem - c;
    uint32_t mask = mask_of(i0);
    r.c_used = c_in; r.i0 = i0; r.mask = mask; r.end = 0;
    // fast path: neither a mask change, nor the end of a permutation, nor the end of the job can
    // happen within SCAN_D accepts
    const bool fast = i0 > (mask >> 1) + SCAN_D && c_in + SCAN_D < limit;
    // r04: ONE pass per wavefront (r03 ran the fast loop for its fast lanes and then the general loop for the others: the
    // wavefront that holds a band change -- the one every round of a computed block waits for -- paid both, ~310
    // instructions).  All lanes fast: the fast loop.  Otherwise every lane takes the general loop; and the job's end is
    // looked for only by wavefronts that can reach it.
    if (!__any(!fast)) {
        uint32_t thr = i0;
        bits_t bits = 0;
        // the slack of an accepted draw is d, of a rejected one -d - 1 = ~d: as UNSIGNED numbers the other one of the pair is
        // >= 2^31 and never the minimum -- two mins on values the loop has anyway, instead of (shift, xor, min)
        uint32_t gacc = 0xffffffffu, grej = 0xffffffffu;
#pragma unroll
        for (int s = 0; s < SCAN_D; ++s) {
            const uint32_t v = u[s] & mask;
            const uint32_t d = thr - v;                  // both < 2^31; accepted iff d < 2^31
            const uint32_t nd = ~d;
            const uint32_t acc = nd >> 31;
            gacc = min(gacc, d);
            grej = min(grej, nd);
            bits |= (bits_t)acc << s;
            thr -= acc;
        }
        const uint32_t gap = min(gacc, grej);
        r.cnt = i0 - thr; r.bits = bits; r.gap = gap; r.fast = 1;
        return;
    }
    // general path, branch-free: the band / permutation bookkeeping is evaluated for every draw (it is the identity
    // unless the draw was accepted) instead of a divergent branch tree
    // (r04, second step: no gap in the general loop.  A wavefront comes here because one of its lanes sits at a band edge or
    // a permutation's end; whatever moves its entering counts moves that edge, and the wavefront is re-evaluated as a whole
    // anyway -- a validity range for its fast lanes bought nothing in the rounds counter, and costs 3 of 12 operations a draw.)
    uint32_t i = i0;
    bits_t bits = 0;
    if (!__any(!(c_in + SCAN_D < limit))) {   // (wavefront-uniform) the job does not end inside these draws
        if (!__any(i0 <= SCAN_D)) {           // (wavefront-uniform) nor does a permutation: mask changes only
#pragma unroll
            for (int s = 0; s < SCAN_D; ++s) {
                const uint32_t v = u[s] & mask;
                const int32_t d = (int32_t)(i - v);          // accepted iff d >= 0
                const uint32_t acc = (uint32_t)(~d) >> 31;
                bits |= (bits_t)acc << s;
                i -= acc;
                const uint32_t half = mask >> 1;
                mask = i <= half ? half : mask;
            }
        } else {
#pragma unroll
            for (int s = 0; s < SCAN_D; ++s) {
                const uint32_t v = u[s] & mask;
                const int32_t d = (int32_t)(i - v);
                const uint32_t acc = (uint32_t)(~d) >> 31;
                bits |= (bits_t)acc << s;
                i -= acc;
                const bool wrap = i == 0;                 // the permutation is complete: the next one starts at M
                const uint32_t half = mask >> 1;
                mask = wrap ? top_mask : (i <= half ? half : mask);
                i = wrap ? M : i;
            }
        }
        r.cnt = (uint32_t)__popcll((unsigned long long)bits);
        r.bits = bits; r.gap = 0u; r.fast = 0u;
        return;
    }
    uint32_t off = c_in, end = 0;
#pragma unroll
    for (int s = 0; s < SCAN_D; ++s) {
        const uint32_t v = u[s] & mask;
        const uint32_t acc = ((off < limit) & (v <= i)) ? 1u : 0u;
        bits |= (bits_t)acc << s;
        off += acc;
        i -= acc;
        end = (acc & (off == limit ? 1u : 0u)) ? (uint32_t)s + 1 : end;
        const bool wrap = i == 0;
        const uint32_t half = mask >> 1;
        mask = wrap ? top_mask : (i <= half ? half : mask);
        i = wrap ? M : i;
    }
    r.end = end;
    r.cnt = off - c_in; r.bits = bits; r.gap = 0; r.fast = 0;
}

// Is the cached result still the exact result for entering count c_new?  On the fast path every
// threshold moves by -(c_new - c_used); no decision flips while the move stays inside the gaps.
// (32-bit arithmetic: entering counts are at most SCAN_BLOCK, thresholds below 2^31.)
__device__ __forceinline__ bool scan_still_valid(const ScanRes &r, uint32_t c_new, uint32_t M, uint32_t limit)
{
    const int32_t delta = (int32_t)c_new - (int32_t)r.c_used;
    const int32_t i0n = (int32_t)r.i0 - delta;  // new first threshold (same permutation, same band required)
    const uint32_t mag = (uint32_t)(delta < 0 ? -delta : delta);
    const bool moved_ok = r.fast && i0n <= (int32_t)M && i0n <= (int32_t)r.mask && i0n > (int32_t)((r.mask >> 1) + SCAN_D) &&
                          c_new + SCAN_D < limit && mag <= r.gap;
    return delta == 0 || moved_ok;
}

// thread tau's 32 draws of the block at `base` (tiled layout, see k_raw_stream): 8 coalesced loads
__device__ __forceinline__ void scan_load(const uint32_t *__restrict__ raw, uint64_t base, uint32_t tau,
                                          uint32_t (&u)[SCAN_D])
{
    const uint4 *src = reinterpret_cast<const uint4 *>(raw + base) + tau;
#pragma unroll
    for (int q = 0; q < SCAN_D / 4; ++q) {
        const uint4 v = src[q * SCAN_THREADS];
        u[4 * q] = v.x; u[4 * q + 1] = v.y; u[4 * q + 2] = v.z; u[4 * q + 3] = v.w;
    }
}

// inclusive prefix sum over the 64 lanes with DPP row shifts / row broadcasts (no LDS round trips)
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x)
{
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);  // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);  // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);  // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);  // row_shr:8
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1,3
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2,3
    return x;
}

// Expected number of accepted steps after q draws, starting with `rem` steps left in the permutation (mean
// field, closed form per mask band: in a band with top = mask + 1 the threshold decays like exp(-q / top)).
// Only the first guess of the in-block fixed point; follows the acceptance rate through band changes and
// permutation ends, where a constant rate is off by thousands of steps.
__device__ __forceinline__ uint32_t expected_steps(uint32_t rem, float q, uint32_t M)
{
    float i = (float)rem, acc = 0.f;
    for (int guard = 0; guard < 64 && q > 0.f; ++guard) {
        uint32_t ii = (uint32_t)i;
        if (ii == 0) { i = (float)M; ii = M; }
        const uint32_t m = mask_of(ii);
        const float top = (float)m + 1.f, lo = (float)((m >> 1) + 1);
        const float need = top * __logf((i + 1.f) / lo);  // draws to leave the band
        if (need <= q) { q -= need; acc += i - lo + 1.f; i = lo - 1.f; }
        else { const float inew = (i + 1.f) * __expf(-q / top) - 1.f; acc += i - inew; q = 0.f; }
    }
    return (uint32_t)(acc + 0.5f);
}

__device__ __forceinline__ uint32_t select64(uint64_t x, uint32_t r)  // position of the set bit of rank r < popc(x)
{
    uint32_t pos = 0;
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const uint32_t c = (uint32_t)__popcll(sc_shr64(x, pos) & ((1ull << sh) - 1ull));   // (sh is a literal: a constant mask)
        if (r >= c) { r -= c; pos += sh; }
    }
    return pos;
}

struct BlockShared {
    uint32_t wsum[2][SCAN_THREADS / 64];   // per wavefront: accept count | (recomputed something last round) << 31; by round parity
};

// inclusive prefix sum inside each row of 16 lanes
__device__ __forceinline__ uint32_t row16_inclusive_scan(uint32_t x)
{
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false);  // row_shr:1
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);  // row_shr:2
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false);  // row_shr:4
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);  // row_shr:8
    return x;
}

// The exact result of ONE block of SCAN_BLOCK draws entered with S_block completed steps, by the whole
// workgroup: every thread ends with its accept mask (r.bits), its entering count (excl = accepted steps of
// the block in front of it) and the block's accept count.  Fixed point on the entering counts: a thread
// recomputes only when its cached result is not provably the result for its new entering count; a thread
// with the right entering count produces the right count, so the correct prefix grows every round.
// One barrier per round: the wavefronts publish their counts together with "one of my threads recomputed in the
// previous round"; a round that learns that nobody did has just rebuilt the entering counts of the previous round,
// for which every cached result was valid: the result.  (r02: the first form paid two barriers and ~150 instructions
// of bookkeeping per wavefront and round -- 16 wavefronts on one CU make a round throughput-bound, ~2.5 us; measured
// 3.6 rounds for an ordinary computed block, 13 for the block in which a permutation ends.)
// Returns 1 if the iteration cap was hit (cannot happen: the prefix grows by at least one thread a round).
__device__ __forceinline__ int block_fixed_point(const uint32_t (&u)[SCAN_D], uint64_t S_block,
                                                 uint32_t rem_block, uint32_t M, uint32_t top_mask, uint64_t total_steps, BlockShared &sh,
                                                 uint32_t &parity, ScanRes &r, uint32_t &excl, uint32_t &total_cnt)
{
    // rem_block = M - S_block % M, the steps left in the current permutation (callers carry it along: a
    // 64-bit modulo per block by every wavefront costs more than a fifth of the block)
    constexpr int NW = SCAN_THREADS / 64;
    static_assert(NW <= 16, "the wavefront counts are combined inside one row of 16 lanes");
    const uint32_t tau = threadIdx.x, lane = tau & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tau >> 6));
    const uint64_t left = total_steps - S_block;
    const uint32_t limit = left > 0xffffffffULL ? 0xffffffffu : (uint32_t)left;
    // first guess of the entering count: the expected count (any guess converges; a good one saves rounds)
    scan_thread(u, expected_steps(rem_block, (float)(tau * SCAN_D), M), rem_block, M, top_mask, limit, r);
    excl = 0; total_cnt = 0;
    uint32_t recomputed = 1u;
    uint32_t incl = 0;
    for (int iter = 0;; ++iter) {
        if (recomputed) incl = wave_inclusive_scan(r.cnt);   // (wavefront-uniform: a wavefront that re-evaluated nothing keeps its sums)
        if (lane == 63) sh.wsum[parity][wave] = incl | (recomputed << 31);
        __syncthreads();
        const uint32_t mine = lane < NW ? sh.wsum[parity][lane] : 0u;
        parity ^= 1u;   // the other buffer is rewritten only after the next barrier, i.e. after everybody has read this one
        const bool anybody = __any((int)(mine >> 31));
        const uint32_t run = row16_inclusive_scan(mine & 0x7fffffffu);
        total_cnt = (uint32_t)__builtin_amdgcn_readlane((int)run, NW - 1);
        const uint32_t before = wave ? (uint32_t)__builtin_amdgcn_readlane((int)run, wave - 1) : 0u;
        excl = before + incl - r.cnt;
        if (!anybody) return 0;   // the counts are those of the previous round, in which every cached result was valid
        const bool stale = !scan_still_valid(r, excl, M, limit);
        recomputed = __ballot(stale) ? 1u : 0u;
        if (recomputed) {
            if (stale) scan_thread(u, excl, rem_block, M, top_mask, limit, r);
        }
        if (iter > SCAN_THREADS + 8) return 1;
    }
}

// steps left in the current permutation after t more steps
__device__ __forceinline__ uint32_t rem_advance(uint32_t rem, uint32_t t, uint32_t M)
{
    if (t >= rem) { t = (t - rem) % M; rem = M; }
    return rem - t;
}
#endif

// One numpy-exact permutation job on the device (sc_permgen.hip, sc_swaps.hip): begin -> {scan, swap} per chunk
// of permutations -> finish.  Scan state lives on the device so chunks chain without host syncs.
struct PermJob {
    int64_t n = 0, n_perm = 0;
    uint64_t h = 0;            // 1 if the generator starts with a buffered 32-bit half
    uint64_t st_hi = 0, st_lo = 0, inc_hi = 0, inc_lo = 0;
    uint32_t buffered = 0;
    uint64_t total_steps = 0;
    uint64_t hi = 0;           // raw indices [0, hi) hold stream draws
    bool trivial = false;      // n == 1
    double draws_per_perm = 0; // expectation
    int64_t p_done = 0;        // permutations covered by the scan launches so far
    int64_t chunk_no = 0;
    bool phi = false;          // block-parallel scan in use
    uint64_t B_done = 0;       // blocks covered by the chain launches so far
    uint64_t unit_start[8] = {};  // first block of the last launch units (ring)
    int64_t unit_no = 0;
    int64_t gate_seen[4] = {};   // per preparation stream: the "units completed by the chain" count its last gate waited for
    int units_ahead = 1;       // launch units prepared ahead of the chain
};
// A generator job whose chunks are (being) enqueued on the generator's streams while the consumer catches up.
struct PermPipe {
    PermJob job;
    std::vector<int64_t> bounds;       // chunk k = permutations [bounds[k], bounds[k + 1])
    std::vector<hipEvent_t> ev;        // per chunk: scanned, swapped
    int table = 0;                     // 0 rows, 1 inverse rows only, 2 both
    int64_t n = 0, n_perm = 0, enqueued = 0;   // generator chunks enqueued so far
    uint64_t state0[6] = {};           // the generator state the job started from (a sequential rerun starts there again)
};
#define SC_PERMGEN_RETRY 1000  // internal: the block-parallel scan failed its verification, rerun sequentially
bool permgen_is_block_parallel(const sc_ctx *c, int64_t n);  // (sc_permgen_phi.hip) which scan form a job of length n takes
// Once per context (again after sc_ctx_set_permgen_mode), before the first block-parallel job and before the job takes
// any stream from the table: choose the placement of the context's streams -- plain, priority-spread or neither, ended
// by a probe -- and with it the scan form.  May destroy and re-create every stream of the context (all idle: it waits
// for the device first), so no stream handle taken before the call may be used after it.  chain_role: where this job's
// chain will run (SR_CHAIN in a pipeline, SR_SCORE for a short job on the context stream).
int permgen_place_streams(sc_ctx *c, int chain_role);
// units_ahead: launch units the block-parallel scan's preparation runs ahead of its chain (clamped to [1, PHI_AHEAD_MAX])
int permgen_begin(sc_ctx *c, const uint64_t *state6, int64_t n, int64_t n_perm, int units_ahead, PermJob *job, hipStream_t s);
int permgen_scan_chunk(sc_ctx *c, PermJob *job, int64_t p1, hipStream_t s, hipStream_t post, hipEvent_t done);
int permgen_swap_chunk(sc_ctx *c, PermJob *job, int64_t p0, int64_t p1, hipStream_t s, bool inverse, int pw_req);
bool permgen_can_swap_inverse(int64_t n);
int permgen_finish(sc_ctx *c, PermJob *job, uint64_t *state6);
// ---- the block-parallel form's share of a job (sc_permgen_phi.hip); phi_begin: the form (placed and probed by the caller), buffers, hand-over words
int phi_begin(sc_ctx *c, PermJob *job, int units_ahead, uint64_t n_blocks, hipStream_t s);
// the *blocks granted to permutations [0, p1): prepared on the preparation streams (*fill_streams: those the verification waits for)
// and chained by ONE launch on s; then, on sp, the verification of the chunk
int phi_chain_chunk(sc_ctx *c, PermJob *job, int64_t p1, hipStream_t s, uint64_t *blocks, unsigned *fill_streams);
int phi_verify_chunk(sc_ctx *c, PermJob *job, const unsigned long long *range, uint64_t blocks, unsigned fill_streams, hipStream_t sp);
// stage B (sc_swaps.hip): rows [p0, p1) of `table` from c->pg.J with the kernel for (n, inverse, permutations per workgroup, whole rounds)
int swaps_launch(sc_ctx *c, int32_t *table, int64_t n, int64_t p0, int64_t p1, bool inverse, int pw, bool full_rounds, hipStream_t s);
