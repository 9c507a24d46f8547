// A1 of the numpy-exact permutation generator (sc_permgen.hip), block-parallel form.  gfx950 only.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "sc_permgen.h"

// ------------------------------------------------------------------------------------------------
// A1 block-parallel: the same exact scan with the per-block work spread over the chip
//
// The only thing block b needs from its predecessors is ONE number, the state S_b (completed steps) it
// is entered with.  S_b is known in advance up to a random-walk error (sigma ~ 0.5 sqrt(draws) since the
// last exactly known state), so the chip prepares every block of a unit in parallel for a WINDOW of
// entry states around a guess G_b (k_phi_events + k_phi_tbuild), a single workgroup then chains the exact states through
// the prepared blocks (k_chain), and the chip finally recomputes every block from its now known exact
// entry state and checks S_b + count_b == S_{b+1} (k_block_exact): the result is exact by induction or
// a failure flag is raised (then the caller reruns the sequential form).
//
// Preparation of block b ("gap transfer").  Let the BASE trajectory enter with G_b and a second one with
// G_b + g (gap g, |g| <= w).  As long as both stay inside one permutation and one mask band, a draw with
// masked value v at a position where the base threshold is t is decided differently only when
//   g > 0 (second is ahead, its threshold is t - g):  base accepts, second rejects  <=>  g > t - v       (>= 0)
//   g < 0 (second is behind, threshold t + |g|):      base rejects, second accepts  <=>  |g| > v - t - 1 (>= 0)
// and each such event shrinks |g| by one.  The map entry gap -> exit gap is therefore monotone with unit
// steps, and it is represented per side by the set of increments d-1 -> d that survive: start with w set
// bits, and for every event of slack s (in draw order) clear the set bit of rank s if it exists.  The exit
// gap of entry gap d is the number of set bits among the first d.  Blocks in which some trajectory of the
// window crosses a mask band, a permutation end or the job end ("hard" blocks, about a fifth at n = 1M),
// or that hold too many events, are not prepared; the chain workgroup computes them itself from the exact
// entry state, exactly like the sequential scan.
// ------------------------------------------------------------------------------------------------

#define PHI_W 16384               // window bits per side
#define PHI_WORDS (PHI_W / 64)
#define PHI_MAX_EV 2048           // events per side a prepared block may hold
#define PHI_WINDOW 2.25           // window half-width in units of sqrt(draws since the reference state) (= 4.5 sigma)
#define PHI_UNIT 512              // blocks per launch unit (the chain pays ~0.17 ms between launches; with 32-draw
                                  // threads: 80 -> 842, 112 -> 900, 160 -> 1017, 224 -> 1024, 320 -> 1020-1033 genes/s in
                                  // the pipeline; with 16-draw threads: 384 -> 1068, 448 -> 1067, 512 -> 1071)
#define PHI_AHEAD_MAX 3
                                  // units prepared ahead of the chain (their guesses use a state ahead + 1 units old):
                                  // 1 when the generator has the chip to itself, 3 next to the scoring kernel, whose
                                  // workgroups hold the CUs for milliseconds (wider windows, ~25 % more computed blocks)
#define PHI_RING 4096
                                // table ring slots: EIGHT units.  Units are cut at chunk ends, so a short unit shifts the ring
                                  // positions of its successors, and unit v + 5 can then land on slots of unit v.  The chain is
                                  // done with unit v by then (k_gate), but k_seg_fill(v) -- which runs behind the chain on stream
                                  // v % 4 -- need not be: with four units of slots, a fill starved of compute units for a
                                  // millisecond read descriptors that unit v + 5's preparation had overwritten (seen as a
                                  // verification fallback when the scoring kernel left 64 or 32 CUs).  With eight, the first
                                  // unit on ANOTHER stream that can reach v's slots is v + 9, whose gate (chain done with unit
                                  // >= v + 5) implies publish(v + 4), which sits behind fill(v) in stream v % 4.
#define PHI_STREAMS 4             // preparation streams (units rotate over them)
#define PHI_MIN_N (1 << 17)       // below this every block holds a band crossing: sequential form

static_assert((PHI_AHEAD_MAX + 1) * PHI_UNIT <= PHI_RING, "a unit's ring slots are reused only after the chain consumed them");

struct PhiDesc {
    unsigned long long G;  // guessed entry state of the block
    uint32_t cnt;          // accepts of the base trajectory
    uint32_t i_in;         // steps left in G's permutation (M - G % M)
    uint16_t w_pos;        // entry states G + d, 0 <= d <= w_pos, are covered (trajectories ahead of the base)
    uint16_t w_neg;        // entry states G - d, 0 <= d <= w_neg, are covered (trajectories behind the base)
    uint16_t n_pos, n_neg; // events per side
    uint32_t prepared;     // 0: the chain computes this block itself
    uint32_t w;            // the window the block was prepared for (w_pos / w_neg are smaller next to a band edge)
};

// Expected state after dq more draws from state S (mean-field, closed form per mask band).  Only a guess:
// exactness never depends on it.
__device__ static unsigned long long phi_expect(unsigned long long S, double dq, uint32_t M, double dpp,
                                                unsigned long long total)
{
    int phase = 0;
    for (int guard = 0; guard < 256 && dq > 0.0 && S < total; ++guard) {
        const uint32_t done = (uint32_t)(S % M);
        if (done == 0 && phase == 0) {  // at a permutation boundary: skip whole permutations
            const double k = floor(dq / dpp);
            if (k >= 1.0) { S += (unsigned long long)k * M; dq -= k * dpp; }
            phase = 1;
            continue;
        }
        const uint32_t i = M - done, m = mask_of(i), lo = (m >> 1) + 1;  // band: i in [lo, m]
        const double top = (double)m + 1.0;
        const double need = top * log(((double)i + 1.0) / (double)lo);  // draws to leave the band
        if (need <= dq) { dq -= need; S += (unsigned long long)(i - lo + 1); }
        else { const double inew = ((double)i + 1.0) * exp(-dq / top) - 1.0; S += (unsigned long long)((double)i - inew + 0.5); dq = 0.0; }
    }
    return S < total ? S : total;
}

// One wavefront builds the surviving-increment bitset of one side (lane l holds bits [256 l, 256 l + 256)).
__device__ __forceinline__ void phi_tbuild(const uint16_t *ev, uint32_t nev, uint32_t w, unsigned long long *out)
{
    const uint32_t lane = threadIdx.x & 63;
    uint64_t w0, w1, w2, w3;
    {
        const uint32_t base = 256 * lane;
#define PHI_INIT(k) (w > base + 64 * (k) ? sc_low_mask64(w - base - 64 * (k) < 64u ? w - base - 64 * (k) : 64u) : 0ull)
        w0 = PHI_INIT(0); w1 = PHI_INIT(1); w2 = PHI_INIT(2); w3 = PHI_INIT(3);
#undef PHI_INIT
    }
    uint32_t cnt = (uint32_t)(__popcll(w0) + __popcll(w1) + __popcll(w2) + __popcll(w3));
    uint32_t pre = wave_inclusive_scan(cnt);
    uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)pre, 63);
    for (uint32_t e0 = 0; e0 < nev; e0 += 64) {
        const uint32_t mine = e0 + lane < nev ? ev[e0 + lane] : 0xffffu;  // 64 events per (coalesced) load
        const uint32_t nb = nev - e0 < 64 ? nev - e0 : 64;
        for (uint32_t j = 0; j < nb; ++j) {
            const uint32_t s = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)j);
            if (s >= total) continue;  // no trajectory of the window has a gap above s any more
            const bool own = (pre - cnt <= s) && (s < pre);
            const uint32_t L = (uint32_t)__builtin_ctzll(__ballot(own));
            if (lane == L) {
                uint32_t r = s - (pre - cnt);
                const uint32_t c0 = (uint32_t)__popcll(w0), c1 = (uint32_t)__popcll(w1), c2 = (uint32_t)__popcll(w2);
                if (r < c0) w0 &= ~sc_bit64(select64(w0, r));
                else if (r < c0 + c1) w1 &= ~sc_bit64(select64(w1, r - c0));
                else if (r < c0 + c1 + c2) w2 &= ~sc_bit64(select64(w2, r - c0 - c1));
                else w3 &= ~sc_bit64(select64(w3, r - c0 - c1 - c2));
                cnt -= 1;
            }
            pre -= (lane >= L) ? 1u : 0u;
            total -= 1;
        }
    }
    ulonglong2 *o = reinterpret_cast<ulonglong2 *>(out + 4 * lane);
    o[0] = make_ulonglong2(w0, w1);
    o[1] = make_ulonglong2(w2, w3);
}

// exit gap of entry gap idx (<= w) on one side: set bits among the first idx (wave 0 only, all lanes)
__device__ __forceinline__ uint32_t phi_lookup(const unsigned long long *tb, uint32_t idx)
{
    const uint32_t lane = threadIdx.x & 63, base = 256 * lane;
    uint32_t t = 0;
    if (idx > base) {
        const ulonglong2 *src = reinterpret_cast<const ulonglong2 *>(tb + 4 * lane);
        const ulonglong2 a = src[0], b = src[1];
        const uint64_t wd[4] = {a.x, a.y, b.x, b.y};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t lo = base + 64 * k;
            if (idx > lo) t += (uint32_t)__popcll(wd[k] & sc_low_mask64(idx - lo < 64u ? idx - lo : 64u));
        }
    }
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_scan(t), 63);
}

// Prepare blocks [b0, b1), part 1: one workgroup per block finds the base trajectory from the guess G_b and
// writes the events of both sides (slacks, in draw order).  The guess comes from the exact state at ref_block
// (ahead + 1 units back), the window from the distance to it.
__global__ __launch_bounds__(SCAN_THREADS) void k_phi_events(const uint32_t *__restrict__ raw, uint32_t n,
                                                             uint64_t total_steps, double dpp, uint64_t b0,
                                                             uint64_t b1, uint64_t ref_block,
                                                             const unsigned long long *__restrict__ sblk,
                                                             PhiDesc *__restrict__ desc,
                                                             uint16_t *__restrict__ events, uint32_t *__restrict__ seglist)
{
    __shared__ BlockShared sh;
    __shared__ unsigned long long shG;
    __shared__ uint32_t shw, shi;
    __shared__ uint32_t wpk[SCAN_THREADS / 64];
    const uint64_t b = b0 + blockIdx.x;
    if (b >= b1) return;
    const uint32_t tau = threadIdx.x, lane = tau & 63, wave = tau >> 6;
    const uint32_t M = n - 1, top_mask = mask_of(M);
    const uint64_t slot = b % PHI_RING;
    if (blockIdx.x == 0 && tau == 0) seglist[0] = 0;   // the unit's list of multi-block segments (filled by k_phi_tbuild)
    if (tau == 0) {
        const double dq = (double)(b - ref_block) * (double)SCAN_BLOCK;
        shG = phi_expect(sblk[ref_block], dq, M, dpp, total_steps);
        // ~4.5 sigma of the random walk since the reference state (sigma = 0.49 sqrt(draws), measured); an entry
        // state outside the window only costs the chain one computed block
        const double wd = PHI_WINDOW * sqrt(dq) + 64.0;
        shw = wd < (double)(PHI_W - 1) ? (uint32_t)wd : (uint32_t)(PHI_W - 1);
        shi = M - (uint32_t)(shG % M);
    }
    uint32_t u[SCAN_D];
    scan_load(raw, b * SCAN_BLOCK, tau, u);
    __syncthreads();
    const uint64_t G = shG;
    const uint32_t w = shw;
    const uint32_t i_in = shi;
    bool easy = G + (uint64_t)SCAN_BLOCK + w + 1 < total_steps;
    if (i_in <= SCAN_BLOCK / 2) easy = false;  // the permutation ends inside the block (acceptance >= 1/2): the chain
                                               // computes it anyway, no need to solve it here first
    ScanRes r;
    uint32_t excl = 0, total_cnt = 0, parity = 0;
    uint32_t mask = 0, w_pos = 0, w_neg = 0;
    if (easy) {  // uniform
        if (block_fixed_point(u, G, i_in, M, top_mask, total_steps, sh, parity, r, excl, total_cnt) > 0) easy = false;
        mask = mask_of(i_in);
        const uint32_t cap = mask < M ? mask : M, low = (mask >> 1) + 1;  // the band is [low, mask], capped by M
        // The base must stay in its band and permutation.  A trajectory that enters d ahead of it stays at
        // thresholds >= i_out - d, one that enters d behind at thresholds <= i_in + d: each side is covered as
        // far as its trajectories cannot leave the band either.
        if (i_in < total_cnt + low) easy = false;
        else {
            const uint32_t i_out = i_in - total_cnt;
            w_pos = w < i_out - low ? w : i_out - low;
            w_neg = w < cap - i_in ? w : cap - i_in;
        }
    }
    uint32_t totP = 0, totN = 0, offP = 0, offN = 0;
    if (easy) {
        uint32_t thr = i_in - excl, np = 0, nn = 0;
#pragma unroll
        for (int s = 0; s < SCAN_D; ++s) {
            const int32_t d = (int32_t)(thr - (u[s] & mask));
            if (d >= 0) { np += ((uint32_t)d < w_pos) ? 1u : 0u; --thr; }
            else nn += ((uint32_t)(-d - 1) < w_neg) ? 1u : 0u;
        }
        const uint32_t pk = np | (nn << 16);  // both totals <= SCAN_BLOCK <= 65535: no carry between the fields
        const uint32_t incl = wave_inclusive_scan(pk);
        if (lane == 63) wpk[wave] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < SCAN_THREADS / 64; ++k) {
            const uint32_t t = wpk[k];
            before += (k < (int)wave) ? t : 0u;
            all += t;
        }
        const uint32_t ex = before + incl - pk;
        offP = ex & 0xffffu; offN = ex >> 16;
        totP = all & 0xffffu; totN = all >> 16;
        if (totP > PHI_MAX_EV || totN > PHI_MAX_EV) easy = false;
    }
    PhiDesc d;
    d.G = G; d.cnt = total_cnt; d.i_in = i_in; d.w = w;
    d.w_pos = (uint16_t)w_pos; d.w_neg = (uint16_t)w_neg; d.n_pos = (uint16_t)totP; d.n_neg = (uint16_t)totN;
    d.prepared = easy ? 1u : 0u;
    if (tau == 0) desc[slot] = d;
    if (!easy) return;
    uint16_t *evP = events + (slot * 2 + 0) * PHI_MAX_EV, *evN = events + (slot * 2 + 1) * PHI_MAX_EV;
    uint32_t thr = i_in - excl;
#pragma unroll
    for (int s = 0; s < SCAN_D; ++s) {
        const int32_t dd = (int32_t)(thr - (u[s] & mask));
        if (dd >= 0) { if ((uint32_t)dd < w_pos) evP[offP++] = (uint16_t)dd; --thr; }
        else if ((uint32_t)(-dd - 1) < w_neg) evN[offN++] = (uint16_t)(-dd - 1);
    }
}

#define PHI_SEG_MAX 16        // blocks per segment at most (segments are cut at multiples of this inside a unit)
#define PHI_COMPOSE_WGS (PHI_UNIT / 2)   // workgroups of k_phi_compose: one per multi-block segment, the others leave at once
#define PHI_NS 6              // segments whose tables the chain stages in LDS at once (a run of prepared blocks)
#define PHI_STAGE_PIECES 64   // 16-byte pieces per side the chain stages: entry gaps up to 8192 (beyond: global memory)

struct PhiSeg {               // one per ring slot, written by k_phi_compose
    unsigned long long G;     // guessed entry state of the segment's first block
    int32_t exit0;            // exit state of the segment for entry state G, relative to G
    uint32_t i_in;            // steps left in G's permutation
    uint16_t vpos, vneg;      // entry states G - vneg .. G + vpos are covered
    uint8_t kind;             // 0: the chain computes this block itself, 1: first block of a segment, 2: inside one
    uint8_t len;              // kind 1: blocks in the segment
    uint8_t own;              // kind 1: the segment's table is the block's own (tbits), else the composed one (ctbits)
    uint8_t bad;              // kind 1: the composition left the windows even for the base trajectory (never seen): no lookup
};
static_assert(sizeof(PhiSeg) == 24, "PhiSeg layout");

__device__ __forceinline__ bool phi_full(const PhiDesc &d) { return d.prepared && d.w_pos == d.w && d.w_neg == d.w; }

// set bits among the first nbit (1 .. 128) bits of a 16-byte piece (32-bit masks only, see xsl_rr32)
__device__ __forceinline__ uint32_t phi_piece_rank(const ulonglong2 a, uint32_t nbit)
{
    const uint32_t wd[4] = {(uint32_t)a.x, (uint32_t)(a.x >> 32), (uint32_t)a.y, (uint32_t)(a.y >> 32)};
    uint32_t T = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t lo = 32u * j;
        const uint32_t m = nbit >= lo + 32u ? 0xffffffffu : (nbit > lo ? ((1u << ((nbit - lo) & 31u)) - 1u) : 0u);
        T += (uint32_t)__popc(wd[j] & m);
    }
    return T;
}

// Which segment a prepared block belongs to (r04, see "SEGMENTS" below): a function of the descriptors of the block, its
// predecessor and its successors alone, so every block classifies ITSELF (thread 0 of its k_phi_tbuild workgroup) and the
// first block of a segment of more than one block enters the unit's list for k_phi_compose.
__device__ __forceinline__ void phi_classify(uint64_t b0, uint64_t b1, uint64_t b, const PhiDesc *__restrict__ desc,
                                             PhiSeg *__restrict__ seg, uint32_t *__restrict__ seglist)
{
    const uint32_t r = (uint32_t)(b - b0), nb = (uint32_t)(b1 - b0);
    const uint64_t slot = b % PHI_RING;
    const PhiDesc cur = desc[slot];
    PhiSeg s;
    s.G = cur.G; s.exit0 = (int32_t)cur.cnt; s.i_in = cur.i_in; s.vpos = cur.w_pos; s.vneg = cur.w_neg;
    s.kind = 0; s.len = 0; s.own = 1; s.bad = 0;
    if (cur.prepared) {
        bool start = r == 0 || (r % PHI_SEG_MAX) == 0 || !phi_full(cur);
        if (!start) start = !phi_full(desc[(b - 1) % PHI_RING]);
        if (!start) s.kind = 2;
        else {
            uint32_t len = 1;
            if (phi_full(cur))
                while (r + len < nb && ((r + len) % PHI_SEG_MAX) != 0 && phi_full(desc[(b + len) % PHI_RING])) ++len;
            s.kind = 1; s.len = (uint8_t)len;
            if (len > 1) {   // its table is composed by k_phi_compose (which completes this descriptor); until then: unusable
                s.bad = 1;
                seglist[1 + atomicAdd(seglist, 1u)] = r;
            }
        }
    }
    seg[slot] = s;
}

// Prepare blocks [b0, b1), part 2: two wavefronts per block turn the event lists into the gap-transfer tables.
__global__ __launch_bounds__(128) void k_phi_tbuild(uint64_t b0, uint64_t b1, const PhiDesc *__restrict__ desc,
                                                    const uint16_t *__restrict__ events,
                                                    unsigned long long *__restrict__ tbits, PhiSeg *__restrict__ seg,
                                                    uint32_t *__restrict__ seglist)
{
    const uint64_t b = b0 + blockIdx.x;
    if (b >= b1) return;
    const uint64_t slot = b % PHI_RING;
    if (threadIdx.x == 64) phi_classify(b0, b1, b, desc, seg, seglist);   // (the second wavefront's first lane; descriptors only)
    const PhiDesc d = desc[slot];
    if (!d.prepared) return;
    const uint32_t side = threadIdx.x >> 6;
    phi_tbuild(events + (slot * 2 + side) * PHI_MAX_EV, side ? d.n_neg : d.n_pos, side ? d.w_neg : d.w_pos,
               tbits + (slot * 2 + side) * PHI_WORDS);
}

// ------------------------------------------------------------------------------------------------
// Hand-over words between the chain workgroup and the preparation launches (r02).
//
// r01 ordered "preparation of unit u -> chain of unit u -> preparation of unit u + ahead + 1" with events: one chain
// launch per unit, a barrier packet in front of it and a marker behind it -- 0.21 ms of idle chain stream per unit
// (37 of 232 ms per bench step).  Now ONE chain launch runs a whole chunk of permutations and both directions are words
// in device memory:  flags[1 + u % 16] = u + 1 once unit u is prepared (k_publish, behind the unit's preparation
// launches in their stream), flags[0] = number of units the chain has completed (k_chain, after each unit; the
// preparation of unit u starts behind k_gate, one wavefront that waits for flags[0] >= u - ahead).
// Every wait gives up after 1 s or when a failure flag is up (e.g. when the streams do not run concurrently: a
// profiler that serialises kernels, fewer hardware queues than streams) and raises flag 8 / 16: the caller then
// reruns the job with the sequential scan, as after a failed verification.
// ------------------------------------------------------------------------------------------------
#define PHI_FLAG_SLOTS 16
#define PHI_WAIT_TICKS 100000000ll    // 1 s of the 100 MHz wall clock; a wait is for ONE launch unit (512 blocks, ~1 ms of work at any n)

// 0: the word arrived; 1: gave up waiting (the caller raises its flag); 2: abandoned, a failure flag is up already
__device__ __forceinline__ int phi_wait_at_least(const uint32_t *flag, uint32_t want, const unsigned long long *st)
{
    const long long t0 = wall_clock64();
    for (uint32_t spins = 0;; ++spins) {
        if (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= want) return 0;
        if (__hip_atomic_load(st + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) return 2;
        if (wall_clock64() - t0 > PHI_WAIT_TICKS || spins > (1u << 28)) return 1;
        __builtin_amdgcn_s_sleep(16);
    }
}

__global__ void k_publish(uint32_t *flags, uint32_t slot, uint32_t value)
{
    if (threadIdx.x == 0) __hip_atomic_store(flags + slot, value, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void k_gate(const uint32_t *flags, uint32_t chain_units_needed, unsigned long long *st)
{
    if (threadIdx.x == 0 && phi_wait_at_least(flags, chain_units_needed, st) == 1) atomicOr(st + 2, 16ull);
}

// Can the generator's streams run concurrently?  The hand-over words need the chain's stream and the four preparation
// streams on different hardware queues (GPU_MAX_HW_QUEUES; a profiler that serialises kernels breaks it too).  Probed
// ONCE per context, before the first block-parallel job, instead of finding out through a one-second give-up inside a
// job: in five rounds each stream in turn hosts a setter kernel that is enqueued LAST, behind waiters on the other four;
// two streams that share a queue deadlock in the round where the waiter of the pair sits in front of the setter, and
// that waiter gives up after 20 ms.
__global__ void k_probe_wait(const uint32_t *flag, uint32_t want, uint32_t *timed_out)
{
    if (threadIdx.x != 0) return;
    const long long t0 = wall_clock64();
    while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < want) {
        if (wall_clock64() - t0 > 2000000ll) { atomicOr(timed_out, 1u); return; }   // 20 ms
        __builtin_amdgcn_s_sleep(8);
    }
}

// ------------------------------------------------------------------------------------------------
// r04: SEGMENTS -- the gap-transfer tables of consecutive prepared blocks composed into one.
//
// r03's clock profile of the chain: 22 % of its time were the table lookups of the prepared blocks (815 clocks per
// block, 75 blocks per permutation of 1M cells), although the tables of a run of prepared blocks are all known before
// the chain gets there.  The map entry gap -> exit gap of one block is monotone with unit steps, and so is a
// composition of such maps (with the constant shifts G_j + cnt_j - G_{j+1} between the blocks' guesses in between):
// the composition is again a bitset of surviving increments.  k_phi_compose builds it on the chip, one workgroup per
// SEGMENT (<= PHI_SEG_MAX consecutive prepared blocks whose windows are not narrowed by a band edge; a block with a
// narrowed window is a segment of its own and keeps its own table), by pushing every entry state of the window through
// the segment's tables.  The chain then pays ONE lookup per segment (every thread evaluates it redundantly from LDS: no
// hand-over between wavefronts), k_seg_fill -- one wavefront per segment, behind the chain's "unit done" word --
// fills in the entry states of the blocks inside the segments from the per-block tables, and k_block_exact verifies all
// of it exactly as before: the composed table of a segment is right or its last block's exit state does not meet the
// chain's.
// ------------------------------------------------------------------------------------------------
// Prepare blocks [b0, b1), part 3: segments.  One workgroup per block; the workgroup of a segment's first block
// composes the segment's table, the others only classify their block.
__device__ __forceinline__ void phi_compose_block(uint64_t b0, uint32_t r, const PhiDesc *__restrict__ desc,
                                                  const unsigned long long *__restrict__ tbits, PhiSeg *__restrict__ seg,
                                                  unsigned long long *__restrict__ ctbits)
{
    static_assert(SCAN_THREADS == 1024 && PHI_W == 16384, "thread t of a side owns entry gaps 32 t .. 32 t + 32");
    __shared__ ulonglong2 tl[2 * 128];      // the current block's tables: [side][128 pieces]
    __shared__ uint32_t tpre[2 * 128];      // set bits in front of each piece inside its wavefront's 64 pieces
    __shared__ uint32_t wtot[4];            // set bits of pieces 0 .. 63 / 64 .. 127 of each side
    __shared__ uint32_t Uw[2 * PHI_W / 32]; // the block's increments on the signed gap axis: bit PHI_W + d = F(d + 1) - F(d)
    __shared__ int32_t shLoT, shHiT, shE0;  // first thread of each side that dropped out; exit state of the base
    const uint64_t b = b0 + r;
    const uint32_t tau = threadIdx.x;
    const uint64_t slot = b % PHI_RING;
    const PhiDesc cur = desc[slot];
    PhiSeg s = seg[slot];                   // kind 1, len > 1 (phi_classify)
    const uint32_t len = s.len;
    __syncthreads();                        // (the shared cells below are reused from the workgroup's previous segment)

    // ---- compose: every entry state of the window through the segment's tables ----
    // Thread (side, t) owns the 33 entry gaps 32 t .. 32 t + 32 of its side, held ASCENDING on the signed state axis
    // (negative side: st[k] belongs to the gap -(32 t + 32 - k)).  The images of neighbouring states differ by 0 or 1
    // (monotone, unit steps), so a block maps the thread's states with ONE rank lookup (its lowest state) and one bit of
    // the block's increment array U per further state:  F(a + 1) - F(a) = U[a - G_j],  U = the negative side's bits
    // reversed, then the positive side's.  A thread whose states are not all inside a block's window drops out; the
    // segment then covers the gaps below that thread (the window's rim, 4.5 sigma out: nothing is lost).
    const uint32_t side = tau >> 9, t = tau & 511u;
    int32_t st[33];
#pragma unroll
    for (int k = 0; k <= 32; ++k) st[k] = side ? -(int32_t)(32u * t + 32u - k) : (int32_t)(32u * t + k);
    bool ok = true;
    if (tau == 0) { shLoT = 512; shHiT = 512; }
    const ulonglong2 *tb2 = reinterpret_cast<const ulonglong2 *>(tbits);
    // the tables and the descriptor of block j + 1 are on their way (registers) while block j is applied: a step is
    // then its ~360 instructions per thread, not those plus two dependent trips to memory (inside the Moran pipeline,
    // next to 6 TB/s of scoring traffic, such a trip takes several microseconds)
    ulonglong2 vnext = make_ulonglong2(0ull, 0ull);
    unsigned long long nG = cur.G;      // (only the three fields a step needs travel ahead: the whole descriptor spilled)
    uint32_t ncnt = cur.cnt, nw = cur.w;
    if (tau < 256) vnext = tb2[((slot * 2 + (tau >> 7)) * PHI_WORDS) / 2 + (tau & 127u)];
    for (uint32_t j = 0; j < len; ++j) {
        const unsigned long long djG = nG;
        const uint32_t djcnt = ncnt, djw = nw;
        const ulonglong2 v = vnext;
        __syncthreads();     // the previous block's lookups are done (and shLoT / shHiT are set)
        if (tau < 256) {     // piece (tau & 127) of side (tau >> 7); a wavefront's 64 pieces are half a side
            const uint32_t piece = tau & 127u;
            const uint32_t ones = (uint32_t)(__popcll(v.x) + __popcll(v.y));
            const uint32_t upto = wave_inclusive_scan(ones);
            tl[tau] = v;
            tpre[tau] = upto - ones;
            if ((tau & 63u) == 63u) wtot[tau >> 6] = upto;
            const uint32_t wd[4] = {(uint32_t)v.x, (uint32_t)(v.x >> 32), (uint32_t)v.y, (uint32_t)(v.y >> 32)};
            if (tau < 128) {   // positive side: bit i of the side is U position PHI_W + i
#pragma unroll
                for (int m = 0; m < 4; ++m) Uw[PHI_W / 32 + 4 * piece + m] = wd[m];
            } else {           // negative side: bit i is U position PHI_W - 1 - i
#pragma unroll
                for (int m = 0; m < 4; ++m) Uw[PHI_W / 32 - 4 * piece - 1 - m] = __brev(wd[m]);
            }
        }
        if (j + 1 < len) {
            const uint64_t sn = (b + j + 1) % PHI_RING;
            nG = desc[sn].G; ncnt = desc[sn].cnt; nw = desc[sn].w;
            if (tau < 256) vnext = tb2[((sn * 2 + (tau >> 7)) * PHI_WORDS) / 2 + (tau & 127u)];
        }
        __syncthreads();
        const int32_t rel = (int32_t)(int64_t)(djG - cur.G);   // this block's guess, relative to the first one's
        const int32_t wj = (int32_t)djw;
        if (ok && (st[0] - rel < -wj || st[32] - rel > wj)) {   // (also: gaps beyond the first block's own window)
            ok = false;
            atomicMin(side ? &shLoT : &shHiT, (int32_t)t);
        }
        if (ok) {
            const int32_t d0 = st[0] - rel;
            const bool neg = d0 < 0;
            const uint32_t idx = (uint32_t)(neg ? -d0 : d0);
            uint32_t T = 0;
            if (idx) {
                const uint32_t piece = (idx - 1u) >> 7, nbit = idx - 128u * piece;
                const uint32_t row = (neg ? 128u : 0u) + piece;
                T = tpre[row] + (piece >= 64u ? wtot[neg ? 2 : 0] : 0u) + phi_piece_rank(tl[row], nbit);
            }
            int32_t run = rel + (int32_t)djcnt + (neg ? -(int32_t)T : (int32_t)T);
#pragma unroll
            for (int k = 0; k < 32; ++k) {
                const int32_t inc = st[k + 1] - st[k];                       // 0 or 1
                const uint32_t q = (uint32_t)(PHI_W + st[k] - rel);          // U position of the step st[k] -> st[k] + 1
                const uint32_t bit = (Uw[q >> 5] >> (q & 31u)) & 1u;
                st[k] = run;
                run += inc & (int32_t)bit;
            }
            st[32] = run;
        }
    }
    if (t == 0 && side == 0) shE0 = ok ? st[0] : (int32_t)0x80000000;
    __syncthreads();
    // surviving increments: positive side bit p = exit(p + 1) - exit(p); negative side bit p = exit(-p) - exit(-p - 1)
    uint32_t word = 0;
    if (ok) {
#pragma unroll
        for (int k = 0; k < 32; ++k)
            if (st[k + 1] != st[k]) word |= 1u << (side ? 31 - k : k);
    }
    reinterpret_cast<uint32_t *>(ctbits + (slot * 2 + side) * PHI_WORDS)[t] = word;
    if (tau == 0) {
        const int32_t hiT = shHiT, loT = shLoT, e0 = shE0;
        s.own = 0;
        s.bad = 0;
        if (e0 == (int32_t)0x80000000 || hiT == 0 || loT == 0) { s.bad = 1; s.vpos = 0; s.vneg = 0; }
        else {
            const uint32_t vp = 32u * (uint32_t)hiT, vn = 32u * (uint32_t)loT;
            s.exit0 = e0;
            s.vpos = (uint16_t)(vp < cur.w ? vp : cur.w);
            s.vneg = (uint16_t)(vn < cur.w ? vn : cur.w);
        }
        seg[slot] = s;
    }
}

// (r04 measured and dropped: the unit published by the LAST workgroup of this kernel -- a device-scope release per
// workgroup, i.e. a write-back of the XCD's L2 512 times per unit: generator alone 119 -> 144 ms, bench step 167 -> 214 ms.
// The kernel boundary in front of k_publish does that once.  Also measured: one 1024-thread workgroup per BLOCK, all but
// the ~35 that start a multi-block segment leaving at once -- inside the Moran pipeline those 512 heavy workgroups queued
// for the 96 free CUs, the chain waited 34-40 k clocks per permutation for its units (3.4 k with the chip to itself).)
__global__ __launch_bounds__(SCAN_THREADS) void k_phi_compose(uint64_t b0, const PhiDesc *__restrict__ desc,
                                                             const unsigned long long *__restrict__ tbits,
                                                             PhiSeg *__restrict__ seg,
                                                             unsigned long long *__restrict__ ctbits,
                                                             const uint32_t *__restrict__ seglist)
{
    const uint32_t count = seglist[0];
    // (one segment per workgroup -- a segment has at least two blocks, so PHI_UNIT / 2 workgroups cover any unit; a loop
    // over segments here made hipcc spill 25 registers of the unrolled state arrays)
    if (blockIdx.x < count) phi_compose_block(b0, seglist[1 + blockIdx.x], desc, tbits, seg, ctbits);
}

// Entry states of the blocks inside the segments of blocks [b0, b1) that the chain resolved by ONE lookup (segmode 1):
// one wavefront per segment walks the per-block tables from the segment's entry state.  Runs behind the chain's
// "unit done" word; k_block_exact then verifies every block (the last one's exit state must meet the chain's).
__global__ __launch_bounds__(64) void k_seg_fill(uint64_t b0, uint64_t b1, const PhiDesc *__restrict__ desc,
                                                 const PhiSeg *__restrict__ seg,
                                                 const unsigned long long *__restrict__ tbits,
                                                 const uint8_t *__restrict__ segmode,
                                                 unsigned long long *__restrict__ sblk, uint8_t *__restrict__ hardmask,
                                                 unsigned long long *__restrict__ st)
{
    const uint64_t b = b0 + blockIdx.x;
    if (b >= b1 || segmode[b] != 1) return;
    const uint32_t len = seg[b % PHI_RING].len;
    const uint32_t lane = threadIdx.x;
    unsigned long long S = sblk[b];
    for (uint32_t j = 0; j < len; ++j) {
        const uint64_t slot = (b + j) % PHI_RING;
        const PhiDesc d = desc[slot];
        const int64_t g = (int64_t)S - (int64_t)d.G;
        const bool neg = g < 0;
        const uint64_t idx = (uint64_t)(neg ? -g : g);
        if (!d.prepared || idx > (neg ? d.w_neg : d.w_pos)) {   // the composed table said this could not happen
            if (lane == 0) atomicOr(st + 2, 32ull);
            return;
        }
        const uint32_t T = idx ? phi_lookup(tbits + (slot * 2 + (neg ? 1 : 0)) * PHI_WORDS, (uint32_t)idx) : 0u;
        if (lane == 0) { sblk[b + j] = S; hardmask[b + j] = 0; }
        S = d.G + d.cnt + (neg ? -(long long)T : (long long)T);
    }
}

// Chain the exact states through blocks [b0, b1) (one workgroup): a SEGMENT of prepared blocks costs one lookup in
// its (composed) table, which every thread evaluates for itself from LDS; the other blocks the full in-block fixed
// point.  While a block is computed, the draws of the next block to compute and the tables of the run of segments
// before it are already on their way (registers, then LDS).  Leaves sblk[b] for every block it computed and for the
// first block of every segment (k_seg_fill adds the blocks inside), hardmask[b], segmode[b] and the accept masks /
// entering counts of the blocks it computed itself.  fault != 0 (testing): corrupt one lookup.
__global__ __launch_bounds__(SCAN_THREADS) void k_chain(const uint32_t *__restrict__ raw, uint64_t n_blocks,
                                                        uint32_t n, uint64_t total_steps, uint64_t B0, uint64_t B1,
                                                        uint64_t S_need, const PhiDesc *__restrict__ desc,
                                                        const unsigned long long *__restrict__ tbits,
                                                        const PhiSeg *__restrict__ seg,
                                                        const unsigned long long *__restrict__ ctbits,
                                                        uint8_t *__restrict__ hardmask, uint8_t *__restrict__ segmode, int fault,
                                                        bits_t *__restrict__ acc_bits, uint32_t *__restrict__ enter,
                                                        unsigned long long *__restrict__ sblk,
                                                        unsigned long long *__restrict__ st, uint32_t *__restrict__ flags,
                                                        uint32_t unit0)
{
    __shared__ BlockShared sh;
    __shared__ uint32_t shReady;
    __shared__ __align__(8) PhiSeg sg[PHI_UNIT];
    __shared__ uint16_t nxt[PHI_UNIT + 2];  // first block >= i (relative to b0) the chain computes itself
    __shared__ ulonglong2 tl[PHI_NS * 2 * PHI_STAGE_PIECES];   // [staged segment][side][64 x 16 B]
    __shared__ uint32_t tpre[PHI_NS * 2 * PHI_STAGE_PIECES];   // set bits in front of each 16-byte piece of its row
    static_assert(PHI_NS * 2 * PHI_STAGE_PIECES <= SCAN_THREADS, "one 16-byte piece per thread");
    __shared__ unsigned long long shS;
    __shared__ uint32_t shRem, shRel;
    const uint32_t tau = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(tau >> 6));
    const uint32_t M = n - 1, top_mask = mask_of(M);
    uint64_t S = st[0];
    if (S >= total_steps || st[1] != B0 || B1 > n_blocks) {  // job complete, or an earlier launch gave up (uniform)
        if (tau == 0) __hip_atomic_store(flags, 0xffffffffu, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);  // no gate waits for us
        return;
    }
    uint32_t parity = 0;
    int failed = 0;
    __shared__ unsigned long long shEnd;   // (raw position of the job's last step, seen by at most one thread of one launch)
    if (tau == 0) shEnd = 0;
    // counters of thread 0 live in LDS (the kernel sits at its 128-VGPR cap): [0] blocks by lookup, [1] computed, [2] segment
    // lookups, [3] slow paths
    __shared__ uint32_t cn[7];   // ([4] .. [6] served the fresh-table variant and stay zero: the kernel's LDS layout is unchanged)
    if (tau < 7) cn[tau] = 0u;
    __syncthreads();
    uint32_t rem = M - (uint32_t)(S % M);  // steps left in the current permutation, carried along from here
    uint64_t b_next = B0;
    // one launch chains several launch units (each prepared by its own launches; the host waited for all of them)
    uint32_t unit = unit0;
    int gave_up = 0;
    const ulonglong2 *tb2 = reinterpret_cast<const ulonglong2 *>(tbits), *ctb2 = reinterpret_cast<const ulonglong2 *>(ctbits);
    for (uint64_t b0 = B0; b0 < B1 && !failed && S < total_steps; b0 += PHI_UNIT, ++unit) {
    const uint64_t b1 = b0 + PHI_UNIT < B1 ? b0 + PHI_UNIT : B1;
    const uint32_t nb = (uint32_t)(b1 - b0);
    __syncthreads();  // the previous unit's readers of sg / nxt / tl are done
    if (tau == 0) shReady = (uint32_t)phi_wait_at_least(flags + 1 + unit % PHI_FLAG_SLOTS, unit + 1, st);
    __syncthreads();
    if (shReady) { gave_up = (int)shReady; break; }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // the unit's descriptors and tables, written by other kernels
    if (tau < nb) sg[tau] = seg[(b0 + tau) % PHI_RING];
    __syncthreads();
    if (tau <= nb) {
        uint32_t j = tau;
        while (j < nb && sg[j].kind != 0) ++j;
        nxt[tau] = (uint16_t)j;
    }
    __syncthreads();
    // The tables of up to PHI_NS consecutive segments that start at relative block `first` (a run ends at the next block
    // the chain computes): thread = (staged segment q, side, piece) loads one 16-byte piece into treg.
#define PHI_STAGE_LOAD(first)                                                                              \
    {                                                                                                      \
        treg = make_ulonglong2(0ull, 0ull);                                                                \
        if (tau < PHI_NS * 2 * PHI_STAGE_PIECES) {                                                         \
            const uint32_t q = tau / (2 * PHI_STAGE_PIECES), sd = (tau / PHI_STAGE_PIECES) & 1u;           \
            uint32_t pos = (first);                                                                        \
            for (uint32_t k = 0; k < q && pos < nb && sg[pos].kind == 1; ++k) pos += sg[pos].len;          \
            if (pos < nb && sg[pos].kind == 1) {                                                           \
                const uint64_t slot = (b0 + pos) % PHI_RING;                                               \
                treg = (sg[pos].own ? tb2 : ctb2)[((slot * 2 + sd) * PHI_WORDS) / 2 + (tau % PHI_STAGE_PIECES)]; \
            }                                                                                              \
        }                                                                                                  \
    }
    ulonglong2 treg;
    uint32_t un[SCAN_D];
    uint32_t rel = 0, h = nxt[0];   // rel: next block to resolve; h: the next block the chain computes itself (>= rel)
    PHI_STAGE_LOAD(rel)
    if (h < nb) scan_load(raw, (b0 + h) * SCAN_BLOCK, tau, un);
    for (;;) {
        // (only wavefront 0 reads the staged tables, and it is behind the barrier that follows its lookups: no barrier here)
        {   // a wavefront's 64 pieces are one (segment, side) row
            const uint32_t ones = (uint32_t)(__popcll(treg.x) + __popcll(treg.y));
            const uint32_t upto = wave_inclusive_scan(ones);
            if (tau < PHI_NS * 2 * PHI_STAGE_PIECES) { tl[tau] = treg; tpre[tau] = upto - ones; }
        }
        __syncthreads();
        // ---- the staged segments, one lookup each, by wavefront 0 (sixteen wavefronts doing the same ~60 dependent
        // instructions take turns on the four SIMDs: four times the clocks of one) ----
        if (wave == 0) {
            bool miss0 = false;
            for (uint32_t q = 0; q < PHI_NS && rel < nb && sg[rel].kind == 1; ++q) {
                const PhiSeg sq = sg[rel];
                const int64_t g = (int64_t)S - (int64_t)sq.G;
                const bool neg = g < 0;
                const uint64_t idx = (uint64_t)(neg ? -g : g);
                if (sq.bad || idx > (neg ? sq.vneg : sq.vpos)) { miss0 = true; break; }   // outside the segment's window
                uint32_t T = 0;
                if (idx) {
                    if (idx <= 128u * PHI_STAGE_PIECES) {
                        const uint32_t piece = ((uint32_t)idx - 1u) >> 7, nbit = (uint32_t)idx - 128u * piece;
                        const uint32_t row = (q * 2 + (neg ? 1u : 0u)) * PHI_STAGE_PIECES + piece;
                        T = tpre[row] + phi_piece_rank(tl[row], nbit);
                    } else {   // beyond the staged bits (|gap| > 8192: ~3 sigma of the widest window)
                        const uint64_t slot = (b0 + rel) % PHI_RING;
                        T = phi_lookup((sq.own ? tbits : ctbits) + (slot * 2 + (neg ? 1 : 0)) * PHI_WORDS, (uint32_t)idx);
                    }
                }
                if (tau == 0) { sblk[b0 + rel] = S; segmode[b0 + rel] = 1; }
                int64_t e = (int64_t)sq.exit0 + (neg ? -(int64_t)T : (int64_t)T);
                if (fault && cn[0] == 0) e += 1;  // testing: the verification must catch this
                S = sq.G + (unsigned long long)e;
                rem = sq.i_in - (uint32_t)e;       // no trajectory of the window leaves G's permutation
                if (tau == 0) { cn[0] += sq.len; ++cn[2]; }
                rel += sq.len;
            }
            if (tau == 0) { shS = S; shRem = rem; shRel = rel | (miss0 ? 0x80000000u : 0u); }
        }
        __syncthreads();
        S = shS;
        rem = shRem;
        rel = shRel & 0x7fffffffu;
        const bool miss = (shRel >> 31) != 0;
        if (rel > h) {   // the block whose draws were prefetched is behind us: the next one to compute, then
            h = nxt[rel];
            if (h < nb) scan_load(raw, (b0 + h) * SCAN_BLOCK, tau, un);
        }
        if (miss) {
            // The entry state lies outside the segment's window (a band edge narrowed it, or the guess was far off):
            // its blocks one by one -- the per-block tables from global memory where they cover the state, the fixed
            // point where they do not.  Rare (about every other permutation at 1M cells), and no slower than r03's path.
            const uint32_t first = rel, last = rel + sg[rel].len;
            for (; rel < last && !failed && S < total_steps; ++rel) {
                const uint64_t bx = b0 + rel, slot = bx % PHI_RING;
                const PhiDesc d = desc[slot];
                const int64_t g = (int64_t)S - (int64_t)d.G;
                const bool neg = g < 0;
                const uint64_t idx = (uint64_t)(neg ? -g : g);
                if (d.prepared && idx <= (neg ? d.w_neg : d.w_pos)) {
                    const uint32_t T = idx ? phi_lookup(tbits + (slot * 2 + (neg ? 1 : 0)) * PHI_WORDS, (uint32_t)idx) : 0u;
                    if (tau == 0) { sblk[bx] = S; hardmask[bx] = 0; }
                    S = d.G + d.cnt + (unsigned long long)(neg ? -(long long)T : (long long)T);
                    rem = d.i_in - (uint32_t)(S - d.G);
                    if (tau == 0) ++cn[0];
                } else {
                    uint32_t u[SCAN_D];
                    scan_load(raw, bx * SCAN_BLOCK, tau, u);
                    ScanRes r;
                    uint32_t excl, total_cnt;
                    if (block_fixed_point(u, S, rem, M, top_mask, total_steps, sh, parity, r, excl, total_cnt) > 0) { failed = 1; break; }
                    acc_bits[bx * SCAN_THREADS + tau] = r.bits;
                    enter[bx * SCAN_THREADS + tau] = excl;
                    if (tau == 0) { sblk[bx] = S; hardmask[bx] = 1; }
                    if (r.end) shEnd = bx * SCAN_BLOCK + (uint64_t)tau * SCAN_D + r.end;
                    S += total_cnt;
                    rem = rem_advance(rem, total_cnt, M);
                    if (tau == 0) ++cn[1];
                }
            }
            if (tau == 0) { segmode[b0 + first] = 2; ++cn[3]; }   // k_seg_fill has nothing to add here
            if (failed || S >= total_steps) break;
        }
        if (rel >= nb) { rel = nb; break; }
        if (sg[rel].kind == 1) {   // the run goes on (more segments than staged at once, or behind a slow path)
            PHI_STAGE_LOAD(rel)
            continue;
        }
        // ---- block rel: computed by the chain itself ----
        const uint32_t x = rel;
        const uint32_t hN = nxt[x + 1];
        uint32_t u[SCAN_D];
        if (x == h) {
#pragma unroll
            for (int q = 0; q < SCAN_D; ++q) u[q] = un[q];
        } else {
            scan_load(raw, (b0 + x) * SCAN_BLOCK, tau, u);
        }
        // on their way while block x is computed: the tables of the run behind it and the draws of the block after that
        PHI_STAGE_LOAD(x + 1)
        if (x == h && hN < nb) scan_load(raw, (b0 + hN) * SCAN_BLOCK, tau, un);
        ScanRes r;
        uint32_t excl, total_cnt;
        if (block_fixed_point(u, S, rem, M, top_mask, total_steps, sh, parity, r, excl, total_cnt) > 0) { failed = 1; break; }
        const uint64_t bx = b0 + x;
        acc_bits[bx * SCAN_THREADS + tau] = r.bits;
        enter[bx * SCAN_THREADS + tau] = excl;
        if (tau == 0) { sblk[bx] = S; hardmask[bx] = 1; }
        if (r.end) shEnd = bx * SCAN_BLOCK + (uint64_t)tau * SCAN_D + r.end;
        S += total_cnt;
        rem = rem_advance(rem, total_cnt, M);
        if (tau == 0) ++cn[1];
        rel = x + 1;
        h = hN;
        if (S >= total_steps) break;
    }
    b_next = b0 + rel;
    if (tau == 0) {  // entry state of the next unit (the reference of a later unit's guesses), then "unit done"
        sblk[b_next] = S;
        __hip_atomic_store(flags, unit + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    }  // units
#undef PHI_STAGE_LOAD
    __syncthreads();
    if (tau == 0) {
        if (shEnd) st[3] = shEnd;
        const uint64_t b = b_next;
        st[0] = S;
        st[1] = b;
        st[6] += cn[2];   // segment lookups
        st[7] += (unsigned long long)cn[3] | ((unsigned long long)cn[4] << 32);  // segments whose window missed the entry state (high half: zero)
        st[4] += cn[0];
        st[5] += cn[1];
        sblk[b] = S;  // entry state of the next block (sblk holds n_blocks + 1 entries)
        unsigned long long f = 0;  // (k_block_exact of the previous chunk may be raising its own flag right now)
        if (failed) f |= 1ull;
        if (gave_up == 1) f |= 8ull;  // a unit's preparation did not arrive in time
        if (S < S_need && S < total_steps) f |= 2ull;  // the blocks granted to this chunk did not complete it
        if (f) atomicOr(st + 2, f);
        if (f || gave_up || S >= total_steps)  // nothing more will come from the chain: release every gate
            __hip_atomic_store(flags, 0xffffffffu, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Recompute every prepared block of range [range[0], range[1]) from its exact entry state (whole chip) and
// verify the chain: S_b + count_b must be the entry state of block b + 1.
__global__ __launch_bounds__(SCAN_THREADS) void k_block_exact(const uint32_t *__restrict__ raw, uint32_t n,
                                                              uint64_t total_steps,
                                                              const unsigned long long *__restrict__ range,
                                                              const uint8_t *__restrict__ hardmask,
                                                              bits_t *__restrict__ acc_bits,
                                                              uint32_t *__restrict__ enter,
                                                              const unsigned long long *__restrict__ sblk,
                                                              unsigned long long *__restrict__ st)
{
    __shared__ BlockShared sh;
    __shared__ uint32_t shrem;
    const uint64_t b = range[0] + blockIdx.x;
    if (b >= range[1] || hardmask[b]) return;
    const uint32_t tau = threadIdx.x;
    const uint32_t M = n - 1, top_mask = mask_of(M);
    const uint64_t S = sblk[b];
    if (tau == 0) shrem = M - (uint32_t)(S % M);
    uint32_t u[SCAN_D];
    scan_load(raw, b * SCAN_BLOCK, tau, u);
    __syncthreads();
    ScanRes r;
    uint32_t excl, total_cnt, parity = 0;
    const int failed = block_fixed_point(u, S, shrem, M, top_mask, total_steps, sh, parity, r, excl, total_cnt) > 0;
    acc_bits[b * SCAN_THREADS + tau] = r.bits;
    enter[b * SCAN_THREADS + tau] = excl;
    if (tau == 0 && (failed || r.end || S + total_cnt != sblk[b + 1])) atomicOr(st + 2, 4ull);
}

// k_probe_wait's question for ALL streams of a context at once (the priority-spread placement, permgen_probe_all_roles): one
// such kernel per stream adds 1 to a counter and waits until all `want` have arrived.  Streams that share a queue never
// meet: the kernel in front gives up after the same 20 ms and says so.
// (Kept BEHIND the generator's kernels.  Defined beside k_probe_wait it moved k_chain in the code object, and the chain
// -- one workgroup, bound by instruction latency -- took 2.3 ms longer per bench step: DESIGN.md 4.3.)
__global__ void k_probe_meet(uint32_t *count, uint32_t want, uint32_t *timed_out)
{
    if (threadIdx.x != 0) return;
    __hip_atomic_fetch_add(count, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    const long long t0 = wall_clock64();
    while (__hip_atomic_load(count, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < want) {
        if (wall_clock64() - t0 > 2000000ll) { atomicOr(timed_out, 1u); return; }   // 20 ms
        __builtin_amdgcn_s_sleep(8);
    }
}

// ---- host: the stream probe, and the block-parallel form's share of a job (called by sc_permgen.hip) ----
bool permgen_is_block_parallel(const sc_ctx *c, int64_t n) { return c->pg.mode != 1 && !c->pg.streams_serial && n >= PHI_MIN_N; }

// The probe of the plain placement: the chain's stream and the four preparation streams, in five rounds (k_probe_wait).
static int permgen_probe_generator(sc_ctx *c, int chain_role, bool *concurrent)
{
    std::vector<hipStream_t> ss;
    SC_TRY(c->streams.ensure(chain_role));
    SC_TRY(c->pg.ensure(true));
    ss.push_back(c->streams.s[chain_role]);
    for (int q = 0; q < 4; ++q) ss.push_back(c->stream_pg[q]);
    SC_TRY(c->perm_flag.ensure(sizeof(unsigned long long), &c->mem));
    uint32_t *words = c->perm_flag.as<uint32_t>();
    SC_HIP(hipDeviceSynchronize());
    SC_HIP(hipMemset(words, 0, 2 * sizeof(uint32_t)));
    // a stream's hardware queue is created at its first launch, which takes milliseconds: warm every stream up first, or
    // the waiters of round one give up before the setter's queue exists (seen with a second context in one process)
    for (hipStream_t sp : ss) hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, sp, words, 0u, 0u);
    for (hipStream_t sp : ss) SC_HIP(hipStreamSynchronize(sp));
    for (size_t setter = 0; setter < ss.size(); ++setter) {
        for (size_t k = 0; k < ss.size(); ++k)
            if (k != setter) hipLaunchKernelGGL(k_probe_wait, dim3(1), dim3(64), 0, ss[k], words, (uint32_t)(setter + 1), words + 1);
        hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, ss[setter], words, 0u, (uint32_t)(setter + 1));
        for (hipStream_t sp : ss) SC_HIP(hipStreamSynchronize(sp));
    }
    uint32_t host[2] = {0, 0};
    SC_HIP(hipMemcpy(host, words, sizeof(host), hipMemcpyDeviceToHost));
    *concurrent = host[1] == 0;
    return SC_OK;
}

// The probe of the priority-spread placement, which fills its queue pools exactly: one foreign stream on a level (a host
// application's, a collective library's, a second context's) makes two of ours share a queue, whichever they are.  So
// every role's stream is created and all of them meet in one round (k_probe_meet).
static int permgen_probe_all_roles(sc_ctx *c, bool *concurrent)
{
    for (int r = 0; r < SR_COUNT; ++r) SC_TRY(c->streams.ensure(r));
    SC_TRY(c->pg.ensure(true));
    SC_TRY(c->perm_flag.ensure(sizeof(unsigned long long), &c->mem));
    uint32_t *words = c->perm_flag.as<uint32_t>();
    SC_HIP(hipDeviceSynchronize());
    SC_HIP(hipMemset(words, 0, 2 * sizeof(uint32_t)));
    for (hipStream_t sp : c->streams.s) hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, sp, words, 0u, 0u);   // (warm-up, as above)
    SC_TRY(c->streams.sync((1u << SR_COUNT) - 1u));
    for (hipStream_t sp : c->streams.s) hipLaunchKernelGGL(k_probe_meet, dim3(1), dim3(64), 0, sp, words, (uint32_t)SR_COUNT, words + 1);
    SC_TRY(c->streams.sync((1u << SR_COUNT) - 1u));
    uint32_t host[2] = {0, 0};
    SC_HIP(hipMemcpy(host, words, sizeof(host), hipMemcpyDeviceToHost));
    *concurrent = host[1] == 0 && host[0] == (uint32_t)SR_COUNT;
    return SC_OK;
}

// The placement ladder.  Step 1: the environment's GPU_MAX_HW_QUEUES holds every role -- plain streams, probed.  Step 2:
// it does not, or the plain probe failed (a runtime that initialised before the library could ask: the environment
// shows 24, the runtime never saw it) -- the priority-spread placement, if its groups fit the limit, probed over all
// roles.  Step 3: neither -- plain streams and the sequential scan, with the note.
int permgen_place_streams(sc_ctx *c, int chain_role)
{
    if (c->pg.probed) return SC_OK;
    c->pg.probed = true;
    c->pg.placement_note.clear();
    const char *q = getenv("GPU_MAX_HW_QUEUES");
    const int limit = q && atoi(q) > 0 ? atoi(q) : 4;   // (unset: the runtime's default)
    int least = 0, greatest = 0;
    SC_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    const bool three_levels = greatest < 0 && least > 0;
    SC_HIP(hipDeviceSynchronize());   // (the streams may be replaced below: all idle from here)
    int level[SR_COUNT] = {};
    bool concurrent = false, plain_failed = false;
    for (int step = 1; step <= 2 && !concurrent; ++step) {
        const int place = sc_place_streams(limit, plain_failed, SC_ROLE_GROUP, SR_COUNT, SC_GROUP_LEVEL, SG_COUNT, level);
        if (place == SC_PLACE_NONE || (place == SC_PLACE_SPREAD && !three_levels)) break;
        SC_TRY(c->streams.replace(place, level));
        if (place == SC_PLACE_PLAIN) {
            SC_TRY(permgen_probe_generator(c, chain_role, &concurrent));
            plain_failed = !concurrent;
        } else {
            SC_TRY(permgen_probe_all_roles(c, &concurrent));
            if (concurrent) {
                char buf[120];
                snprintf(buf, sizeof(buf), "streams spread over three priority levels (GPU_MAX_HW_QUEUES=%s)", q ? q : "unset");
                c->pg.placement_note = buf;
            }
            break;
        }
    }
    if (concurrent) return SC_OK;
    // step 3.  Neither placement tried (fewer queues per level than the largest group needs): the plain probe decides, as
    // it always did -- a runtime that runs the streams concurrently all the same keeps the block-parallel form
    SC_TRY(c->streams.replace(SC_PLACE_PLAIN, level));
    if (!plain_failed) SC_TRY(permgen_probe_generator(c, chain_role, &concurrent));
    if (!concurrent) {
        c->pg.streams_serial = true;
        char buf[320];
        snprintf(buf, sizeof(buf), "the HIP streams of this process do not run concurrently (GPU_MAX_HW_QUEUES=%s; the library "
                 "asks for 24 when it is loaded BEFORE the HIP runtime initialises, or a profiler serialises kernels): the "
                 "permutation generator uses its sequential scan (same results, about half the speed)", q ? q : "unset");
        c->pg.note = buf;
    }
    return SC_OK;
}

// ---- r04: the generator's form, asked for instead of discovered (sc_init / spatialcore_amd.init) ----
// Probe the context's generator streams NOW (the first block-parallel job would do it otherwise) and report whether they
// run concurrently, together with the hardware-queue request the runtime saw when it initialised.
extern "C" int sc_ctx_probe_streams(sc_ctx *c, int *concurrent, int *hw_queues_requested)
{
    SC_REQUIRE(c && concurrent, SC_ERR_INVALID, "sc_ctx_probe_streams: null pointer");
    SC_HIP(hipSetDevice(c->device));
    SC_REQUIRE(c->pg.probed || !c->pipe, SC_ERR_STATE, "sc_ctx_probe_streams: a job begun by sc_moran_seeded_begin is in flight");
    SC_TRY(permgen_place_streams(c, SR_CHAIN));
    *concurrent = c->pg.streams_serial ? 0 : 1;
    if (hw_queues_requested) {
        const char *q = getenv("GPU_MAX_HW_QUEUES");
        *hw_queues_requested = q ? atoi(q) : 0;   // 0: unset (the runtime's default of 4)
    }
    return SC_OK;
}

// Which scan a permutation job of length n takes on this context right now, in words (for provenance records).
extern "C" int sc_ctx_permgen_form(sc_ctx *c, int64_t n, const char **form)
{
    SC_REQUIRE(c && form, SC_ERR_INVALID, "sc_ctx_permgen_form: null pointer");
    if (n < PHI_MIN_N) c->pg.form = "sequential (permutations shorter than 131072: every block holds a band change)";
    else if (c->pg.mode == 1) c->pg.form = "sequential (sc_ctx_set_permgen_mode 1)";
    else if (c->pg.streams_serial) c->pg.form = "sequential: " + c->pg.note;
    else {
        c->pg.form = "block-parallel";
        for (const std::string *s : {&c->pg.placement_note, &c->pg.note})
            if (!s->empty()) c->pg.form += "; " + *s;
    }
    *form = c->pg.form.c_str();
    return SC_OK;
}

int phi_begin(sc_ctx *c, PermJob *job, int units_ahead, uint64_t n_blocks, hipStream_t s)
{
    job->phi = permgen_is_block_parallel(c, job->n);   // (a job starts from a fresh PermJob: no unit, no gate yet)
    job->units_ahead = units_ahead >= 1 && units_ahead <= PHI_AHEAD_MAX ? units_ahead : 1;
    // (the caller took `s` from the table after permgen_place_streams, which may replace every stream)
    SC_REQUIRE(!job->phi || c->pg.probed, SC_ERR_STATE, "permutation generator: block-parallel job on streams that were never placed");
    SC_TRY(c->pg.ensure(job->phi));
    if (job->phi) {
        SC_TRY(c->pg.desc.ensure(sizeof(PhiDesc) * (size_t)PHI_RING, &c->mem));
        SC_TRY(c->pg.tbits.ensure(sizeof(unsigned long long) * (size_t)PHI_RING * 2 * PHI_WORDS, &c->mem));
        SC_TRY(c->pg.events.ensure(sizeof(uint16_t) * (size_t)PHI_RING * 2 * PHI_MAX_EV, &c->mem));
        SC_TRY(c->pg.hard.ensure((size_t)n_blocks + 1, &c->mem));
        SC_TRY(c->pg.seg.ensure(sizeof(PhiSeg) * (size_t)PHI_RING, &c->mem));
        SC_TRY(c->pg.ctbits.ensure(sizeof(unsigned long long) * (size_t)PHI_RING * 2 * PHI_WORDS, &c->mem));
        SC_TRY(c->pg.segmode.ensure((size_t)n_blocks + 1, &c->mem));
        SC_TRY(c->pg.seglist.ensure(sizeof(uint32_t) * (size_t)PHI_FLAG_SLOTS * (1 + PHI_UNIT), &c->mem));
        SC_HIP(hipMemsetAsync(c->pg.segmode.p, 0, (size_t)n_blocks + 1, s));
    }
    // [0] units the chain has completed, [1 .. 16] "unit prepared" words
    SC_TRY(c->pg.flags.ensure(sizeof(uint32_t) * (1 + 2 * PHI_FLAG_SLOTS), &c->mem));
    SC_HIP(hipMemsetAsync(c->pg.flags.p, 0, sizeof(uint32_t) * (1 + 2 * PHI_FLAG_SLOTS), s));
    return SC_OK;
}

int phi_chain_chunk(sc_ctx *c, PermJob *job, int64_t p1, hipStream_t s, uint64_t *blocks, unsigned *fill_streams)
{
    const uint64_t n_blocks = job->hi / SCAN_BLOCK, target = (uint64_t)p1 * (uint64_t)(job->n - 1);
    unsigned long long *st = c->pg.out.as<unsigned long long>();
    // Blocks granted to this chunk: the expected draws of permutations [0, p1) + ~10 sigma + one block
    // (k_chain raises a flag if they do not complete the chunk); the last chunk takes all blocks.
    const double need = (double)p1 * job->draws_per_perm + 9000.0 * sqrt((double)p1) + (double)SCAN_BLOCK;
    uint64_t B_end = (uint64_t)(need / SCAN_BLOCK) + 1;
    // ... rounded UP to whole launch units (r04).  A chunk that ends inside a unit leaves a SHORT last unit, which the
    // chain finishes in a fraction of a unit's time -- and the first unit of the next chunk, prepared `ahead` units ahead
    // in chain time, is then not ready: the clock profile of the chain inside the Moran pipeline showed ~13 such waits
    // per 1000 x 1M job, 1-2 ms each (20 of the chain's 130 ms), and nothing in between.  The extra blocks (< 6
    // permutations' worth) are simply scanned one chunk earlier.
    B_end = (B_end + PHI_UNIT - 1) / PHI_UNIT * PHI_UNIT;
    if (B_end > n_blocks || p1 >= job->n_perm) B_end = n_blocks;
    KernelTimerScope ts(c, SC_K_PERM_SCAN, s);
    // the chunk's launch units: each prepared by its own launches (4 rotating streams), all chained by ONE launch
    const uint64_t g0 = job->B_done;
    const int64_t u_first = job->unit_no;
    uint32_t *flags = c->pg.flags.as<uint32_t>();
    while (job->B_done < B_end) {
        const uint64_t b0 = job->B_done;
        const uint64_t b1 = b0 + PHI_UNIT < B_end ? b0 + PHI_UNIT : B_end;
        const int64_t u = job->unit_no;
        hipStream_t sp = c->stream_pg[(size_t)(u % PHI_STREAMS)];
        // The guess of unit u uses the exact state at the start of unit u - ahead, which the chain leaves when it
        // completes unit u - ahead - 1; that unit also is the last reader of the ring slots unit u overwrites.
        const int64_t dep = u - job->units_ahead - 1;
        uint32_t *seglist = c->pg.seglist.as<uint32_t>() + (size_t)(u % PHI_FLAG_SLOTS) * (1 + PHI_UNIT);
        const uint64_t ref = u >= job->units_ahead ? job->unit_start[(size_t)((u - job->units_ahead) % 8)] : 0;
        if (u < PHI_STREAMS) SC_HIP(hipStreamWaitEvent(sp, c->pg.ev[32], 0));  // the raw stream (recorded by permgen_begin)
        // (a gate in front of this stream's last k_seg_fill has waited for the same or a later "unit done" already)
        if (dep >= 0 && dep + 1 > job->gate_seen[(size_t)(u % PHI_STREAMS)])
            hipLaunchKernelGGL(k_gate, dim3(1), dim3(64), 0, sp, flags, (uint32_t)(dep + 1), st);
        hipLaunchKernelGGL(k_phi_events, dim3((unsigned)(b1 - b0)), dim3(SCAN_THREADS), 0, sp, c->pg.raw.as<uint32_t>(), (uint32_t)job->n,
                           job->total_steps, job->draws_per_perm, b0, b1, ref, c->pg.sblk.as<unsigned long long>(),
                           c->pg.desc.as<PhiDesc>(), c->pg.events.as<uint16_t>(), seglist);
        hipLaunchKernelGGL(k_phi_tbuild, dim3((unsigned)(b1 - b0)), dim3(128), 0, sp, b0, b1, c->pg.desc.as<PhiDesc>(),
                           c->pg.events.as<uint16_t>(), c->pg.tbits.as<unsigned long long>(), c->pg.seg.as<PhiSeg>(), seglist);
        hipLaunchKernelGGL(k_phi_compose, dim3(PHI_COMPOSE_WGS), dim3(SCAN_THREADS), 0, sp, b0, c->pg.desc.as<PhiDesc>(),
                           c->pg.tbits.as<unsigned long long>(), c->pg.seg.as<PhiSeg>(), c->pg.ctbits.as<unsigned long long>(), seglist);
        hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, sp, flags, (uint32_t)(1 + u % PHI_FLAG_SLOTS), (uint32_t)(u + 1));
        // behind the chain's "unit u done": the entry states of the blocks inside the unit's segments (this stream's
        // next unit, u + PHI_STREAMS, overwrites the ring slots they are read from and is enqueued behind this)
        hipLaunchKernelGGL(k_gate, dim3(1), dim3(64), 0, sp, flags, (uint32_t)(u + 1), st);
        job->gate_seen[(size_t)(u % PHI_STREAMS)] = u + 1;
        hipLaunchKernelGGL(k_seg_fill, dim3((unsigned)(b1 - b0)), dim3(64), 0, sp, b0, b1, c->pg.desc.as<PhiDesc>(),
                           c->pg.seg.as<PhiSeg>(), c->pg.tbits.as<unsigned long long>(), c->pg.segmode.as<uint8_t>(),
                           c->pg.sblk.as<unsigned long long>(), c->pg.hard.as<uint8_t>(), st);
        *fill_streams |= 1u << (unsigned)(u % PHI_STREAMS);
        job->unit_start[(size_t)(u % 8)] = b0;
        job->B_done = b1;
        job->unit_no = u + 1;
    }
    hipLaunchKernelGGL(k_chain, dim3(1), dim3(SCAN_THREADS), 0, s, c->pg.raw.as<uint32_t>(), n_blocks, (uint32_t)job->n,
                       job->total_steps, g0, B_end, target, c->pg.desc.as<PhiDesc>(), c->pg.tbits.as<unsigned long long>(),
                       c->pg.seg.as<PhiSeg>(), c->pg.ctbits.as<unsigned long long>(), c->pg.hard.as<uint8_t>(), c->pg.segmode.as<uint8_t>(),
                       (c->pg.mode == 2 && u_first == 0) ? 1 : 0, c->pg.bits.as<bits_t>(), c->pg.enter.as<uint32_t>(),
                       c->pg.sblk.as<unsigned long long>(), st, flags, (uint32_t)u_first);
    SC_HIP(hipGetLastError());
    // the verification / expansion of this chunk reads the entry states k_seg_fill leaves on the preparation streams
    for (unsigned q = 0; q < PHI_STREAMS; ++q)
        if (*fill_streams & (1u << q)) SC_HIP(hipEventRecord(c->pg.ev[q], c->stream_pg[q]));
    *blocks = B_end > g0 ? B_end - g0 : 1;
    return SC_OK;
}

int phi_verify_chunk(sc_ctx *c, PermJob *job, const unsigned long long *range, uint64_t blocks, unsigned fill_streams, hipStream_t sp)
{
    for (unsigned q = 0; q < PHI_STREAMS; ++q)
        if (fill_streams & (1u << q)) SC_HIP(hipStreamWaitEvent(sp, c->pg.ev[q], 0));
    // the prepared blocks again, from their exact entry states, on the whole chip + verification of the chain
    KernelTimerScope ts(c, SC_K_PERM_SCAN, sp);
    hipLaunchKernelGGL(k_block_exact, dim3((unsigned)blocks), dim3(SCAN_THREADS), 0, sp, c->pg.raw.as<uint32_t>(), (uint32_t)job->n,
                       job->total_steps, range, c->pg.hard.as<uint8_t>(), c->pg.bits.as<bits_t>(), c->pg.enter.as<uint32_t>(),
                       c->pg.sblk.as<unsigned long long>(), c->pg.out.as<unsigned long long>());
    return SC_OK;
}
