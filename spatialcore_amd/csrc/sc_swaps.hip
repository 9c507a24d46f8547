// Stage B of the permutation generators (sc_permgen.hip, sc_perm_counter.hip): the Fisher-Yates swaps.  gfx950 only.
#include <stdlib.h>

#include "sc_permgen.h"

// ------------------------------------------------------------------------------------------------
// B: apply the swaps, one wavefront per permutation
// ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(64) void k_apply_swaps(const int32_t *__restrict__ J, int32_t *__restrict__ perm,
                                                    int64_t pstride, uint32_t n, int64_t p0, int64_t n_perm)
{
    const int64_t p = p0 + blockIdx.x;
    if (p >= n_perm) return;
    const uint32_t lane = threadIdx.x;
    const uint32_t M = n - 1;
    int32_t *A = perm + p * pstride;
    const int32_t *Jp = J + p * (int64_t)M;
    for (uint32_t x = lane; x < n; x += 64) A[x] = (int32_t)x;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

    int64_t i_top = (int64_t)n - 1;
    while (i_top >= 1) {
        const int64_t i = i_top - lane;
        const bool valid = i >= 1;
        // step index inside the permutation: s = n-1-i (lanes read consecutive entries)
        int32_t j = valid ? Jp[(int64_t)M - i] : -1;
        if (valid && (uint32_t)j > (uint32_t)i) j = (int32_t)i;  // never index outside [0, i], whatever J holds
        const int32_t ii = valid ? (int32_t)i : -2;
        // loads first (latency overlaps the conflict search); L1 is bypassed so that the values the
        // previous round stored (write-through to L2, completed by the vmcnt wait) are seen
        int32_t a_i = 0, a_j = 0;
        if (valid) {
            a_i = __hip_atomic_load(&A[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a_j = __hip_atomic_load(&A[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        // lane l conflicts if an EARLIER step m < l targets l's own slot (j_m == i_l) or the same slot
        // (j_m == j_l); (j_l == i_m cannot happen: j_l <= i_l < i_m).  Self swaps j == i are harmless.
        bool flag = false;
        for (int m = 0; m < 63; ++m) {
            const int32_t jm = __builtin_amdgcn_readlane(j, m);
            flag |= ((int)lane > m) && (jm == ii || jm == j);
        }
        const unsigned long long conf = __ballot(flag && valid);
        const unsigned long long vmask = __ballot(valid);
        int count = conf ? (int)__builtin_ctzll(conf) : 64;
        const int nvalid = (int)__builtin_popcountll(vmask);
        if (count > nvalid) count = nvalid;
        if ((int)lane < count) {
            A[i] = a_j;
            if (j != (int32_t)i) A[j] = a_i;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        i_top -= count;
    }
}

// The same rule with a whole workgroup per permutation: SW_T consecutive steps per round.  Two steps of a round
// touch a common slot only if a later step's own slot i_t is an earlier step's target (j_m == i_t, found by index
// arithmetic since the i are consecutive) or two steps share a target (j_m == j_l, found with an LDS hash table
// keyed by the target: CAS insert with linear probing, minimum step index per key).  The longest prefix without
// such a pair is applied in parallel; the round trip to L2 that bounds a round is paid once per ~SW_T steps.
#define SW_T 512
#define SWAPS_WG_MIN_N 65536  // shorter permutations: conflicts are frequent, one wavefront per permutation is enough
#define SW_HASH 2048

// ASC = false: the shuffle itself (steps i = n-1 .. 1), the table numpy returns.
// ASC = true:  the same transpositions applied in the opposite order (i = 1 .. n-1) to the identity.  With position
//              swaps s_1 .. s_m applied in order the array is s_1 o s_2 o .. o s_m (position -> value), so the opposite
//              order yields its inverse: the INVERSE permutation table comes out of the same kernel, no scatter pass.
//              Two steps of a round then collide when a later step's target is an earlier step's own slot
//              (j_l == i_m, again index arithmetic) or two steps share a target.
// r03: (i) the swap partners j of the coming rounds are PREFETCHED into an LDS ring (they do not depend on anything the
// rounds do; only WHICH steps a round holds does, by up to SW_T), so a round's memory latency is one dependent access
// (the values at the partners' slots) instead of two; (ii) in the ascending mode a step's own slot has never been touched
// when its turn comes (every earlier step i' < i writes slots <= i'), so its value is i itself: no load, and no identity
// fill of the row beyond slot 0.
#define SW_RING 2048   // partners of steps [done, done + <= 1536) live here

// r04: PW permutations per workgroup (PW x SW_T threads, each SW_T-thread half runs its own permutation with its own LDS
// structures, the barriers are shared: a round is latency-bound, two of them in lockstep cost what one costs).  Why: a
// swap workgroup lives ~10 ms, and 128 of them with 8 wavefronts each, spread over the CUs the scoring kernel leaves,
// fragment the wavefront slots that the generator's 1024-thread preparation workgroups need sixteen of on one CU (4.3 of
// the chain's 7-9 ms waits).  With PW = 2 a chunk is 64 workgroups of the preparation kernels' own size.
template <bool ASC, int PW>
__global__ __launch_bounds__(SW_T * PW) void k_apply_swaps_wg(const int32_t *__restrict__ J, int32_t *__restrict__ perm,
                                                              int64_t pstride, uint32_t n, int64_t p0, int64_t n_perm)
{
    __shared__ uint32_t hkey_[PW][SW_HASH], hmin_[PW][SW_HASH];
    __shared__ uint32_t first_conf_[PW][2];
    __shared__ uint32_t act[2];
    __shared__ int32_t jring_[PW][SW_RING];
    const uint32_t half = PW > 1 ? threadIdx.x / SW_T : 0u;
    const uint32_t l = PW > 1 ? threadIdx.x % SW_T : threadIdx.x;
    uint32_t *hkey = hkey_[half], *hmin = hmin_[half], *first_conf = first_conf_[half];
    int32_t *jring = jring_[half];
    const int64_t p = p0 + (int64_t)blockIdx.x * PW + half;
    const bool exists = p < n_perm;          // (an odd chunk: the last workgroup's second half has nothing to do but meet the barriers)
    const uint32_t M = n - 1;
    int32_t *A = perm + (exists ? p : p0) * pstride;
    const int32_t *Jp = J + (exists ? p : p0) * (int64_t)M;
    // step k = 0 .. M - 1 of the processing order: i = 1 + k (ascending) or n - 1 - k; its partner is Jp[M - i]
    auto step_i = [&](int64_t k) -> int64_t { return ASC ? 1 + k : (int64_t)n - 1 - k; };
    if (exists) {
        if (!ASC) { for (uint32_t x = l; x < n; x += SW_T) A[x] = (int32_t)x; }
        else if (l == 0) A[0] = 0;
        for (int r = 0; r < 2; ++r) {   // partners of the first 2 SW_T steps
            const int64_t k = (int64_t)r * SW_T + l;
            jring[k & (SW_RING - 1)] = k < (int64_t)M ? Jp[(int64_t)M - step_i(k)] : -1;
        }
    }
    int64_t filled = 2 * SW_T;      // partners of steps [done, filled) are in the ring
    int64_t i_cur = ASC ? 1 : (int64_t)n - 1;  // first step of the round
    if (!exists) i_cur = ASC ? (int64_t)n : 0; // (done)
    if (l < 2) first_conf[l] = SW_T;
    if (l == 0) act[half] = (ASC ? i_cur <= (int64_t)n - 1 : i_cur >= 1) ? 1u : 0u;
    if (PW == 1 && l == 0) act[1] = 0u;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    uint32_t round = 0;
    while (act[0] | act[1]) {       // (uniform: the words are rewritten in front of the round's last barrier)
        const int64_t i = ASC ? i_cur + l : i_cur - l;
        const bool valid = exists && (ASC ? (i_cur <= (int64_t)n - 1 && i <= (int64_t)n - 1) : (i_cur >= 1 && i >= 1));
        const int64_t done = ASC ? i_cur - 1 : (int64_t)n - 1 - i_cur;   // steps applied so far
        int32_t j = valid ? jring[(done + l) & (SW_RING - 1)] : -1;
        // the ring's next SW_T partners are on their way while this round works (stored at its end)
        const bool top_up = exists && filled - done <= 2 * SW_T;
        const int64_t kf = filled + l;
        int32_t j_next = -1;
        if (top_up && kf < (int64_t)M) j_next = Jp[(int64_t)M - step_i(kf)];
        if (valid && (uint32_t)j > (uint32_t)i) j = (int32_t)i;  // never index outside [0, i], whatever J holds
        int32_t a_i = 0, a_j = 0;
        if (valid) {  // L1 is bypassed: the values the previous round stored are in L2 (vmcnt wait + barrier)
            a_i = ASC ? (int32_t)i : __hip_atomic_load(&A[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a_j = (ASC && j == (int32_t)i) ? a_i : __hip_atomic_load(&A[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int k = 0; k < SW_HASH / SW_T; ++k) { hkey[l + SW_T * k] = 0xffffffffu; hmin[l + SW_T * k] = 0xffffffffu; }
        __syncthreads();
        uint32_t *fc = &first_conf[round & 1];
        uint32_t h = 0;
        if (valid) {
            if (ASC) {
                const int64_t t = j - i_cur;  // the step whose own slot is my target (t <= l; t == l is a self swap)
                if (t >= 0 && t < (int64_t)l) atomicMin(fc, l);
            } else {
                const int64_t t = i_cur - j;  // the step whose own slot is j (t >= l; t == l is a self swap)
                if (t < SW_T && t != (int64_t)l) atomicMin(fc, (uint32_t)t);
            }
            h = ((uint32_t)j * 2654435761u) >> 21;
            for (;;) {
                const uint32_t old = atomicCAS(&hkey[h], 0xffffffffu, (uint32_t)j);
                if (old == 0xffffffffu || old == (uint32_t)j) break;
                h = (h + 1) & (SW_HASH - 1);
            }
            atomicMin(&hmin[h], l);
        }
        __syncthreads();
        if (valid && hmin[h] < l) atomicMin(fc, l);
        if (l == 0) first_conf[(round + 1) & 1] = SW_T;  // next round's cell (nobody touches it this round)
        __syncthreads();
        uint32_t count = *fc;
        const int64_t left = ASC ? (int64_t)n - i_cur : i_cur;  // steps not yet applied (<= 0: this half is done)
        const int64_t nvalid = left < 0 ? 0 : (left < SW_T ? left : SW_T);
        if ((int64_t)count > nvalid) count = (uint32_t)nvalid;
        if (valid && l < count) {
            A[i] = a_j;
            if (j != (int32_t)i) A[j] = a_i;
        }
        if (top_up) { jring[kf & (SW_RING - 1)] = j_next; filled += SW_T; }   // (uniform per half; slots of steps already applied)
        i_cur += ASC ? (int64_t)count : -(int64_t)count;
        ++round;
        if (l == 0) act[half] = (exists && (ASC ? i_cur <= (int64_t)n - 1 : i_cur >= 1)) ? 1u : 0u;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
}

// r04: FULL rounds.  The kernel above ends a round at the first step that shares a slot with an earlier step of the round
// (the birthday bound: ~0.9 sqrt(i) steps, 470 of 512 at i = 10^6, 2670 rounds per 10^6-step permutation, each a round trip
// to L2 and four barriers: 10-12 ms per chunk, and the scoring of a chunk waits for exactly that).  But a round's hazards
// all run through the PARTNER slots of earlier steps, and the hash table that finds them can also resolve them:
//   descending (the shuffle): step k reads its own slot i_k and its partner slot j_k.  An earlier step a of the round can
//     have touched either one only as ITS partner (j_a == i_k or j_a == j_k: own slots of earlier steps lie above i_k), and
//     what it left there is the value v_a its own slot held.  So v_k = v_a of the latest such a for i_k (else memory), the
//     value that ends up in slot i_k is v_a of the latest such a for j_k (else memory), and slot j_k ends up with v of the
//     LAST step of the round that has it as partner -- unless it is a processed step's own slot (written by that step).
//   ascending (the inverse table): a step's own slot is untouched (v_k = i_k); its partner slot may have been touched by
//     an earlier step as partner (leaving that step's i_a) or as own slot (leaving w_a, what that step took from ITS
//     partner slot); slot i_k ends up with i_b of the last LATER step that has it as partner, else with w_k.
// Per key (slot) the table keeps the smallest and the largest step index: enough while no key has three steps below the
// round's end, so a round ends at the first MIDDLE step of a key (~i^(2/3) steps: every round of 1024 is whole down to
// i ~ 30 000).  Chains (v_k = v_a = v_a' ...) are rare and resolved by pointer jumping in LDS.  1054 rounds per 10^6-step
// permutation instead of 2670 (simulation and rule: scripts/swap_rounds_sim.py); sixteen wavefronts per workgroup, the
// size of the generator's preparation workgroups.
#define SF_T 1024
#define SF_HASH 8192      // eight slots per step: a CAS insert seldom probes twice (at two slots per step the slowest wavefront
                          // of sixteen probed ~10 times, 6000 clocks per round); 96 KB of the CU's 160 KB LDS, cleared entry by entry
#define SF_HASH_SHIFT 19
#define SF_RING 4096
#define SF_NONE 0xffffffffu
// A barrier that orders LDS only: __syncthreads() carries a global-memory fence, i.e. a wait for every load in flight,
// and the point of a round is that the hash work runs UNDER the latency of the round's loads (measured, clocks per round
// with __syncthreads(): loads + first barrier 3800, insert 2600, detect + look-up 6000, values 2000, stores 1800).
__device__ __forceinline__ void sf_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <bool ASC>
__global__ __launch_bounds__(SF_T) void k_apply_swaps_full(const int32_t *__restrict__ J, int32_t *__restrict__ perm,
                                                           int64_t pstride, uint32_t n, int64_t p0, int64_t n_perm)
{
    __shared__ uint32_t hkey[SF_HASH], hmin[SF_HASH], hmax[SF_HASH];   // key (slot) | smallest step | 1 + largest step
    __shared__ uint32_t omin[SF_T], omax[SF_T];   // the same two for the round's OWN slots as somebody's partner, by step (no probing)
    __shared__ int32_t jring[SF_RING];
    __shared__ int32_t val[SF_T];       // v_k (descending) / w_k (ascending) once ptr[k] == SF_NONE
    __shared__ uint32_t ptr[SF_T];      // the step whose value step k takes
    __shared__ uint32_t first_conf[2], chains[2];
    const uint32_t l = threadIdx.x;
    const int64_t p = p0 + blockIdx.x;
    if (p >= n_perm) return;
    const uint32_t M = n - 1;           // steps; step s = 0 .. M - 1 handles i = 1 + s (ascending) or n - 1 - s
    int32_t *A = perm + p * pstride;
    const int32_t *Jp = J + p * (int64_t)M;
    // partner of step s: Jp[M - i]
    auto partner_at = [&](uint32_t s) -> int32_t { return Jp[ASC ? M - 1u - s : s]; };
    if (!ASC) { for (uint32_t x = l; x < n; x += SF_T) A[x] = (int32_t)x; }
    else if (l == 0) A[0] = 0;
    for (uint32_t r = 0; r < 2; ++r) {
        const uint32_t s = r * SF_T + l;
        jring[s & (SF_RING - 1)] = s < M ? partner_at(s) : -1;
    }
#pragma unroll
    for (int k = 0; k < SF_HASH / SF_T; ++k) { hkey[l + SF_T * k] = SF_NONE; hmin[l + SF_T * k] = SF_NONE; hmax[l + SF_T * k] = 0u; }
    omin[l] = SF_NONE; omax[l] = 0u;
    uint32_t filled = 2 * SF_T;          // partners of steps [done, filled) are in the ring
    uint32_t done = 0;                  // steps applied so far
    if (l < 2) { first_conf[l] = SF_T; chains[l] = 0u; }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // the processed steps of a key below k / below the round's end (see above: at most hmin and hmax)
    auto last_lt = [](uint32_t mn, uint32_t mx1, uint32_t k) -> uint32_t {
        return (mx1 != 0u && mx1 - 1u < k) ? mx1 - 1u : (mn < k ? mn : SF_NONE);
    };
    uint32_t round = 0;
    while (done < M) {
        const uint32_t i_cur = ASC ? 1u + done : n - 1u - done;   // the round's first step
        const uint32_t left = M - done;
        const uint32_t nvalid = left < SF_T ? left : SF_T;
        const bool valid = l < nvalid;
        const uint32_t i = ASC ? i_cur + l : i_cur - l;           // (meaningful if valid)
        int32_t j = valid ? jring[(done + l) & (SF_RING - 1)] : -1;
        const bool top_up = filled - done <= 2 * SF_T;
        const uint32_t sf = filled + l;
        int32_t j_next = -1;
        if (top_up && sf < M) j_next = partner_at(sf);
        if (valid && (uint32_t)j > i) j = (int32_t)i;  // never index outside [0, i], whatever J holds
        int32_t a_i = (int32_t)i, a_j = 0;
        if (valid) {  // L1 is bypassed: the values the previous round stored are in L2 (vmcnt wait + barrier)
            if (!ASC) a_i = __hip_atomic_load(&A[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a_j = __hip_atomic_load(&A[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (ascending: may be a slot nobody has written yet; not used then)
        }
        // ---- insert: the tables were cleared behind the previous round's last reads ----
        uint32_t *fc = &first_conf[round & 1];
        uint32_t h = 0;
        if (valid) {
            h = ((uint32_t)j * 2654435761u) >> SF_HASH_SHIFT;
            for (;;) {
                const uint32_t old = atomicCAS(&hkey[h], SF_NONE, (uint32_t)j);
                if (old == SF_NONE || old == (uint32_t)j) break;
                h = (h + 1) & (SF_HASH - 1);
            }
            atomicMin(&hmin[h], l);
            atomicMax(&hmax[h], l + 1u);
            const uint32_t t = ASC ? (uint32_t)j - i_cur : i_cur - (uint32_t)j;   // the step whose own slot is j (if < SF_T)
            if (t < SF_T) { atomicMin(&omin[t], l); atomicMax(&omax[t], l + 1u); }
        }
        sf_lds_barrier();
        // ---- hazards: middle steps end the round; every step finds where its two values come from ----
        uint32_t mn = SF_NONE, mx1 = 0u, imn = SF_NONE, imx1 = 0u;   // of the key j / of the key i (my own slot as somebody's partner)
        uint32_t myptr = SF_NONE, p2 = SF_NONE;
        if (valid) {
            mn = hmin[h]; mx1 = hmax[h];
            imn = omin[l]; imx1 = omax[l];
            if (mn < l && l + 1u < mx1) atomicMin(fc, l);   // a middle step of its key
            int32_t v = a_i;
            if (!ASC) {
                const uint32_t p1 = last_lt(imn, imx1, l);
                p2 = j == (int32_t)i ? p1 : last_lt(mn, mx1, l);
                myptr = p1;
            } else if (j != (int32_t)i) {
                const uint32_t a_p = last_lt(mn, mx1, l);
                const uint32_t t = (uint32_t)j - i_cur;       // the step whose own slot is j (wraps to a large number below i_cur)
                const bool own = t < l;
                if (a_p == SF_NONE && !own) v = a_j;
                else if (a_p != SF_NONE && (!own || a_p >= t)) v = (int32_t)(i_cur + a_p);
                else myptr = t;
            }
            val[l] = v;
            ptr[l] = myptr;
            if (myptr != SF_NONE) chains[round & 1] = 1u;
        }
        if (l == 0) { first_conf[(round + 1) & 1] = SF_T; chains[(round + 1) & 1] = 0u; }
        sf_lds_barrier();
        uint32_t count = *fc;
        if (count > nvalid) count = nvalid;
        // chains: a step takes the value of an earlier one, which may itself be waiting (rare; usually no pointer at all;
        // a pointer of a step beyond the round's end is resolved too, harmlessly)
        if (chains[round & 1]) {
            for (;;) {
                int32_t got = 0;
                bool ok = false;
                if (myptr != SF_NONE && ptr[myptr] == SF_NONE) { got = val[myptr]; ok = true; }
                const int pending = __syncthreads_or(myptr != SF_NONE && !ok);   // (all reads of the iteration are done)
                if (ok) { val[l] = got; ptr[l] = SF_NONE; myptr = SF_NONE; }
                __syncthreads();
                if (!pending) break;
            }
        }
        if (valid && l < count) {
            const uint32_t my_last = (mx1 != 0u && mx1 - 1u < count) ? mx1 - 1u : (mn < count ? mn : SF_NONE);   // last processed step of key j
            if (!ASC) {
                A[i] = p2 == SF_NONE ? a_j : val[p2];
                if (j != (int32_t)i && (uint32_t)j + count <= i_cur && my_last == l) A[j] = val[l];
            } else {
                const uint32_t b = (imx1 != 0u && imx1 - 1u < count) ? imx1 - 1u : (imn < count ? imn : SF_NONE);   // last processed step with partner i
                if (!(b != SF_NONE && b > l)) A[i] = val[l];
                if (j != (int32_t)i && my_last == l) A[j] = (int32_t)i;
            }
        }
        sf_lds_barrier();   // every read of the tables and of val is done: clear what this round wrote, under the stores
        if (valid) {
            hkey[h] = SF_NONE; hmin[h] = SF_NONE; hmax[h] = 0u;
            const uint32_t t = ASC ? (uint32_t)j - i_cur : i_cur - (uint32_t)j;
            if (t < SF_T) { omin[t] = SF_NONE; omax[t] = 0u; }
        }
        if (top_up) { jring[sf & (SF_RING - 1)] = j_next; filled += SF_T; }   // (slots of steps already applied)
        done += count;
        ++round;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
}

int swaps_launch(sc_ctx *c, int32_t *table, int64_t n, int64_t p0, int64_t p1, bool inverse, int pw, bool full_rounds, hipStream_t s)
{
    void (*kernel)(const int32_t *, int32_t *, int64_t, uint32_t, int64_t, int64_t) = k_apply_swaps;
    unsigned grid = (unsigned)(p1 - p0), block = 64;
    if (full_rounds && n >= SWAPS_WG_MIN_N) { kernel = inverse ? k_apply_swaps_full<true> : k_apply_swaps_full<false>; block = SF_T; }
    else if (inverse || n >= SWAPS_WG_MIN_N) {
        if (pw == 2) { kernel = inverse ? k_apply_swaps_wg<true, 2> : k_apply_swaps_wg<false, 2>; grid = (unsigned)((p1 - p0 + 1) / 2); }
        else kernel = inverse ? k_apply_swaps_wg<true, 1> : k_apply_swaps_wg<false, 1>;
        block = pw == 2 ? 2 * SW_T : SW_T;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, c->pg.J.as<int32_t>(), table, c->p_stride, (uint32_t)n, p0, p1);
    SC_HIP(hipGetLastError());
    return SC_OK;
}

bool permgen_can_swap_inverse(int64_t n) { return n >= SWAPS_WG_MIN_N; }

// inverse = false: rows [p0, p1) of the permutation table (c->perm); true: of its inverse (c->inv), by the same
// transpositions in ascending order (workgroup kernel only: see permgen_can_swap_inverse)
int permgen_swap_chunk(sc_ctx *c, PermJob *job, int64_t p0, int64_t p1, hipStream_t s, bool inverse, int pw_req)
{
    if (job->trivial || p1 <= p0) {
        if (job->trivial && inverse && p1 > p0)
            SC_HIP(hipMemsetAsync(c->inv.as<int32_t>() + p0 * c->p_stride, 0, sizeof(int32_t) * (size_t)(c->p_stride * (p1 - p0)), s));
        return SC_OK;
    }
    SC_REQUIRE(!inverse || permgen_can_swap_inverse(job->n), SC_ERR_STATE, "permgen_swap_chunk: inverse tables need n >= %d",
               SWAPS_WG_MIN_N);
    KernelTimerScope ts(c, SC_K_PERM_SWAP, s);
    const char *pw_e = getenv("SC_SWAP_PW");   // (development and tests: A/B; read per call)
    const int pw_env = pw_e ? atoi(pw_e) : 0;
    const int pw = pw_env ? pw_env : pw_req;   // permutations per workgroup
    // r04 NEGATIVE RESULT, opt-in (SC_SWAP_FULL_ROUNDS=1): whole rounds of 1024 steps (k_apply_swaps_full).  1058 instead of
    // 2880 rounds per 10^6-step permutation, but a round of sixteen wavefronts on one CU is bound by instruction issue, not by
    // its trip to L2 (13 k clocks against 6 k): 6.2 instead of 7.2 ms per 128-permutation chunk alone; inside the Moran
    // pipeline the swaps take 77 instead of 115 ms per step and the generator's chain, which now finds 2048 instead of 1024
    // long-lived wavefronts and 128 KB of LDS per workgroup in its way, 148 instead of 131 ms: the step 161 against 157.5 ms.
    const bool full_rounds = getenv("SC_SWAP_FULL_ROUNDS") != nullptr;
    return swaps_launch(c, (inverse ? c->inv : c->perm).as<int32_t>(), job->n, p0, p1, inverse, pw, full_rounds, s);
}
