// A4 on the device: the numpy-exact permutation table, generated in parallel.  gfx950 only.
// numpy's stream (see sc_perm.hip header) is sequential: every Fisher-Yates step consumes a data-dependent number of 32-bit draws
// (masked rejection), so exactness needs the TRUE stream position of every step, and speculative chunking cannot be made exact
// (two offset rejection scans over the same draws never re-synchronise).  The generator is exact by construction and parallel:
//  A0  raw stream  PCG64 is an LCG, so output m is a pure function of m (jump-ahead in O(log m) 128-bit multiplies): one
//                  kernel writes the whole raw 32-bit stream (k_raw_stream).
//  A1  rejection   in blocks of 16384 draws.  Inside a block 1024 threads simulate their 16 draws each from a guessed number of
//                  accepts in front of them, until a prefix sum of the accept counts changes no guess (block_fixed_point,
//                  sc_permgen.h).  A block needs ONE number from its predecessors, the steps completed before it: one workgroup
//                  walks the blocks in order (k_scan), or -- from 131072 cells on, while the context's streams overlap -- the
//                  chip prepares every block for a window of entry states, one workgroup chains the exact states through them
//                  and the chip verifies every block (sc_permgen_phi.hip; a job that fails is rerun with k_scan).  k_expand
//                  turns the accept masks into J[step], the accepted value j of every Fisher-Yates step.
//  B   swaps       permutations are independent given J: rounds of consecutive swaps that touch pairwise-distinct slots are
//                  applied in parallel, which equals the sequential shuffle bit for bit (sc_swaps.hip).
// This unit: the job (permgen_begin -> permgen_scan_chunk per chunk of permutations -> permgen_finish), A0, the sequential A1,
// the expansion.  sc_permgen_phi.hip: the block-parallel A1.  sc_swaps.hip: B.  sc_perm_counter.hip: the counter-based source,
// which shares B and nothing else.  sc_perm.hip: host generator, table, pipeline.  sc_permgen.h: what they share.
#include <stdio.h>

#include "sc_permgen.h"

// ---- A0: the raw 32-bit stream, stored in the layout the scan reads (sc_permgen.h) ----
__global__ __launch_bounds__(256) void k_raw_stream(uint64_t st_hi, uint64_t st_lo, uint64_t inc_hi,
                                                    uint64_t inc_lo, uint64_t n_blocks, uint64_t jm_hi,
                                                    uint64_t jm_lo, uint64_t jp_hi, uint64_t jp_lo,
                                                    uint32_t *__restrict__ raw)
{
    const u128 state0 = ((u128)st_hi << 64) | st_lo, inc = ((u128)inc_hi << 64) | inc_lo;
    const u128 jm = ((u128)jm_hi << 64) | jm_lo, jp = ((u128)jp_hi << 64) | jp_lo;  // LCG^16384
    const u128 mult = pcg_mult();
    // thread = (block group, g, tau): consecutive threads write consecutive 16-byte groups
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t tau = (uint32_t)(t % SCAN_THREADS), g = (uint32_t)((t / SCAN_THREADS) % SCAN_GROUPS);
    uint64_t b = (t / (SCAN_THREADS * SCAN_GROUPS)) * RAW_BLOCKS;
    if (b >= n_blocks) return;
    // first draw of the group: r = b*SCAN_BLOCK + SCAN_D*tau + 4*g  ->  64-bit output m = r / 2
    const uint64_t m = b * (SCAN_BLOCK / 2) + (uint64_t)(SCAN_D / 2) * tau + 2ull * g;
    const Affine j = lcg_pow(inc, m + 1);  // output m is made from the state after m + 1 steps
    u128 s = j.mult * state0 + j.plus;
    for (int k = 0; k < RAW_BLOCKS && b < n_blocks; ++k, ++b) {
        const uint64_t o0 = xsl_rr32(s);
        const uint64_t o1 = xsl_rr32(s * mult + inc);
        uint4 v;
        v.x = (uint32_t)o0; v.y = (uint32_t)(o0 >> 32); v.z = (uint32_t)o1; v.w = (uint32_t)(o1 >> 32);
        *reinterpret_cast<uint4 *>(raw + b * SCAN_BLOCK + (uint64_t)g * (4 * SCAN_THREADS) + 4ull * tau) = v;
        s = jm * s + jp;
    }
}

// ------------------------------------------------------------------------------------------------
// A1: rejection scan by one workgroup
// ------------------------------------------------------------------------------------------------

// Per processed block the scan leaves: sblk[b] = steps completed before the block, and per thread
// acc_bits[b*SCAN_THREADS + tau], enter[b*SCAN_THREADS + tau] (accepted steps of the block in front of the thread).
// k_expand turns these into J with the whole chip; one CU cannot store 4 bytes per step fast enough.
//
// st[0] = steps completed so far, st[1] = next block to process, st[2] = sticky failure flags,
// st[3] = number of raw draws consumed when the job's last step completed.
// A launch processes WHOLE blocks while fewer than S_target steps are complete (the last block may
// run past the target; only the end of the job, total_steps, stops mid-block).
// This is the sequential form of the scan: every block is entered with the exact state its predecessor
// left.  It is the whole generator for short permutations and the fallback of the block-parallel form below.
__global__ __launch_bounds__(SCAN_THREADS) void k_scan(const uint32_t *__restrict__ raw, uint64_t n_blocks,
                                                       uint32_t n, uint64_t S_target, uint64_t total_steps,
                                                       bits_t *__restrict__ acc_bits,
                                                       uint32_t *__restrict__ enter,
                                                       unsigned long long *__restrict__ sblk,
                                                       unsigned long long *__restrict__ st)
{
    __shared__ BlockShared sh;
    static_assert(SCAN_THREADS % 64 == 0 && SCAN_D % 4 == 0 && SCAN_D <= 64, "scan geometry");
    const uint32_t tau = threadIdx.x;
    const uint32_t M = n - 1;
    const uint32_t top_mask = mask_of(M);
    uint64_t S_block = st[0];
    uint64_t b = st[1];
    uint32_t rem_block = M - (uint32_t)(S_block % M);
    uint32_t parity = 0;
    int failed = 0;
    uint64_t endpos = 0;

    uint32_t un[SCAN_D];  // the next block's draws, loaded while the current block is processed
    if (b < n_blocks) scan_load(raw, b * SCAN_BLOCK, tau, un);
    for (; b < n_blocks && S_block < S_target; ++b) {
        uint32_t u[SCAN_D];
#pragma unroll
        for (int s = 0; s < SCAN_D; ++s) u[s] = un[s];
        if (b + 1 < n_blocks) scan_load(raw, (b + 1) * SCAN_BLOCK, tau, un);
        ScanRes r;
        uint32_t excl, total_cnt;
        if (block_fixed_point(u, S_block, rem_block, M, top_mask, total_steps, sh, parity, r, excl, total_cnt) > 0) {
            failed = 1;
            break;
        }
        acc_bits[b * SCAN_THREADS + tau] = r.bits;
        enter[b * SCAN_THREADS + tau] = excl;
        if (tau == 0) sblk[b] = S_block;
        if (r.end) endpos = b * SCAN_BLOCK + (uint64_t)tau * SCAN_D + r.end;
        S_block += total_cnt;
        rem_block = rem_advance(rem_block, total_cnt, M);
    }
    if (endpos) st[3] = endpos;  // exactly one thread of one launch sees the job's last step
    if (tau == 0) {
        st[0] = S_block;
        st[1] = b;
        if (failed) st[2] = st[2] | 1ull;
    }
}

// J[step] for every accepted draw of blocks [range[0], range[1]) -- the whole chip, one workgroup per scan block
// at a time, one thread per scan thread.  The accepted draws of a block are the contiguous run
// J[sblk[b] .. sblk[b] + count): a thread that stored its own up-to-16 draws at its own offset made every store
// instruction of a wavefront touch 64 separate segments (13.0 GB written per bench step for a J of 4.0 GB).  So the
// threads put their draws into LDS at enter[] -- shifted by sblk[b] & 3, so that LDS word 4 v lands on a 16-byte
// boundary of J -- and the workgroup writes the run as 16-byte stores; the words of the first and the last group
// that belong to the neighbouring blocks' runs (or lie past the job's end) are left to them: single 4-byte stores.
__global__ __launch_bounds__(SCAN_THREADS) void k_expand(const uint32_t *__restrict__ raw,
                                                         const bits_t *__restrict__ acc_bits,
                                                         const uint32_t *__restrict__ enter,
                                                         const unsigned long long *__restrict__ sblk,
                                                         const unsigned long long *__restrict__ range, uint32_t n,
                                                         uint64_t total_steps, int32_t *__restrict__ J)
{
    __shared__ int4 stage4[SCAN_BLOCK / 4 + 1];
    __shared__ uint32_t block_cnt;
    int32_t *stage = reinterpret_cast<int32_t *>(stage4);
    const uint32_t tau = threadIdx.x;
    const uint32_t M = n - 1;
    const uint32_t top_mask = mask_of(M);
    for (uint64_t b = range[0] + blockIdx.x; b < range[1]; b += gridDim.x) {
        const bits_t bits = acc_bits[b * SCAN_THREADS + tau];
        const uint32_t ent = enter[b * SCAN_THREADS + tau];
        const uint64_t S0 = sblk[b];
        const uint32_t a = (uint32_t)S0 & 3u;
        if (tau == SCAN_THREADS - 1) block_cnt = ent + (uint32_t)__popcll((unsigned long long)bits);
        if (bits) {
            const uint64_t S = S0 + ent;
            uint32_t i = M - (uint32_t)(S % M);
            uint32_t mask = mask_of(i);
            uint32_t pos = a + ent;
            const uint4 *src = reinterpret_cast<const uint4 *>(raw + b * SCAN_BLOCK) + tau;
#pragma unroll
            for (int q = 0; q < SCAN_D / 4; ++q) {
                if (!((uint32_t)(bits >> (4 * q)) & 0xfu)) continue;
                const uint4 v4 = src[q * SCAN_THREADS];
                const uint32_t vv[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if ((uint32_t)(bits >> (4 * q + e)) & 1u) {
                        if (pos < SCAN_BLOCK + 4) stage[pos] = (int32_t)(vv[e] & mask);   // (always, unless the scan's tables are broken)
                        ++pos; --i;
                        if (i == 0) { i = M; mask = top_mask; }
                        else if (i <= (mask >> 1)) mask >>= 1;
                    }
                }
            }
        }
        __syncthreads();
        // the run in LDS words: [a, end); word w is J[S0 - a + w]; cut at the job's end
        uint32_t cnt = block_cnt < (uint32_t)SCAN_BLOCK ? block_cnt : (uint32_t)SCAN_BLOCK;
        if (S0 >= total_steps) cnt = 0;
        else if (total_steps - S0 < cnt) cnt = (uint32_t)(total_steps - S0);
        const uint32_t end = a + cnt;
        int32_t *dst = J + (S0 - a);   // 16-byte aligned
        for (uint32_t w = 4 * tau; w < end; w += 4 * SCAN_THREADS) {
            if (w >= a && w + 4 <= end) {
                *reinterpret_cast<int4 *>(dst + w) = stage4[w / 4];
            } else {
#pragma unroll
                for (uint32_t e = 0; e < 4; ++e)
                    if (w + e >= a && w + e < end) dst[w + e] = stage[w + e];
            }
        }
        __syncthreads();   // the next block's draws overwrite the staging buffer
    }
}

// ---- host orchestration ----
static double expected_draws_per_perm(int64_t n)
{
    double e = 0.0;
    for (int64_t i = 1; i < n; ++i) e += ((double)smear_mask((uint32_t)i) + 1.0) / ((double)i + 1.0);
    return e;
}

int permgen_begin(sc_ctx *c, const uint64_t *state6, int64_t n, int64_t n_perm, int units_ahead, PermJob *job, hipStream_t s)
{
    job->n = n;
    job->n_perm = n_perm;
    job->h = state6[4] ? 1 : 0;
    job->st_hi = state6[0]; job->st_lo = state6[1]; job->inc_hi = state6[2]; job->inc_lo = state6[3];
    job->buffered = (uint32_t)state6[5];
    job->trivial = (n == 1);
    if (job->trivial) {  // nothing is drawn, every permutation is [0]
        SC_HIP(hipMemsetAsync(c->perm.p, 0, sizeof(int32_t) * (size_t)(c->p_stride * n_perm), s));
        return SC_OK;
    }
    const int64_t M = n - 1;
    const u128 inc = ((u128)job->inc_hi << 64) | job->inc_lo;
    job->total_steps = (uint64_t)n_perm * (uint64_t)M;
    // raw draws: expectation + 0.3 % + slack (the spread of the total is ~sqrt(total), far below that)
    job->draws_per_perm = expected_draws_per_perm(n);
    const double want = (double)n_perm * job->draws_per_perm * 1.003 + 262144.0;
    const uint64_t n_blocks = ((uint64_t)want + SCAN_BLOCK - 1) / SCAN_BLOCK;
    job->hi = n_blocks * SCAN_BLOCK;  // raw draw r = half (r & 1) of 64-bit output r / 2
    SC_TRY(c->pg.raw.ensure(sizeof(uint32_t) * (size_t)job->hi, &c->mem));
    SC_TRY(c->pg.J.ensure(sizeof(int32_t) * (size_t)job->total_steps, &c->mem));
    SC_TRY(c->pg.bits.ensure(sizeof(bits_t) * (size_t)(n_blocks * SCAN_THREADS), &c->mem));
    SC_TRY(c->pg.enter.ensure(sizeof(uint32_t) * (size_t)(n_blocks * SCAN_THREADS), &c->mem));
    SC_TRY(c->pg.sblk.ensure(sizeof(unsigned long long) * (size_t)(n_blocks + 1), &c->mem));
    SC_TRY(phi_begin(c, job, units_ahead, n_blocks, s));
    // pg.out: [0..3] scan state, [4] prepared blocks used, [5] blocks computed by the chain, then one
    // {first block, end block} pair per chunk for k_expand
    const int64_t chunks = ceil_div64(n_perm, PERM_CHUNK) + 2;  // the fused pipeline splits its first chunk
    SC_TRY(c->pg.out.ensure(sizeof(unsigned long long) * (size_t)(8 + 2 * (chunks + 1)), &c->mem));
    // A generator that starts with a buffered 32-bit half: that half is the first draw of the
    // stream.  It is consumed here, so that raw draw 0 is always the low half of output 0.
    unsigned long long st0[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (job->h) {
        const uint32_t v = job->buffered & smear_mask((uint32_t)M);
        if (v <= (uint32_t)M) {  // first Fisher-Yates step (i = n-1) accepts it
            const int32_t j0 = (int32_t)v;
            SC_HIP(hipMemcpyAsync(c->pg.J.p, &j0, sizeof(int32_t), hipMemcpyHostToDevice, s));
            st0[0] = 1;
        }
    }
    SC_HIP(hipMemcpyAsync(c->pg.out.p, st0, sizeof(st0), hipMemcpyHostToDevice, s));
    SC_HIP(hipMemcpyAsync(c->pg.sblk.p, st0, sizeof(unsigned long long), hipMemcpyHostToDevice, s));  // state at block 0
    SC_HIP(hipStreamSynchronize(s));  // st0 / j0 are stack variables
    const Affine jb = lcg_pow(inc, SCAN_BLOCK / 2);
    const uint64_t threads = ((n_blocks + RAW_BLOCKS - 1) / RAW_BLOCKS) * (uint64_t)(SCAN_THREADS * SCAN_GROUPS);
    hipLaunchKernelGGL(k_raw_stream, dim3((unsigned)(threads / 256)), dim3(256), 0, s, job->st_hi, job->st_lo,
                       job->inc_hi, job->inc_lo, n_blocks, (uint64_t)(jb.mult >> 64), (uint64_t)jb.mult,
                       (uint64_t)(jb.plus >> 64), (uint64_t)jb.plus, c->pg.raw.as<uint32_t>());
    SC_HIP(hipGetLastError());
    if (job->phi) SC_HIP(hipEventRecord(c->pg.ev[32], s));  // the preparation streams start after the raw stream
    return SC_OK;
}

// Advance the rejection scan until permutations [0, p1) are complete, then expand the accept masks
// of the blocks it processed into J (both on stream s; the expansion uses the whole chip).
int permgen_scan_chunk(sc_ctx *c, PermJob *job, int64_t p1, hipStream_t s, hipStream_t post, hipEvent_t done)
{
    if (job->trivial) return SC_OK;
    unsigned long long *st = c->pg.out.as<unsigned long long>();
    unsigned long long *range = st + 8 + 2 * job->chunk_no;
    // range[0] = first block of this launch (= st[1] now), range[1] = st[1] afterwards
    SC_HIP(hipMemcpyAsync(range, st + 1, sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    // blocks this launch can have covered: the chunk's expected draws + 1 % + 2 blocks (block-parallel: those it was granted)
    uint64_t max_blocks = (uint64_t)((double)(p1 - job->p_done) * job->draws_per_perm * 1.01 / SCAN_BLOCK) + 3;
    unsigned fill_streams = 0;
    if (job->phi) {
        SC_TRY(phi_chain_chunk(c, job, p1, s, &max_blocks, &fill_streams));
    } else {
        KernelTimerScope ts(c, SC_K_PERM_SCAN, s);
        hipLaunchKernelGGL(k_scan, dim3(1), dim3(SCAN_THREADS), 0, s, c->pg.raw.as<uint32_t>(), job->hi / SCAN_BLOCK,
                           (uint32_t)job->n, (uint64_t)p1 * (uint64_t)(job->n - 1), job->total_steps, c->pg.bits.as<bits_t>(),
                           c->pg.enter.as<uint32_t>(), c->pg.sblk.as<unsigned long long>(), st);
    }
    SC_HIP(hipMemcpyAsync(range + 1, st + 1, sizeof(unsigned long long), hipMemcpyDeviceToDevice, s));
    // Verification and expansion of the chunk use the whole chip for ~2.5 ms: on `post` (if given) they do not hold
    // up the chain of the next chunk on s.  They only read what this chunk's chain left and write J.
    hipStream_t sp = post ? post : s;
    if (sp != s) {
        SC_HIP(hipEventRecord(c->pg.ev[33], s));
        SC_HIP(hipStreamWaitEvent(sp, c->pg.ev[33], 0));
    }
    if (job->phi) SC_TRY(phi_verify_chunk(c, job, range, max_blocks, fill_streams, sp));
    hipLaunchKernelGGL(k_expand, dim3((unsigned)max_blocks), dim3(SCAN_THREADS), 0, sp, c->pg.raw.as<uint32_t>(),
                       c->pg.bits.as<bits_t>(), c->pg.enter.as<uint32_t>(), c->pg.sblk.as<unsigned long long>(), range,
                       (uint32_t)job->n, job->total_steps, c->pg.J.as<int32_t>());
    if (done) SC_HIP(hipEventRecord(done, sp));
    SC_HIP(hipGetLastError());
    job->p_done = p1;
    job->chunk_no += 1;
    return SC_OK;
}

// after every stream that ran chunks has been synchronised: verify and write the final state
int permgen_finish(sc_ctx *c, PermJob *job, uint64_t *state6)
{
    if (job->trivial) return SC_OK;
    unsigned long long st[8];
    SC_HIP(hipMemcpy(st, c->pg.out.p, sizeof(st), hipMemcpyDeviceToHost));
    if (job->phi) { c->pg.blocks_prepared += (int64_t)st[4]; c->pg.blocks_chain += (int64_t)st[5]; }
    if (job->phi && st[2] != 0) {  // verification of the block-parallel scan failed: the caller reruns sequentially
        c->pg.fallbacks += 1;
        sc_set_error("sc_perm_generate: block-parallel scan failed its verification (flags %llu)", st[2]);
        if (st[2] & 24ull) {   // a hand-over wait gave up (flags 8 / 16): later jobs take the sequential scan at once
            c->pg.streams_serial = true;
            c->pg.note = "a hand-over wait of the block-parallel permutation generator gave up after 1 s (kernels of its streams did "
                         "not overlap: GPU shared with another process, a profiler, too few hardware queues); this context now uses "
                         "the sequential scan (same results); sc_ctx_set_permgen_mode(ctx, 0) re-arms the block-parallel form";
        } else {   // (a one-off: the context stays on the block-parallel form, but the event is on record)
            char buf[200];
            snprintf(buf, sizeof(buf), "a block-parallel permutation job failed its verification (flags %llu) and was rerun with the "
                     "sequential scan (same results)", st[2]);
            c->pg.note = buf;
        }
        return SC_PERMGEN_RETRY;
    }
    SC_REQUIRE(st[2] == 0, SC_ERR_STATE, "sc_perm_generate: rejection scan did not converge");
    (job->phi ? c->pg.jobs_parallel : c->pg.jobs_sequential) += 1;
    SC_REQUIRE(st[0] == job->total_steps, SC_ERR_STATE,
               "sc_perm_generate: raw stream exhausted after %llu of %llu steps", st[0],
               (unsigned long long)job->total_steps);
    const uint64_t h = job->h;
    const uint64_t pos = st[3] + h;  // draws consumed: raw draws + the buffered half taken on the host
    const u128 state0 = ((u128)job->st_hi << 64) | job->st_lo, inc = ((u128)job->inc_hi << 64) | job->inc_lo;
    if (pos > h) {
        const uint64_t tl = pos - 1;           // last consumed position (>= h)
        const uint64_t m_last = (tl - h) / 2;  // its 64-bit output
        const Affine a = lcg_pow(inc, m_last + 1);
        const u128 sN = a.mult * state0 + a.plus;
        state6[0] = (uint64_t)(sN >> 64);
        state6[1] = (uint64_t)sN;
        state6[4] = ((tl - h) & 1) == 0 ? 1 : 0;  // low half consumed -> high half buffered
        state6[5] = (uint32_t)(xsl_rr(sN) >> 32);
    } else if (pos == 1 && h == 1) {
        state6[4] = 0;  // only the buffered half was consumed; uinteger keeps its value
    }
    return SC_OK;
}

static int perm_generate_once(sc_ctx *c, uint64_t *state6, int64_t n, int64_t n_perm)
{
    if (permgen_is_block_parallel(c, n) && n_perm > 3 * PERM_CHUNK) {
        // a long job: the chunked pipeline of the seeded statistics with nothing to consume -- the Fisher-Yates swaps of
        // chunk k run (on their own streams) beside the rejection scan of chunk k + 1 instead of all behind the scan
        // (r03, 999 permutations of 1M cells: 55 ms of swaps out of the call's critical path)
        const int rc = sc_perm_pipeline(c, state6, n, n_perm, 0, 2, nullptr, nullptr, [](int64_t, int64_t) -> int { return SC_OK; });
        if (rc == SC_OK) c->perm_forward_valid = true;
        return rc;
    }
    PermJob job;
    if (permgen_is_block_parallel(c, n)) SC_TRY(permgen_place_streams(c, SR_SCORE));   // (first such job of the context only)
    SC_TRY(permgen_begin(c, state6, n, n_perm, 1, &job, c->stream));
    for (int64_t p0 = 0; p0 < n_perm; p0 += PERM_CHUNK) {
        const int64_t p1 = p0 + PERM_CHUNK < n_perm ? p0 + PERM_CHUNK : n_perm;
        SC_TRY(permgen_scan_chunk(c, &job, p1, c->stream, nullptr, nullptr));
    }
    SC_TRY(permgen_swap_chunk(c, &job, 0, n_perm, c->stream, false, 1));
    c->perm_forward_valid = true;
    SC_HIP(hipStreamSynchronize(c->stream));
    SC_TRY(c->pg.sync());
    return permgen_finish(c, &job, state6);
}

int sc_perm_generate_device(sc_ctx *c, uint64_t *state6, int64_t n, int64_t n_perm)
{
    // (state6 is only written on success: nothing to undo before the sequential rerun)
    return permgen_rerun_on_failure(c, [&]() { return perm_generate_once(c, state6, n, n_perm); }, nullptr);
}
