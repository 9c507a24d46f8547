// A4: numpy-exact permutation source.  gfx950 only.
//
// The reference draws its permutations from numpy: `rng = np.random.default_rng(seed)` followed by
// `rng.permutation(n)` / `rng.permutation(values)` per permutation (autocorrelation.py:839,879,
// 1109,324, 1367,1404; squidpy's _score_helper likewise).  numpy's algorithm (Generator.shuffle ->
// random_interval on PCG64): PCG64 = 128-bit LCG (mult 0x2360ed051fc65da44385df649fccf645) with the
// XSL-RR 64-bit output; 32-bit draws take the low half first and buffer the high half; a bounded
// draw on [0, i] masks with the next power of two minus one and rejects values > i; the shuffle is
// `for i = n-1 .. 1: j = interval(i); swap(a[i], a[j])`.
//
// The stream is sequential (rejections make the draws per permutation data dependent).  The host
// generator below is the simple exact form (sc_perm_numpy_host); the device table is produced by
// the parallel exact generator of sc_permgen.hip (its units: sc_permgen.h).
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "sc_permgen.h"

namespace {

struct Pcg64 {
    u128 state, inc;
    int has32;
    uint32_t buf;
};

inline uint64_t next64(Pcg64 &g)
{
    g.state = g.state * pcg_mult() + g.inc;
    return xsl_rr(g.state);
}

inline uint32_t next32(Pcg64 &g)
{
    if (g.has32) {
        g.has32 = 0;
        return g.buf;
    }
    uint64_t v = next64(g);
    g.has32 = 1;
    g.buf = (uint32_t)(v >> 32);
    return (uint32_t)v;
}

inline uint32_t bounded32(Pcg64 &g, uint32_t mx, uint32_t mask)
{
    uint32_t v;
    while ((v = next32(g) & mask) > mx) {}
    return v;
}

void load(Pcg64 &g, const uint64_t *s)
{
    g.state = ((u128)s[0] << 64) | s[1];
    g.inc = ((u128)s[2] << 64) | s[3];
    g.has32 = s[4] != 0;
    g.buf = (uint32_t)s[5];
}

void store(const Pcg64 &g, uint64_t *s)
{
    s[0] = (uint64_t)(g.state >> 64);
    s[1] = (uint64_t)g.state;
    s[2] = (uint64_t)(g.inc >> 64);
    s[3] = (uint64_t)g.inc;
    s[4] = (uint64_t)g.has32;
    s[5] = g.buf;
}

// one permutation of length n into a[0..n)
void shuffle_one(Pcg64 &g, int32_t *a, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) a[i] = (int32_t)i;
    if (n < 2) return;
    uint32_t mask = smear_mask((uint32_t)(n - 1));
    for (int64_t i = n - 1; i >= 1; --i) {
        // the mask only shrinks when i drops below a power of two
        while ((mask >> 1) >= (uint32_t)i) mask >>= 1;
        uint32_t j = bounded32(g, (uint32_t)i, mask);
        int32_t t = a[j];
        a[j] = a[i];
        a[i] = t;
    }
}

}  // namespace

extern "C" int sc_perm_numpy_host(uint64_t *state6, int64_t n, int64_t n_perm, int32_t *perm_out)
{
    SC_REQUIRE(state6 && (perm_out || n_perm == 0 || n == 0), SC_ERR_INVALID, "sc_perm_numpy_host: null pointer");
    SC_REQUIRE(n >= 0 && n <= 0x7fffffffLL && n_perm >= 0, SC_ERR_INVALID, "sc_perm_numpy_host: bad sizes");
    Pcg64 g;
    load(g, state6);
    for (int64_t p = 0; p < n_perm; ++p) shuffle_one(g, perm_out + p * n, n);
    store(g, state6);
    return SC_OK;
}

__global__ __launch_bounds__(256) void k_check_perm(const int32_t *__restrict__ perm, int64_t n, int64_t stride,
                                                    int64_t rows, int *__restrict__ flag)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t total = rows * n;
    int bad = 0;
    for (; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        int64_t r = t / n, i = t - r * n;
        int32_t v = perm[r * stride + i];
        if (v < 0 || v >= n) bad = 1;
    }
    if (bad) atomicOr(flag, 1);
}

int sc_perm_alloc(sc_ctx *c, int64_t n, int64_t n_perm)
{
    SC_REQUIRE(n >= 1 && n <= 0x7fffffffLL, SC_ERR_INVALID, "permutation length %lld out of range", (long long)n);
    SC_REQUIRE(n_perm >= 1, SC_ERR_INVALID, "n_perm must be >= 1");
    sc_perm_pipe_abort(c);   // a generator job begun with sc_moran_seeded_begin and never finished owns the table
    int64_t stride = align_up64(n, 32);
    // +32 elements of slack so that the 8-wide tail reads of the last row stay inside the buffer
    SC_TRY(c->perm.ensure(sizeof(int32_t) * (size_t)(stride * n_perm + 32), &c->mem));
    c->p_n = n;
    c->p_count = 0;
    c->p_stride = stride;
    c->perm_bijective = false;
    c->perm_checked = false;
    c->perm_forward_valid = true;
    c->inv_rows_valid = 0;
    return SC_OK;
}

extern "C" int sc_perm_set(sc_ctx *c, const int32_t *perm, int64_t n, int64_t n_perm)
{
    SC_REQUIRE(c && perm, SC_ERR_INVALID, "sc_perm_set: null pointer");
    SC_HIP(hipSetDevice(c->device));
    SC_TRY(sc_perm_alloc(c, n, n_perm));
    SC_TRY(c->perm_flag.ensure(sizeof(unsigned long long), &c->mem));
    SC_HIP(hipMemsetAsync(c->perm.p, 0, sizeof(int32_t) * (size_t)(c->p_stride * n_perm + 32), c->stream));
    SC_HIP(hipMemcpy2DAsync(c->perm.p, sizeof(int32_t) * (size_t)c->p_stride, perm, sizeof(int32_t) * (size_t)n,
                            sizeof(int32_t) * (size_t)n, (size_t)n_perm, hipMemcpyHostToDevice, c->stream));
    // every index must be a valid cell: the gather kernels trust the table
    SC_HIP(hipMemsetAsync(c->perm_flag.p, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(k_check_perm, dim3(2048), dim3(256), 0, c->stream, c->perm.as<int32_t>(), n, c->p_stride,
                       n_perm, c->perm_flag.as<int>());
    int flag = 0;
    SC_HIP(hipMemcpyAsync(&flag, c->perm_flag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    SC_REQUIRE(!flag, SC_ERR_INVALID, "sc_perm_set: table contains an index outside [0, %lld)", (long long)n);
    c->p_count = n_perm;
    return SC_OK;
}

extern "C" int sc_perm_generate(sc_ctx *c, uint64_t *state6, int64_t n, int64_t n_perm, int32_t *perm_out)
{
    SC_REQUIRE(c && state6, SC_ERR_INVALID, "sc_perm_generate: null pointer");
    SC_HIP(hipSetDevice(c->device));
    SC_TRY(sc_perm_alloc(c, n, n_perm));
    {
        KernelTimerScope ts(c, SC_K_PERMGEN);
        SC_TRY(sc_perm_generate_device(c, state6, n, n_perm));
    }
    c->p_count = n_perm;
    c->perm_bijective = true;  // generated rows are permutations by construction
    if (perm_out) {
        SC_HIP(hipMemcpy2DAsync(perm_out, sizeof(int32_t) * (size_t)n, c->perm.p, sizeof(int32_t) * (size_t)c->p_stride,
                                sizeof(int32_t) * (size_t)n, (size_t)n_perm, hipMemcpyDeviceToHost, c->stream));
        SC_HIP(hipStreamSynchronize(c->stream));
    }
    return SC_OK;
}

// ---- the generator / consumer pipeline of the seeded statistics ----
#define PIPE_FIRST 32        // permutations of the first pipeline chunk
#define PIPE_SWAP_STREAMS 2  // swap chunks in flight (they are latency-bound: two overlap almost for free)
#define PIPE_LOOKAHEAD 3     // chunks enqueued beyond the one whose scoring is enqueued next (pipe_consume)
// The job ends with what is left once the generator's chain has finished: the swaps of its last chunk (~10 ms whatever
// its size: one workgroup per permutation, latency-bound) and the consumption of every chunk not consumed yet.  Behind
// a 128-permutation chunk that is its swaps AND its 10-ms consumption; tapering chunks (PIPE_TAIL) leave a few milliseconds (bench
// step, same box, ms: one 32-permutation last chunk 173.5 / 174.6; 64,32: 172.4 / 178.8; 64,32,16: 172.8 / 173.1; 96,48,24: 169.4 / 169.4).

// The generator / consumer pipeline shared by sc_moran_seeded and sc_lee_seeded: numpy-exact permutation rows
// [0, n_perm) of length n are produced chunk by chunk on the generator's streams (stream2: rejection scan chain,
// stream_pg: its preparation, stream_px: verification + expansion, stream3/4: Fisher-Yates swaps) while
// `score(p0, p1)` consumes finished chunks on the context stream.  table: 0 = permutation rows (c->perm),
// 1 = inverse rows only (c->inv; the same transpositions in ascending order), 2 = both (rows + k_invert_perm).
// The consumer's set-up (`enqueue`, `complete`: pipe_consume) runs on the host after the first chunks of the generator
// have been enqueued (the generator is the longest chain and depends on nothing else).
static int pipe_generate(sc_ctx *c, PermPipe &pp, int64_t k)
{
    hipEvent_t &scanned = pp.ev[(size_t)(2 * k)], &swapped = pp.ev[(size_t)(2 * k + 1)];
    // Two swap kernels in flight only for the job's LAST chunks (r04).  A swap workgroup is 8 wavefronts that live ~10 ms;
    // two chunks' worth of them (256) spread over the ~96 CUs the scoring kernel leaves, next to the table builders' two-
    // wavefront workgroups, left no CU with the 16 free wavefront slots a 1024-thread preparation workgroup needs: the
    // chain's clock profile showed its units arriving 1-8 ms late behind every chunk boundary (55 k clocks of waiting per
    // permutation; 37 k with one swap kernel at a time).  The tapering last chunks arrive 2-6 ms apart after the chain
    // is all but done, and keep overlapping.
    const int64_t chunks = (int64_t)pp.bounds.size() - 1;
    const bool overlap = PIPE_SWAP_STREAMS > 1 && (k & 1) && k >= chunks - 3;
    hipStream_t sw = overlap ? c->stream4 : c->stream3;
    SC_HIP(hipEventCreateWithFlags(&scanned, hipEventDisableTiming));
    SC_HIP(hipEventCreateWithFlags(&swapped, hipEventDisableTiming));
    SC_TRY(permgen_scan_chunk(c, &pp.job, pp.bounds[(size_t)k + 1], c->stream2, c->stream_px, scanned));
    SC_HIP(hipStreamWaitEvent(sw, scanned, 0));
    // Two permutations per swap workgroup while the chain still runs -- workgroups of the preparation kernels' own size --
    // but only beside the Moran scoring kernel (the one consumer that fills its CUs with wavefronts that live for
    // milliseconds): there the step gains 5 ms (151 against 156).  Two permutations in lockstep take 13-15 ms per chunk
    // instead of 10-12, and a light consumer (Lee's row sums, the local counts) leaves the chain at 12.8 ms per chunk:
    // with the pairs the swap stream became the bottleneck (Lee 10 x 10 pairs: 27.8 against 24.9 ms per pair).
    const int pw = (k < chunks - 3 && c->score_leave_cus > 8) ? 2 : 1;
    SC_TRY(permgen_swap_chunk(c, &pp.job, pp.bounds[(size_t)k], pp.bounds[(size_t)k + 1], sw, pp.table == 1, pw));
    if (pp.table == 2) SC_TRY(invert_rows(c, pp.bounds[(size_t)k], pp.bounds[(size_t)k + 1], sw));
    SC_HIP(hipEventRecord(swapped, sw));
    pp.enqueued = k + 1;
    return SC_OK;
}

void pipe_drain(sc_ctx *c, PermPipe &pp)
{
    (void)c->streams.sync(SR_MASK_PIPELINE);   // (SR_FINALISE: a consumer's launches beside its scoring, Moran's finalise)
    for (hipEvent_t e : pp.ev)
        if (e) (void)hipEventDestroy(e);
    pp.ev.clear();
}

// Begin: allocations, chunk schedule, the generator's set-up and its first `chunks_ahead` chunks (all of them when
// chunks_ahead >= the number of chunks).  Needs nothing but n and the generator state -- no graph, no expression.
// units_ahead: launch units the scan's preparation runs ahead of its chain (permgen_begin).
int pipe_begin(sc_ctx *c, const uint64_t *state6, int64_t n, int64_t n_perm, int table, int units_ahead, PermPipe &pp,
               int64_t chunks_ahead, const std::function<int()> &after_first_chunk)
{
    SC_REQUIRE(state6, SC_ERR_INVALID, "permutation pipeline: null generator state");
    SC_REQUIRE(n_perm >= 1, SC_ERR_INVALID, "permutation pipeline: n_perm must be >= 1");
    SC_REQUIRE(table == 0 || permgen_can_swap_inverse(n) || table == 2, SC_ERR_STATE, "inverse-only tables need a longer permutation");
    SC_TRY(sc_perm_alloc(c, n, n_perm));
    // the resident table is being overwritten from here on: nothing may take it for valid until the job has been consumed
    // (sc_moran / sc_local_moran / sc_lee_shared with a resident table then fail with "holds 0 rows" instead of reading
    // rows the generator's streams are still writing)
    c->p_count = 0;
    c->inv_rows_valid = 0;
    c->perm_forward_valid = false;
    // (the pipeline's streams first, the preparation streams behind them: the order the runtime has always seen them in)
    for (int r : {SR_CHAIN, SR_EXPAND, SR_SWAP_A, SR_SWAP_B}) SC_TRY(c->streams.ensure(r));
    // first block-parallel job of the context only.  May replace the streams: they are taken from the table below here
    if (permgen_is_block_parallel(c, n)) SC_TRY(permgen_place_streams(c, SR_CHAIN));
    // allocations first (hipMalloc synchronises the device), then the streams run freely
    if (table >= 1) SC_TRY(c->inv.ensure(sizeof(int32_t) * (size_t)(c->p_stride * n_perm + 32), &c->mem));
    // chunk schedule: a short first chunk so that the consumer starts early, PERM_CHUNK each in the middle, a short
    // last chunk (the job ends with the swaps and the consumption of the last chunk after the scan is done)
    pp.bounds.clear();
    pp.bounds.push_back(0);
    if (n_perm > 3 * PERM_CHUNK) {
        const int64_t rest = (n_perm - PIPE_TAIL_TOTAL - PIPE_FIRST) % PERM_CHUNK;
        int64_t p = PIPE_FIRST;
        pp.bounds.push_back(p);
        if (rest > 0) { p += rest; pp.bounds.push_back(p); }   // the remainder: a chunk of its own, second
        for (; p < n_perm - PIPE_TAIL_TOTAL; ) { p += PERM_CHUNK; pp.bounds.push_back(p); }
        for (int64_t v : PIPE_TAIL) { p += v; pp.bounds.push_back(p); }
    } else {
        for (int64_t p = PERM_CHUNK; p < n_perm; p += PERM_CHUNK) pp.bounds.push_back(p);
        pp.bounds.push_back(n_perm);
    }
    const int64_t chunks = (int64_t)pp.bounds.size() - 1;
    // stream2: scan(0) scan(1) ...   stream3/4: swaps(k) (+ inverse(k)) after scan(k)   stream: score(k) after swaps(k)
    pp.ev.assign((size_t)chunks * 2, nullptr);
    pp.table = table; pp.n = n; pp.n_perm = n_perm; pp.enqueued = 0;
    for (int k = 0; k < 6; ++k) pp.state0[k] = state6[k];
    pp.job = PermJob();
    int rc = permgen_begin(c, state6, n, n_perm, units_ahead, &pp.job, c->stream2);
    for (int64_t k = 0; k < chunks && k < chunks_ahead && rc == SC_OK; ++k) {
        rc = pipe_generate(c, pp, k);
        if (k == 0 && rc == SC_OK && after_first_chunk) rc = after_first_chunk();
    }
    if (rc != SC_OK) pipe_drain(c, pp);
    return rc;
}

// Consume: the consumer's set-up runs once, then `score(p0, p1)` behind every chunk's
// swaps on the context stream, with the generator kept TWO chunks ahead in the host's enqueue order (r03 timeline: with
// one chunk ahead the chain sat idle for 5 ms behind the consumer's set-up; a chunk is some 250 API calls).
// The set-up is two callbacks.  `enqueue` only enqueues; `complete` is everything that waits for the device (and all of
// the set-up for a consumer that has no such split: it passes no `enqueue` and is run exactly as before).  Between the
// two the generator is topped up to PIPE_LOOKAHEAD + 1 chunks, what the loop below asks for as soon as it has enqueued the
// first chunk's scoring (k = 1), so that those launches are in their queues before the host waits and before the first
// scoring launch: DESIGN.md 4.3 for where that pays (a process whose streams share hardware queues) and where it does not.
int pipe_consume(sc_ctx *c, PermPipe &pp, uint64_t *state6, const std::function<int()> &enqueue,
                 const std::function<int()> &complete, const std::function<int(int64_t, int64_t)> &score)
{
    const int64_t chunks = (int64_t)pp.bounds.size() - 1;
    int rc = SC_OK;
    if (enqueue) {
        rc = enqueue();
        while (rc == SC_OK && pp.enqueued < chunks && pp.enqueued < PIPE_LOOKAHEAD + 1) rc = pipe_generate(c, pp, pp.enqueued);
    }
    if (rc == SC_OK && complete) rc = complete();
    c->perm_bijective = true;  // device-generated rows are permutations by construction
    c->perm_forward_valid = pp.table != 1;
    for (int64_t k = 0; k < chunks && rc == SC_OK; ++k) {
        while (rc == SC_OK && pp.enqueued < chunks && pp.enqueued < k + PIPE_LOOKAHEAD) rc = pipe_generate(c, pp, pp.enqueued);
        if (rc == SC_OK && hipStreamWaitEvent(c->stream, pp.ev[(size_t)(2 * k + 1)], 0) != hipSuccess) {
            sc_set_error("permutation pipeline: event plumbing failed");
            rc = SC_ERR_HIP;
        }
        if (rc == SC_OK) rc = score(pp.bounds[(size_t)k], pp.bounds[(size_t)k + 1]);
    }
    pipe_drain(c, pp);
    if (rc != SC_OK) return rc;
    SC_TRY(permgen_finish(c, &pp.job, state6));
    c->p_count = pp.n_perm;
    c->inv_rows_valid = pp.table >= 1 ? pp.n_perm : 0;
    return SC_OK;
}

void sc_perm_pipe_abort(sc_ctx *c)
{
    if (!c->pipe) return;
    pipe_drain(c, *c->pipe);
    c->pipe.reset();
    c->p_count = 0;
}

int sc_perm_pipeline(sc_ctx *c, uint64_t *state6, int64_t n, int64_t n_perm, int table, int units_ahead,
                     const std::function<int()> &enqueue, const std::function<int()> &complete,
                     const std::function<int(int64_t, int64_t)> &score)
{
    sc_perm_pipe_abort(c);   // (a job begun with sc_moran_seeded_begin and never finished)
    PermPipe pp;
    SC_TRY(pipe_begin(c, state6, n, n_perm, table, units_ahead, pp, 2));
    return pipe_consume(c, pp, state6, enqueue, complete, score);
}

int permgen_rerun_on_failure(sc_ctx *c, const std::function<int()> &attempt, const std::function<int()> &undo)
{
    int rc = attempt();
    if (rc != SC_PERMGEN_RETRY) return rc;
    if (undo) SC_TRY(undo());
    struct ModeRestore { sc_ctx *c; int mode; ~ModeRestore() { c->pg.mode = mode; } } restore{c, c->pg.mode};
    c->pg.mode = 1;
    return attempt();
}

// ---- inverse rows of the table (the Moran scoring kernels gather through them), and the forward table from them ----
#define INV_BLOCKS_PER_ROW 64

// inv[row][perm[row][i]] = i.  Blocks of one row share blockIdx % 8 (one XCD under round-robin placement,
// speed only) so that the 4n-byte inverse row is assembled in one L2.
__global__ __launch_bounds__(256) void k_invert_perm(const int32_t *__restrict__ perm, int32_t *__restrict__ inv,
                                                     int64_t n, int64_t stride, int rows)
{
    const int id = blockIdx.x;
    const int rest = id >> 3;
    const int row = (rest / INV_BLOCKS_PER_ROW) * 8 + (id & 7);
    const int part = rest % INV_BLOCKS_PER_ROW;
    if (row >= rows) return;
    const int64_t per = (n + INV_BLOCKS_PER_ROW - 1) / INV_BLOCKS_PER_ROW;
    const int64_t i0 = (int64_t)part * per, i1 = i0 + per < n ? i0 + per : n;
    const int32_t *src = perm + (int64_t)row * stride;
    int32_t *dst = inv + (int64_t)row * stride;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) dst[src[i]] = (int32_t)i;
}

__global__ __launch_bounds__(256) void k_check_inverse(const int32_t *__restrict__ perm,
                                                       const int32_t *__restrict__ inv, int64_t n, int64_t stride,
                                                       int64_t rows, int *__restrict__ flag)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = rows * n;
    int bad = 0;
    for (; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = t / n, i = t - r * n;
        if (inv[r * stride + perm[r * stride + i]] != (int32_t)i) bad = 1;
    }
    if (bad) atomicOr(flag, 1);
}

// inverse rows [p0, p1) of the active table on stream s
int invert_rows(sc_ctx *c, int64_t p0, int64_t p1, hipStream_t s)
{
    const int rows = (int)(p1 - p0);
    if (rows <= 0) return SC_OK;
    const int groups = (rows + 7) / 8;
    // (the table's own length, not the expression's: a generator job may run before any expression is loaded)
    hipLaunchKernelGGL(k_invert_perm, dim3((unsigned)(groups * INV_BLOCKS_PER_ROW * 8)), dim3(256), 0, s,
                       c->perm.as<int32_t>() + p0 * c->p_stride, c->inv.as<int32_t>() + p0 * c->p_stride, c->p_n,
                       c->p_stride, rows);
    SC_HIP(hipGetLastError());
    return SC_OK;
}

// After a seeded pipeline that only generated the inverse table: materialise the permutation table itself (the
// inverse of the inverse) for callers that use the resident table afterwards.
int sc_perm_forward_ensure(sc_ctx *c)
{
    if (c->perm_forward_valid || c->p_count <= 0) return SC_OK;
    const int rows = (int)c->p_count;
    const int groups = (rows + 7) / 8;
    hipLaunchKernelGGL(k_invert_perm, dim3((unsigned)(groups * INV_BLOCKS_PER_ROW * 8)), dim3(256), 0, c->stream,
                       c->inv.as<int32_t>(), c->perm.as<int32_t>(), c->p_n, c->p_stride, rows);
    SC_HIP(hipGetLastError());
    SC_HIP(hipStreamSynchronize(c->stream));
    c->perm_forward_valid = true;
    return SC_OK;
}

// The scoring kernels gather through the INVERSE rows, which exist only for true permutations: a table uploaded by
// the caller is checked once (inverse of the inverse).  *bijective = false: its rows are arbitrary index maps and
// take the index-row kernel (k_moran_perm).
int sc_perm_table_is_bijective(sc_ctx *c, int64_t n_perm, bool *bijective)
{
    *bijective = false;
    if (n_perm <= 0) return SC_OK;
    const int64_t rows = c->p_count > n_perm ? c->p_count : n_perm;  // the WHOLE table is checked once
    SC_TRY(c->inv.ensure(sizeof(int32_t) * (size_t)(c->p_stride * rows + 32), &c->mem));
    if (!c->perm_bijective && !c->perm_checked) {
        SC_TRY(invert_rows(c, 0, rows, c->stream));
        SC_TRY(c->perm_flag.ensure(sizeof(unsigned long long), &c->mem));
        SC_HIP(hipMemsetAsync(c->perm_flag.p, 0, sizeof(int), c->stream));
        hipLaunchKernelGGL(k_check_inverse, dim3(2048), dim3(256), 0, c->stream, c->perm.as<int32_t>(),
                           c->inv.as<int32_t>(), c->p_n, c->p_stride, rows, c->perm_flag.as<int>());
        int bad = 0;
        SC_HIP(hipMemcpyAsync(&bad, c->perm_flag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        SC_HIP(hipStreamSynchronize(c->stream));
        c->perm_checked = true;
        c->perm_bijective = (bad == 0);
        if (c->perm_bijective) c->inv_rows_valid = rows;
    }
    *bijective = c->perm_bijective;
    return SC_OK;
}
