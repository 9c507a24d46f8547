// Context, error and timer plumbing of libspatialcore_hip.so.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include "sc_permgen.h"

static thread_local char g_err[1024] = "";

// The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4), and kernels of
// streams that share a hardware queue run strictly one after the other.  The generator / scoring pipeline of
// sc_moran_seeded uses eleven streams whose kernels should overlap (a 25-ms scoring launch in front of the generator's
// sub-millisecond chain launches doubles the step), so the library asks for one hardware queue per stream -- before
// the runtime initialises, i.e. when the library is loaded, and only if the user has not set the variable.  It is a
// REQUEST, not a requirement: a host application that initialised HIP earlier (or set a smaller value) keeps its
// setting; the context then spreads its streams over the stream priority levels, each of which has the setting's
// worth of queues, probes them before its first block-parallel job (permgen_place_streams), uses the sequential scan
// when they still cannot overlap, and says so through sc_ctx_permgen_note (logged once by the Python layer).
// 24 = two contexts' worth: a context creates up to 11 streams, and once a process's streams outnumber the setting the
// runtime lets them SHARE queues (r03: with 16, a second context in one process found its generator streams on shared
// queues and fell back; 24 and 32 were measured: same bench step as 16, every test with two live contexts green).
__attribute__((constructor)) static void sc_request_hw_queues(void) { setenv("GPU_MAX_HW_QUEUES", "24", 0); }

void sc_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int DBuf::ensure(size_t bytes, int64_t *charge_to)
{
    if (bytes <= cap) return SC_OK;
    release();
    acct = charge_to;
    // round up so that small growth does not re-allocate
    size_t want = (bytes + 255) & ~(size_t)255;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
        p = nullptr;
        sc_set_error("hipMalloc(%zu bytes) failed: %s", want, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? SC_ERR_NOMEM : SC_ERR_HIP;
    }
    cap = want;
    *acct += (int64_t)cap;
    return SC_OK;
}

void DBuf::release()
{
    if (p) {
        (void)hipFree(p);
        *acct -= (int64_t)cap;
    }
    p = nullptr;
    cap = 0;
}

sc_ctx::sc_ctx() { pg.streams = &streams; }
sc_ctx::~sc_ctx() = default;

// ---- the context's streams (sc_ctx.h: StreamTable) ----
int StreamTable::ensure(int role)
{
    if (s[role]) return SC_OK;
    if (placement != SC_PLACE_SPREAD) {
        SC_HIP(hipStreamCreateWithFlags(&s[role], hipStreamNonBlocking));
        return SC_OK;
    }
    int least = 0, greatest = 0;   // numerically: greatest priority <= normal (0) <= least priority
    SC_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    const int prio = level[role] == SL_HIGH ? greatest : level[role] == SL_LOW ? least : 0;
    SC_HIP(hipStreamCreateWithPriority(&s[role], hipStreamNonBlocking, prio));
    return SC_OK;
}

int StreamTable::sync(unsigned roles)
{
    for (int r = 0; r < SR_COUNT; ++r)
        if ((roles >> r & 1u) && s[r]) SC_HIP(hipStreamSynchronize(s[r]));
    return SC_OK;
}

int StreamTable::replace(int new_placement, const int *new_level)
{
    bool same = new_placement == placement;
    for (int r = 0; r < SR_COUNT && same && placement == SC_PLACE_SPREAD; ++r) same = level[r] == new_level[r];
    if (same) return SC_OK;
    // The context stream stays what it is: a timer scope around the caller holds its handle, and a stream of the normal
    // level is a plain stream -- which is why sc_streams.h keeps SR_SCORE's group there.
    SC_REQUIRE(new_placement != SC_PLACE_SPREAD || new_level[SR_SCORE] == SL_NORMAL, SC_ERR_STATE,
               "stream placement: the context stream belongs on the normal level");
    bool had[SR_COUNT];
    for (int r = 0; r < SR_COUNT; ++r) {
        had[r] = s[r] != nullptr;
        if (s[r]) SC_HIP(hipStreamSynchronize(s[r]));
    }
    for (int r = 0; r < SR_COUNT; ++r) {
        level[r] = new_placement == SC_PLACE_SPREAD ? new_level[r] : SL_NORMAL;
        if (r == SR_SCORE) continue;
        if (s[r]) (void)hipStreamDestroy(s[r]);
        s[r] = nullptr;
    }
    placement = new_placement;
    for (int r = 0; r < SR_COUNT; ++r)
        if (had[r]) SC_TRY(ensure(r));
    return SC_OK;
}

StreamTable::~StreamTable()
{
    for (hipStream_t sp : s)
        if (sp) (void)hipStreamDestroy(sp);
}

KTimer::~KTimer()
{
    for (auto *list : {&pending, &pool})
        for (auto &ev : *list) {
            (void)hipEventDestroy(ev.first);
            (void)hipEventDestroy(ev.second);
        }
}

KernelTimerScope::KernelTimerScope(sc_ctx *ctx, int kid, hipStream_t on) : c(ctx), id(kid), s(on ? on : ctx->stream)
{
    if (!c->timing) return;
    KTimer &t = c->timers[id];
    if (!t.pool.empty()) {
        a = t.pool.back().first;
        b = t.pool.back().second;
        t.pool.pop_back();
    } else {
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
            a = b = nullptr;
            return;
        }
    }
    (void)hipEventRecord(a, s);
}

KernelTimerScope::~KernelTimerScope()
{
    if (!a) return;
    (void)hipEventRecord(b, s);
    KTimer &t = c->timers[id];
    t.pending.emplace_back(a, b);
    t.launches += 1;
}

int sc_timer_collect(sc_ctx *c)
{
    SC_TRY(c->streams.sync(SR_MASK_PIPELINE));
    for (int k = 0; k < SC_K_END_; ++k) {
        KTimer &t = c->timers[k];
        for (auto &ev : t.pending) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) t.ms += ms;
            t.pool.push_back(ev);
        }
        t.pending.clear();
    }
    return SC_OK;
}

extern "C" {

int sc_version(void) { return 100; }

const char *sc_last_error(void) { return g_err; }

int sc_device_count(int *count)
{
    SC_REQUIRE(count, SC_ERR_INVALID, "sc_device_count: null pointer");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        sc_set_error("hipGetDeviceCount failed: %s", hipGetErrorString(e));
        return SC_ERR_HIP;
    }
    *count = n;
    return SC_OK;
}

int sc_ctx_create(int device, sc_ctx **out)
{
    SC_REQUIRE(out, SC_ERR_INVALID, "sc_ctx_create: null out pointer");
    *out = nullptr;
    int n = 0;
    SC_HIP(hipGetDeviceCount(&n));
    SC_REQUIRE(device >= 0 && device < n, SC_ERR_INVALID,
               "sc_ctx_create: device %d out of range (%d visible)", device, n);
    SC_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    SC_HIP(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
        sc_set_error("sc_ctx_create: device %d is %s; this library is built for gfx950 only", device,
                     prop.gcnArchName);
        return SC_ERR_STATE;
    }
    sc_ctx *c = new sc_ctx();
    c->device = device;
    const int rc = c->streams.ensure(SR_SCORE);
    if (rc != SC_OK) {
        delete c;
        return rc;
    }
    *out = c;
    return SC_OK;
}

int sc_ctx_destroy(sc_ctx *c)
{
    if (!c) return SC_OK;
    (void)hipSetDevice(c->device);
    sc_perm_pipe_abort(c);
    sc_graph_moments_drain(c);
    if (c->mom_host) (void)hipHostFree(c->mom_host);
    if (c->prep_host) (void)hipHostFree(c->prep_host);
    if (c->mom_ready) (void)hipEventDestroy(c->mom_ready);
    if (c->mom_done) (void)hipEventDestroy(c->mom_done);
    if (c->knn_done) (void)hipEventDestroy(c->knn_done);
    (void)hipStreamSynchronize(c->stream);
    // the members free themselves, in the order sc_ctx (sc_ctx.h) states: buffers and resident problems, the generator,
    // the timer events, the streams last
    delete c;
    return SC_OK;
}

int sc_ctx_sync(sc_ctx *c)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "null context");
    SC_HIP(hipSetDevice(c->device));
    SC_HIP(hipDeviceSynchronize());  // every stream of the device (what torch.cuda.synchronize() would do)
    return SC_OK;
}

// Development aid: copy `bytes` bytes at `offset` of one of the generator's device buffers to the host.
int sc_debug_copy(sc_ctx *c, int which, int64_t offset, void *out, int64_t bytes)
{
    SC_REQUIRE(c && out && offset >= 0 && bytes >= 0, SC_ERR_INVALID, "sc_debug_copy: bad argument");
    SC_HIP(hipSetDevice(c->device));
    const DBuf *bufs[] = {&c->pg.J, &c->pg.raw, &c->pg.bits, &c->pg.enter, &c->pg.sblk, &c->pg.out, &c->perm, &c->inv};
    SC_REQUIRE(which >= 0 && which < (int)(sizeof(bufs) / sizeof(bufs[0])), SC_ERR_INVALID, "sc_debug_copy: unknown buffer %d", which);
    const DBuf *b = bufs[which];
    SC_REQUIRE((size_t)(offset + bytes) <= b->cap, SC_ERR_INVALID, "sc_debug_copy: range exceeds the buffer (%zu bytes)", b->cap);
    SC_HIP(hipDeviceSynchronize());
    SC_HIP(hipMemcpy(out, (const char *)b->p + offset, (size_t)bytes, hipMemcpyDeviceToHost));
    return SC_OK;
}

int sc_ctx_kernel_time(sc_ctx *c, int kernel_id, double *ms, int64_t *launches)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "null context");
    SC_REQUIRE(kernel_id >= 0 && kernel_id < SC_K_END_, SC_ERR_INVALID, "bad kernel id %d", kernel_id);
    SC_TRY(sc_timer_collect(c));
    if (ms) *ms = c->timers[kernel_id].ms;
    if (launches) *launches = c->timers[kernel_id].launches;
    return SC_OK;
}

int sc_ctx_reset_timers(sc_ctx *c)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "null context");
    SC_TRY(sc_timer_collect(c));
    for (int k = 0; k < SC_K_END_; ++k) {
        c->timers[k].ms = 0.0;
        c->timers[k].launches = 0;
    }
    return SC_OK;
}

int sc_ctx_set_timing(sc_ctx *c, int enabled)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "null context");
    c->timing = enabled != 0;
    return SC_OK;
}

int sc_ctx_set_permgen_mode(sc_ctx *c, int mode)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "null context");
    SC_REQUIRE(mode >= 0 && mode <= 2, SC_ERR_INVALID, "sc_ctx_set_permgen_mode: mode %d not in {0, 1, 2}", mode);
    c->pg.rearm(mode);
    return SC_OK;
}

int sc_ctx_permgen_note(sc_ctx *c, const char **message)
{
    SC_REQUIRE(c && message, SC_ERR_INVALID, "null pointer");
    *message = c->pg.note.c_str();   // "" while the block-parallel generator is in use; valid until the next generator call
    return SC_OK;
}

int sc_ctx_set_moran_source_bits(sc_ctx *c, int min_bits)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "null context");
    SC_REQUIRE(min_bits == 4 || min_bits == 8 || min_bits == 16 || min_bits == 32 || min_bits == 64, SC_ERR_INVALID,
               "sc_ctx_set_moran_source_bits: %d not in {4, 8, 16, 32, 64}", min_bits);
    c->source_bits_min = min_bits;
    return SC_OK;
}

int sc_ctx_moran_source_bits(sc_ctx *c, int *bits)
{
    SC_REQUIRE(c && bits, SC_ERR_INVALID, "null pointer");
    *bits = c->last_source_bits;
    return SC_OK;
}

int sc_ctx_moran_lag_bits(sc_ctx *c, int *bits)
{
    SC_REQUIRE(c && bits, SC_ERR_INVALID, "null pointer");
    *bits = c->lag_u16 ? 16 : 64;
    return SC_OK;
}

int sc_ctx_moran_row_groups(sc_ctx *c, int *groups)
{
    SC_REQUIRE(c && groups, SC_ERR_INVALID, "null pointer");
    const int64_t gp = c->narrow_bits == 8 ? 128 : c->narrow_bits == 16 ? 64 : c->narrow_bits == 32 ? 32 : 16;
    *groups = c->narrow_bits == 4 ? c->nib_groups : (int)ceil_div64(c->e_tiles * SC_TILE, gp);
    return SC_OK;
}

int sc_ctx_permgen_stats(sc_ctx *c, int64_t *jobs_parallel, int64_t *jobs_sequential, int64_t *fallbacks,
                         int64_t *blocks_prepared, int64_t *blocks_chain)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "null context");
    if (jobs_parallel) *jobs_parallel = c->pg.jobs_parallel;
    if (jobs_sequential) *jobs_sequential = c->pg.jobs_sequential;
    if (fallbacks) *fallbacks = c->pg.fallbacks;
    if (blocks_prepared) *blocks_prepared = c->pg.blocks_prepared;
    if (blocks_chain) *blocks_chain = c->pg.blocks_chain;
    return SC_OK;
}

int sc_ctx_device_mem(sc_ctx *c, int64_t *bytes)
{
    SC_REQUIRE(c && bytes, SC_ERR_INVALID, "null pointer");
    *bytes = c->mem;
    return SC_OK;
}

int sc_ctx_device_free(sc_ctx *c, int64_t *bytes_free)
{
    SC_REQUIRE(c && bytes_free, SC_ERR_INVALID, "null pointer");
    SC_HIP(hipSetDevice(c->device));
    size_t free_b = 0, total_b = 0;
    SC_HIP(hipMemGetInfo(&free_b, &total_b));
    *bytes_free = (int64_t)free_b;
    return SC_OK;
}

}  // extern "C"
