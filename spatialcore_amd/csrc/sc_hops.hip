// sc_hops.hip -- sc_hop_*: the shells of a graph pattern (cells at shortest-path distance exactly l of every cell) hop by
// hop, and the mean / variance of an embedding over the resident shell: CellCharter's neighbourhood aggregation (Varrone
// et al. 2024; restated by tests/hops_restated.py).  The state lives on the device between sc_hop_begin
// and sc_hop_end; the loop over the hops is the caller's (spatial/hops.py).  gfx950 only.
//
// Expansion of shell l into shell l + 1, per cell i: an open-addressing table (integer atomicCAS on the key, the scheme
// of sc_louvain.hip's move kernel) first takes i and the shells 1 .. l of i as old keys; then the adjacency rows of shell
// l's members are read, 16 lanes a member, and every key whose insert succeeds is a new member.  The set of new members
// does not depend on which lane wins an insert, and the radix sort on (row << 32 | column) behind the fill puts them in
// ascending order: the shell is the same canonical CSR whichever class a row takes.  Classes by
//     bound(i) = 1 + sum_{s <= l} |S_s(i)| + sum_{j in S_l(i)} deg(j)      (at least the keys the table will hold)
//   wavefront: bound <= SC_HOP_WAVE_KEYS, a workgroup of one wavefront, at most 1024 slots of LDS;
//   workgroup: bound <= SC_HOP_WG_KEYS, 256 threads, at most 32768 slots (128 KiB of the CU's 160 KiB) of dynamic LDS: the
//              rows are launched by table size (2048, 4096, .. slots), so that small tables leave room for more workgroups;
//   global:    beyond, 256 threads, a table of 2 min(bound, n) slots rounded up to a power of two in global memory, in
//              batches whose tables take at most HOP_GLOBAL_BYTES together (one row alone may take more).
// A row uses the power of two >= 2 bound slots (at least 64) of its table, so a table is never more than half full.
// Count -> exclusive scan -> fill -> sort; the expansion runs twice.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>

#include "sc_lane_group.h"
#include "sc_sortscan.h"

namespace {

typedef unsigned long long u64;

constexpr int HOP_WAVE_SLOTS = 2 * SC_HOP_WAVE_KEYS;
constexpr int HOP_WG_SLOTS = 2 * SC_HOP_WG_KEYS;
constexpr int HOP_WG_SIZES = 5;   // table sizes of the workgroup class: 2 HOP_WAVE_SLOTS << 0 .. 4 = 2048 .. HOP_WG_SLOTS
static_assert((2 * HOP_WAVE_SLOTS) << (HOP_WG_SIZES - 1) == HOP_WG_SLOTS, "the workgroup class's table sizes end at HOP_WG_SLOTS");
constexpr int HOP_TPB = 256;
constexpr int64_t HOP_GLOBAL_BYTES = (int64_t)64 << 20;   // the tables of one batch of the global class
constexpr int64_t HOP_MARGIN_BYTES = (int64_t)64 << 20;   // kept free beside a new shell's arrays
constexpr uint32_t HOP_EMPTY = 0xffffffffu;
constexpr int HOP_DMAX = 64;

// the shells 1 .. count of the resident graph; shell 1 is the pattern itself, shell `count` the current one
struct HopShells {
    const int64_t *ptr[SC_HOP_MAX];
    const int32_t *idx[SC_HOP_MAX];
    int count;
};

__host__ __device__ __forceinline__ uint32_t hop_slots_for(long long keys)   // the power of two >= 2 keys, at least 64
{
    uint32_t s = 64;
    while ((long long)s < 2 * keys) s <<= 1;
    return s;
}

// true if c was not in the table; the table is never full (sizes above)
__device__ __forceinline__ bool hop_insert(uint32_t *tab, uint32_t mask, uint32_t shift, uint32_t c)
{
    uint32_t h = (c * 0x9E3779B1u) >> shift;
    for (;;) {
        const uint32_t old = atomicCAS(&tab[h], HOP_EMPTY, c);
        if (old == HOP_EMPTY) return true;
        if (old == c) return false;
        h = (h + 1u) & mask;
    }
}

// bound[i] of every row (the head of this file)
__global__ __launch_bounds__(256) void k_hop_bound(HopShells sh, int64_t n, long long *__restrict__ bound)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    long long b = 1;
    for (int s = 0; s < sh.count; ++s) b += sh.ptr[s][i + 1] - sh.ptr[s][i];
    const int64_t *__restrict__ aptr = sh.ptr[0];
    const int32_t *__restrict__ cur = sh.idx[sh.count - 1];
    for (int64_t p = sh.ptr[sh.count - 1][i], e = sh.ptr[sh.count - 1][i + 1]; p < e; ++p) b += aptr[cur[p] + 1] - aptr[cur[p]];
    bound[i] = b;
}

// One workgroup per row rows[blockIdx.x].  FILL = false: count[row] = new members; FILL = true: their (row << 32 | column)
// keys and columns at off[row] .. in any order.  GLOBAL: the table is gtab + gofs[blockIdx.x], gofs[blockIdx.x + 1] -
// gofs[blockIdx.x] slots (the host's 2 min(bound, n) rounded up); else lds_slots of LDS, static (SLOTS of them) or dynamic
// (SLOTS = 0), of which the row uses what it needs.
template <int TPB, int SLOTS, bool GLOBAL, bool FILL>
__global__ __launch_bounds__(TPB) void k_hop_expand(HopShells sh, const int32_t *__restrict__ rows, const long long *__restrict__ bound,
                                                    uint32_t *__restrict__ gtab, const int64_t *__restrict__ gofs, uint32_t lds_slots,
                                                    long long *__restrict__ count, const long long *__restrict__ off,
                                                    u64 *__restrict__ keys, uint32_t *__restrict__ vals)
{
    __shared__ uint32_t stab[SLOTS ? SLOTS : 1];
    extern __shared__ uint32_t dtab[];
    __shared__ int s_cnt;
    const int tid = threadIdx.x;
    const int32_t i = rows[blockIdx.x];
    const int last = sh.count - 1;
    const int64_t p0 = sh.ptr[last][i], p1 = sh.ptr[last][i + 1];
    if (p0 == p1) {   // nothing to expand: an empty shell stays empty
        if (!FILL && tid == 0) count[i] = 0;
        return;
    }
    uint32_t *tab = SLOTS ? stab : dtab;
    uint32_t slots;
    if (GLOBAL) {
        tab = gtab + gofs[blockIdx.x];
        slots = (uint32_t)(gofs[blockIdx.x + 1] - gofs[blockIdx.x]);
    } else {
        slots = hop_slots_for(bound[i]);
        if (slots > lds_slots) slots = lds_slots;   // never taken: the host classed the row by the same bound
    }
    const uint32_t mask = slots - 1u, shift = (uint32_t)__clz(slots) + 1u;
    if (!GLOBAL)   // (a batch's tables in global memory are cleared in front of its launch)
        for (uint32_t s = tid; s < slots; s += TPB) tab[s] = HOP_EMPTY;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    // the visited set: i and its shells so far
    if (tid == 0) hop_insert(tab, mask, shift, (uint32_t)i);
    for (int s = 0; s <= last; ++s) {
        const int32_t *__restrict__ idx = sh.idx[s];
        for (int64_t p = sh.ptr[s][i] + tid, e = sh.ptr[s][i + 1]; p < e; p += TPB) hop_insert(tab, mask, shift, (uint32_t)idx[p]);
    }
    __syncthreads();
    // the members' rows, 16 lanes a member
    const int64_t *__restrict__ aptr = sh.ptr[0];
    const int32_t *__restrict__ aidx = sh.idx[0];
    const int32_t *__restrict__ cur = sh.idx[last];
    const int sub = tid >> 4, l16 = tid & 15;
    const long long base = FILL ? off[i] : 0;
    int mine = 0;
    for (int64_t m = p0 + sub; m < p1; m += TPB / 16) {
        const int32_t j = cur[m];
        for (int64_t p = aptr[j] + l16, e = aptr[j + 1]; p < e; p += 16) {
            const uint32_t c = (uint32_t)aidx[p];
            if (hop_insert(tab, mask, shift, c)) {
                if (FILL) {
                    const int k = atomicAdd(&s_cnt, 1);
                    keys[base + k] = ((u64)(uint32_t)i << 32) | c;
                    vals[base + k] = c;
                } else {
                    ++mine;
                }
            }
        }
    }
    if (!FILL) {
        for (int h = 1; h < 64; h <<= 1) mine += __shfl_xor(mine, h, 64);
        if ((tid & 63) == 0 && mine) atomicAdd(&s_cnt, mine);
        __syncthreads();
        if (tid == 0) count[i] = s_cnt;
    }
}

// One group of w lanes per cell, lane = component: the sums of x and x x over the cell's row of the shell in ascending
// index order (lane_group_walk_pattern), then out = mean or variance.  T = float widens on load.
template <class T>
__global__ __launch_bounds__(256) void k_hop_aggregate(const int64_t *__restrict__ ptr, const int32_t *__restrict__ idx,
                                                       const T *__restrict__ X, int64_t n, int d, int w, int what, double *__restrict__ out)
{
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / w;
    const int lane = threadIdx.x & (w - 1);
    if (i >= n) return;   // whole groups: w divides the workgroup
    const int64_t p0 = ptr[i], p1 = ptr[i + 1];
    double s = 0.0, q = 0.0;
    lane_group_walk_pattern(
        idx, p0, p1, w, lane, [&](int32_t id) { return lane < d ? (double)X[(int64_t)id * d + lane] : 0.0; },
        [&](double x) {
            s = s + x;
            q = q + x * x;
        });
    if (lane >= d) return;
    double r = 0.0;
    if (p1 > p0) {
        const double c = (double)(p1 - p0), m = s / c;
        r = what == SC_HOP_MEAN ? m : q / c - m * m;
    }
    out[i * d + lane] = r;
}

struct HopShell {
    DBuf indptr, indices;   // int64 [n + 1], int32 [nnz]
    int64_t nnz = 0;
};

}  // namespace

// the graph resident between sc_hop_begin and sc_hop_end
struct HopState : Resident {
    int64_t n = 0;
    std::vector<HopShell> shells;   // [l - 1] = shell l
    DBuf bound, count, rows, gofs, gtab, keys, keys2, vals, sort_tmp, scan_tmp;   // the expansion's scratch
    DBuf X, out;
    const void *x_host = nullptr;   // what X was uploaded from
    int x_dtype = -1, x_d = 0;
    hipEvent_t ev[8] = {};          // count, fill, sort, aggregate: begin and end
    bool timed[4] = {};
    ~HopState() override
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};
static HopState *hop_state(const sc_ctx *c) { return resident<HopState>(c->hops); }

namespace {

HopShells hop_shells(const HopState &s)
{
    HopShells sh = {};
    sh.count = (int)s.shells.size();
    for (int k = 0; k < sh.count; ++k) sh.ptr[k] = s.shells[k].indptr.as<int64_t>(), sh.idx[k] = s.shells[k].indices.as<int32_t>();
    return sh;
}

int hop_events(HopState &s)
{
    for (hipEvent_t &e : s.ev)
        if (!e) SC_HIP(hipEventCreate(&e));
    return SC_OK;
}

struct HopBatch {
    int64_t first, rows, ofs_first, slots;   // rows [first, first + rows) of the global list; their offsets start at gofs[ofs_first]; all their slots
};

// the count pass (FILL = false) or the fill pass over the row lists: [wavefront | workgroup by table size | global]
template <bool FILL>
int hop_launch(HopState &s, hipStream_t st, const HopShells &sh, int64_t n_wave, const int64_t *n_wg, const std::vector<HopBatch> &batches,
               const long long *off)
{
    const int32_t *rows = s.rows.as<int32_t>();
    const long long *bound = s.bound.as<long long>();
    long long *count = s.count.as<long long>();
    u64 *keys = s.keys.as<u64>();
    uint32_t *vals = s.vals.as<uint32_t>();
    if (n_wave)
        hipLaunchKernelGGL((k_hop_expand<64, HOP_WAVE_SLOTS, false, FILL>), dim3((unsigned)n_wave), dim3(64), 0, st, sh, rows, bound, nullptr, nullptr,
                           (uint32_t)HOP_WAVE_SLOTS, count, off, keys, vals);
    rows += n_wave;
    SC_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_hop_expand<HOP_TPB, 0, false, FILL>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)(sizeof(uint32_t) * HOP_WG_SLOTS)));
    for (int b = 0; b < HOP_WG_SIZES; ++b) {
        const uint32_t slots = (uint32_t)(2 * HOP_WAVE_SLOTS) << b;
        if (n_wg[b])
            hipLaunchKernelGGL((k_hop_expand<HOP_TPB, 0, false, FILL>), dim3((unsigned)n_wg[b]), dim3(HOP_TPB), sizeof(uint32_t) * slots, st, sh, rows,
                               bound, nullptr, nullptr, slots, count, off, keys, vals);
        rows += n_wg[b];
    }
    for (const HopBatch &b : batches) {   // in stream order: every batch has the tables to itself
        (void)hipMemsetAsync(s.gtab.p, 0xff, sizeof(uint32_t) * (size_t)b.slots, st);   // HOP_EMPTY; a failure shows in hipGetLastError
        hipLaunchKernelGGL((k_hop_expand<HOP_TPB, 1, true, FILL>), dim3((unsigned)b.rows), dim3(HOP_TPB), 0, st, sh, rows + b.first, bound,
                           s.gtab.as<uint32_t>(), s.gofs.as<int64_t>() + b.ofs_first, 0u, count, off, keys, vals);
    }
    return SC_OK;
}

template <class T> int hop_check_finite(const char *who, const T *X, int64_t n, int d)
{
    for (int64_t i = 0; i < n; ++i)
        for (int j = 0; j < d; ++j)
            SC_REQUIRE(std::isfinite((double)X[i * d + j]), SC_ERR_INVALID, "%s: X[%lld][%d] is not finite", who, (long long)i, j);
    return SC_OK;
}

}  // namespace

extern "C" int sc_hop_begin(sc_ctx *c, const int64_t *indptr, const int32_t *indices, int64_t n)
{
    const char *who = "sc_hop_begin";
    SC_REQUIRE(c && indptr && indices, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(n >= 1 && n <= INT32_MAX, SC_ERR_INVALID, "%s: need 1 <= n <= 2^31 - 1, got %lld", who, (long long)n);
    SC_REQUIRE(indptr[0] == 0, SC_ERR_INVALID, "%s: indptr[0] must be 0, got %lld", who, (long long)indptr[0]);
    for (int64_t i = 0; i < n; ++i)
        SC_REQUIRE(indptr[i + 1] >= indptr[i], SC_ERR_INVALID, "%s: indptr decreases at row %lld", who, (long long)i);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t p = indptr[i]; p < indptr[i + 1]; ++p) {
            const int32_t j = indices[p];
            SC_REQUIRE(j >= 0 && j < n, SC_ERR_INVALID, "%s: row %lld: column %d is outside 0 .. n - 1", who, (long long)i, j);
            SC_REQUIRE(j != i, SC_ERR_INVALID, "%s: row %lld holds a diagonal entry", who, (long long)i);
            SC_REQUIRE(p == indptr[i] || indices[p - 1] < j, SC_ERR_INVALID, "%s: row %lld: columns are not strictly ascending", who,
                       (long long)i);
        }
    const int64_t nnz = indptr[n];

    SC_HIP(hipSetDevice(c->device));
    sc_resident_drop(c, c->hops);
    c->hops.reset(new HopState());
    HopState &s = *hop_state(c);
    s.n = n;
    s.shells.emplace_back();
    HopShell &a = s.shells[0];
    a.nnz = nnz;
    int rc = a.indptr.ensure(sizeof(int64_t) * (size_t)(n + 1), &c->mem);
    if (rc == SC_OK) rc = a.indices.ensure(sizeof(int32_t) * (size_t)nnz, &c->mem);
    if (rc == SC_OK) {
        hipStream_t st = c->stream;
        bool ok = hipMemcpyAsync(a.indptr.p, indptr, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, st) == hipSuccess;
        ok = ok && (nnz == 0 || hipMemcpyAsync(a.indices.p, indices, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, st) == hipSuccess);
        if (!ok || hipStreamSynchronize(st) != hipSuccess) {   // the caller's arrays are free again
            sc_set_error("%s: failed on the device: %s", who, hipGetErrorString(hipGetLastError()));
            rc = SC_ERR_HIP;
        }
    }
    if (rc != SC_OK) sc_resident_drop(c, c->hops);
    return rc;
}

extern "C" int sc_hop_next(sc_ctx *c, int64_t *nnz_out, int32_t *max_row_out, int64_t *empty_rows_out)
{
    const char *who = "sc_hop_next";
    SC_REQUIRE(c && nnz_out && max_row_out && empty_rows_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(c->hops, SC_ERR_STATE, "%s: no graph is resident (sc_hop_begin)", who);
    HopState &s = *hop_state(c);
    SC_REQUIRE((int)s.shells.size() < SC_HOP_MAX, SC_ERR_STATE, "%s: %d shells are resident, the most there can be", who, SC_HOP_MAX);
    SC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int64_t n = s.n;
    const size_t np1 = sizeof(long long) * (size_t)(n + 1);
    s.timed[0] = s.timed[1] = s.timed[2] = false;
    HopShell next;
    SC_TRY(next.indptr.ensure(np1, &c->mem));
    if (s.shells.back().nnz == 0) {   // past the diameter everywhere: every later shell is empty
        SC_HIP(hipMemsetAsync(next.indptr.p, 0, np1, st));
        SC_HIP(hipStreamSynchronize(st));
        s.shells.push_back(std::move(next));
        *nnz_out = 0, *max_row_out = 0, *empty_rows_out = n;
        return SC_OK;
    }
    SC_TRY(hop_events(s));
    SC_TRY(s.bound.ensure(np1, &c->mem));
    SC_TRY(s.count.ensure(np1, &c->mem));
    SC_TRY(s.rows.ensure(sizeof(int32_t) * (size_t)n, &c->mem));
    const HopShells sh = hop_shells(s);
    std::vector<long long> host((size_t)n + 1);
    std::vector<int32_t> rows((size_t)n);
    std::vector<HopBatch> batches;
    std::vector<int64_t> gofs;
    StreamWaitOnExit wait{c->stream};   // after the host vectors: an early return waits before they go

    // ---- the bounds, the classes, the batches of the global class ----
    SC_HIP(hipEventRecord(s.ev[0], st));
    hipLaunchKernelGGL(k_hop_bound, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, st, sh, n, s.bound.as<long long>());
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(host.data(), s.bound.p, sizeof(long long) * (size_t)n, hipMemcpyDeviceToHost, st));
    SC_HIP(hipStreamSynchronize(st));
    // list position of every row: 0 wavefront, 1 .. HOP_WG_SIZES workgroup by table size, HOP_WG_SIZES + 1 global
    auto list_of = [&](long long b) {
        if (b <= SC_HOP_WAVE_KEYS) return 0;
        if (b > SC_HOP_WG_KEYS) return HOP_WG_SIZES + 1;
        int k = 0;
        while (((uint32_t)(2 * HOP_WAVE_SLOTS) << k) < hop_slots_for(b)) ++k;
        return 1 + k;
    };
    int64_t lists[HOP_WG_SIZES + 2] = {}, first[HOP_WG_SIZES + 2] = {};
    for (int64_t i = 0; i < n; ++i) ++lists[list_of(host[i])];
    for (int k = 1; k < HOP_WG_SIZES + 2; ++k) first[k] = first[k - 1] + lists[k - 1];
    {
        int64_t cursor[HOP_WG_SIZES + 2];
        std::copy(first, first + HOP_WG_SIZES + 2, cursor);
        for (int64_t i = 0; i < n; ++i) rows[(size_t)cursor[list_of(host[i])]++] = (int32_t)i;
    }
    const int64_t n_wave = lists[0], *n_wg = lists + 1, n_gl = lists[HOP_WG_SIZES + 1], gl_first = first[HOP_WG_SIZES + 1];
    int64_t gtab_slots = 0;
    for (int64_t r = 0; r < n_gl;) {
        HopBatch b{r, 0, (int64_t)gofs.size(), 0};
        int64_t used = 0;
        gofs.push_back(0);
        for (; r < n_gl; ++r, ++b.rows) {
            const long long keys = std::min<long long>(host[rows[(size_t)(gl_first + r)]], n);
            int64_t slots = 64;
            while (slots < 2 * keys && slots < ((int64_t)1 << 31)) slots <<= 1;   // 2^31 slots hold any n keys with one to spare
            if (b.rows && (used + slots) * (int64_t)sizeof(uint32_t) > HOP_GLOBAL_BYTES) break;
            used += slots;
            gofs.push_back(used);
        }
        b.slots = used;
        gtab_slots = std::max(gtab_slots, used);
        batches.push_back(b);
    }
    SC_HIP(hipMemcpyAsync(s.rows.p, rows.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, st));
    if (n_gl) {
        SC_TRY(s.gofs.ensure(sizeof(int64_t) * gofs.size(), &c->mem));
        SC_TRY(s.gtab.ensure(sizeof(uint32_t) * (size_t)gtab_slots, &c->mem));
        SC_HIP(hipMemcpyAsync(s.gofs.p, gofs.data(), sizeof(int64_t) * gofs.size(), hipMemcpyHostToDevice, st));
    }

    // ---- count, scan ----
    SC_HIP(hipMemsetAsync((char *)s.count.p + sizeof(long long) * (size_t)n, 0, sizeof(long long), st));
    SC_TRY(hop_launch<false>(s, st, sh, n_wave, n_wg, batches, nullptr));
    SC_HIP(hipGetLastError());
    SC_HIP(hipEventRecord(s.ev[1], st));
    s.timed[0] = true;
    SC_HIP(hipMemcpyAsync(host.data(), s.count.p, sizeof(long long) * (size_t)n, hipMemcpyDeviceToHost, st));
    SC_TRY(sc_exclusive_sum(c, s.scan_tmp, st, s.count.as<long long>(), next.indptr.as<long long>(), n + 1));
    SC_HIP(hipStreamSynchronize(st));
    int64_t total = 0, longest = 0, empty = 0;
    for (int64_t i = 0; i < n; ++i) total += host[i], longest = std::max<int64_t>(longest, host[i]), empty += host[i] == 0;

    if (total) {
        // ---- the memory account, before anything of the shell is written ----
        struct { DBuf *b; size_t bytes; } want[] = {{&s.keys, sizeof(u64) * (size_t)total}, {&s.keys2, sizeof(u64) * (size_t)total},
                                                    {&s.vals, sizeof(uint32_t) * (size_t)total}, {&next.indices, sizeof(int32_t) * (size_t)total}};
        int64_t need = HOP_MARGIN_BYTES;
        for (auto &w : want)
            if (w.bytes > w.b->cap) need += (int64_t)(w.bytes - w.b->cap);   // a buffer that grows gives its old bytes back first
        size_t free_b = 0, total_b = 0;
        SC_HIP(hipMemGetInfo(&free_b, &total_b));
        SC_REQUIRE(need <= (int64_t)free_b, SC_ERR_NOMEM, "%s: shell %d has %lld entries and needs %lld bytes of device memory, %lld are free", who,
                   (int)s.shells.size() + 1, (long long)total, (long long)need, (long long)free_b);
        for (auto &w : want) SC_TRY(w.b->ensure(w.bytes, &c->mem));
        // ---- fill, sort ----
        SC_HIP(hipEventRecord(s.ev[2], st));
        SC_TRY(hop_launch<true>(s, st, sh, n_wave, n_wg, batches, next.indptr.as<long long>()));
        SC_HIP(hipGetLastError());
        SC_HIP(hipEventRecord(s.ev[3], st));
        SC_HIP(hipEventRecord(s.ev[4], st));
        SC_TRY((sc_sort_pairs<u64, uint32_t>(c, s.sort_tmp, st, s.keys.as<u64>(), s.keys2.as<u64>(), s.vals.as<uint32_t>(),
                                             next.indices.as<uint32_t>(), total, 32 + sc_bits_for(n))));
        SC_HIP(hipEventRecord(s.ev[5], st));
        SC_HIP(hipStreamSynchronize(st));
        s.timed[1] = s.timed[2] = true;
    }
    next.nnz = total;
    s.shells.push_back(std::move(next));
    *nnz_out = total, *max_row_out = (int32_t)longest, *empty_rows_out = empty;
    return SC_OK;
}

extern "C" int sc_hop_get(sc_ctx *c, int64_t *indptr_out, int32_t *indices_out)
{
    const char *who = "sc_hop_get";
    SC_REQUIRE(c && indptr_out && indices_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(c->hops, SC_ERR_STATE, "%s: no graph is resident (sc_hop_begin)", who);
    HopState &s = *hop_state(c);
    const HopShell &sh = s.shells.back();
    SC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    SC_HIP(hipMemcpyAsync(indptr_out, sh.indptr.p, sizeof(int64_t) * (size_t)(s.n + 1), hipMemcpyDeviceToHost, st));
    if (sh.nnz) SC_HIP(hipMemcpyAsync(indices_out, sh.indices.p, sizeof(int32_t) * (size_t)sh.nnz, hipMemcpyDeviceToHost, st));
    SC_HIP(hipStreamSynchronize(st));
    return SC_OK;
}

extern "C" int sc_hop_aggregate(sc_ctx *c, const void *X, int dtype, int32_t d, int32_t what, double *out)
{
    const char *who = "sc_hop_aggregate";
    SC_REQUIRE(c && X && out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "%s: dtype must be SC_F32 or SC_F64", who);
    SC_REQUIRE(d >= 1 && d <= HOP_DMAX, SC_ERR_INVALID, "%s: need 1 <= d <= %d, got %d", who, HOP_DMAX, d);
    SC_REQUIRE(what == SC_HOP_MEAN || what == SC_HOP_VAR, SC_ERR_INVALID, "%s: what must be SC_HOP_MEAN or SC_HOP_VAR, got %d", who, what);
    SC_REQUIRE(c->hops, SC_ERR_STATE, "%s: no graph is resident (sc_hop_begin)", who);
    HopState &s = *hop_state(c);
    const int64_t n = s.n;
    const size_t x_bytes = (dtype == SC_F32 ? sizeof(float) : sizeof(double)) * (size_t)n * d, o_bytes = sizeof(double) * (size_t)n * d;
    const bool upload = X != s.x_host || dtype != s.x_dtype || d != s.x_d;
    if (upload) SC_TRY(dtype == SC_F32 ? hop_check_finite(who, (const float *)X, n, d) : hop_check_finite(who, (const double *)X, n, d));
    SC_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    SC_TRY(hop_events(s));
    s.timed[3] = false;
    if (upload) {
        s.x_host = nullptr;
        SC_TRY(s.X.ensure(x_bytes, &c->mem));
        SC_HIP(hipMemcpyAsync(s.X.p, X, x_bytes, hipMemcpyHostToDevice, st));
        SC_HIP(hipStreamSynchronize(st));
        s.x_host = X, s.x_dtype = dtype, s.x_d = d;
    }
    SC_TRY(s.out.ensure(o_bytes, &c->mem));
    const HopShell &sh = s.shells.back();
    const int w = lanes_for(d, 8, 64);
    const unsigned grid = (unsigned)ceil_div64(n, 256 / w);
    SC_HIP(hipEventRecord(s.ev[6], st));
    if (dtype == SC_F32)
        hipLaunchKernelGGL(k_hop_aggregate<float>, dim3(grid), dim3(256), 0, st, sh.indptr.as<int64_t>(), sh.indices.as<int32_t>(), s.X.as<float>(), n,
                           (int)d, w, (int)what, s.out.as<double>());
    else
        hipLaunchKernelGGL(k_hop_aggregate<double>, dim3(grid), dim3(256), 0, st, sh.indptr.as<int64_t>(), sh.indices.as<int32_t>(), s.X.as<double>(), n,
                           (int)d, w, (int)what, s.out.as<double>());
    SC_HIP(hipGetLastError());
    SC_HIP(hipEventRecord(s.ev[7], st));
    SC_HIP(hipMemcpyAsync(out, s.out.p, o_bytes, hipMemcpyDeviceToHost, st));
    SC_HIP(hipStreamSynchronize(st));
    s.timed[3] = true;
    return SC_OK;
}

extern "C" int sc_hop_times(sc_ctx *c, double *ms_out_4)
{
    const char *who = "sc_hop_times";
    SC_REQUIRE(c && ms_out_4, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(c->hops, SC_ERR_STATE, "%s: no graph is resident (sc_hop_begin)", who);
    HopState &s = *hop_state(c);
    for (int k = 0; k < 4; ++k) {
        float ms = 0.f;
        if (s.timed[k]) SC_HIP(hipEventElapsedTime(&ms, s.ev[2 * k], s.ev[2 * k + 1]));
        ms_out_4[k] = ms;
    }
    return SC_OK;
}

extern "C" int sc_hop_end(sc_ctx *c)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "sc_hop_end: null pointer");
    if (!c->hops) return SC_OK;
    SC_HIP(hipSetDevice(c->device));
    sc_resident_drop(c, c->hops);
    return SC_OK;
}
