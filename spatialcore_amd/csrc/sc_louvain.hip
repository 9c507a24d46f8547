// sc_louvain.hip -- sc_louvain_*: deterministic Louvain communities with a connectivity split (restated by
// tests/louvain_restated.py).  Louvain, not Leiden: there is no randomised refinement, only the guarantee that every
// community handed to the next level is connected.
//
// Input: a symmetric graph in canonical CSR (rows sorted by column, no duplicates, n <= 2^31 - 1, nnz <= 2^31 - 1), integer
// weights q_ij = q_ji in [1, 65535]; diagonal entries count once in the degree and never as a neighbour.  g = the
// resolution times 2^16, in [1, 2^23].
// One level on a graph A with n_l vertices: k_i = sum_j A_ij (diagonal included), M = sum_i k_i (the same at every level),
// comm_i = i, Qnum(comm) = 2^16 M sum_{comm_i = comm_j} A_ij - g sum_c tot_c^2 with tot_c = sum_{comm_i = c} k_i; best = the
// singletons, stale = 0.
// Round r = 0, 1, ...: all vertices read one snapshot of comm and tot.  The candidates of vertex i are comm_i and
// {comm_j : j != i, A_ij stored}; k_ic = sum_{j != i, comm_j = c} A_ij; S_i(c) = 2^16 M k_ic - g k_i (tot_c - [c = comm_i] k_i).
// Allowed: comm_i always, c > comm_i in even rounds, c < comm_i in odd rounds.  Vertex i takes the allowed c with the
// largest S; on equal S the current community wins, then the lowest c.  All moves are applied at once; then Qnum of the
// new comm: if it exceeds the best so far it becomes best and stale = 0, otherwise stale += 1.  The level ends when
// stale = 2 or after max_rounds rounds; the search continues from comm, not from best.
// Split: inside best, the connected components of the edges whose two ends share a community (i != j); a component's
// label is the rank of its smallest vertex among all components, ascending (the union-find's roots, then a prefix sum).
// Aggregate: if the number of components equals n_l the hierarchy is finished; otherwise A'_ab = sum_{i in a, j in b} A_ij
// (a = b gives the diagonal) and the next level runs on A'.
// Final labels: clusters numbered by descending size, ties to the smaller smallest-member index.
// All of it is exact integer arithmetic: degrees and totals 64-bit, S and Qnum 128-bit, integer atomics only (exact and
// order-free), no floating point on the device.  Vertices without edges stay singletons; M = 0 gives all singletons.
//
// How a round runs here.  The move kernels of round t read the snapshot P_t, write P_{t+1} and, from the same pass over
// the CSR, the in-community weight of P_t (a vertex's k_{i,comm_i} plus its diagonal), so Qnum(P_t) costs no second pass: the
// host learns it one launch late, and the level costs rounds + 1 passes.  The moves of the launch that only served to
// evaluate the last partition are dropped.  tot is copied, then changed by 64-bit atomics of the vertices that moved.
// A row's candidates are aggregated in an open-addressing table, atomicCAS on the key and a 64-bit integer add on the
// value; the argmax over the slots by (S, current first, lowest c) does not depend on the order the atomics landed in.
// Three row classes, chosen per level from the row lengths (k_lv_classify):
//   wavefront: rows of at most LV_SHORT = 64 entries, one entry per lane, a 128-slot table per wavefront in LDS;
//   workgroup: rows of at most LV_LONG = 2048 entries, one workgroup per row, a 4096-slot table in LDS (48 KiB) of which
//              the row uses the power of two >= 2 (len + 1) slots, at least 256;
//   global:    longer rows, one workgroup per row, a table of the next power of two >= 2 (len + 1) in global memory.
// Table indices and hashes are 32-bit arithmetic (no per-lane variable 64-bit shifts).
#include <climits>
#include <algorithm>
#include <vector>

#include "sc_csr_input.h"
#include "sc_list_graph.h"
#include "sc_sortscan.h"
#include "sc_unionfind.h"

namespace {

typedef unsigned long long u64;
typedef unsigned __int128 u128;
typedef __int128 i128;

constexpr int LV_TPB = 256;
constexpr int LV_SHORT = 64;           // longest row of the wavefront class: one entry per lane
constexpr int LV_WAVE_SLOTS = 128;     // its table: at most 65 keys
constexpr int LV_LONG = 2048;          // longest row of the workgroup class
constexpr int LV_WG_SLOTS = 4096;      // its table: at most 2049 keys; 16 KiB of keys + 32 KiB of values
constexpr uint32_t LV_WG_MIN_SLOTS = 256;   // ... of which a row clears and scans the part it needs: 2 (len + 1) slots, at least these
constexpr int LV_GRID = 2048;          // workgroups of the wavefront-class kernel (rows are taken by stride)
constexpr int LV_ACC_IN = 64;          // words the wavefronts spread their in-community sums over
constexpr int LV_ACC = 2 + LV_ACC_IN;  // [0] sum tot^2 high, [1] low, [2 ..] in-community weight
constexpr uint32_t LV_EMPTY = 0xffffffffu;
constexpr int LV_GMAX = 1 << 23;       // resolution 128
constexpr int LV_CHUNK = 8;            // sorted entries one thread of k_lv_fill adds up before it touches memory

__device__ __forceinline__ uint32_t lv_hash(uint32_t c) { return c * 2654435761u; }

__device__ __forceinline__ u64 lv_shfl_xor64(u64 v, int m)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, m, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), m, 64);
    return ((u64)hi << 32) | lo;
}

// acc[0] = high word, acc[1] = low word (rs_add128 of sc_ranksum.hip: the add that wraps the low word carries)
__device__ __forceinline__ void lv_add128(u64 *acc, u128 x)
{
    const u64 lo = (u64)x, hi = (u64)(x >> 64);
    const u64 old = atomicAdd(&acc[1], lo);
    const u64 carry = (u64)(old + lo < old);
    if (hi + carry) atomicAdd(&acc[0], hi + carry);
}

// a candidate of a vertex and the order the vertex chooses by: S, then the current community, then the lowest c
struct LvCand {
    i128 S;
    int32_t c;
    int cur;
};
__device__ __forceinline__ LvCand lv_none() { return LvCand{(i128)((u128)1 << 127), INT32_MAX, 0}; }
__device__ __forceinline__ bool lv_better(const LvCand &a, const LvCand &b)
{
    if (a.S != b.S) return a.S > b.S;
    if (a.cur != b.cur) return a.cur > b.cur;
    return a.c < b.c;
}
__device__ __forceinline__ LvCand lv_wave_best(LvCand v)
{
    for (int h = 1; h < 64; h <<= 1) {
        LvCand o;
        o.S = (i128)(((u128)lv_shfl_xor64((u64)((u128)v.S >> 64), h) << 64) | lv_shfl_xor64((u64)(u128)v.S, h));
        o.c = __shfl_xor(v.c, h, 64);
        o.cur = __shfl_xor(v.cur, h, 64);
        if (lv_better(o, v)) v = o;
    }
    return v;
}

// what a vertex needs to score a candidate
struct LvVertex {
    int32_t ci;      // its community
    u64 ki;          // its degree
    u64 m16;         // 2^16 M
    uint32_t g;      // resolution 2^16
    int odd;         // round parity
};
// the slot (c, k_ic) as a candidate of v, if it is allowed; *inside receives k_ic of the vertex's own community
__device__ __forceinline__ void lv_score(const LvVertex &v, uint32_t key, u64 kic, const u64 *__restrict__ tot, LvCand &best, u64 &inside)
{
    const int32_t c = (int32_t)key;
    const bool cur = c == v.ci;
    if (cur) inside += kic;
    if (!cur && (v.odd ? c > v.ci : c < v.ci)) return;   // even rounds move up, odd rounds move down
    const u64 t = tot[c] - (cur ? v.ki : 0ull);
    LvCand x;
    x.S = (i128)((u128)v.m16 * kic) - (i128)((u128)v.ki * t * v.g);   // < 2^110 and < 2^117
    x.c = c;
    x.cur = cur ? 1 : 0;
    if (lv_better(x, best)) best = x;
}

// (c, w) into an open-addressing table of `mask + 1` slots; the table is never full (sizes above)
__device__ __forceinline__ void lv_insert(uint32_t *keys, u64 *vals, uint32_t mask, uint32_t shift, uint32_t c, u64 w)
{
    uint32_t h = lv_hash(c) >> shift;
    for (;;) {
        const uint32_t old = atomicCAS(&keys[h], LV_EMPTY, c);
        if (old == LV_EMPTY || old == c) break;
        h = (h + 1u) & mask;
    }
    if (w) atomicAdd(&vals[h], w);
}

__device__ __forceinline__ void lv_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the move of vertex i is decided: written, and tot of the two communities changed if it moved
__device__ __forceinline__ void lv_apply(int64_t i, const LvVertex &v, int32_t c, int32_t *__restrict__ next, u64 *__restrict__ tot_next)
{
    next[i] = c;
    if (c != v.ci) {
        atomicAdd(&tot_next[c], v.ki);
        atomicAdd(&tot_next[v.ci], 0ull - v.ki);   // modulo 2^64: the sum of the adds is exact
    }
}

// ---- the wavefront class: rows of at most 64 entries, a wavefront per row, rows by stride ----------------------------
template <class W>
__global__ __launch_bounds__(256) void k_lv_move_wave(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                      const W *__restrict__ w, int64_t n, const int32_t *__restrict__ comm,
                                                      const u64 *__restrict__ tot, const u64 *__restrict__ k, u64 m16, uint32_t g, int odd,
                                                      int32_t *__restrict__ next, u64 *__restrict__ tot_next, u64 *__restrict__ acc)
{
    __shared__ uint32_t skeys[LV_TPB / 64][LV_WAVE_SLOTS];
    __shared__ u64 svals[LV_TPB / 64][LV_WAVE_SLOTS];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t *keys = skeys[wave];
    u64 *vals = svals[wave];
    u64 inside = 0;
    for (int64_t i = (int64_t)blockIdx.x * (LV_TPB / 64) + wave; i < n; i += (int64_t)gridDim.x * (LV_TPB / 64)) {
        const int64_t p0 = indptr[i], len = indptr[i + 1] - p0;
        if (len > LV_SHORT) continue;   // the whole wavefront: another class's row
        LvVertex v{comm[i], k[i], m16, g, odd};
        keys[lane] = LV_EMPTY, keys[lane + 64] = LV_EMPTY;
        vals[lane] = 0, vals[lane + 64] = 0;
        lv_wave_sync();
        if (lane < len) {
            const int32_t j = indices[p0 + lane];
            const u64 x = (u64)w[p0 + lane];
            if (j == i) inside += x;
            else lv_insert(keys, vals, LV_WAVE_SLOTS - 1, 32 - 7, (uint32_t)comm[j], x);
        }
        if (lane == 63) lv_insert(keys, vals, LV_WAVE_SLOTS - 1, 32 - 7, (uint32_t)v.ci, 0);   // its own community is always a candidate
        lv_wave_sync();
        LvCand best = lv_none();
#pragma unroll
        for (int s = lane; s < LV_WAVE_SLOTS; s += 64) {
            const uint32_t key = keys[s];
            if (key != LV_EMPTY) lv_score(v, key, vals[s], tot, best, inside);
        }
        best = lv_wave_best(best);
        if (lane == 0) lv_apply(i, v, best.c, next, tot_next);
        lv_wave_sync();   // the table is read before the next row clears it
    }
    for (int h = 1; h < 64; h <<= 1) inside += lv_shfl_xor64(inside, h);
    if (lane == 0 && inside) atomicAdd(&acc[2 + ((blockIdx.x * (LV_TPB / 64) + wave) & (LV_ACC_IN - 1))], inside);
}

// ---- the workgroup and global classes: one workgroup per listed row --------------------------------------------------
// GLOBAL: the row's table is gkeys / gvals + coff[blockIdx.x], ccap[blockIdx.x] slots, cleared by the host before the launch
template <class W, bool GLOBAL>
__global__ __launch_bounds__(256) void k_lv_move_wg(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                    const W *__restrict__ w, const int32_t *__restrict__ list,
                                                    const u64 *__restrict__ coff, const uint32_t *__restrict__ ccap, uint32_t *gkeys, u64 *gvals,
                                                    const int32_t *__restrict__ comm, const u64 *__restrict__ tot, const u64 *__restrict__ k,
                                                    u64 m16, uint32_t g, int odd, int32_t *__restrict__ next, u64 *__restrict__ tot_next,
                                                    u64 *__restrict__ acc)
{
    __shared__ uint32_t skeys[GLOBAL ? 1 : LV_WG_SLOTS];
    __shared__ u64 svals[GLOBAL ? 1 : LV_WG_SLOTS];
    __shared__ u64 r_hi[LV_TPB / 64], r_lo[LV_TPB / 64], r_in[LV_TPB / 64];
    __shared__ int32_t r_c[LV_TPB / 64], r_cur[LV_TPB / 64];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int64_t i = list[blockIdx.x];
    uint32_t *keys = skeys;
    u64 *vals = svals;
    const int64_t p1 = indptr[i + 1], len = p1 - indptr[i];
    uint32_t cap = LV_WG_MIN_SLOTS;   // the part of the LDS table this row uses: the power of two >= 2 (len + 1), at most all of it
    if (GLOBAL) {
        keys = gkeys + coff[blockIdx.x];
        vals = gvals + coff[blockIdx.x];
        cap = ccap[blockIdx.x];
    } else {
        while (cap < LV_WG_SLOTS && (int64_t)cap < 2 * (len + 1)) cap <<= 1;
        for (uint32_t s = t; s < cap; s += LV_TPB) skeys[s] = LV_EMPTY, svals[s] = 0;
    }
    const uint32_t mask = cap - 1u, shift = 32u - (uint32_t)(31 - __builtin_clz(cap));   // cap = 2^b, 2 <= b <= 31: shift in [1, 30]
    __syncthreads();
    LvVertex v{comm[i], k[i], m16, g, odd};
    u64 inside = 0;
    if (t == 0) lv_insert(keys, vals, mask, shift, (uint32_t)v.ci, 0);
    for (int64_t p = p1 - len + t; p < p1; p += LV_TPB) {
        const int32_t j = indices[p];
        const u64 x = (u64)w[p];
        if (j == i) inside += x;
        else lv_insert(keys, vals, mask, shift, (uint32_t)comm[j], x);
    }
    if (GLOBAL) __threadfence();   // the LDS table needs the barrier alone; a device-scope fence per row cost 68 us of L2 write-back
    __syncthreads();
    LvCand best = lv_none();
    for (uint32_t s = t; s < cap; s += LV_TPB) {
        // global table: written by atomics at the L2, read there too
        const uint32_t key = GLOBAL ? __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : keys[s];
        if (key == LV_EMPTY) continue;
        const u64 kic = GLOBAL ? __hip_atomic_load(&vals[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : vals[s];
        lv_score(v, key, kic, tot, best, inside);
    }
    best = lv_wave_best(best);
    for (int h = 1; h < 64; h <<= 1) inside += lv_shfl_xor64(inside, h);
    if (lane == 0) {
        r_hi[wave] = (u64)((u128)best.S >> 64), r_lo[wave] = (u64)(u128)best.S;
        r_c[wave] = best.c, r_cur[wave] = best.cur, r_in[wave] = inside;
    }
    __syncthreads();
    if (t == 0) {
        for (int q = 1; q < LV_TPB / 64; ++q) {
            LvCand o{(i128)(((u128)r_hi[q] << 64) | r_lo[q]), r_c[q], r_cur[q]};
            if (lv_better(o, best)) best = o;
            inside += r_in[q];
        }
        lv_apply(i, v, best.c, next, tot_next);
        if (inside) atomicAdd(&acc[2 + (blockIdx.x & (LV_ACC_IN - 1))], inside);
    }
}

// acc[0 .. 1] += sum tot_c^2
__global__ __launch_bounds__(256) void k_lv_sumsq(const u64 *__restrict__ tot, int64_t n, u64 *__restrict__ acc)
{
    u128 s = 0;
    for (int64_t i = (int64_t)blockIdx.x * LV_TPB + threadIdx.x; i < n; i += (int64_t)gridDim.x * LV_TPB) s += (u128)tot[i] * tot[i];
    for (int h = 1; h < 64; h <<= 1) s += ((u128)lv_shfl_xor64((u64)(s >> 64), h) << 64) | lv_shfl_xor64((u64)s, h);
    if ((threadIdx.x & 63) == 0 && s) lv_add128(acc, s);
}

// ---- per level: degrees, start, row classes --------------------------------------------------------------------------
template <class W>
__global__ __launch_bounds__(256) void k_lv_degree(const int64_t *__restrict__ indptr, const W *__restrict__ w, int64_t n, u64 *__restrict__ k)
{
    const int64_t i = (int64_t)blockIdx.x * LV_TPB + threadIdx.x;
    if (i >= n) return;
    u64 s = 0;
    for (int64_t p = indptr[i]; p < indptr[i + 1]; ++p) s += (u64)w[p];
    k[i] = s;
}

__global__ __launch_bounds__(256) void k_lv_start(const u64 *__restrict__ k, int64_t n, int32_t *__restrict__ comm, u64 *__restrict__ tot)
{
    const int64_t i = (int64_t)blockIdx.x * LV_TPB + threadIdx.x;
    if (i >= n) return;
    comm[i] = (int32_t)i;
    tot[i] = k[i];
}

// cls[0] workgroup-class rows, cls[1] global-class rows, cls[2] slots of all global tables; the lists take the rows in the
// order the atomics land in, which no result depends on: a row's move is a function of the snapshot alone
__global__ __launch_bounds__(256) void k_lv_classify(const int64_t *__restrict__ indptr, int64_t n, u64 *__restrict__ cls,
                                                     int32_t *__restrict__ list_wg, int32_t *__restrict__ list_gl, u64 *__restrict__ coff,
                                                     uint32_t *__restrict__ ccap)
{
    const int64_t i = (int64_t)blockIdx.x * LV_TPB + threadIdx.x;
    if (i >= n) return;
    const int64_t len = indptr[i + 1] - indptr[i];
    if (len <= LV_SHORT) return;
    if (len <= LV_LONG) {
        list_wg[atomicAdd(&cls[0], 1ull)] = (int32_t)i;
        return;
    }
    uint32_t cap = 8192;   // 2 (len + 1) <= 2^32: len <= 2^31 - 1
    while ((int64_t)cap < 2 * (len + 1)) cap <<= 1;
    const u64 pos = atomicAdd(&cls[1], 1ull);
    list_gl[pos] = (int32_t)i;
    ccap[pos] = cap;
    coff[pos] = atomicAdd(&cls[2], (u64)cap);
}

// ---- the split -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lv_parent(int32_t *__restrict__ parent, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * LV_TPB + threadIdx.x;
    if (i < n) parent[i] = (int32_t)i;
}
__global__ __launch_bounds__(256) void k_lv_union(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                  const int32_t *__restrict__ best, int64_t n, int32_t *parent)
{
    const int64_t i = (int64_t)blockIdx.x * LV_TPB + threadIdx.x;
    if (i >= n) return;
    const int32_t ci = best[i];
    for (int64_t p = indptr[i]; p < indptr[i + 1]; ++p) {
        const int32_t j = indices[p];
        if (j >= i) break;   // each edge once, from its larger end; the diagonal never
        if (best[j] == ci) uf_union(parent, (int32_t)i, j);
    }
}
// root[i], is_root[i] (and is_root[n] = 0 for the scan); used[best[i]] = 1
__global__ __launch_bounds__(256) void k_lv_roots(int32_t *parent, const int32_t *__restrict__ best, int64_t n, int32_t *__restrict__ root,
                                                  long long *__restrict__ is_root, long long *used)
{
    const int64_t i = (int64_t)blockIdx.x * LV_TPB + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        is_root[n] = 0;
        return;
    }
    const int32_t r = uf_find(parent, (int32_t)i);
    root[i] = r;
    is_root[i] = r == (int32_t)i;
    used[best[i]] = 1;   // every writer stores the same value
}
__global__ __launch_bounds__(256) void k_lv_label(const int32_t *__restrict__ root, const long long *__restrict__ rank, const u64 *__restrict__ k,
                                                  int64_t n, int32_t *__restrict__ label, u64 *__restrict__ knew)
{
    const int64_t i = (int64_t)blockIdx.x * LV_TPB + threadIdx.x;
    if (i >= n) return;
    const int32_t a = (int32_t)rank[root[i]];
    label[i] = a;
    if (k[i]) atomicAdd(&knew[a], k[i]);
}
__global__ __launch_bounds__(256) void k_lv_compose(int32_t *__restrict__ map, const int32_t *__restrict__ label, int64_t n0)
{
    const int64_t v = (int64_t)blockIdx.x * LV_TPB + threadIdx.x;
    if (v < n0) map[v] = label[map[v]];
}

// ---- the aggregation: sort the entries by (a, b), add the runs ---------------------------------------------------------
__global__ __launch_bounds__(256) void k_lv_keys(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                 const int32_t *__restrict__ label, int64_t n, u64 *__restrict__ keys, uint32_t *__restrict__ pay)
{
    const int64_t i = (int64_t)blockIdx.x * LV_TPB + threadIdx.x;
    if (i >= n) return;
    const u64 a = (u64)(uint32_t)label[i] << 32;
    for (int64_t p = indptr[i]; p < indptr[i + 1]; ++p) {
        keys[p] = a | (uint32_t)label[indices[p]];
        pay[p] = (uint32_t)p;
    }
}
// head = 1 at the first of every run of equal sorted keys (sc_sortscan.h: sc_run_heads), seg = exclusive sums of head: entry p
// belongs to run seg[p] + head[p] - 1.  A thread adds LV_CHUNK consecutive entries and touches memory when the run changes.  The first entry of a run writes its column; the first run of a row, and the
// last entry of all, write the row offsets.
template <class W>
__global__ __launch_bounds__(256) void k_lv_fill(const u64 *__restrict__ keys, const uint32_t *__restrict__ pay, const long long *__restrict__ head,
                                                 const long long *__restrict__ seg, const W *__restrict__ w_old, int64_t nnz, int64_t nc,
                                                 int64_t *__restrict__ indptr_new, int32_t *__restrict__ indices_new, u64 *__restrict__ w_new)
{
    const int64_t q0 = ((int64_t)blockIdx.x * LV_TPB + threadIdx.x) * LV_CHUNK;
    if (q0 >= nnz) return;
    const int64_t q1 = q0 + LV_CHUNK < nnz ? q0 + LV_CHUNK : nnz;
    long long run = -1;
    u64 sum = 0;
    for (int64_t p = q0; p < q1; ++p) {
        const long long r = seg[p] + head[p] - 1;
        if (r != run) {
            if (sum) atomicAdd(&w_new[run], sum);
            run = r, sum = 0;
        }
        sum += (u64)w_old[pay[p]];
        if (head[p]) {
            indices_new[r] = (int32_t)(uint32_t)keys[p];
            const int64_t a = (int64_t)(keys[p] >> 32), before = p == 0 ? -1 : (int64_t)(keys[p - 1] >> 32);
            for (int64_t row = before + 1; row <= a; ++row) indptr_new[row] = r;   // empty rows before a start where a starts
        }
        if (p == nnz - 1)
            for (int64_t row = (int64_t)(keys[p] >> 32) + 1; row <= nc; ++row) indptr_new[row] = seg[nnz];
    }
    if (sum) atomicAdd(&w_new[run], sum);
}

// the adopted graph of sc_diffmap_graph: flag[0] = 1 + the first entry found whose mirror is missing or weighs otherwise
__global__ __launch_bounds__(256) void k_lv_symmetric(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                      const uint16_t *__restrict__ w, int64_t n, u64 *flag)
{
    const int64_t i = (int64_t)blockIdx.x * LV_TPB + threadIdx.x;
    if (i >= n) return;
    for (int64_t p = indptr[i]; p < indptr[i + 1]; ++p) {
        const int32_t j = indices[p];
        int64_t lo = indptr[j], hi = indptr[j + 1];
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (indices[mid] < i) lo = mid + 1;
            else hi = mid;
        }
        if (lo == indptr[j + 1] || indices[lo] != i || w[lo] != w[p]) atomicMin(flag, (u64)p + 1ull);
    }
}

inline unsigned lv_blocks(int64_t count) { return (unsigned)ceil_div64(count > 0 ? count : 1, LV_TPB); }

}  // namespace

struct LvGraph {
    DBuf indptr, indices, w;
    int64_t n = 0, nnz = 0;
    bool wide = false;   // weights: uint16 (level 0) or 64-bit (the aggregated levels)
};

// everything between sc_louvain_begin and sc_louvain_end
struct LouvainState : Resident {
    LvGraph gr[2];
    int cur = 0;
    DBuf k, knew, comm, next, best, tot, tot2, acc, cls, map, parent, root, flag, rank, used, label, list_wg, list_gl, coff, ccap, gkeys, gvals;
    DBuf keys, keys2, pay, pay2, tmp;
    int64_t n0 = 0;
    u64 M = 0;
    int32_t g = 0, max_rounds = 0, levels = 0;
    bool finished = false;
};
static LouvainState *lv_state(const sc_ctx *c) { return resident<LouvainState>(c->louvain); }

namespace {

// offsets[0 .. cnt] = exclusive sums of counts[0 .. cnt] on the state's own scratch; *total = offsets[cnt] after the caller's wait
int lv_scan(sc_ctx *c, LouvainState &s, long long *counts, long long *offsets, int64_t cnt, long long *total)
{
    SC_TRY(sc_exclusive_sum(c, s.tmp, c->stream, counts, offsets, cnt + 1));
    SC_HIP(hipMemcpyAsync(total, offsets + cnt, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    return SC_OK;
}

int lv_check_common(const char *who, const sc_ctx *c, int32_t g, int32_t max_rounds)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(g >= 1 && g <= LV_GMAX, SC_ERR_INVALID, "%s: need 1 <= resolution 2^16 <= 2^23, got %d", who, g);
    SC_REQUIRE(max_rounds >= 1, SC_ERR_INVALID, "%s: need max_rounds >= 1, got %d", who, max_rounds);
    return SC_OK;
}

// a fresh state whose level 0 has room for (n, nnz)
int lv_new_state(sc_ctx *c, int64_t n, int64_t nnz, u64 M, int32_t g, int32_t max_rounds)
{
    sc_resident_drop(c, c->louvain);
    c->louvain.reset(new LouvainState());
    LouvainState &s = *lv_state(c);
    s.n0 = n, s.M = M, s.g = g, s.max_rounds = max_rounds;
    LvGraph &G = s.gr[0];
    G.n = n, G.nnz = nnz, G.wide = false;
    SC_TRY(G.indptr.ensure(sizeof(int64_t) * (size_t)(n + 1), &c->mem));
    SC_TRY(G.indices.ensure(sizeof(int32_t) * (size_t)(nnz ? nnz : 1), &c->mem));
    SC_TRY(G.w.ensure(sizeof(uint16_t) * (size_t)(nnz ? nnz : 1), &c->mem));
    SC_TRY(s.k.ensure(sizeof(u64) * (size_t)n, &c->mem));
    SC_TRY(s.map.ensure(sizeof(int32_t) * (size_t)n, &c->mem));
    return SC_OK;
}

// after the upload of level 0: degrees, the identity map
int lv_finish_begin(sc_ctx *c)
{
    LouvainState &s = *lv_state(c);
    LvGraph &G = s.gr[0];
    hipStream_t st = c->stream;
    KernelTimerScope ts(c, SC_K_LOUVAIN_LEVEL);
    hipLaunchKernelGGL(k_lv_degree<uint16_t>, dim3(lv_blocks(G.n)), dim3(LV_TPB), 0, st, G.indptr.as<int64_t>(), G.w.as<uint16_t>(), G.n, s.k.as<u64>());
    hipLaunchKernelGGL(k_lv_parent, dim3(lv_blocks(G.n)), dim3(LV_TPB), 0, st, s.map.as<int32_t>(), G.n);
    SC_HIP(hipGetLastError());
    return SC_OK;
}

template <class W>
int lv_launch_moves(sc_ctx *c, LouvainState &s, const LvGraph &G, int odd, int64_t n_wave, int64_t n_wg, int64_t n_gl)
{
    hipStream_t st = c->stream;
    const u64 m16 = s.M << 16;
    const int64_t *indptr = G.indptr.as<int64_t>();
    const int32_t *indices = G.indices.as<int32_t>();
    const W *w = G.w.as<W>();
    if (n_wave) {
        const int64_t want = ceil_div64(G.n, LV_TPB / 64);
        hipLaunchKernelGGL(k_lv_move_wave<W>, dim3((unsigned)(want < LV_GRID ? want : LV_GRID)), dim3(LV_TPB), 0, st, indptr, indices, w, G.n,
                           s.comm.as<int32_t>(), s.tot.as<u64>(), s.k.as<u64>(), m16, (uint32_t)s.g, odd, s.next.as<int32_t>(), s.tot2.as<u64>(),
                           s.acc.as<u64>());
    }
    if (n_wg)
        hipLaunchKernelGGL((k_lv_move_wg<W, false>), dim3((unsigned)n_wg), dim3(LV_TPB), 0, st, indptr, indices, w, s.list_wg.as<int32_t>(),
                           (const u64 *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (u64 *)nullptr, s.comm.as<int32_t>(), s.tot.as<u64>(),
                           s.k.as<u64>(), m16, (uint32_t)s.g, odd, s.next.as<int32_t>(), s.tot2.as<u64>(), s.acc.as<u64>());
    if (n_gl)
        hipLaunchKernelGGL((k_lv_move_wg<W, true>), dim3((unsigned)n_gl), dim3(LV_TPB), 0, st, indptr, indices, w, s.list_gl.as<int32_t>(),
                           s.coff.as<u64>(), s.ccap.as<uint32_t>(), s.gkeys.as<uint32_t>(), s.gvals.as<u64>(), s.comm.as<int32_t>(), s.tot.as<u64>(),
                           s.k.as<u64>(), m16, (uint32_t)s.g, odd, s.next.as<int32_t>(), s.tot2.as<u64>(), s.acc.as<u64>());
    return SC_OK;
}

// A' from the level's graph and its labels into the other slot
template <class W>
int lv_aggregate(sc_ctx *c, LouvainState &s, const LvGraph &G, LvGraph &H, int64_t nc)
{
    hipStream_t st = c->stream;
    const int64_t nnz = G.nnz;
    const size_t cap = (size_t)(nnz ? nnz : 1);
    SC_TRY(s.keys.ensure(sizeof(u64) * cap, &c->mem));
    SC_TRY(s.keys2.ensure(sizeof(u64) * cap, &c->mem));
    SC_TRY(s.pay.ensure(sizeof(uint32_t) * cap, &c->mem));
    SC_TRY(s.pay2.ensure(sizeof(uint32_t) * cap, &c->mem));
    SC_TRY(s.flag.ensure(sizeof(long long) * (cap + 1), &c->mem));
    SC_TRY(s.rank.ensure(sizeof(long long) * (cap + 1), &c->mem));
    hipLaunchKernelGGL(k_lv_keys, dim3(lv_blocks(G.n)), dim3(LV_TPB), 0, st, G.indptr.as<int64_t>(), G.indices.as<int32_t>(), s.label.as<int32_t>(), G.n,
                       s.keys.as<u64>(), s.pay.as<uint32_t>());
    SC_TRY(sc_sort_pairs(c, s.tmp, st, s.keys.as<u64>(), s.keys2.as<u64>(), s.pay.as<uint32_t>(), s.pay2.as<uint32_t>(), nnz,
                         32 + sc_bits_for(nc)));
    sc_run_heads(st, s.keys2.as<u64>(), nnz, s.flag.as<long long>());
    long long runs = 0;
    SC_TRY(lv_scan(c, s, s.flag.as<long long>(), s.rank.as<long long>(), nnz, &runs));
    SC_HIP(hipStreamSynchronize(st));
    SC_REQUIRE(runs >= 1 && runs <= nnz, SC_ERR_HIP, "sc_louvain_level: %lld aggregated entries out of range", runs);
    H.n = nc, H.nnz = runs, H.wide = true;
    SC_TRY(H.indptr.ensure(sizeof(int64_t) * (size_t)(nc + 1), &c->mem));
    SC_TRY(H.indices.ensure(sizeof(int32_t) * (size_t)runs, &c->mem));
    SC_TRY(H.w.ensure(sizeof(u64) * (size_t)runs, &c->mem));
    SC_HIP(hipMemsetAsync(H.w.p, 0, sizeof(u64) * (size_t)runs, st));
    hipLaunchKernelGGL(k_lv_fill<W>, dim3(lv_blocks(ceil_div64(nnz, LV_CHUNK))), dim3(LV_TPB), 0, st, s.keys2.as<u64>(), s.pay2.as<uint32_t>(),
                       s.flag.as<long long>(), s.rank.as<long long>(), G.w.as<W>(), nnz, nc, H.indptr.as<int64_t>(), H.indices.as<int32_t>(),
                       H.w.as<u64>());
    SC_HIP(hipGetLastError());
    return SC_OK;
}

template <class W>
int lv_level(sc_ctx *c, LouvainState &s, int64_t *info, int32_t *labels_out)
{
    LvGraph &G = s.gr[s.cur];
    hipStream_t st = c->stream;
    const int64_t n = G.n;
    const size_t vn = (size_t)n;
    for (DBuf *b : {&s.comm, &s.next, &s.best, &s.label, &s.parent, &s.root, &s.list_wg, &s.list_gl}) SC_TRY(b->ensure(sizeof(int32_t) * vn, &c->mem));
    for (DBuf *b : {&s.tot, &s.tot2, &s.knew, &s.coff}) SC_TRY(b->ensure(sizeof(u64) * vn, &c->mem));
    SC_TRY(s.ccap.ensure(sizeof(uint32_t) * vn, &c->mem));
    SC_TRY(s.acc.ensure(sizeof(u64) * LV_ACC, &c->mem));
    SC_TRY(s.cls.ensure(sizeof(u64) * 3, &c->mem));
    SC_TRY(s.flag.ensure(sizeof(long long) * (vn + 1), &c->mem));
    SC_TRY(s.rank.ensure(sizeof(long long) * (vn + 1), &c->mem));
    SC_TRY(s.used.ensure(sizeof(long long) * (vn + 1), &c->mem));
    const dim3 rows(lv_blocks(n)), tpb(LV_TPB);

    // the start and the row classes
    u64 cls[3] = {0, 0, 0};
    SC_HIP(hipMemsetAsync(s.cls.p, 0, sizeof(u64) * 3, st));
    hipLaunchKernelGGL(k_lv_start, rows, tpb, 0, st, s.k.as<u64>(), n, s.comm.as<int32_t>(), s.tot.as<u64>());
    hipLaunchKernelGGL(k_lv_classify, rows, tpb, 0, st, G.indptr.as<int64_t>(), n, s.cls.as<u64>(), s.list_wg.as<int32_t>(), s.list_gl.as<int32_t>(),
                       s.coff.as<u64>(), s.ccap.as<uint32_t>());
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(cls, s.cls.p, sizeof(cls), hipMemcpyDeviceToHost, st));
    SC_HIP(hipStreamSynchronize(st));
    const int64_t n_wg = (int64_t)cls[0], n_gl = (int64_t)cls[1], n_wave = n - n_wg - n_gl;
    SC_REQUIRE(n_wave >= 0 && cls[2] <= 4ull * (u64)G.nnz + 8192ull * (u64)n_gl, SC_ERR_HIP, "sc_louvain_level: row classes out of range");
    if (n_gl) {
        SC_TRY(s.gkeys.ensure(sizeof(uint32_t) * (size_t)cls[2], &c->mem));
        SC_TRY(s.gvals.ensure(sizeof(u64) * (size_t)cls[2], &c->mem));
    }

    // the rounds: launch t reads P_t, writes P_{t+1} and gives Qnum(P_t)
    i128 best_q = 0;
    u64 best_in = 0;
    int32_t stale = 0, rounds = 0;
    for (int32_t t = 0;; ++t) {
        u64 acc[LV_ACC];
        SC_HIP(hipMemcpyAsync(s.tot2.p, s.tot.p, sizeof(u64) * vn, hipMemcpyDeviceToDevice, st));
        SC_HIP(hipMemsetAsync(s.acc.p, 0, sizeof(u64) * LV_ACC, st));
        if (n_gl) {
            SC_HIP(hipMemsetAsync(s.gkeys.p, 0xff, sizeof(uint32_t) * (size_t)cls[2], st));
            SC_HIP(hipMemsetAsync(s.gvals.p, 0, sizeof(u64) * (size_t)cls[2], st));
        }
        {
            KernelTimerScope ts(c, SC_K_LOUVAIN_MOVE);
            SC_TRY(lv_launch_moves<W>(c, s, G, t & 1, n_wave, n_wg, n_gl));
            hipLaunchKernelGGL(k_lv_sumsq, dim3((unsigned)std::min<int64_t>(lv_blocks(n), 256)), tpb, 0, st, s.tot.as<u64>(), n, s.acc.as<u64>());
        }
        SC_HIP(hipGetLastError());
        SC_HIP(hipMemcpyAsync(acc, s.acc.p, sizeof(acc), hipMemcpyDeviceToHost, st));
        SC_HIP(hipStreamSynchronize(st));
        u64 inside = 0;
        for (int q = 0; q < LV_ACC_IN; ++q) inside += acc[2 + q];
        const u128 sq = ((u128)acc[0] << 64) | acc[1];
        const i128 q = (i128)((u128)(s.M << 16) * inside) - (i128)(sq * (u128)(uint32_t)s.g);
        if (t == 0 || q > best_q) {
            best_q = q, best_in = inside, stale = 0;
            SC_HIP(hipMemcpyAsync(s.best.p, s.comm.p, sizeof(int32_t) * vn, hipMemcpyDeviceToDevice, st));
        } else {
            ++stale;
        }
        rounds = t;
        if (stale == 2 || t == s.max_rounds) break;   // the moves just computed are dropped
        std::swap(s.comm, s.next);
        std::swap(s.tot, s.tot2);
    }

    // the split of best, the components' degrees
    long long n_comp = 0, n_best = 0;
    {
        KernelTimerScope ts(c, SC_K_LOUVAIN_LEVEL);
        SC_HIP(hipMemsetAsync(s.used.p, 0, sizeof(long long) * (vn + 1), st));
        SC_HIP(hipMemsetAsync(s.knew.p, 0, sizeof(u64) * vn, st));
        SC_HIP(hipMemsetAsync(s.acc.p, 0, sizeof(u64) * 2, st));
        hipLaunchKernelGGL(k_lv_parent, rows, tpb, 0, st, s.parent.as<int32_t>(), n);
        hipLaunchKernelGGL(k_lv_union, rows, tpb, 0, st, G.indptr.as<int64_t>(), G.indices.as<int32_t>(), s.best.as<int32_t>(), n, s.parent.as<int32_t>());
        hipLaunchKernelGGL(k_lv_roots, dim3(lv_blocks(n + 1)), tpb, 0, st, s.parent.as<int32_t>(), s.best.as<int32_t>(), n, s.root.as<int32_t>(),
                           s.flag.as<long long>(), s.used.as<long long>());
        SC_TRY(lv_scan(c, s, s.flag.as<long long>(), s.rank.as<long long>(), n, &n_comp));
        hipLaunchKernelGGL(k_lv_label, rows, tpb, 0, st, s.root.as<int32_t>(), s.rank.as<long long>(), s.k.as<u64>(), n, s.label.as<int32_t>(),
                           s.knew.as<u64>());
        SC_TRY(lv_scan(c, s, s.used.as<long long>(), s.flag.as<long long>(), n, &n_best));   // flag: free again
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipStreamSynchronize(st));
    SC_REQUIRE(n_comp >= 1 && n_comp <= n && n_best >= 1 && n_best <= n_comp, SC_ERR_HIP, "sc_louvain_level: %lld components of %lld communities", n_comp,
               n_best);
    // Qnum of the split partition: the edges inside are those inside best, tot is the components' degrees
    u64 acc2[2];
    hipLaunchKernelGGL(k_lv_sumsq, dim3((unsigned)std::min<int64_t>(lv_blocks(n_comp), 256)), tpb, 0, st, s.knew.as<u64>(), (int64_t)n_comp, s.acc.as<u64>());
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(acc2, s.acc.p, sizeof(acc2), hipMemcpyDeviceToHost, st));
    if (labels_out) SC_HIP(hipMemcpyAsync(labels_out, s.label.p, sizeof(int32_t) * vn, hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(k_lv_compose, dim3(lv_blocks(s.n0)), tpb, 0, st, s.map.as<int32_t>(), s.label.as<int32_t>(), s.n0);
    SC_HIP(hipGetLastError());
    SC_HIP(hipStreamSynchronize(st));
    const i128 q_split = (i128)((u128)(s.M << 16) * best_in) - (i128)((((u128)acc2[0] << 64) | acc2[1]) * (u128)(uint32_t)s.g);
    s.finished = n_comp == n;
    info[0] = n, info[1] = rounds, info[2] = n_best, info[3] = n_comp;
    info[4] = (int64_t)(q_split >> 64), info[5] = (int64_t)(u64)(u128)q_split;
    info[6] = s.finished, info[7] = rounds == s.max_rounds && stale < 2;
    info[8] = n_wave, info[9] = n_wg, info[10] = n_gl, info[11] = G.nnz;
    ++s.levels;
    if (s.finished) return SC_OK;
    {
        KernelTimerScope ts(c, SC_K_LOUVAIN_LEVEL);
        SC_TRY(lv_aggregate<W>(c, s, G, s.gr[s.cur ^ 1], (int64_t)n_comp));
    }
    std::swap(s.k, s.knew);
    s.cur ^= 1;
    SC_HIP(hipStreamSynchronize(st));
    return SC_OK;
}

}  // namespace

extern "C" int sc_louvain_begin(sc_ctx *c, const int64_t *indptr, const int32_t *indices, const uint16_t *q, int64_t n, int32_t g,
                                int32_t max_rounds)
{
    const char *who = "sc_louvain_begin";
    SC_TRY(lv_check_common(who, c, g, max_rounds));
    SC_REQUIRE(indptr, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(n >= 1 && n <= INT32_MAX, SC_ERR_INVALID, "%s: need 1 <= n <= 2^31 - 1, got %lld", who, (long long)n);
    int64_t nnz = 0;
    SC_TRY(csr_check_offsets(who, indptr, n, &nnz));
    SC_REQUIRE(nnz <= INT32_MAX, SC_ERR_INVALID, "%s: need stored entries <= 2^31 - 1, got %lld", who, (long long)nnz);
    SC_REQUIRE(nnz == 0 || (indices && q), SC_ERR_INVALID, "%s: null pointer", who);
    u64 M = 0;
    SC_TRY(csr_check_columns(who, indptr, indices, n, n, "n", [&](int64_t i, int64_t p) -> int {
        SC_REQUIRE(q[p] >= 1, SC_ERR_INVALID, "%s: weight %lld (row %lld, column %d) is 0: weights are integers in [1, 65535]", who, (long long)p,
                   (long long)i, indices[p]);
        M += q[p];
        return SC_OK;
    }));
    for (int64_t i = 0; i < n; ++i)
        for (int64_t p = indptr[i]; p < indptr[i + 1]; ++p) {
            const int32_t j = indices[p];
            const int32_t *b = indices + indptr[j], *e = indices + indptr[j + 1];
            const int32_t *m = std::lower_bound(b, e, (int32_t)i);
            SC_REQUIRE(m != e && *m == i, SC_ERR_INVALID, "%s: the graph is not symmetric: entry (%lld, %d) is stored, (%d, %lld) is not", who,
                       (long long)i, j, j, (long long)i);
            SC_REQUIRE(q[m - indices] == q[p], SC_ERR_INVALID, "%s: the graph is not symmetric: entry (%lld, %d) weighs %d, (%d, %lld) weighs %d", who,
                       (long long)i, j, (int)q[p], j, (long long)i, (int)q[m - indices]);
        }

    SC_HIP(hipSetDevice(c->device));
    int rc = lv_new_state(c, n, nnz, M, g, max_rounds);
    if (rc == SC_OK) {
        LvGraph &G = lv_state(c)->gr[0];
        hipStream_t st = c->stream;
        bool ok = hipMemcpyAsync(G.indptr.p, indptr, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, st) == hipSuccess;
        if (ok && nnz)
            ok = hipMemcpyAsync(G.indices.p, indices, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, st) == hipSuccess &&
                 hipMemcpyAsync(G.w.p, q, sizeof(uint16_t) * (size_t)nnz, hipMemcpyHostToDevice, st) == hipSuccess;
        if (ok) rc = lv_finish_begin(c);
        if (rc == SC_OK && (!ok || hipStreamSynchronize(st) != hipSuccess)) {   // the caller's arrays are free again
            sc_set_error("%s: upload failed on the device: %s", who, hipGetErrorString(hipGetLastError()));
            rc = SC_ERR_HIP;
        }
    }
    if (rc != SC_OK) sc_resident_drop(c, c->louvain);
    return rc;
}

extern "C" int sc_louvain_resident_weights(sc_ctx *c, double *w_out, int64_t nnz)
{
    const char *who = "sc_louvain_resident_weights";
    SC_REQUIRE(c && w_out, SC_ERR_INVALID, "%s: null pointer", who);
    const sc_ctx::ListGraph *f = nullptr;
    SC_TRY(lg_resident(c, who, " (sc_diffmap_graph)", &f));
    SC_REQUIRE(nnz == f->nnz, SC_ERR_INVALID, "%s: the resident graph stores %lld entries, not %lld", who, (long long)f->nnz, (long long)nnz);
    SC_HIP(hipSetDevice(c->device));
    SC_HIP(hipMemcpyAsync(w_out, f->w.p, sizeof(double) * (size_t)nnz, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}

extern "C" int sc_louvain_begin_resident(sc_ctx *c, const uint16_t *q, int64_t nnz, int32_t g, int32_t max_rounds)
{
    const char *who = "sc_louvain_begin_resident";
    SC_TRY(lv_check_common(who, c, g, max_rounds));
    const sc_ctx::ListGraph *resident = nullptr;
    SC_TRY(lg_resident(c, who, " (sc_diffmap_graph)", &resident));
    const sc_ctx::ListGraph &f = *resident;
    SC_REQUIRE(nnz == f.nnz, SC_ERR_INVALID, "%s: the resident graph stores %lld entries, not %lld", who, (long long)f.nnz, (long long)nnz);
    SC_REQUIRE(nnz <= INT32_MAX, SC_ERR_INVALID, "%s: need stored entries <= 2^31 - 1, got %lld", who, (long long)nnz);
    std::vector<uint16_t> ones;
    u64 M = (u64)nnz;   // q == nullptr: every edge weighs 1
    if (q) {
        M = 0;
        for (int64_t p = 0; p < nnz; ++p) {
            SC_REQUIRE(q[p] >= 1, SC_ERR_INVALID, "%s: weight %lld is 0: weights are integers in [1, 65535]", who, (long long)p);
            M += q[p];
        }
    } else {
        ones.assign((size_t)nnz, (uint16_t)1);
        q = ones.data();
    }
    SC_HIP(hipSetDevice(c->device));
    const int64_t n = f.n;
    int rc = lv_new_state(c, n, nnz, M, g, max_rounds);
    u64 flag = ~0ull;
    if (rc == SC_OK) {
        LouvainState &s = *lv_state(c);
        LvGraph &G = s.gr[0];
        hipStream_t st = c->stream;
        rc = s.acc.ensure(sizeof(u64) * LV_ACC, &c->mem);
        bool ok = rc == SC_OK &&
                  hipMemcpyAsync(G.indptr.p, f.indptr.p, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToDevice, st) == hipSuccess &&
                  hipMemcpyAsync(G.indices.p, f.indices.p, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToDevice, st) == hipSuccess &&
                  hipMemcpyAsync(G.w.p, q, sizeof(uint16_t) * (size_t)nnz, hipMemcpyHostToDevice, st) == hipSuccess &&
                  hipMemsetAsync(s.acc.p, 0xff, sizeof(u64), st) == hipSuccess;
        if (ok) {
            hipLaunchKernelGGL(k_lv_symmetric, dim3(lv_blocks(n)), dim3(LV_TPB), 0, st, G.indptr.as<int64_t>(), G.indices.as<int32_t>(), G.w.as<uint16_t>(), n,
                               s.acc.as<u64>());
            rc = lv_finish_begin(c);
            ok = hipMemcpyAsync(&flag, s.acc.p, sizeof(u64), hipMemcpyDeviceToHost, st) == hipSuccess;
        }
        if (rc == SC_OK && (!ok || hipStreamSynchronize(st) != hipSuccess)) {   // `ones` lives until here
            sc_set_error("%s: upload failed on the device: %s", who, hipGetErrorString(hipGetLastError()));
            rc = SC_ERR_HIP;
        }
        if (rc == SC_OK && flag != ~0ull) {
            sc_set_error("%s: the graph is not symmetric in structure and weight at stored entry %llu", who, flag - 1ull);
            rc = SC_ERR_INVALID;
        }
    }
    if (rc != SC_OK) sc_resident_drop(c, c->louvain);
    return rc;
}

extern "C" int sc_louvain_level(sc_ctx *c, int64_t *info_out, int32_t *labels_out)
{
    const char *who = "sc_louvain_level";
    SC_REQUIRE(c && info_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(c->louvain, SC_ERR_STATE, "%s: no graph is resident (sc_louvain_begin)", who);
    SC_REQUIRE(!lv_state(c)->finished, SC_ERR_STATE, "%s: the hierarchy is finished", who);
    SC_HIP(hipSetDevice(c->device));
    LouvainState &s = *lv_state(c);
    return s.gr[s.cur].wide ? lv_level<u64>(c, s, info_out, labels_out) : lv_level<uint16_t>(c, s, info_out, labels_out);
}

extern "C" int sc_louvain_labels(sc_ctx *c, int32_t *labels_out, int64_t *n_clusters_out)
{
    const char *who = "sc_louvain_labels";
    SC_REQUIRE(c && labels_out && n_clusters_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(c->louvain, SC_ERR_STATE, "%s: no graph is resident (sc_louvain_begin)", who);
    LouvainState &s = *lv_state(c);
    SC_REQUIRE(s.levels >= 1, SC_ERR_STATE, "%s: no level has run (sc_louvain_level)", who);
    SC_HIP(hipSetDevice(c->device));
    SC_HIP(hipMemcpyAsync(labels_out, s.map.p, sizeof(int32_t) * (size_t)s.n0, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    // numbered by descending size, ties to the smaller smallest member: n steps of host bookkeeping on the fetched labels
    int32_t top = 0;
    for (int64_t v = 0; v < s.n0; ++v) top = labels_out[v] > top ? labels_out[v] : top;
    const size_t C = (size_t)top + 1;
    std::vector<int64_t> size(C, 0), first(C, -1);
    for (int64_t v = 0; v < s.n0; ++v) {
        const int32_t a = labels_out[v];
        SC_REQUIRE(a >= 0, SC_ERR_HIP, "%s: negative label at vertex %lld", who, (long long)v);
        if (size[a]++ == 0) first[a] = v;
    }
    std::vector<int32_t> order(C), rank(C);
    for (size_t a = 0; a < C; ++a) order[a] = (int32_t)a;
    std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return size[a] != size[b] ? size[a] > size[b] : first[a] < first[b]; });
    for (size_t r = 0; r < C; ++r) rank[order[r]] = (int32_t)r;
    for (int64_t v = 0; v < s.n0; ++v) labels_out[v] = rank[labels_out[v]];
    *n_clusters_out = (int64_t)C;
    return SC_OK;
}

extern "C" int sc_louvain_end(sc_ctx *c)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "sc_louvain_end: null pointer");
    if (!c->louvain) return SC_OK;
    SC_HIP(hipSetDevice(c->device));
    sc_resident_drop(c, c->louvain);
    return SC_OK;
}
