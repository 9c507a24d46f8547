// Everything that reads coordinates: binning, exact kNN / radius graphs and nearest-target queries on a uniform bin
// grid (the walks over it are in sc_search.h), brute-force pairwise distances.  gfx950 only.
//
// kNN design: points are counting-sorted into square bins (SoA x[], y[], id[] in bin order, so a
// row of bins is one contiguous, coalesced range).  One thread owns one query and walks square
// rings of bins around it, keeping its k best (distance, index) pairs in registers (fully unrolled
// insertion network, no scratch memory).  It stops as soon as the k-th best distance is provably
// smaller than the distance to anything outside the visited window, so the result is the exact
// kNN set, ordered by (squared distance, index).  Consecutive threads are consecutive points of the
// same bin, so a wavefront reads the same candidate ranges (L1 broadcast).
#include <float.h>
#include <math.h>

#include <vector>

#include "sc_search.h"
#include "sc_sortscan.h"
#include "sc_topk.h"

// ------------------------------------------------------------------------------------------------
// binning
// ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_split_xy(const double *__restrict__ xy, double *__restrict__ x,
                                                  double *__restrict__ y, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double2 v = reinterpret_cast<const double2 *>(xy)[i];
    x[i] = v.x;
    y[i] = v.y;
}

__global__ __launch_bounds__(256) void k_bin_keys(const double *__restrict__ x, const double *__restrict__ y,
                                                  int64_t n, double x0, double y0, double inv_h, int nbx, int nby,
                                                  uint32_t *__restrict__ keys, int32_t *__restrict__ ids)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int bx = bin_coord(x[i], x0, inv_h, nbx), by = bin_coord(y[i], y0, inv_h, nby);
    keys[i] = (uint32_t)by * (uint32_t)nbx + (uint32_t)bx;
    ids[i] = (int32_t)i;
}

__global__ __launch_bounds__(256) void k_gather_sorted(const double *__restrict__ x, const double *__restrict__ y,
                                                       const int32_t *__restrict__ sid, int64_t n,
                                                       double *__restrict__ sx, double *__restrict__ sy)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t j = sid[i];
    sx[i] = x[j];
    sy[i] = y[j];
}

// bin_start[b] = first sorted position whose key >= b  (keys sorted ascending)
__global__ __launch_bounds__(256) void k_bin_start(const uint32_t *__restrict__ keys, int64_t n, int64_t nbins,
                                                   int32_t *__restrict__ bin_start)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    uint32_t cur = i < n ? keys[i] : (uint32_t)nbins;
    uint32_t prev = i > 0 ? keys[i - 1] + 1 : 0;  // first bin not yet closed
    for (uint32_t b = prev; b <= cur && b <= (uint32_t)nbins; ++b) bin_start[b] = (int32_t)i;
}

int sc_bin_points(sc_ctx *c, const double *xy, int64_t n, double target_per_bin, double min_h)
{
    // what is only meaningful on the bins this call replaces: the Ripley pair list holds positions of their order, and
    // the fill pass of a pending radius count walks them with rows sized by the count pass
    c->rp_valid = false;
    c->rg_valid = false;
    c->radius = -1.0;
    SC_REQUIRE(n >= 1 && n <= 0x7fffffffLL, SC_ERR_INVALID, "n=%lld out of range", (long long)n);
    double xmin = DBL_MAX, xmax = -DBL_MAX, ymin = DBL_MAX, ymax = -DBL_MAX;
    for (int64_t i = 0; i < n; ++i) {
        double x = xy[2 * i], y = xy[2 * i + 1];
        SC_REQUIRE(isfinite(x) && isfinite(y), SC_ERR_INVALID, "coordinate %lld is not finite", (long long)i);
        xmin = x < xmin ? x : xmin; xmax = x > xmax ? x : xmax;
        ymin = y < ymin ? y : ymin; ymax = y > ymax ? y : ymax;
    }
    double w = xmax - xmin, hgt = ymax - ymin;
    double area = (w > 0 ? w : 1.0) * (hgt > 0 ? hgt : 1.0);
    double h = sqrt(area * target_per_bin / (double)n);
    if (h < min_h) h = min_h;
    double ext = w > hgt ? w : hgt;
    if (!(h > 0)) h = 1.0;
    // cap the grid at 4096 x 4096 bins
    if (ext / h > 4096.0) h = ext / 4096.0;
    int nbx = (int)floor(w / h) + 1, nby = (int)floor(hgt / h) + 1;
    c->nbx = nbx; c->nby = nby; c->gx0 = xmin; c->gy0 = ymin; c->gh = h;
    int64_t nbins = (int64_t)nbx * nby;

    SC_TRY(c->e_tmp_data.ensure(sizeof(double) * 2 * (size_t)n, &c->mem));  // staging for AoS upload
    SC_TRY(c->px.ensure(sizeof(double) * (size_t)n, &c->mem));
    SC_TRY(c->py.ensure(sizeof(double) * (size_t)n, &c->mem));
    SC_TRY(c->sx.ensure(sizeof(double) * (size_t)n, &c->mem));
    SC_TRY(c->sy.ensure(sizeof(double) * (size_t)n, &c->mem));
    SC_TRY(c->sid.ensure(sizeof(int32_t) * (size_t)n, &c->mem));
    SC_TRY(c->sid2.ensure(sizeof(int32_t) * (size_t)n, &c->mem));
    SC_TRY(c->bin_keys.ensure(sizeof(uint32_t) * (size_t)n, &c->mem));
    SC_TRY(c->bin_keys2.ensure(sizeof(uint32_t) * (size_t)n, &c->mem));
    SC_TRY(c->bin_start.ensure(sizeof(int32_t) * (size_t)(nbins + 1), &c->mem));
    SC_HIP(hipMemcpyAsync(c->e_tmp_data.p, xy, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    unsigned grid = (unsigned)ceil_div64(n, 256);
    hipLaunchKernelGGL(k_split_xy, dim3(grid), dim3(256), 0, c->stream, c->e_tmp_data.as<double>(),
                       c->px.as<double>(), c->py.as<double>(), n);
    hipLaunchKernelGGL(k_bin_keys, dim3(grid), dim3(256), 0, c->stream, c->px.as<double>(), c->py.as<double>(), n,
                       xmin, ymin, 1.0 / h, nbx, nby, c->bin_keys.as<uint32_t>(), c->sid2.as<int32_t>());
    SC_TRY(sc_sort_pairs(c, c->cub_tmp, c->stream, c->bin_keys.as<uint32_t>(), c->bin_keys2.as<uint32_t>(), c->sid2.as<int32_t>(),
                         c->sid.as<int32_t>(), n, sc_bits_for(nbins)));
    hipLaunchKernelGGL(k_gather_sorted, dim3(grid), dim3(256), 0, c->stream, c->px.as<double>(), c->py.as<double>(),
                       c->sid.as<int32_t>(), n, c->sx.as<double>(), c->sy.as<double>());
    hipLaunchKernelGGL(k_bin_start, dim3((unsigned)ceil_div64(n + 1, 256)), dim3(256), 0, c->stream,
                       c->bin_keys2.as<uint32_t>(), n, nbins, c->bin_start.as<int32_t>());
    SC_HIP(hipGetLastError());
    c->pts_n = n;
    return SC_OK;
}

BinGrid sc_bin_grid(const sc_ctx *c)
{
    return BinGrid{c->sx.as<double>(), c->sy.as<double>(), c->sid.as<int32_t>(), c->bin_start.as<int32_t>(),
                   c->gx0, c->gy0, c->gh, c->nbx, c->nby};
}

int sc_window_rings(const sc_ctx *c, double radius)
{
    const int rings = (int)ceil(radius / c->gh * (1.0 + 1e-9));
    return rings < 1 ? 1 : rings;
}

int sc_counts_to_offsets(sc_ctx *c, long long *counts, long long *offsets, int64_t n, long long *total)
{
    SC_TRY(sc_exclusive_sum(c, c->cub_tmp, c->stream, counts, offsets, n + 1));
    SC_HIP(hipMemcpyAsync(total, offsets + n, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    return SC_OK;
}

// ------------------------------------------------------------------------------------------------
// A1: exact kNN
// ------------------------------------------------------------------------------------------------

template <int K>
__global__ __launch_bounds__(256) void k_knn(BinGrid g, int64_t n, int k, int include_self,
                                             int32_t *__restrict__ idx_out, double *__restrict__ rd_out)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double qx = g.sx[t], qy = g.sy[t];
    const int qid = g.sid[t];
    TopK<K> best;
    best.init();
    double kth = DBL_MAX;
    ring_walk(g, qx, qy,
              [&](int s) {
                  const int cid = g.sid[s];
                  const double d = BinGrid::dist2(qx, qy, g.sx[s], g.sy[s]);
                  if (cid == qid && !include_self) return;
                  if (cand_better(d, cid, best.d[K - 1], best.id[K - 1])) {
                      best.insert(d, cid);
                      kth = best.kth(k);
                  }
              },
              [&] { return kth; });
    // scatter to the original query order
    int32_t *o = idx_out + (int64_t)qid * k;
    double *od = rd_out ? rd_out + (int64_t)qid * k : nullptr;
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (j < k) {
            o[j] = best.id[j];
            if (od) od[j] = best.d[j];
        }
}

// k > 32 (any k < n): the k best candidates of a query live in a binary MAX-heap in global memory (slot j of query t
// at [j * n + t]: the root, every thread's hottest slot, is a coalesced row), keyed by (squared distance, index); a
// candidate that beats the root replaces it and sifts down.  The ring walk and the tie rule are those of k_knn; at the
// end the heap is sorted in place (heap sort) and scattered to the query's row.  The register form needs 3 K registers
// per lane: K = 64 spilled 130 of them (r02) -- 33 <= k <= 64 come here too.
__device__ __forceinline__ bool cand_worse(double d, int id, double ed, int eid) { return cand_better(ed, eid, d, id); }

__device__ __forceinline__ void heap_sift_down(double *__restrict__ hd, int32_t *__restrict__ hi, int64_t n, int64_t t,
                                               int size, double cd, int cid)
{
    // place (cd, cid) into the heap of `size` slots starting at the root, whose old content is dropped
    int pos = 0;
    for (;;) {
        const int l = 2 * pos + 1, r = l + 1;
        if (l >= size) break;
        double wd = hd[(int64_t)l * n + t];
        int wi = hi[(int64_t)l * n + t], w = l;
        if (r < size) {
            const double rd = hd[(int64_t)r * n + t];
            const int ri = hi[(int64_t)r * n + t];
            if (cand_worse(rd, ri, wd, wi)) { wd = rd; wi = ri; w = r; }
        }
        if (!cand_worse(wd, wi, cd, cid)) break;     // the candidate is at least as bad as both children: it stays here
        hd[(int64_t)pos * n + t] = wd;
        hi[(int64_t)pos * n + t] = wi;
        pos = w;
    }
    hd[(int64_t)pos * n + t] = cd;
    hi[(int64_t)pos * n + t] = cid;
}

__global__ __launch_bounds__(256) void k_knn_heap(BinGrid g, int64_t n, int k, int include_self,
                                                  double *__restrict__ hd, int32_t *__restrict__ hi,
                                                  int32_t *__restrict__ idx_out, double *__restrict__ rd_out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double qx = g.sx[t], qy = g.sy[t];
    const int qid = g.sid[t];
    for (int j = 0; j < k; ++j) { hd[(int64_t)j * n + t] = DBL_MAX; hi[(int64_t)j * n + t] = 0x7fffffff; }   // a valid heap
    double root_d = DBL_MAX;      // the root is the k-th best so far
    int root_i = 0x7fffffff;
    ring_walk(g, qx, qy,
              [&](int s) {
                  const int cid = g.sid[s];
                  const double d = BinGrid::dist2(qx, qy, g.sx[s], g.sy[s]);
                  if (cid == qid && !include_self) return;
                  if (cand_better(d, cid, root_d, root_i)) {
                      heap_sift_down(hd, hi, n, t, k, d, cid);
                      root_d = hd[t];
                      root_i = hi[t];
                  }
              },
              [&] { return root_d; });
    // heap sort: the worst of the remaining heap goes to its end; slots end up ascending by (distance, index)
    for (int m = k - 1; m >= 1; --m) {
        const double ld = hd[(int64_t)m * n + t];
        const int li = hi[(int64_t)m * n + t];
        hd[(int64_t)m * n + t] = hd[t];
        hi[(int64_t)m * n + t] = hi[t];
        heap_sift_down(hd, hi, n, t, m, ld, li);
    }
    int32_t *o = idx_out + (int64_t)qid * k;
    double *od = rd_out ? rd_out + (int64_t)qid * k : nullptr;
    for (int j = 0; j < k; ++j) {
        o[j] = hi[(int64_t)j * n + t];
        if (od) od[j] = hd[(int64_t)j * n + t];
    }
}

template <int K>
static void launch_knn(sc_ctx *c, int64_t n, int k, int include_self)
{
    hipLaunchKernelGGL(k_knn<K>, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, c->stream, sc_bin_grid(c), n, k,
                       include_self, c->knn_idx.as<int32_t>(), c->knn_rd.as<double>());
}

extern "C" int sc_knn_2d(sc_ctx *c, const double *xy, int64_t n, int k, int include_self, int32_t *idx_out,
                         double *rdist_out)
{
    SC_REQUIRE(c && xy, SC_ERR_INVALID, "sc_knn_2d: null pointer");
    SC_REQUIRE(k >= 1 && k <= (1 << 16), SC_ERR_INVALID, "sc_knn_2d: k=%d unsupported (1..65536)", k);
    SC_REQUIRE(n >= 1, SC_ERR_INVALID, "sc_knn_2d: n must be >= 1");
    SC_REQUIRE((int64_t)k <= n - (include_self ? 0 : 1), SC_ERR_INVALID,
               "sc_knn_2d: k=%d needs more than the %lld available points", k, (long long)n);
    SC_HIP(hipSetDevice(c->device));
    c->knn_n = 0;
    SC_TRY(sc_bin_points(c, xy, n, 0.5 * (k + 1) > 4.0 ? 0.5 * (k + 1) : 4.0, 0.0));
    SC_TRY(c->knn_idx.ensure(sizeof(int32_t) * (size_t)n * k, &c->mem));
    SC_TRY(c->knn_rd.ensure(sizeof(double) * (size_t)n * k, &c->mem));
    {
        KernelTimerScope ts(c, SC_K_KNN);
        if (k <= 8) launch_knn<8>(c, n, k, include_self);
        else if (k <= 16) launch_knn<16>(c, n, k, include_self);
        else if (k <= 32) launch_knn<32>(c, n, k, include_self);
        else {
            SC_TRY(c->knn_hd.ensure(sizeof(double) * (size_t)n * k, &c->mem));
            SC_TRY(c->knn_hi.ensure(sizeof(int32_t) * (size_t)n * k, &c->mem));
            hipLaunchKernelGGL(k_knn_heap, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, c->stream, sc_bin_grid(c), n, k,
                               include_self, c->knn_hd.as<double>(), c->knn_hi.as<int32_t>(), c->knn_idx.as<int32_t>(),
                               c->knn_rd.as<double>());
        }
    }
    SC_HIP(hipGetLastError());
    if (idx_out)
        SC_HIP(hipMemcpyAsync(idx_out, c->knn_idx.p, sizeof(int32_t) * (size_t)n * k, hipMemcpyDeviceToHost,
                              c->stream));
    if (rdist_out)
        SC_HIP(hipMemcpyAsync(rdist_out, c->knn_rd.p, sizeof(double) * (size_t)n * k, hipMemcpyDeviceToHost,
                              c->stream));
    // nothing to hand back: the result stays on the device and every consumer is ordered behind it on the context's
    // stream, so the host need not wait (the caller's coordinate array has been staged by the pageable-memory copy)
    if (idx_out || rdist_out) SC_HIP(hipStreamSynchronize(c->stream));
    else {   // for a later sc_knn_fetch on the copy stream
        if (!c->knn_done) SC_HIP(hipEventCreateWithFlags(&c->knn_done, hipEventDisableTiming));
        SC_HIP(hipEventRecord(c->knn_done, c->stream));
    }
    c->knn_n = n;
    c->knn_k = k;
    return SC_OK;
}

// The result of the last sc_knn_2d that was called without output arrays, copied out on the context's side stream (ordered
// behind the search by an event): the copy neither waits for what the context's stream has been given since, nor holds
// it up -- a caller's thread can fetch the neighbour lists while another uploads the expression (PCIe is full duplex).
extern "C" int sc_knn_fetch(sc_ctx *c, int32_t *idx_out, double *rdist_out)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "sc_knn_fetch: null context");
    SC_REQUIRE(c->knn_n > 0 && c->knn_done, SC_ERR_STATE, "sc_knn_fetch: no resident kNN result (sc_knn_2d without output arrays first)");
    SC_HIP(hipSetDevice(c->device));
    // the side stream of the graph moments serves as the copy stream (a stream more per context would be a hardware queue
    // more: a process whose streams outnumber GPU_MAX_HW_QUEUES has them share queues, which the generator must avoid)
    sc_graph_moments_drain(c);
    SC_TRY(c->streams.ensure(SR_MOMENTS));
    const size_t nk = (size_t)c->knn_n * (size_t)c->knn_k;
    SC_HIP(hipStreamWaitEvent(c->stream_m, c->knn_done, 0));
    if (idx_out) SC_HIP(hipMemcpyAsync(idx_out, c->knn_idx.p, sizeof(int32_t) * nk, hipMemcpyDeviceToHost, c->stream_m));
    if (rdist_out) SC_HIP(hipMemcpyAsync(rdist_out, c->knn_rd.p, sizeof(double) * nk, hipMemcpyDeviceToHost, c->stream_m));
    SC_HIP(hipStreamSynchronize(c->stream_m));
    return SC_OK;
}

// ------------------------------------------------------------------------------------------------
// A2: radius graph (closed ball, self removed), two passes
// ------------------------------------------------------------------------------------------------

template <bool FILL>
__global__ __launch_bounds__(256) void k_radius(BinGrid g, int64_t n, double r2, int rings,
                                                long long *__restrict__ counts,
                                                const long long *__restrict__ indptr,
                                                int32_t *__restrict__ indices)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double qx = g.sx[t], qy = g.sy[t];
    const int qid = g.sid[t];
    long long cnt = 0;
    int32_t *row = FILL ? indices + indptr[qid] : nullptr;
    // short rows are kept ascending by insertion; long ones (large radii) are appended and heap-sorted at the end:
    // insertion in global memory is O(degree^2) writes
    const bool by_insertion = FILL ? (indptr[qid + 1] - indptr[qid] <= 32) : true;
    window_walk<false>(g, qx, qy, rings, 0, [&](int s) {
        const int cid = g.sid[s];
        const double d = BinGrid::dist2(qx, qy, g.sx[s], g.sy[s]);
        // (& not &&: with the short circuit the compiler loads sid[s], waits and branches before it loads sx[s] / sy[s],
        // two or three memory latencies per candidate instead of one)
        if ((cid != qid) & (d <= r2)) {
            if (FILL) {
                long long j = cnt;
                if (by_insertion)
                    while (j > 0 && row[j - 1] > cid) { row[j] = row[j - 1]; --j; }
                row[j] = cid;
            }
            ++cnt;
        }
    });
    if (!FILL) counts[qid] = cnt;
    if (FILL && !by_insertion) {   // in-place heapsort, ascending
        auto sift = [&](long long root, long long end) {
            for (;;) {
                long long child = 2 * root + 1;
                if (child >= end) break;
                if (child + 1 < end && row[child] < row[child + 1]) ++child;
                if (row[root] >= row[child]) break;
                const int32_t tmp = row[root]; row[root] = row[child]; row[child] = tmp;
                root = child;
            }
        };
        for (long long k = cnt / 2 - 1; k >= 0; --k) sift(k, cnt);
        for (long long end = cnt - 1; end > 0; --end) {
            const int32_t tmp = row[0]; row[0] = row[end]; row[end] = tmp;
            sift(0, end);
        }
    }
}

extern "C" int sc_radius_count_2d(sc_ctx *c, const double *xy, int64_t n, double radius, int64_t *indptr_out)
{
    SC_REQUIRE(c && xy && indptr_out, SC_ERR_INVALID, "sc_radius_count_2d: null pointer");
    SC_REQUIRE(radius > 0 && isfinite(radius), SC_ERR_INVALID, "radius must be > 0, got %g", radius);
    SC_HIP(hipSetDevice(c->device));
    sc_graph_moments_drain(c);   // (a moments job on the side stream uses gt_cursor and reads the graph's arrays)
    // bins no smaller than the radius: a 3x3 window always covers the closed ball
    SC_TRY(sc_bin_points(c, xy, n, 4.0, radius));
    SC_TRY(c->rad_indptr.ensure(sizeof(long long) * (size_t)(n + 1), &c->mem));
    SC_TRY(c->gt_cursor.ensure(sizeof(long long) * (size_t)(n + 1), &c->mem));
    long long *counts = c->gt_cursor.as<long long>();
    SC_HIP(hipMemsetAsync(counts, 0, sizeof(long long) * (size_t)(n + 1), c->stream));
    hipLaunchKernelGGL(k_radius<false>, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, c->stream, sc_bin_grid(c), n,
                       radius * radius, sc_window_rings(c, radius), counts, (const long long *)nullptr, (int32_t *)nullptr);
    SC_HIP(hipGetLastError());
    SC_TRY(sc_counts_to_offsets(c, counts, c->rad_indptr.as<long long>(), n, &c->rad_nnz));
    SC_HIP(hipMemcpyAsync(indptr_out, c->rad_indptr.p, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost,
                          c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    c->radius = radius;   // the count is pending: until the next sc_bin_points, i.e. the next neighbour search of any kind
    return SC_OK;
}

extern "C" int sc_radius_fill_2d(sc_ctx *c, int64_t nnz, int32_t *indices_out)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "null context");
    SC_HIP(hipSetDevice(c->device));
    SC_REQUIRE(c->radius > 0 && c->pts_n > 0, SC_ERR_STATE, "sc_radius_fill_2d: call sc_radius_count_2d first");
    const int64_t n = c->pts_n;
    SC_REQUIRE(c->rad_nnz == nnz, SC_ERR_INVALID, "sc_radius_fill_2d: nnz=%lld but the count pass found %lld",
               (long long)nnz, c->rad_nnz);
    SC_REQUIRE(nnz == 0 || indices_out, SC_ERR_INVALID, "sc_radius_fill_2d: null output");
    sc_graph_drop(c);   // this pass uses g_indices as scratch (overwrites it, maybe reallocates it)
    SC_TRY(c->g_indices.ensure(sizeof(int32_t) * (size_t)(nnz > 0 ? nnz : 1), &c->mem));
    hipLaunchKernelGGL(k_radius<true>, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, c->stream, sc_bin_grid(c), n,
                       c->radius * c->radius, sc_window_rings(c, c->radius), (long long *)nullptr,
                       c->rad_indptr.as<long long>(), c->g_indices.as<int32_t>());
    SC_HIP(hipGetLastError());
    if (nnz > 0)
        SC_HIP(hipMemcpyAsync(indices_out, c->g_indices.p, sizeof(int32_t) * (size_t)nnz, hipMemcpyDeviceToHost,
                              c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}

// ------------------------------------------------------------------------------------------------
// N3: domain distances (reference src/spatialcore/spatial/distance.py)
// ------------------------------------------------------------------------------------------------

// nearest target of every query: ring walk over the TARGET bin grid (queries may lie outside it).
// Ties go to the lowest target index.  dist = sqrt(fl(fl(dx*dx)+fl(dy*dy))), as cKDTree.query / cdist.
// EXCL: a target whose group code equals the query's exclusion code is skipped (idx -1 / +inf when nothing is left).
template <bool EXCL>
__global__ __launch_bounds__(256) void k_nearest(BinGrid g, const double *__restrict__ qxy, int64_t n_q,
                                                 int32_t *__restrict__ idx_out, double *__restrict__ dist_out,
                                                 const int32_t *__restrict__ tgt_code,
                                                 const int32_t *__restrict__ q_excl)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_q) return;
    const double qx = qxy[2 * t], qy = qxy[2 * t + 1];
    const int32_t excl = EXCL ? q_excl[t] : -1;
    double best = DBL_MAX;
    int best_id = 0x7fffffff;
    ring_walk(g, qx, qy,
              [&](int s) {
                  const double d = BinGrid::dist2(qx, qy, g.sx[s], g.sy[s]);
                  const int cid = g.sid[s];
                  if (EXCL && tgt_code[cid] == excl) return;
                  if (cand_better(d, cid, best, best_id)) { best = d; best_id = cid; }
              },
              [&] { return best; });
    const bool none = best_id == 0x7fffffff;
    idx_out[t] = none ? -1 : best_id;
    dist_out[t] = none ? HUGE_VAL : __dsqrt_rn(best);
}

static int nearest_impl(sc_ctx *c, const char *who, const double *xy_targets, const int32_t *tgt_code,
                        int64_t n_targets, const double *xy_queries, const int32_t *q_excl, int64_t n_queries,
                        int32_t *idx_out, double *dist_out)
{
    SC_REQUIRE(c && xy_targets && xy_queries && idx_out && dist_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(n_targets >= 1 && n_queries >= 1 && n_queries <= 0x7fffffffLL, SC_ERR_INVALID,
               "%s: need at least one target and one query", who);
    SC_HIP(hipSetDevice(c->device));
    c->knn_n = 0;   // (not for the bins' sake: the queries' result overwrites knn_idx / knn_rd, the last kNN result's buffers)
    SC_TRY(sc_bin_points(c, xy_targets, n_targets, 4.0, 0.0));
    for (int64_t i = 0; i < n_queries; ++i)
        SC_REQUIRE(isfinite(xy_queries[2 * i]) && isfinite(xy_queries[2 * i + 1]), SC_ERR_INVALID,
                   "query coordinate %lld is not finite", (long long)i);
    SC_TRY(c->e_tmp_data.ensure(sizeof(double) * 2 * (size_t)n_queries, &c->mem));
    SC_TRY(c->knn_idx.ensure(sizeof(int32_t) * (size_t)n_queries, &c->mem));
    SC_TRY(c->knn_rd.ensure(sizeof(double) * (size_t)n_queries, &c->mem));
    SC_HIP(hipMemcpyAsync(c->e_tmp_data.p, xy_queries, sizeof(double) * 2 * (size_t)n_queries, hipMemcpyHostToDevice,
                          c->stream));
    const bool excl = tgt_code && q_excl;
    if (excl) {
        SC_TRY(c->e_tmp_indices.ensure(sizeof(int32_t) * (size_t)(n_targets + n_queries), &c->mem));
        SC_HIP(hipMemcpyAsync(c->e_tmp_indices.p, tgt_code, sizeof(int32_t) * (size_t)n_targets, hipMemcpyHostToDevice,
                              c->stream));
        SC_HIP(hipMemcpyAsync(c->e_tmp_indices.as<int32_t>() + n_targets, q_excl, sizeof(int32_t) * (size_t)n_queries,
                              hipMemcpyHostToDevice, c->stream));
    }
    {
        KernelTimerScope ts(c, SC_K_KNN);
        const int32_t *codes = excl ? c->e_tmp_indices.as<int32_t>() : nullptr;
        const auto kernel = excl ? k_nearest<true> : k_nearest<false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)ceil_div64(n_queries, 256)), dim3(256), 0, c->stream, sc_bin_grid(c),
                           c->e_tmp_data.as<double>(), n_queries, c->knn_idx.as<int32_t>(), c->knn_rd.as<double>(), codes,
                           excl ? codes + n_targets : nullptr);
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(idx_out, c->knn_idx.p, sizeof(int32_t) * (size_t)n_queries, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipMemcpyAsync(dist_out, c->knn_rd.p, sizeof(double) * (size_t)n_queries, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}

extern "C" int sc_nearest_2d(sc_ctx *c, const double *xy_targets, int64_t n_targets, const double *xy_queries,
                             int64_t n_queries, int32_t *idx_out, double *dist_out)
{
    return nearest_impl(c, "sc_nearest_2d", xy_targets, nullptr, n_targets, xy_queries, nullptr, n_queries, idx_out,
                        dist_out);
}

extern "C" int sc_nearest_excluding_2d(sc_ctx *c, const double *xy_targets, const int32_t *target_code,
                                       int64_t n_targets, const double *xy_queries, const int32_t *query_excluded_code,
                                       int64_t n_queries, int32_t *idx_out, double *dist_out)
{
    SC_REQUIRE(target_code && query_excluded_code, SC_ERR_INVALID, "sc_nearest_excluding_2d: null code array");
    return nearest_impl(c, "sc_nearest_excluding_2d", xy_targets, target_code, n_targets, xy_queries,
                        query_excluded_code, n_queries, idx_out, dist_out);
}

// brute-force pairwise euclidean distances between two point sets, LDS-tiled: block = 256 points of A
// (one per thread, in registers) x the whole of B streamed through LDS in tiles of 1024 points.
// partial[block] = {sum of distances, min distance} for the block's A points.
#define PW_BTILE 1024

// (a NaN distance would be kept by `sum += d` and skipped by `d < mn`: a NaN mean beside a finite minimum)
int require_finite_points(const char *who, const char *set, const double *xy, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        SC_REQUIRE(isfinite(xy[2 * i]) && isfinite(xy[2 * i + 1]), SC_ERR_INVALID, "%s: %s coordinate %lld is not finite",
                   who, set, (long long)i);
    return SC_OK;
}

__global__ __launch_bounds__(256) void k_pairwise(const double *__restrict__ a, int64_t n_a,
                                                  const double *__restrict__ b, int64_t n_b,
                                                  double *__restrict__ partial)
{
    __shared__ double2 tile[PW_BTILE];
    __shared__ double red_s[256], red_m[256];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n_a;
    const double ax = live ? a[2 * i] : 0.0, ay = live ? a[2 * i + 1] : 0.0;
    double sum = 0.0, mn = DBL_MAX;
    for (int64_t j0 = 0; j0 < n_b; j0 += PW_BTILE) {
        const int cnt = (int)(n_b - j0 < PW_BTILE ? n_b - j0 : PW_BTILE);
        __syncthreads();
        for (int k = threadIdx.x; k < cnt; k += 256) tile[k] = reinterpret_cast<const double2 *>(b)[j0 + k];
        __syncthreads();
        if (live) {
            for (int k = 0; k < cnt; ++k) {
                const double d = __dsqrt_rn(BinGrid::dist2(ax, ay, tile[k].x, tile[k].y));
                sum += d;
                mn = d < mn ? d : mn;
            }
        }
    }
    red_s[threadIdx.x] = sum;
    red_m[threadIdx.x] = mn;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red_s[threadIdx.x] += red_s[threadIdx.x + s];
            red_m[threadIdx.x] = red_m[threadIdx.x + s] < red_m[threadIdx.x] ? red_m[threadIdx.x + s] : red_m[threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = red_s[0];
        partial[2 * blockIdx.x + 1] = red_m[0];
    }
}

extern "C" int sc_pairwise_2d(sc_ctx *c, const double *xy_a, int64_t n_a, const double *xy_b, int64_t n_b,
                              double *mean_out, double *min_out)
{
    SC_REQUIRE(c && xy_a && xy_b, SC_ERR_INVALID, "sc_pairwise_2d: null pointer");
    SC_REQUIRE(n_a >= 1 && n_b >= 1, SC_ERR_INVALID, "sc_pairwise_2d: empty point set");
    SC_TRY(require_finite_points("sc_pairwise_2d", "a", xy_a, n_a));
    SC_TRY(require_finite_points("sc_pairwise_2d", "b", xy_b, n_b));
    SC_HIP(hipSetDevice(c->device));
    const int blocks = (int)ceil_div64(n_a, 256);
    SC_TRY(c->e_tmp_data.ensure(sizeof(double) * 2 * (size_t)(n_a + n_b), &c->mem));
    SC_TRY(c->red_tmp.ensure(sizeof(double) * 2 * (size_t)blocks, &c->mem));
    double *da = c->e_tmp_data.as<double>(), *db = da + 2 * n_a;
    SC_HIP(hipMemcpyAsync(da, xy_a, sizeof(double) * 2 * (size_t)n_a, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(db, xy_b, sizeof(double) * 2 * (size_t)n_b, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_pairwise, dim3(blocks), dim3(256), 0, c->stream, da, n_a, db, n_b, c->red_tmp.as<double>());
    SC_HIP(hipGetLastError());
    std::vector<double> h((size_t)blocks * 2);
    SC_HIP(hipMemcpyAsync(h.data(), c->red_tmp.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    double s = 0.0, m = DBL_MAX;
    for (int k = 0; k < blocks; ++k) { s += h[2 * k]; m = h[2 * k + 1] < m ? h[2 * k + 1] : m; }
    if (mean_out) *mean_out = s / ((double)n_a * (double)n_b);
    if (min_out) *min_out = m;
    return SC_OK;
}

// Every (source group, target group) block of the all-pairs distance matrix in one launch: the A points are sorted by
// group and cut into chunks of <= 256 points that never straddle a group; workgroup (chunk, t) streams target group
// t through LDS and leaves {sum, min} of its block.  Replaces the reference's per-pair cdist(src, tgt).mean()/.min()
// loops (distance.py:266-270, 340-350, 387-398).
__global__ __launch_bounds__(256) void k_pair_table(const double *__restrict__ a, const int64_t *__restrict__ chunk_a0,
                                                    const int32_t *__restrict__ chunk_cnt,
                                                    const double *__restrict__ b, const int64_t *__restrict__ b_off,
                                                    int n_groups_b, double *__restrict__ partial)
{
    __shared__ double2 tile[PW_BTILE];
    __shared__ double red_s[256], red_m[256];
    const int64_t a0 = chunk_a0[blockIdx.x];
    const bool live = (int)threadIdx.x < chunk_cnt[blockIdx.x];
    const double ax = live ? a[2 * (a0 + threadIdx.x)] : 0.0, ay = live ? a[2 * (a0 + threadIdx.x) + 1] : 0.0;
    const int64_t b0 = b_off[blockIdx.y], b1 = b_off[blockIdx.y + 1];
    double sum = 0.0, mn = DBL_MAX;
    for (int64_t j0 = b0; j0 < b1; j0 += PW_BTILE) {
        const int cnt = (int)(b1 - j0 < PW_BTILE ? b1 - j0 : PW_BTILE);
        __syncthreads();
        for (int k = threadIdx.x; k < cnt; k += 256) tile[k] = reinterpret_cast<const double2 *>(b)[j0 + k];
        __syncthreads();
        if (live) {
            for (int k = 0; k < cnt; ++k) {
                const double d = __dsqrt_rn(BinGrid::dist2(ax, ay, tile[k].x, tile[k].y));
                sum += d;
                mn = d < mn ? d : mn;
            }
        }
    }
    red_s[threadIdx.x] = sum;
    red_m[threadIdx.x] = mn;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red_s[threadIdx.x] += red_s[threadIdx.x + s];
            red_m[threadIdx.x] = red_m[threadIdx.x + s] < red_m[threadIdx.x] ? red_m[threadIdx.x + s] : red_m[threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double *o = partial + 2 * ((int64_t)blockIdx.x * n_groups_b + blockIdx.y);
        o[0] = red_s[0];
        o[1] = red_m[0];
    }
}

extern "C" int sc_pair_table_2d(sc_ctx *c, const double *xy_a, const int64_t *a_off, int32_t n_groups_a,
                                const double *xy_b, const int64_t *b_off, int32_t n_groups_b, double *sum_out,
                                double *min_out)
{
    SC_REQUIRE(c && xy_a && xy_b && a_off && b_off && sum_out && min_out, SC_ERR_INVALID, "sc_pair_table_2d: null pointer");
    SC_REQUIRE(n_groups_a >= 1 && n_groups_b >= 1 && n_groups_b <= 65535, SC_ERR_INVALID,
               "sc_pair_table_2d: group counts out of range (%d, %d)", n_groups_a, n_groups_b);
    SC_REQUIRE(a_off[0] == 0 && b_off[0] == 0, SC_ERR_INVALID, "sc_pair_table_2d: offsets must start at 0");
    for (int g = 0; g < n_groups_a; ++g)
        SC_REQUIRE(a_off[g + 1] >= a_off[g], SC_ERR_INVALID, "sc_pair_table_2d: source offsets not monotone");
    for (int g = 0; g < n_groups_b; ++g)
        SC_REQUIRE(b_off[g + 1] >= b_off[g], SC_ERR_INVALID, "sc_pair_table_2d: target offsets not monotone");
    const int64_t n_a = a_off[n_groups_a], n_b = b_off[n_groups_b];
    SC_REQUIRE(n_a >= 1 && n_b >= 1, SC_ERR_INVALID, "sc_pair_table_2d: empty point set");
    SC_TRY(require_finite_points("sc_pair_table_2d", "source", xy_a, n_a));
    SC_TRY(require_finite_points("sc_pair_table_2d", "target", xy_b, n_b));
    SC_HIP(hipSetDevice(c->device));
    std::vector<int64_t> ch0;
    std::vector<int32_t> chn, chg;
    for (int g = 0; g < n_groups_a; ++g)
        for (int64_t p = a_off[g]; p < a_off[g + 1]; p += 256) {
            ch0.push_back(p);
            chn.push_back((int32_t)(a_off[g + 1] - p < 256 ? a_off[g + 1] - p : 256));
            chg.push_back(g);
        }
    const size_t chunks = ch0.size();
    SC_REQUIRE(chunks <= 0x7fffffffULL, SC_ERR_INVALID, "sc_pair_table_2d: too many points");
    SC_TRY(c->e_tmp_data.ensure(sizeof(double) * 2 * (size_t)(n_a + n_b), &c->mem));
    SC_TRY(c->e_tmp_indptr.ensure(sizeof(int64_t) * (chunks + (size_t)n_groups_b + 1), &c->mem));
    SC_TRY(c->e_tmp_indices.ensure(sizeof(int32_t) * chunks, &c->mem));
    SC_TRY(c->red_tmp.ensure(sizeof(double) * 2 * chunks * (size_t)n_groups_b, &c->mem));
    double *da = c->e_tmp_data.as<double>(), *db = da + 2 * n_a;
    int64_t *d_ch0 = c->e_tmp_indptr.as<int64_t>(), *d_boff = d_ch0 + chunks;
    SC_HIP(hipMemcpyAsync(da, xy_a, sizeof(double) * 2 * (size_t)n_a, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(db, xy_b, sizeof(double) * 2 * (size_t)n_b, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(d_ch0, ch0.data(), sizeof(int64_t) * chunks, hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(d_boff, b_off, sizeof(int64_t) * (size_t)(n_groups_b + 1), hipMemcpyHostToDevice, c->stream));
    SC_HIP(hipMemcpyAsync(c->e_tmp_indices.p, chn.data(), sizeof(int32_t) * chunks, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_pair_table, dim3((unsigned)chunks, (unsigned)n_groups_b), dim3(256), 0, c->stream, da, d_ch0,
                       c->e_tmp_indices.as<int32_t>(), db, d_boff, (int)n_groups_b, c->red_tmp.as<double>());
    SC_HIP(hipGetLastError());
    std::vector<double> h(2 * chunks * (size_t)n_groups_b);
    SC_HIP(hipMemcpyAsync(h.data(), c->red_tmp.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    // chunks of a group are reduced in ascending order: run-to-run reproducible
    for (int64_t k = 0; k < (int64_t)n_groups_a * n_groups_b; ++k) { sum_out[k] = 0.0; min_out[k] = HUGE_VAL; }
    for (size_t ch = 0; ch < chunks; ++ch)
        for (int t = 0; t < n_groups_b; ++t) {
            if (b_off[t + 1] == b_off[t]) continue;
            const size_t o = (size_t)chg[ch] * n_groups_b + t;
            sum_out[o] += h[2 * (ch * n_groups_b + t)];
            const double m = h[2 * (ch * n_groups_b + t) + 1];
            if (m < min_out[o]) min_out[o] = m;
        }
    return SC_OK;
}
