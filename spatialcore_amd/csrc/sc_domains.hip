// N7: spatial domains by buffer - union - shrink over discs (make_spatial_domains; the reference hands this step to R:
// src/spatialcore/spatial/domains.py:579-638, r_functions.R:34-124).  gfx950 only.
//
// T = target points, d = buffer radius, s = the shrink (d minus the margin kept).  U = union of the closed discs of
// radius d about T.  Two kernels on the bin grid of the targets (sc_search.h):
//  - k_dom_link: the polygons of U are the connected components of the graph on T with an edge iff
//    dist2 <= (2d)^2.  Lock-free union-find on an int32 parent array indexed by TARGET INDEX: every edge hooks the
//    larger root under the smaller (atomicCAS), finds halve their path (atomicMin), so a parent is never larger than
//    its child and the root of a finished tree is the smallest index of the component -- a function of the input, not
//    of the order in which the atomics landed.  k_dom_flatten then points every target at its root.
//  - k_dom_cover: a query p is in the shrunken region iff the closed disc of radius s about p lies in U, i.e. iff
//    clearance(p) = min(s, dist(p, complement of U)) >= s.  The nearest boundary point closer than s is a foot point
//    t_i + d (p - t_i) / |p - t_i| of a circle that contains p, or an intersection point of two circles, and counts
//    only if no other disc holds it strictly inside.  One query per lane; the candidate and validity loops are window
//    walks nested in each other (nothing is gathered into memory), behind two exits that decide most queries: a
//    target within d - s (inside, clearance s) and no target within d (outside, -1).
#include <float.h>
#include <math.h>

#include "sc_search.h"
#include "sc_unionfind.h"

// ------------------------------------------------------------------------------------------------
// components
// ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_dom_init(int32_t *__restrict__ parent, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) parent[i] = (int32_t)i;
}

__global__ __launch_bounds__(256) void k_dom_link(BinGrid g, int64_t n, double link2, int rings,
                                                  int32_t *__restrict__ parent)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double qx = g.sx[t], qy = g.sy[t];
    const int32_t qid = g.sid[t];
    window_walk<true>(g, qx, qy, rings, (int)t, [&](int s) {
        if (BinGrid::dist2(qx, qy, g.sx[s], g.sy[s]) <= link2) uf_union(parent, qid, g.sid[s]);
    });
}

__global__ __launch_bounds__(256) void k_dom_flatten(int32_t *__restrict__ parent, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t root = uf_find(parent, (int32_t)i);
    atomicMin(parent + i, root);
}

// ------------------------------------------------------------------------------------------------
// coverage
// ------------------------------------------------------------------------------------------------

// is the boundary candidate (cx, cy), a point of the circles about (ax, ay) and (bx, by), strictly inside no other disc?
// Targets on the very spot of one of the two are the same circle, not another disc.  Every disc that can hold a
// candidate closer than s to the query has its centre within d + s of the query: inside the window.
__device__ __forceinline__ bool dom_on_boundary(const BinGrid &g, double qx, double qy, int rings, double d2, double cx,
                                                double cy, double ax, double ay, double bx, double by)
{
    bool covered = false;
    window_walk<false>(g, qx, qy, rings, 0, [&](int k) {
        if (covered) return;
        const double kx = g.sx[k], ky = g.sy[k];
        const bool own = ((kx == ax) & (ky == ay)) | ((kx == bx) & (ky == by));
        covered = !own & (BinGrid::dist2(cx, cy, kx, ky) < d2);
    });
    return !covered;
}

__global__ __launch_bounds__(256) void k_dom_cover(BinGrid g, const double *__restrict__ qxy, int64_t n_q, double d,
                                                   double s, int rings, const int32_t *__restrict__ comp,
                                                   int32_t *__restrict__ qcomp, double *__restrict__ clear_out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_q) return;
    const double qx = qxy[2 * t], qy = qxy[2 * t + 1];
    const double d2 = d * d, m = d - s, m2 = m * m, link2 = (d + d) * (d + d);
    // the nearest target decides both exits and names the component
    double near2 = DBL_MAX;
    int near_id = 0x7fffffff;
    window_walk<false>(g, qx, qy, rings, 0, [&](int i) {
        const double r2 = BinGrid::dist2(qx, qy, g.sx[i], g.sy[i]);
        const int id = g.sid[i];
        if (r2 < near2 || (r2 == near2 && id < near_id)) { near2 = r2; near_id = id; }
    });
    if (!(near2 <= d2)) {   // outside U
        qcomp[t] = -1;
        clear_out[t] = -1.0;
        return;
    }
    double best = s;
    if (!(near2 <= m2)) {   // the rim of U: the boundary may be closer than s
        // foot points on the circles that contain the query
        window_walk<false>(g, qx, qy, rings, 0, [&](int i) {
            const double ix = g.sx[i], iy = g.sy[i];
            const double r2 = BinGrid::dist2(qx, qy, ix, iy);
            if (!(r2 > 0.0) | !(r2 <= d2)) return;
            const double r = __dsqrt_rn(r2), fd = d - r;
            if (!(fd < best)) return;
            const double sc = d / r;
            const double cx = ix + sc * (qx - ix), cy = iy + sc * (qy - iy);
            if (dom_on_boundary(g, qx, qy, rings, d2, cx, cy, ix, iy, ix, iy)) best = fd;
        });
        // intersection points of two circles: one closer than `best` to the query lies on circles whose centres are
        // between d - best and d + best from it
        window_walk<false>(g, qx, qy, rings, 0, [&](int i) {
            const double ix = g.sx[i], iy = g.sy[i];
            const double ri = __dsqrt_rn(BinGrid::dist2(qx, qy, ix, iy));
            if (!(ri < d + best) | !(ri > d - best)) return;
            window_walk<false>(g, qx, qy, rings, 0, [&](int j) {
                if (j <= i) return;
                const double jx = g.sx[j], jy = g.sy[j];
                const double rj = __dsqrt_rn(BinGrid::dist2(qx, qy, jx, jy));
                if (!(rj < d + best) | !(rj > d - best)) return;
                const double D2 = BinGrid::dist2(ix, iy, jx, jy);
                if (!(D2 > 0.0) | !(D2 <= link2)) return;
                const double D = __dsqrt_rn(D2), half = D / 2.0;
                const double h2 = d2 - half * half;
                const double h = __dsqrt_rn(h2 > 0.0 ? h2 : 0.0);
                const double ux = (jx - ix) / D, uy = (jy - iy) / D;
                const double mx = (ix + jx) / 2.0, my = (iy + jy) / 2.0;
#pragma unroll
                for (int side = 0; side < 2; ++side) {
                    const double sg = side ? -1.0 : 1.0;
                    const double cx = mx - sg * h * uy, cy = my + sg * h * ux;
                    const double cd = __dsqrt_rn(BinGrid::dist2(qx, qy, cx, cy));
                    if (cd < best && dom_on_boundary(g, qx, qy, rings, d2, cx, cy, ix, iy, jx, jy)) best = cd;
                }
            });
        });
    }
    qcomp[t] = best >= s ? comp[near_id] : -1;
    clear_out[t] = best;
}

// ------------------------------------------------------------------------------------------------

extern "C" int sc_domains_2d(sc_ctx *c, const double *xy_targets, int64_t n_targets, const double *xy_queries,
                             int64_t n_queries, double cell_dist, double shrink, int32_t *target_component_out,
                             int32_t *query_component_out, double *clearance_out)
{
    SC_REQUIRE(c && xy_targets && target_component_out, SC_ERR_INVALID, "sc_domains_2d: null pointer");
    SC_REQUIRE(n_targets >= 1 && n_targets <= 0x7fffffffLL, SC_ERR_INVALID, "sc_domains_2d: n_targets=%lld out of range",
               (long long)n_targets);
    SC_REQUIRE(n_queries >= 0 && n_queries <= 0x7fffffffLL, SC_ERR_INVALID, "sc_domains_2d: n_queries=%lld out of range",
               (long long)n_queries);
    SC_REQUIRE(n_queries == 0 || (xy_queries && query_component_out), SC_ERR_INVALID,
               "sc_domains_2d: null query array with n_queries=%lld", (long long)n_queries);
    SC_REQUIRE(isfinite(cell_dist) && cell_dist > 0.0, SC_ERR_INVALID, "sc_domains_2d: cell_dist must be finite and > 0, got %g",
               cell_dist);
    SC_REQUIRE(isfinite(shrink) && shrink >= 0.0 && shrink < cell_dist, SC_ERR_INVALID,
               "sc_domains_2d: shrink must lie in [0, cell_dist), got %g with cell_dist=%g", shrink, cell_dist);
    for (int64_t i = 0; i < n_queries; ++i)
        SC_REQUIRE(isfinite(xy_queries[2 * i]) && isfinite(xy_queries[2 * i + 1]), SC_ERR_INVALID,
                   "sc_domains_2d: query coordinate %lld is not finite", (long long)i);
    SC_HIP(hipSetDevice(c->device));
    const double d = cell_dist, link = d + d;
    // bins no smaller than d: two rings cover the linking distance 2d and the coverage reach d + s
    SC_TRY(sc_bin_points(c, xy_targets, n_targets, 4.0, d));
    SC_TRY(c->dm_parent.ensure(sizeof(int32_t) * (size_t)n_targets, &c->mem));
    int32_t *parent = c->dm_parent.as<int32_t>();
    const unsigned grid_t = (unsigned)ceil_div64(n_targets, 256);
    hipLaunchKernelGGL(k_dom_init, dim3(grid_t), dim3(256), 0, c->stream, parent, n_targets);
    hipLaunchKernelGGL(k_dom_link, dim3(grid_t), dim3(256), 0, c->stream, sc_bin_grid(c), n_targets, link * link,
                       sc_window_rings(c, link), parent);
    hipLaunchKernelGGL(k_dom_flatten, dim3(grid_t), dim3(256), 0, c->stream, parent, n_targets);
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(target_component_out, parent, sizeof(int32_t) * (size_t)n_targets, hipMemcpyDeviceToHost,
                          c->stream));
    if (n_queries > 0) {
        SC_TRY(c->e_tmp_data.ensure(sizeof(double) * 2 * (size_t)n_queries, &c->mem));
        SC_TRY(c->dm_qcomp.ensure(sizeof(int32_t) * (size_t)n_queries, &c->mem));
        SC_TRY(c->dm_clear.ensure(sizeof(double) * (size_t)n_queries, &c->mem));
        SC_HIP(hipMemcpyAsync(c->e_tmp_data.p, xy_queries, sizeof(double) * 2 * (size_t)n_queries, hipMemcpyHostToDevice,
                              c->stream));
        hipLaunchKernelGGL(k_dom_cover, dim3((unsigned)ceil_div64(n_queries, 256)), dim3(256), 0, c->stream, sc_bin_grid(c),
                           c->e_tmp_data.as<double>(), n_queries, d, shrink, sc_window_rings(c, d + shrink), parent,
                           c->dm_qcomp.as<int32_t>(), c->dm_clear.as<double>());
        SC_HIP(hipGetLastError());
        SC_HIP(hipMemcpyAsync(query_component_out, c->dm_qcomp.p, sizeof(int32_t) * (size_t)n_queries,
                              hipMemcpyDeviceToHost, c->stream));
        if (clearance_out)
            SC_HIP(hipMemcpyAsync(clearance_out, c->dm_clear.p, sizeof(double) * (size_t)n_queries, hipMemcpyDeviceToHost,
                                  c->stream));
    }
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}
