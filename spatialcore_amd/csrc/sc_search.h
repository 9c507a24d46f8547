// The uniform bin grid of the neighbour searches and the two ways kernels walk it (device helpers; sc_search.hip,
// sc_labelperm.hip).  Every search result is pinned bit for bit, so what decides it is written here once: the distance
// arithmetic, the order in which positions are visited, and the rule that ends a ring walk.
#pragma once

#include <float.h>

#include "sc_ctx.h"

// bin of a coordinate, clamped to the grid
__device__ __forceinline__ int bin_coord(double v, double v0, double inv_h, int nb)
{
    int b = (int)floor((v - v0) * inv_h);
    return b < 0 ? 0 : (b >= nb ? nb - 1 : b);
}

// The bin-sorted points of the last sc_bin_points (built by sc_bin_grid, passed to kernels by value): position s holds
// point sid[s] at (sx[s], sy[s]); bin (bx, by) holds positions [bin_start[by * nbx + bx], bin_start[by * nbx + bx + 1]),
// so a row of bins is one contiguous range and positions grow with by.
struct BinGrid {
    const double *sx, *sy;
    const int32_t *sid, *bin_start;
    double x0, y0, h;
    int nbx, nby;
    // squared distance with the products and the sum rounded separately, as the tree codes do it: the project's tie
    // rule rests on these bits ("Tie rule for kNN")
    static __device__ __forceinline__ double dist2(double ax, double ay, double bx, double by)
    {
        const double dx = ax - bx, dy = ay - by;
        return __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
    }
};

// Square rings of bins around the query, nearest first: visit(s) for every position s of a ring (rows bottom to top;
// the ring's bottom and top rows in full, of the rows between only the two end bins), then stop once bound() -- the
// squared distance beyond which the caller wants nothing more -- is below the squared distance from the query to the
// nearest unvisited region.  That makes the result exact: nothing outside the visited window can beat what was kept.
// The query may lie outside the grid.
template <class Visit, class Bound>
__device__ __forceinline__ void ring_walk(const BinGrid &g, double qx, double qy, Visit visit, Bound bound)
{
    const double x0 = g.x0, y0 = g.y0, h = g.h;
    const int nbx = g.nbx, nby = g.nby;
    const double inv_h = 1.0 / h;
    const int bx = bin_coord(qx, x0, inv_h, nbx), by = bin_coord(qy, y0, inv_h, nby);
    const int rmax = (nbx > nby ? nbx : nby);
    const double slack = 1e-9 * h;
    for (int r = 0; r <= rmax; ++r) {
        const int ylo = by - r, yhi = by + r, xlo = bx - r, xhi = bx + r;
        const int cxlo = xlo < 0 ? 0 : xlo, cxhi = xhi >= nbx ? nbx - 1 : xhi;
        for (int yy = (ylo < 0 ? 0 : ylo); yy <= (yhi >= nby ? nby - 1 : yhi); ++yy) {
            const bool full = (yy == ylo) || (yy == yhi);
            // full row of the ring: bins [cxlo, cxhi]; interior rows: only the two end bins
            for (int seg = 0; seg < (full ? 1 : 2); ++seg) {
                int b0, b1;
                if (full) { b0 = cxlo; b1 = cxhi; }
                else if (seg == 0) { if (xlo < 0) continue; b0 = b1 = xlo; }
                else { if (xhi >= nbx || r == 0) continue; b0 = b1 = xhi; }
                const int s0 = g.bin_start[yy * nbx + b0], s1 = g.bin_start[yy * nbx + b1 + 1];
                for (int s = s0; s < s1; ++s) visit(s);
            }
        }
        // distance from the query to the nearest unvisited region
        const bool l_out = xlo <= 0, r_out = xhi >= nbx - 1, b_out = ylo <= 0, t_out = yhi >= nby - 1;
        if (l_out && r_out && b_out && t_out) break;  // everything visited
        double m = DBL_MAX;
        if (!l_out) m = fmin(m, qx - (x0 + (double)xlo * h));
        if (!r_out) m = fmin(m, (x0 + (double)(xhi + 1) * h) - qx);
        if (!b_out) m = fmin(m, qy - (y0 + (double)ylo * h));
        if (!t_out) m = fmin(m, (y0 + (double)(yhi + 1) * h) - qy);
        m -= slack;
        if (m > 0.0 && bound() < m * m) break;
    }
}

// The window of `rings` bins to every side of the query's bin (rings from sc_window_rings: it covers the closed ball),
// row by row, ascending positions: visit(s) for every position s of it.  UPPER: only the positions behind `own`, the
// query's own position, i.e. every unordered pair once; rows below the query's hold only smaller positions (positions
// grow with the bin key) and are not looked at.
template <bool UPPER, class Visit>
__device__ __forceinline__ void window_walk(const BinGrid &g, double qx, double qy, int rings, int own, Visit visit)
{
    const int nbx = g.nbx, nby = g.nby;
    const double inv_h = 1.0 / g.h;
    const int bx = bin_coord(qx, g.x0, inv_h, nbx), by = bin_coord(qy, g.y0, inv_h, nby);
    const int ylo = UPPER ? by : (by - rings < 0 ? 0 : by - rings), yhi = by + rings >= nby ? nby - 1 : by + rings;
    const int xlo = bx - rings < 0 ? 0 : bx - rings, xhi = bx + rings >= nbx ? nbx - 1 : bx + rings;
    for (int yy = ylo; yy <= yhi; ++yy) {
        int s0 = g.bin_start[yy * nbx + xlo];
        const int s1 = g.bin_start[yy * nbx + xhi + 1];
        if (UPPER && s0 <= own) s0 = own + 1;   // (the query's own row only: the rows above start behind it)
        for (int s = s0; s < s1; ++s) visit(s);
    }
}
