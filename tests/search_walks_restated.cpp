// Host restatement check of csrc/sc_search.h: ring_walk and window_walk against the loops written out the way the
// search kernels had them before the helpers existed -- same positions in the same order, same stopping point -- and
// against brute force (exact k nearest, closed ball inside the window).  Queries inside and outside the grid,
// degenerate extents, duplicate coordinates.  Built and run by tests/test_cpu_search_walks.py; no GPU.
#include <math.h>
#include <float.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include <algorithm>
static inline double __dadd_rn(double a, double b) { return a + b; }   // (built with -ffp-contract=off)
static inline double __dmul_rn(double a, double b) { return a * b; }
#include "sc_search.h"

static bool cand_better(double d, int id, double ed, int eid) { return d < ed || (d == ed && id < eid); }

// the ring walk written out in full (as k_knn, k_knn_heap and k_nearest each had it), recording visits; k best kept
static void old_ring(const double *sx, const double *sy, const int32_t *sid, const int32_t *bin_start, double qx, double qy,
                     double x0, double y0, double h, int nbx, int nby, int K, std::vector<int> &vis, std::vector<double> &bestd)
{
    const double inv_h = 1.0 / h;
    const int bx = bin_coord(qx, x0, inv_h, nbx), by = bin_coord(qy, y0, inv_h, nby);
    std::vector<std::pair<double,int>> best;
    auto kth = [&] { return (int)best.size() < K ? DBL_MAX : best[K - 1].first; };
    const int rmax = (nbx > nby ? nbx : nby);
    const double slack = 1e-9 * h;
    for (int r = 0; r <= rmax; ++r) {
        const int ylo = by - r, yhi = by + r, xlo = bx - r, xhi = bx + r;
        const int cxlo = xlo < 0 ? 0 : xlo, cxhi = xhi >= nbx ? nbx - 1 : xhi;
        for (int yy = (ylo < 0 ? 0 : ylo); yy <= (yhi >= nby ? nby - 1 : yhi); ++yy) {
            const bool full = (yy == ylo) || (yy == yhi);
            for (int seg = 0; seg < (full ? 1 : 2); ++seg) {
                int b0, b1;
                if (full) { b0 = cxlo; b1 = cxhi; }
                else if (seg == 0) { if (xlo < 0) continue; b0 = b1 = xlo; }
                else { if (xhi >= nbx || r == 0) continue; b0 = b1 = xhi; }
                const int s0 = bin_start[yy * nbx + b0], s1 = bin_start[yy * nbx + b1 + 1];
                for (int s = s0; s < s1; ++s) {
                    const double dx = qx - sx[s], dy = qy - sy[s];
                    const double d = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
                    vis.push_back(s);
                    best.push_back({d, sid[s]}); std::sort(best.begin(), best.end()); if ((int)best.size() > K) best.pop_back();
                }
            }
        }
        const bool l_out = xlo <= 0, r_out = xhi >= nbx - 1, b_out = ylo <= 0, t_out = yhi >= nby - 1;
        if (l_out && r_out && b_out && t_out) break;
        double m = DBL_MAX;
        if (!l_out) m = fmin(m, qx - (x0 + (double)xlo * h));
        if (!r_out) m = fmin(m, (x0 + (double)(xhi + 1) * h) - qx);
        if (!b_out) m = fmin(m, qy - (y0 + (double)ylo * h));
        if (!t_out) m = fmin(m, (y0 + (double)(yhi + 1) * h) - qy);
        m -= slack;
        if (m > 0.0 && kth() < m * m) break;
    }
    for (auto &b : best) bestd.push_back(b.first);
}

int main()
{
    srand(7);
    long checked = 0;
    for (int trial = 0; trial < 60; ++trial) {
        const int n = 1 + rand() % 3000;
        const double W = 1 + rand() % 500, H = (trial % 7 == 0) ? 0.0 : 1 + rand() % 500;
        std::vector<double> x(n), y(n);
        for (int i = 0; i < n; ++i) { x[i] = W * (rand() / (double)RAND_MAX); y[i] = H * (rand() / (double)RAND_MAX); if (trial % 5 == 0) { x[i] = floor(x[i] / 10) * 10; y[i] = floor(y[i] / 10) * 10; } }
        double xmin = *std::min_element(x.begin(), x.end()), xmax = *std::max_element(x.begin(), x.end());
        double ymin = *std::min_element(y.begin(), y.end()), ymax = *std::max_element(y.begin(), y.end());
        double w = xmax - xmin, hgt = ymax - ymin, area = (w > 0 ? w : 1.0) * (hgt > 0 ? hgt : 1.0);
        const double radius = 5 + rand() % 40;
        double h = sqrt(area * 4.0 / n); if (trial % 2) { if (h < radius) h = radius; } if (!(h > 0)) h = 1.0;
        int nbx = (int)floor(w / h) + 1, nby = (int)floor(hgt / h) + 1;
        std::vector<int> key(n), sid(n);
        for (int i = 0; i < n; ++i) { key[i] = bin_coord(y[i], ymin, 1.0 / h, nby) * nbx + bin_coord(x[i], xmin, 1.0 / h, nbx); sid[i] = i; }
        std::stable_sort(sid.begin(), sid.end(), [&](int a, int b) { return key[a] < key[b]; });
        std::vector<double> sx(n), sy(n); std::vector<int32_t> bs(nbx * nby + 1, 0);
        for (int s = 0; s < n; ++s) { sx[s] = x[sid[s]]; sy[s] = y[sid[s]]; bs[key[sid[s]] + 1]++; }
        for (int b = 0; b < nbx * nby; ++b) bs[b + 1] += bs[b];
        BinGrid g{sx.data(), sy.data(), sid.data(), bs.data(), xmin, ymin, h, nbx, nby};
        int rings = (int)ceil(radius / h * (1.0 + 1e-9)); if (rings < 1) rings = 1;
        for (int q = 0; q < 300; ++q) {
            const int K = 1 + rand() % 20;
            double qx, qy; int t = rand() % n;
            if (q % 3 == 0) { qx = xmin - 50 + (w + 100) * (rand() / (double)RAND_MAX); qy = ymin - 50 + (hgt + 100) * (rand() / (double)RAND_MAX); }
            else { qx = sx[t]; qy = sy[t]; }
            std::vector<int> v_old, v_new; std::vector<double> b_old;
            old_ring(sx.data(), sy.data(), sid.data(), bs.data(), qx, qy, xmin, ymin, h, nbx, nby, K, v_old, b_old);
            std::vector<std::pair<double,int>> best;
            ring_walk(g, qx, qy, [&](int s) { v_new.push_back(s); best.push_back({BinGrid::dist2(qx, qy, g.sx[s], g.sy[s]), g.sid[s]}); std::sort(best.begin(), best.end()); if ((int)best.size() > K) best.pop_back(); },
                      [&] { return (int)best.size() < K ? DBL_MAX : best[K - 1].first; });
            if (v_old != v_new) { printf("RING MISMATCH trial %d q %d\n", trial, q); return 1; }
            // exactness against brute force
            std::vector<double> all(n); for (int s = 0; s < n; ++s) all[s] = BinGrid::dist2(qx, qy, sx[s], sy[s]);
            std::sort(all.begin(), all.end());
            for (int j = 0; j < K && j < n; ++j) if (all[j] != b_old[j]) { printf("NOT EXACT trial %d q %d\n", trial, q); return 1; }
            if (trial % 2 == 0) continue;   // the window needs bins no smaller than the radius
            qx = sx[t]; qy = sy[t];
            // the window written out as k_radius had it
            {
                std::vector<int> a, b;
                const double inv_h = 1.0 / h;
                const int bx = bin_coord(qx, xmin, inv_h, nbx), by = bin_coord(qy, ymin, inv_h, nby);
                const int ylo = by - rings < 0 ? 0 : by - rings, yhi = by + rings >= nby ? nby - 1 : by + rings;
                const int xlo = bx - rings < 0 ? 0 : bx - rings, xhi = bx + rings >= nbx ? nbx - 1 : bx + rings;
                for (int yy = ylo; yy <= yhi; ++yy) { const int s0 = bs[yy * nbx + xlo], s1 = bs[yy * nbx + xhi + 1]; for (int s = s0; s < s1; ++s) a.push_back(s); }
                window_walk<false>(g, qx, qy, rings, 0, [&](int s) { b.push_back(s); });
                if (a != b) { printf("WINDOW MISMATCH\n"); return 1; }
                // ... and as k_ripley_pairs had it: own row upwards, behind the own position
                a.clear(); b.clear();
                for (int yy = by; yy <= yhi; ++yy) { int s0 = bs[yy * nbx + xlo]; const int s1 = bs[yy * nbx + xhi + 1]; if (s0 <= t) s0 = (int)t + 1; for (int s = s0; s < s1; ++s) a.push_back(s); }
                window_walk<true>(g, qx, qy, rings, t, [&](int s) { b.push_back(s); });
                if (a != b) { printf("UPPER WINDOW MISMATCH\n"); return 1; }
                // and the closed ball is inside the window
                long inball = 0, seen = 0;
                for (int s = 0; s < n; ++s) inball += BinGrid::dist2(qx, qy, sx[s], sy[s]) <= radius * radius;
                window_walk<false>(g, qx, qy, rings, 0, [&](int s) { seen += BinGrid::dist2(qx, qy, g.sx[s], g.sy[s]) <= radius * radius; });
                if (inball != seen) { printf("BALL NOT COVERED\n"); return 1; }
            }
            ++checked;
        }
    }
    printf("walks ok: %ld window queries, every ring walk equal to the written-out loop\n", checked);
    return 0;
}
