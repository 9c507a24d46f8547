// sc_lane_group.h -- the lane-group walk over a run of stored entries of a sparse row or column chunk, shared by
// sc_nmf.hip (k_nmf_w, k_nmf_h), sc_annotate.hip (k_an_rows, k_an_gradcols) and sc_pca.hip (k_pca_rows); DESIGN.md 4.6l,
// 4.6n, 4.6o.  A group of w lanes (a power of two, groups aligned to w inside a wavefront) serves one run; every lane
// owns one slot of the gathered operand row (a component, or NB classes).
#pragma once

#include "sc_ctx.h"

namespace {

// the lanes of a group that serves `count` slots: the power of two >= count, at least `floor`, at most `cap`
inline int lanes_for(int count, int floor, int cap)
{
    int w = floor;
    while (w < count && w < cap) w <<= 1;
    return w;
}

// the adjacent-pair tree over the w lanes of a group: lane l takes lane l ^ 1, then l ^ 2, ...; every lane of the group
// ends with the same bits, since a + b = b + a
__device__ __forceinline__ double group_sum(double v, int w)
{
    for (int h = 1; h < w; h <<= 1) v = v + __shfl_xor(v, h, 64);
    return v;
}

// Walks the entries [p0, p1) of (idx, val) in index order; p0, p1 and w are uniform over the group, lane = its lane.
// The group fetches w entries at once (lane j holds entry base + j; lanes past the end hold id 0 and value 0.0) and hands
// them round with __shfl.  fetch(id) returns this lane's part of the operand row `id` (a double or a small struct);
// add(x, operand) accumulates one entry.  The order is fixed:
//  - four operand rows in flight: fetch of the entries j, j + 1, j + 2, j + 3, each from its shuffled id, then the four
//    adds in ascending j, each with its shuffled value;
//  - the tail of fewer than four entries: fetch, then add, per entry.
// So the entries are added one by one in index order whatever w is, and add may itself shuffle inside the group.
template <class Fetch, class Add>
__device__ __forceinline__ void lane_group_walk(const int32_t *__restrict__ idx, const double *__restrict__ val, int64_t p0,
                                                int64_t p1, int w, int lane, Fetch fetch, Add add)
{
    for (int64_t base = p0; base < p1; base += w) {
        const int cnt = (int)(p1 - base < w ? p1 - base : w);
        const int32_t id_mine = lane < cnt ? idx[base + lane] : 0;
        const double x_mine = lane < cnt ? val[base + lane] : 0.0;
        int j = 0;
        for (; j + 4 <= cnt; j += 4) {
            const auto r0 = fetch(__shfl(id_mine, j, w)), r1 = fetch(__shfl(id_mine, j + 1, w));
            const auto r2 = fetch(__shfl(id_mine, j + 2, w)), r3 = fetch(__shfl(id_mine, j + 3, w));
            add(__shfl(x_mine, j, w), r0);
            add(__shfl(x_mine, j + 1, w), r1);
            add(__shfl(x_mine, j + 2, w), r2);
            add(__shfl(x_mine, j + 3, w), r3);
        }
        for (; j < cnt; ++j) {
            const auto r = fetch(__shfl(id_mine, j, w));
            add(__shfl(x_mine, j, w), r);
        }
    }
}

// The same walk over a pattern, entries without values (sc_hops.hip's k_hop_aggregate): add(operand) per entry, in the
// same fixed order.
template <class Fetch, class Add>
__device__ __forceinline__ void lane_group_walk_pattern(const int32_t *__restrict__ idx, int64_t p0, int64_t p1, int w, int lane,
                                                        Fetch fetch, Add add)
{
    for (int64_t base = p0; base < p1; base += w) {
        const int cnt = (int)(p1 - base < w ? p1 - base : w);
        const int32_t id_mine = lane < cnt ? idx[base + lane] : 0;
        int j = 0;
        for (; j + 4 <= cnt; j += 4) {
            const auto r0 = fetch(__shfl(id_mine, j, w)), r1 = fetch(__shfl(id_mine, j + 1, w));
            const auto r2 = fetch(__shfl(id_mine, j + 2, w)), r3 = fetch(__shfl(id_mine, j + 3, w));
            add(r0);
            add(r1);
            add(r2);
            add(r3);
        }
        for (; j < cnt; ++j) add(fetch(__shfl(id_mine, j, w)));
    }
}

}  // namespace
