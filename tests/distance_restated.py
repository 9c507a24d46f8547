"""The distance and radius kernels restated, independently of the device code (test infrastructure; numpy only).

Every distance is ``sqrt(fl(fl(dx dx) + fl(dy dy)))`` (include/spatialcore_hip.h, N3; numpy rounds ``dx * dx``,
``dy * dy`` and their sum separately: there is no fused multiply-add in an elementwise expression of temporaries), and
every choice among equal distances goes to the lowest index.  So indices, distances, minima and neighbour lists of the
device are compared bit for bit; only a sum of distances depends on the order of its additions, and for that
``pair_table_brute`` returns the exact sum and the length of the device's longest chain of additions.

* ``nearest_brute``: nearest target of every query, optionally skipping the targets of one group per query.
* ``pair_table_brute``: exact sum and minimum of every (source group, target group) block.
* ``radius_brute``: the closed-ball radius graph, from ``ripley_restated.pair_list``.
* ``profile_brute``: neighbour counts by label.
* ``ScipyGeometry``: the three geometry calls of ``spatialcore_amd._lib.Context`` on top of the functions above, for
  the tests that run ``calculate_domain_distances`` without a device.
The input builders at the end are shared by tests/test_cpu_distance_restated.py, which pins the restatement against
scipy before the GPU is asked anything, and tests/test_gpu_distance.py.
"""
import math

import numpy as np

from ripley_restated import pair_list

CHUNK = 256        # source points per workgroup of k_pairwise / k_pair_table
TREE_LEVELS = 8    # the LDS tree over a workgroup's 256 partial sums


def dist2_matrix(a, b):
    """(len(a), len(b)) squared distances, products and sum rounded separately."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 2)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 2)
    dx = a[:, 0, None] - b[None, :, 0]
    dy = a[:, 1, None] - b[None, :, 1]
    d2 = dx * dx
    d2 += dy * dy
    return d2


def dist_matrix(a, b):
    return np.sqrt(dist2_matrix(a, b))


def nearest_brute(targets, queries, target_code=None, excluded=None, block=512):
    """(dist float64, idx int32): the nearest target of every query, the lowest index among equally near ones.  With
    codes, targets whose code equals the query's excluded code do not count; where none is left idx is -1 and dist
    +inf."""
    targets = np.asarray(targets, dtype=np.float64).reshape(-1, 2)
    queries = np.asarray(queries, dtype=np.float64).reshape(-1, 2)
    n_q = queries.shape[0]
    dist = np.empty(n_q, dtype=np.float64)
    idx = np.empty(n_q, dtype=np.int32)
    if target_code is not None:
        target_code = np.asarray(target_code)
        excluded = np.asarray(excluded)
    for q0 in range(0, n_q, block):
        q1 = min(q0 + block, n_q)
        d2 = dist2_matrix(queries[q0:q1], targets)
        if target_code is not None:
            d2[excluded[q0:q1, None] == target_code[None, :]] = np.inf
        i = d2.argmin(axis=1)                      # the first minimum: the lowest index
        best = d2[np.arange(q1 - q0), i]
        none = np.isinf(best)
        dist[q0:q1] = np.sqrt(best)
        idx[q0:q1] = np.where(none, -1, i)
    return dist, idx


def pair_depth(a_sizes, b_sizes):
    """depth[s, t] = |B_t| + 8 + ceil(|A_s| / 256): the longest chain of additions behind one sum of the device -- a
    thread's sequential pass over the target group, the 8-level LDS tree, the host's pass over the group's chunks."""
    a_sizes = np.asarray(a_sizes, dtype=np.int64)
    b_sizes = np.asarray(b_sizes, dtype=np.int64)
    return b_sizes[None, :] + TREE_LEVELS + -(-a_sizes[:, None] // CHUNK)


def pair_table_brute(a, a_off, b, b_off):
    """(exact_sum, min, depth), each (groups of a, groups of b): ``math.fsum`` of the block's distances (the correctly
    rounded sum), their minimum, and ``pair_depth``.  An empty block has sum 0 and min +inf."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 2)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 2)
    a_off, b_off = np.asarray(a_off, dtype=np.int64), np.asarray(b_off, dtype=np.int64)
    S, T = a_off.size - 1, b_off.size - 1
    tot, mn = np.zeros((S, T)), np.full((S, T), np.inf)
    for s in range(S):
        for t in range(T):
            blk = dist_matrix(a[a_off[s]:a_off[s + 1]], b[b_off[t]:b_off[t + 1]])
            if blk.size:
                tot[s, t] = math.fsum(blk.ravel().tolist())
                mn[s, t] = blk.min()
    return tot, mn, pair_depth(np.diff(a_off), np.diff(b_off))


def sum_bound(depth, exact_sum):
    """|device sum - exact sum| allowed: the terms are the same bits on both sides and non-negative, so a chain of
    ``depth`` additions is off by at most depth * u * sum (u = 2^-53) to first order; doubled for the second-order
    terms and fsum's own rounding."""
    return depth * 2.0 ** -52 * exact_sum


def radius_brute(coords, r):
    """(indptr int64, indices int32) of the closed-ball graph fl(d^2) <= fl(r^2), self removed by index, rows
    ascending (``pair_list``'s ``nonzero`` order is row-major with ascending columns)."""
    n = np.asarray(coords).reshape(-1, 2).shape[0]
    rows, cols, _ = pair_list(coords, [r])
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    return indptr, cols.astype(np.int32)


def profile_brute(indptr, indices, codes, T):
    """(n, T) float32: neighbours of every label in every row of the CSR pattern."""
    indptr = np.asarray(indptr, dtype=np.int64)
    codes = np.asarray(codes, dtype=np.int64)
    n = indptr.size - 1
    out = np.zeros((n, T), dtype=np.float32)
    np.add.at(out, (np.repeat(np.arange(n), np.diff(indptr)), codes[np.asarray(indices, dtype=np.int64)]), 1)
    return out


class ScipyGeometry:
    """Test double for the three geometry calls of spatialcore_amd._lib.Context (the name is historical: its ties follow
    the header's rule, lowest index, which cKDTree does not promise)."""

    def nearest(self, targets, queries):
        return nearest_brute(targets, queries)

    def nearest_excluding(self, targets, target_code, queries, query_excluded_code):
        return nearest_brute(targets, queries, target_code, query_excluded_code)

    def pair_table(self, a, a_off, b, b_off):
        tot, mn, _ = pair_table_brute(a, a_off, b, b_off)
        return tot, mn


# ---- inputs shared by the CPU pin and the device tests -----------------------------------------------------------------

def tie_free_case():
    """The draws of test_gpu_kernels.py::test_nearest_and_pairwise_vs_scipy: (targets, queries, a, b)."""
    rng = np.random.default_rng(12)
    targets = rng.normal([300, 300], 40, (5000, 2))
    queries = np.concatenate([rng.uniform(0, 1000, (3000, 2)), rng.normal([300, 300], 40, (500, 2)),
                              [[-5e4, 7e4], [300.0, 300.0]]])
    a, b = rng.uniform(0, 100, (1300, 2)), rng.uniform(50, 400, (2111, 2))
    return targets, queries, a, b


def lattice(m, seed=None):
    """The m x m integer lattice, as float64; shuffled when a seed is given."""
    g = np.stack(np.meshgrid(np.arange(float(m)), np.arange(float(m))), -1).reshape(-1, 2)
    if seed is not None:
        g = g[np.random.default_rng(seed).permutation(len(g))]
    return np.ascontiguousarray(g)


def lattice_tie_case(m=40, seed=3):
    """(targets, queries): a shuffled lattice and queries with 4, 2 and 1 nearest targets (cell centres, edge
    midpoints, the lattice points themselves)."""
    g = lattice(m, seed)
    return g, np.concatenate([g + [0.5, 0.5], g + [0.5, 0.0], g])


LATTICE_RADII = (1.0, math.sqrt(2.0), 2.0, math.sqrt(5.0), 3.0, 5.0)       # each one a distance of the integer lattice
SCALED_LATTICE_RADII = (0.1, 0.1 * math.sqrt(2.0), 0.2, 0.3, 0.5)           # the same on the lattice times 0.1

DEGREE_STEPS = (30, 31, 32, 33, 34, 35, 64, 1, 0)


def degree_step_case(seed=21):
    """(coords, radius, degree per point): clusters of m + 1 points within +-0.3 of centres 100 apart, indices
    shuffled; at radius 1 every point of a cluster has degree exactly m -- both sides of the switch at 32 / 33 between
    rows kept sorted by insertion and rows heap-sorted at the end."""
    rng = np.random.default_rng(seed)
    pts, deg = [], []
    for c, m in enumerate(DEGREE_STEPS):
        pts.append([100.0 * c, 50.0] + rng.uniform(-0.3, 0.3, (m + 1, 2)))
        deg += [m] * (m + 1)
    order = rng.permutation(len(deg))
    return np.concatenate(pts)[order], 1.0, np.asarray(deg)[order]


def sparse_pairs_case(seed=22):
    """(coords, radius): 3000 uniform points on [0, 1000]^2 and 300 partners planted at (0.005, 0), (0, r) and
    (1.0001 r, 0) from the first 300, r = 0.01: extent / r = 1e5, most rows empty."""
    rng = np.random.default_rng(seed)
    r = 0.01
    base = rng.uniform(0, 1000, (3000, 2))
    off = np.array([[0.005, 0.0], [0.0, r], [1.0001 * r, 0.0]])
    pts = np.concatenate([base, base[:300] + off[np.arange(300) % 3]])
    return pts[rng.permutation(len(pts))], r
