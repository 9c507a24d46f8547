"""GPU (run with -m gpu on an MI355X): the geometry kernels behind calculate_domain_distances,
compute_neighborhood_profile and the radius graphs against tests/distance_restated.py, at the shapes where their code
takes another path -- more than one chunk of 256 source points, more than one LDS tile of 1024 targets, ragged last
chunks and tiles, empty groups, exact ties, duplicates, degenerate and capped bin grids, far-away coordinates, the
degree at which a radius row changes its sort.

Indices, integer results, distances and minima are compared bit for bit: every distance is
sqrt(fl(fl(dx dx) + fl(dy dy))) on both sides and every tie goes to the lowest index.  Only the order of additions is
free, so only sums get a tolerance, and it is derived, not measured: ``distance_restated.sum_bound``."""
import math

import numpy as np
import pandas as pd
import pytest
from scipy.spatial import cKDTree

import distance_restated as dr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    # the process-wide context, as in test_gpu_kernels.py: a second live context's streams would share hardware queues
    from spatialcore_amd import _lib

    return _lib.default_context(0)


def assert_nearest(got, targets, queries, target_code=None, excluded=None):
    dist, idx = got
    want_d, want_i = dr.nearest_brute(targets, queries, target_code, excluded)
    np.testing.assert_array_equal(idx, want_i)
    np.testing.assert_array_equal(dist, want_d)
    assert idx.dtype == np.int32 and dist.dtype == np.float64


def assert_radius(ctx, coords, r):
    indptr, indices = ctx.radius_graph(coords, r)
    want_p, want_i = dr.radius_brute(coords, r)
    np.testing.assert_array_equal(indptr, want_p)
    np.testing.assert_array_equal(indices, want_i)
    return indptr, indices


# ---- nearest target ----------------------------------------------------------------------------------------------------

def test_nearest_takes_the_lowest_index_on_ties(ctx):
    """N1: 4, 2 and 1 equally near lattice targets; cKDTree returns another of them for hundreds of these queries
    (test_cpu_distance_restated.py), so only the restatement can pin the header's rule."""
    targets, queries = dr.lattice_tie_case()
    assert_nearest(ctx.nearest(targets, queries), targets, queries)


def test_nearest_duplicate_targets(ctx):
    """N2: every target three times; a query on a target finds distance 0 at the lowest of its three indices."""
    rng = np.random.default_rng(31)
    base = rng.uniform(0, 500, (1000, 2))
    order = rng.permutation(3000)
    targets = np.repeat(base, 3, axis=0)[order]
    dist, idx = ctx.nearest(targets, targets)
    first = np.full(1000, 3000)
    np.minimum.at(first, np.repeat(np.arange(1000), 3)[order], np.arange(3000))
    np.testing.assert_array_equal(idx, first[np.repeat(np.arange(1000), 3)[order]])
    np.testing.assert_array_equal(dist, np.zeros(3000))
    assert_nearest((dist, idx), targets, targets)


def test_nearest_queries_outside_the_grid(ctx):
    """N3: strongly non-uniform targets and an isolated one (the layout of test_knn_include_self_and_clustered);
    queries far outside the grid, a hair outside its box, on its corners and all over three times its extent."""
    rng = np.random.default_rng(5)
    targets = np.concatenate([rng.normal(0, 1, (3000, 2)), rng.normal(50, 0.01, (500, 2)), [[1e4, -1e4]]])
    lo, hi = targets.min(axis=0), targets.max(axis=0)
    mid, size = (lo + hi) / 2, hi - lo
    ang = np.arange(64) * (2 * np.pi / 64)
    ring = mid + 1e6 * np.stack([np.cos(ang), np.sin(ang)], 1)
    eps = 1e-9
    xs, ys = (lo[0] - eps, mid[0], hi[0] + eps), (lo[1] - eps, mid[1], hi[1] + eps)
    outside = np.array([[x, y] for x in xs for y in ys if (x, y) != (mid[0], mid[1])])
    corners = np.array([[lo[0], lo[1]], [lo[0], hi[1]], [hi[0], lo[1]], [hi[0], hi[1]]])
    assert outside.shape == (8, 2) and ((outside < lo) | (outside > hi)).any(axis=1).all()
    queries = np.concatenate([ring, outside, corners, mid + rng.uniform(-1.5, 1.5, (2000, 2)) * size])
    assert_nearest(ctx.nearest(targets, queries), targets, queries)


@pytest.mark.parametrize("n_q", [1, 255, 256, 257])
def test_nearest_degenerate_grids(ctx, n_q):
    """N4: grids of one bin, one row and one column of bins (the row long enough for the 4096-bin cap), at query counts
    around one workgroup."""
    rng = np.random.default_rng(40 + n_q)
    queries = rng.uniform(-50, 150, (n_q, 2))
    one = np.array([[3.0, -7.0]])
    same = np.tile([[12.5, 40.25]], (500, 1))
    hline = np.stack([rng.uniform(0, 1e6, 500), np.full(500, 20.0)], 1)     # extent / bin size > 4096
    vline = np.stack([np.full(500, 20.0), rng.uniform(0, 100, 500)], 1)
    for targets, q in ((one, queries), (same, queries), (vline, queries), (hline, queries * [5e3, 1.0])):
        assert_nearest(ctx.nearest(targets, q), targets, q)
    assert (ctx.nearest(same, queries)[1] == 0).all()


def _offset_case():
    rng = np.random.default_rng(50)
    shift = np.array([1e7, -3e6])
    return rng.uniform(0, 3000, (4000, 2)) + shift, rng.uniform(-200, 3200, (2000, 2)) + shift


def test_nearest_large_offset(ctx):
    """N5: coordinates far from the origin (12 of the 53 bits go to the offset); tie-free, so cKDTree agrees too."""
    targets, queries = _offset_case()
    got = ctx.nearest(targets, queries)
    assert_nearest(got, targets, queries)
    wd, wi = cKDTree(targets).query(queries, k=1)
    np.testing.assert_array_equal(got[1], wi)
    np.testing.assert_array_equal(got[0], wd)


# ---- nearest target outside the query's own group ----------------------------------------------------------------------

def test_nearest_excluding_mixed_codes(ctx):
    """E1: 7 interleaved codes, every query excludes one of them or none (-1, what distance.py passes for a cell that
    has no own domain): those answers are ctx.nearest's."""
    rng = np.random.default_rng(60)
    targets, queries = rng.uniform(0, 1000, (5000, 2)), rng.uniform(-50, 1050, (3000, 2))
    code = rng.integers(0, 7, 5000).astype(np.int32)
    excluded = rng.integers(-1, 7, 3000).astype(np.int32)
    dist, idx = ctx.nearest_excluding(targets, code, queries, excluded)
    assert_nearest((dist, idx), targets, queries, code, excluded)
    assert (code[idx] != excluded).all()
    free = excluded == -1
    assert free.sum() > 200
    plain_d, plain_i = ctx.nearest(targets, queries)
    np.testing.assert_array_equal(idx[free], plain_i[free])
    np.testing.assert_array_equal(dist[free], plain_d[free])
    none_d, none_i = ctx.nearest_excluding(targets, code, queries, np.full(3000, -1, dtype=np.int32))
    np.testing.assert_array_equal(none_i, plain_i)
    np.testing.assert_array_equal(none_d, plain_d)


def test_nearest_excluding_walks_on_past_excluded_rings(ctx):
    """E2: everything near the queries is excluded, the eligible targets lie on a circle many rings of bins away: the
    walk must go on while its best is still DBL_MAX."""
    rng = np.random.default_rng(61)
    ang = rng.uniform(0, 2 * np.pi, 40)
    targets = np.concatenate([rng.normal(0, 5, (3000, 2)), 2000 * np.stack([np.cos(ang), np.sin(ang)], 1)])
    code = np.concatenate([np.zeros(3000, np.int32), np.ones(40, np.int32)])
    order = rng.permutation(3040)
    targets, code = targets[order], code[order]
    queries = rng.normal(0, 5, (300, 2))
    dist, idx = ctx.nearest_excluding(targets, code, queries, np.zeros(300, np.int32))
    assert_nearest((dist, idx), targets, queries, code, np.zeros(300, np.int32))
    assert (code[idx] == 1).all() and (dist > 1900).all()


def test_nearest_excluding_ties_between_excluded_and_eligible(ctx):
    """E3: an excluded target as near as an eligible one of higher index; two eligible ones as near as each other."""
    targets = np.array([[-1.0, 0.0], [1.0, 0.0], [10.0, 1.0], [10.0, -1.0]])
    code = np.array([0, 1, 1, 1], dtype=np.int32)
    queries = np.array([[0.0, 0.0], [0.0, 0.0], [10.0, 0.0]])
    dist, idx = ctx.nearest_excluding(targets, code, queries, np.array([0, -1, 0], dtype=np.int32))
    np.testing.assert_array_equal(idx, [1, 0, 2])
    np.testing.assert_array_equal(dist, [1.0, 1.0, 1.0])
    # the same on a grid with many bins: a checkerboard of codes under the 4- and 2-fold ties of the lattice
    targets, queries = dr.lattice_tie_case(30, seed=7)
    code = ((targets[:, 0] + targets[:, 1]) % 2).astype(np.int32)
    for excluded in (np.zeros(len(queries), np.int32), np.ones(len(queries), np.int32),
                     code[dr.nearest_brute(targets, queries)[1]]):       # the code of the unrestricted winner
        assert_nearest(ctx.nearest_excluding(targets, code, queries, excluded), targets, queries, code, excluded)


def test_nearest_excluding_nothing_left(ctx):
    """E4: every target excluded: -1 and +inf; one query of the same call that excludes another code is answered."""
    rng = np.random.default_rng(63)
    targets, queries = rng.uniform(0, 100, (700, 2)), rng.uniform(-20, 120, (300, 2))
    code = np.full(700, 3, dtype=np.int32)
    dist, idx = ctx.nearest_excluding(targets, code, queries, np.full(300, 3, dtype=np.int32))
    np.testing.assert_array_equal(idx, np.full(300, -1))
    assert np.isposinf(dist).all()
    excluded = np.full(300, 3, dtype=np.int32)
    excluded[123] = 4
    dist, idx = ctx.nearest_excluding(targets, code, queries, excluded)
    assert_nearest((dist, idx), targets, queries, code, excluded)
    assert idx[123] >= 0 and (np.delete(idx, 123) == -1).all()


def test_nearest_argument_errors(ctx):
    """E5."""
    rng = np.random.default_rng(64)
    targets, queries = rng.uniform(0, 1, (10, 2)), rng.uniform(0, 1, (4, 2))
    code, excluded = np.zeros(10, np.int32), np.zeros(4, np.int32)
    with pytest.raises(ValueError, match="one group code per target and per query"):
        ctx.nearest_excluding(targets, code[:9], queries, excluded)
    with pytest.raises(ValueError, match="one group code per target and per query"):
        ctx.nearest_excluding(targets, code, queries, np.zeros(5, np.int32))
    with pytest.raises(ValueError, match="sc_nearest_excluding_2d: "):
        ctx.nearest_excluding(targets, code, np.zeros((0, 2)), np.zeros(0, np.int32))
    with pytest.raises(ValueError, match="sc_nearest_2d: "):
        ctx.nearest(targets, np.zeros((0, 2)))
    bad = queries.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="query coordinate 2 is not finite"):
        ctx.nearest_excluding(targets, code, bad, excluded)
    with pytest.raises(ValueError, match="query coordinate 2 is not finite"):
        ctx.nearest(targets, bad)
    bad = targets.copy()
    bad[7, 0] = np.inf
    with pytest.raises(ValueError, match="coordinate 7 is not finite"):
        ctx.nearest(bad, queries)
    assert_nearest(ctx.nearest(targets, queries), targets, queries)      # the context is none the worse for it


# ---- all-pairs sums and minima -----------------------------------------------------------------------------------------

A_SIZES = [0, 1, 255, 256, 257, 0, 513, 700, 0]
B_SIZES = [0, 1023, 1024, 1025, 1, 0, 2049, 3, 0]


@pytest.fixture(scope="module")
def p1():
    """The chunk- and tile-edge groups and their brute-force table, computed once."""
    rng = np.random.default_rng(70)
    a = np.concatenate([rng.uniform(0, 100, (m, 2)) + [30.0 * s, 10.0 * s] for s, m in enumerate(A_SIZES)])
    b = np.concatenate([rng.uniform(0, 150, (m, 2)) + [50.0 + 20.0 * t, 40.0] for t, m in enumerate(B_SIZES)])
    a_off, b_off = np.concatenate([[0], np.cumsum(A_SIZES)]), np.concatenate([[0], np.cumsum(B_SIZES)])
    return a, a_off, b, b_off, dr.pair_table_brute(a, a_off, b, b_off)


def assert_sums(got, exact, depth):
    err, bound = np.abs(got - exact), dr.sum_bound(depth, exact)
    print("sum error / bound, worst block:", np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)))
    assert (err <= bound).all(), (err, bound)


def test_pair_table_chunk_and_tile_edges(ctx, p1):
    """P1: source groups of 1, 255, 256, 257, 513 and 700 points (1 to 3 chunks, the last one ragged or full), target
    groups of 1, 3, 1023, 1024, 1025 and 2049 (1 to 3 tiles), empty groups first, inside and last.

    Minima are exact.  |sum - exact| <= depth 2^-52 exact with depth = |B_t| + 8 + ceil(|A_s| / 256), the device's
    longest chain of additions (distance_restated.sum_bound): the terms are the same bits on both sides and
    non-negative, only their order differs.  CPU-side evidence that the device's order sits inside it: a numpy run of
    that order (each thread's pass over the tiles, the 8-level tree, the chunks in turn) over these very points stayed
    at 0.17 of depth 2^-53 exact in its worst block, a twelfth of the bound."""
    a, a_off, b, b_off, (exact, mn, depth) = p1
    tot, got_mn = ctx.pair_table(a, a_off, b, b_off)
    np.testing.assert_array_equal(got_mn, mn)
    assert_sums(tot, exact, depth)
    empty = np.outer(A_SIZES, B_SIZES) == 0
    assert empty.sum() == 45 and (tot[empty] == 0.0).all() and np.isposinf(got_mn[empty]).all()
    assert (tot[~empty] > 0).all() and np.isfinite(got_mn[~empty]).all()


def assert_pairwise(ctx, a, b):
    exact, mn, depth = (v[0, 0] for v in dr.pair_table_brute(a, [0, len(a)], b, [0, len(b)]))
    mean, got_mn = ctx.pairwise(a, b)
    assert got_mn == mn
    pairs = float(len(a)) * float(len(b))
    assert abs(mean - exact / pairs) <= dr.sum_bound(depth + 1, exact) / pairs      # (+1: the division)
    return mean, got_mn


def test_pairwise_agrees_with_the_pair_table_and_at_its_own_edges(ctx, p1):
    """P2: sc_pairwise_2d on three blocks of P1, then at one point, one full chunk / tile and one more."""
    a, a_off, b, b_off, (exact, mn, depth) = p1
    for s, t in ((4, 3), (7, 6), (1, 4)):
        A, B = a[a_off[s]:a_off[s + 1]], b[b_off[t]:b_off[t + 1]]
        _, got_mn = assert_pairwise(ctx, A, B)
        assert got_mn == mn[s, t]
    rng = np.random.default_rng(71)
    A, B = rng.uniform(0, 100, (257, 2)), rng.uniform(20, 300, (1025, 2))
    for n_a in (1, 256, 257):
        for n_b in (1, 1024, 1025):
            assert_pairwise(ctx, A[:n_a], B[:n_b])


def test_pair_table_zero_minimum(ctx):
    """P3: a point that is in a source and in a target group; a group of coincident points against itself."""
    rng = np.random.default_rng(72)
    a, b = rng.uniform(0, 100, (300, 2)), rng.uniform(0, 100, (1100, 2))
    b[1077] = a[290]
    a_off, b_off = [0, 260, 300], [0, 40, 1100]
    tot, mn = ctx.pair_table(a, a_off, b, b_off)
    exact, want_mn, depth = dr.pair_table_brute(a, a_off, b, b_off)
    np.testing.assert_array_equal(mn, want_mn)
    assert mn[1, 1] == 0.0 and (np.delete(mn.ravel(), 3) > 0).all()
    assert_sums(tot, exact, depth)
    same = np.tile([[1e3 / 3, -7.7]], (300, 1))
    tot, mn = ctx.pair_table(same, [0, 300], same, [0, 300])
    assert tot[0, 0] == 0.0 and mn[0, 0] == 0.0
    assert ctx.pairwise(same, same) == (0.0, 0.0)


def test_pair_table_is_reproducible(ctx, p1):
    """P4: the chunks of a group are reduced in ascending order on the host: the same bits every time."""
    a, a_off, b, b_off, _ = p1
    first, second = ctx.pair_table(a, a_off, b, b_off), ctx.pair_table(a, a_off, b, b_off)
    np.testing.assert_array_equal(first[0], second[0])
    np.testing.assert_array_equal(first[1], second[1])


def test_pair_table_and_pairwise_argument_errors(ctx):
    """P5."""
    rng = np.random.default_rng(73)
    a, b = rng.uniform(0, 1, (6, 2)), rng.uniform(0, 1, (9, 2))
    with pytest.raises(ValueError, match="offsets must start at 0"):
        ctx.pair_table(a, [1, 6], b, [0, 9])
    with pytest.raises(ValueError, match="offsets must start at 0"):
        ctx.pair_table(a, [0, 6], b, [2, 5, 9])
    with pytest.raises(ValueError, match="source offsets not monotone"):
        ctx.pair_table(a, [0, 4, 3, 6], b, [0, 9])
    with pytest.raises(ValueError, match="target offsets not monotone"):
        ctx.pair_table(a, [0, 6], b, [0, 9, 8, 9])
    with pytest.raises(ValueError, match="do not cover"):
        ctx.pair_table(a, [0, 5], b, [0, 9])
    with pytest.raises(ValueError, match="do not cover"):
        ctx.pair_table(a, [0, 6], b, [0, 10])
    with pytest.raises(ValueError, match="sc_pair_table_2d: "):
        ctx.pair_table(a, [0, 6], np.zeros((0, 2)), [0, 0, 0])            # every target group empty
    with pytest.raises(ValueError, match="sc_pair_table_2d: "):
        ctx.pair_table(np.zeros((0, 2)), [0, 0], b, [0, 9])
    with pytest.raises(ValueError, match="group counts out of range"):
        ctx.pair_table(a, [0, 6], b, np.concatenate([np.zeros(65536, np.int64), [9]]))     # 65 536 target groups
    tot, mn = ctx.pair_table(a, [0, 6], b, np.concatenate([np.zeros(65535, np.int64), [9]]))   # 65 535 are served
    assert tot.shape == (1, 65535) and (tot[0, :-1] == 0).all() and tot[0, -1] > 0 and np.isposinf(mn[0, :-1]).all()
    # a non-finite coordinate would give a NaN sum beside a finite minimum: refused, with its index
    for value in (np.nan, np.inf, -np.inf):
        bad_a, bad_b = a.copy(), b.copy()
        bad_a[4, 1], bad_b[8, 0] = value, value
        with pytest.raises(ValueError, match="sc_pair_table_2d: source coordinate 4 is not finite"):
            ctx.pair_table(bad_a, [0, 6], b, [0, 9])
        with pytest.raises(ValueError, match="sc_pair_table_2d: target coordinate 8 is not finite"):
            ctx.pair_table(a, [0, 6], bad_b, [0, 9])
        with pytest.raises(ValueError, match="sc_pairwise_2d: a coordinate 4 is not finite"):
            ctx.pairwise(bad_a, b)
        with pytest.raises(ValueError, match="sc_pairwise_2d: b coordinate 8 is not finite"):
            ctx.pairwise(a, bad_b)
    with pytest.raises(ValueError, match="sc_pairwise_2d: "):
        ctx.pairwise(a, np.zeros((0, 2)))
    assert_pairwise(ctx, a, b)


# ---- radius graph ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale,radii", [(1.0, dr.LATTICE_RADII), (0.1, dr.SCALED_LATTICE_RADII)])
def test_radius_graph_closed_ball_ties(ctx, scale, radii):
    """R1: every radius is a distance of the lattice, so whole shells of neighbours sit on fl(d^2) <= fl(r^2)."""
    g = dr.lattice(40, seed=80) * scale
    for r in radii:
        indptr, _ = assert_radius(ctx, g, r)
        assert indptr[-1] > 0


def test_radius_graph_duplicates(ctx):
    """R2: duplicates are neighbours of each other at any radius; self is removed by index only."""
    rng = np.random.default_rng(81)
    pts = np.repeat(rng.uniform(0, 300, (800, 2)), 3, axis=0)[rng.permutation(2400)]
    indptr, _ = assert_radius(ctx, pts, 1e-9)
    assert (np.diff(indptr) == 2).all()
    indptr, _ = assert_radius(ctx, pts, 20.0)
    assert 2 <= np.diff(indptr).min() <= 32 < np.diff(indptr).max()


def test_radius_graph_degree_steps(ctx):
    """R3: rows of degree 30 .. 35 and 64, 1, 0: both sides of the switch between insertion and heap sort."""
    coords, r, degree = dr.degree_step_case()
    indptr, _ = assert_radius(ctx, coords, r)
    np.testing.assert_array_equal(np.diff(indptr), degree)


def test_radius_graph_radius_far_below_the_bin_size(ctx):
    """R4: extent / r = 1e5 on a square, and 1e8 on a strip whose density-sized bins would outnumber the 4096-bin cap:
    in both most rows are empty and the result is not."""
    coords, r = dr.sparse_pairs_case()
    indptr, _ = assert_radius(ctx, coords, r)
    assert 100 <= indptr[-1] < 1000
    strip = coords * [1e3, 1e-3]
    strip[3000:] = strip[:300] + [0.005, 0.0]
    indptr, _ = assert_radius(ctx, strip, r)
    assert indptr[-1] >= 600


def test_radius_graph_radius_beyond_the_extent(ctx):
    """R5: one bin; every row holds all the other points, heap-sorted."""
    rng = np.random.default_rng(84)
    pts = rng.uniform(0, 10, (1500, 2))
    indptr, indices = assert_radius(ctx, pts, 20.0)
    np.testing.assert_array_equal(np.diff(indptr), np.full(1500, 1499))
    rows = indices.reshape(1500, 1499)
    assert (np.diff(rows, axis=1) > 0).all()


def test_radius_graph_smallest_shapes(ctx):
    """R6."""
    indptr, indices = ctx.radius_graph(np.array([[4.0, 2.0]]), 1.0)
    np.testing.assert_array_equal(indptr, [0, 0])
    assert indices.size == 0 and indptr.dtype == np.int64 and indices.dtype == np.int32
    two = np.array([[0.0, 0.0], [3.0, 4.0]])
    indptr, indices = assert_radius(ctx, two, 5.0)            # on the ball's edge: inside
    np.testing.assert_array_equal(indptr, [0, 1, 2])
    np.testing.assert_array_equal(indices, [1, 0])
    indptr, indices = assert_radius(ctx, two, math.nextafter(5.0, 0.0))
    np.testing.assert_array_equal(indptr, [0, 0, 0])
    rng = np.random.default_rng(85)
    t = rng.uniform(0, 100, 500)
    for line in (np.stack([t, np.full(500, 3.0)], 1), np.stack([np.full(500, -3.0), t], 1), np.stack([t, 2 * t + 1], 1)):
        indptr, _ = assert_radius(ctx, line, 1.5)
        assert indptr[-1] > 0


def test_radius_graph_large_offset(ctx):
    """R7."""
    targets, _ = _offset_case()
    indptr, _ = assert_radius(ctx, targets, 60.0)
    assert indptr[-1] > 4000


# ---- neighbourhood profile ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 300])
def test_profile_counts_narrow_and_wide(ctx, T):
    """F1: one type and 300 types, on a radius graph fed back as CSR and on the resident kNN graph."""
    rng = np.random.default_rng(90 + T)
    g = dr.lattice(40, seed=80)
    indptr, indices = ctx.radius_graph(g, 2.0)
    ctx.set_graph_csr(indptr, indices, np.ones(indices.size), len(g))
    pts = rng.uniform(0, 500, (3000, 2))
    for n, graph in ((len(g), (indptr, indices)), (3000, None)):
        if graph is None:
            ctx.knn(pts, 15, fetch=False)
            ctx.graph_from_knn(1.0)
            graph = ctx.get_graph()[:2]
            np.testing.assert_array_equal(np.diff(graph[0]), np.full(3000, 15))
        codes = rng.integers(0, T, n).astype(np.int32)
        got = ctx.profile_counts(codes, T)
        assert got.dtype == np.float32 and got.shape == (n, T)
        np.testing.assert_array_equal(got, dr.profile_brute(graph[0], graph[1], codes, T))
        np.testing.assert_array_equal(got.sum(axis=1, dtype=np.float64), np.diff(graph[0]))


def test_profile_counts_empty_rows_and_bad_labels(ctx):
    """F2: the error carries the exact number of empty rows."""
    coords, r, degree = dr.degree_step_case()
    indptr, indices = ctx.radius_graph(coords, r)
    n = len(coords)
    codes = (np.arange(n) % 4).astype(np.int32)
    ctx.set_graph_csr(indptr, indices, np.ones(indices.size), n)
    with pytest.raises(ValueError, match="^1 cells have empty neighborhood profiles"):
        ctx.profile_counts(codes, 4)
    # six more: the rows of the two points of degree 1 and of four of degree 30 are emptied
    keep = np.ones(indices.size, dtype=bool)
    for i in np.concatenate([np.flatnonzero(degree == 1), np.flatnonzero(degree == 30)[:4]]):
        keep[indptr[i]:indptr[i + 1]] = False
    rows = np.repeat(np.arange(n), np.diff(indptr))[keep]
    indptr7 = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
    assert (np.diff(indptr7) == 0).sum() == 7
    ctx.set_graph_csr(indptr7, indices[keep], np.ones(keep.sum()), n)
    with pytest.raises(ValueError, match="^7 cells have empty neighborhood profiles"):
        ctx.profile_counts(codes, 4)
    for bad in (4, -1):
        wrong = codes.copy()
        wrong[17] = bad
        with pytest.raises(ValueError, match=f"label {bad} of cell 17 out of range"):
            ctx.profile_counts(wrong, 4)


# ---- the public function at real sizes ---------------------------------------------------------------------------------

SOURCE_DOMAINS = {"S_small": 40, "S_mid": 300, "shared": 700, "S_big": 2600}
TARGET_DOMAINS = {"T_small": 90, "shared": 1100, "T_big": 2300}


@pytest.fixture(scope="module")
def slide():
    """12 000 cells; domains are the cells nearest to a centre (thousands of cells: several chunks and tiles per block),
    most cells belong to none, and the two columns share one name."""
    rng = np.random.default_rng(100)
    coords = rng.uniform(0, 3000, (12000, 2))
    columns = {}
    for col, domains in (("dom_a", SOURCE_DOMAINS), ("dom_b", TARGET_DOMAINS)):
        names = np.full(12000, None, dtype=object)
        for name, size in domains.items():
            d = np.linalg.norm(coords - rng.uniform(300, 2700, 2), axis=1)
            d[pd.notna(names)] = np.inf
            names[np.argsort(d, kind="stable")[:size]] = name
        columns[col] = names
    return coords, columns


def _run(slide, context, monkeypatch, **kw):
    from spatialcore_amd import SimpleAnnData, _lib
    from spatialcore_amd.spatial import calculate_domain_distances, get_distance_matrix

    coords, columns = slide
    obs = pd.DataFrame({k: v.copy() for k, v in columns.items()}, index=pd.RangeIndex(len(coords)).astype(str))
    ad = SimpleAnnData(np.zeros((len(coords), 1)), obs=obs, var_names=["g0"], obsm={"spatial": coords})
    with monkeypatch.context() as m:
        if context is not None:
            m.setattr(_lib, "default_context", lambda device=0: context)
        calculate_domain_distances(ad, output_mode="both", **kw)
    near = np.array([x if isinstance(x, str) else "" for x in ad.obs["nearest_target_domain"].values])
    return get_distance_matrix(ad), ad.obs["distance_to_target"].values.astype(float), near


@pytest.mark.parametrize("target_column", ["dom_b", "dom_a"])        # dom_a: the self case, own domains excluded
@pytest.mark.parametrize("metric", ["minimum", "mean", "centroid"])
def test_calculate_domain_distances_at_real_sizes(ctx, slide, monkeypatch, metric, target_column):
    """A1: the public function on the device against the same function on the stand-in.  Everything but the mean
    matrix is equal; a mean is within the pair table's bound (and the division's rounding) over the pair count."""
    kw = dict(source_domain_column="dom_a", target_domain_column=target_column, distance_metric=metric)
    m, dist, near = _run(slide, None, monkeypatch, **kw)
    want_m, want_dist, want_near = _run(slide, dr.ScipyGeometry(), monkeypatch, **kw)
    sizes = TARGET_DOMAINS if target_column == "dom_b" else SOURCE_DOMAINS
    rows, cols = list(m.index), list(m.columns)
    assert rows == list(want_m.index) and sorted(rows) == sorted(SOURCE_DOMAINS)
    assert cols == list(want_m.columns) and sorted(cols) == sorted(sizes)
    np.testing.assert_array_equal(dist, want_dist)
    np.testing.assert_array_equal(near, want_near)
    assert np.isfinite(dist).sum() == sum(SOURCE_DOMAINS.values()) and (near != "").sum() == sum(SOURCE_DOMAINS.values())
    got, want = m.values.astype(float), want_m.values.astype(float)
    assert np.isfinite(want).all()
    own = (np.asarray(rows)[:, None] == np.asarray(cols)[None, :]) & (target_column == "dom_a")
    if metric == "mean":
        depth = dr.pair_depth([SOURCE_DOMAINS[r] for r in rows], [sizes[c] for c in cols]) + 1
        assert (np.abs(got - want) <= dr.sum_bound(depth, want)).all(), (got, want)
        assert (want[~own] > 0).all()
    else:
        np.testing.assert_array_equal(got, want)
    if target_column == "dom_a":
        assert own.sum() == len(SOURCE_DOMAINS) and (got[own] == 0.0).all()
        if metric == "centroid":
            assert (near != np.asarray(slide[1]["dom_a"], dtype=object).astype(str))[near != ""].all()
