"""CPU-only: tests/distance_restated.py pinned against scipy, before tests/test_gpu_distance.py asks the GPU anything.

Where scipy decides the same question (tie-free nearest targets, cdist's distances, closed-ball neighbour lists) the
restatement must give scipy's bits.  Where it does not -- cKDTree promises nothing about which of several equally near
targets it returns -- the restatement is checked against the rule itself, and the test asserts that scipy's answer
differs, so that the input keeps telling the two apart."""
import math

import numpy as np
import pytest
from scipy.spatial import cKDTree
from scipy.spatial.distance import cdist

import distance_restated as dr


def test_nearest_brute_is_ckdtree_and_sqrt_d2_is_cdist_on_tie_free_input():
    targets, queries, a, b = dr.tie_free_case()
    dist, idx = dr.nearest_brute(targets, queries)
    wd, wi = cKDTree(targets).query(queries, k=1)
    np.testing.assert_array_equal(idx, wi)
    np.testing.assert_array_equal(dist, wd)
    assert idx.dtype == np.int32 and dist.dtype == np.float64
    np.testing.assert_array_equal(dr.dist_matrix(a, b), cdist(a, b))
    np.testing.assert_array_equal(dr.dist_matrix(queries[:700], targets), cdist(queries[:700], targets))


def test_nearest_brute_takes_the_lowest_index_on_ties_and_ckdtree_does_not():
    targets, queries = dr.lattice_tie_case()
    assert queries.shape == (4800, 2)
    dist, idx = dr.nearest_brute(targets, queries)
    wd, wi = cKDTree(targets).query(queries, k=1)
    np.testing.assert_array_equal(dist, wd)
    D = cdist(queries, targets)                                   # (bit-equal to dist_matrix: the test above)
    at_best = D == wd[:, None]
    ties = at_best.sum(axis=1)                                    # (queries beyond the last column or row see fewer)
    assert (ties[:1600] == 4).sum() == 39 * 39 and (ties[1600:3200] == 2).sum() == 39 * 40 and (ties[3200:] == 1).all()
    np.testing.assert_array_equal(idx, at_best.argmax(axis=1))    # the lowest index among the targets at that distance
    assert (wi != idx).sum() > 100, "cKDTree happens to follow the rule here: the input no longer discriminates"


def test_nearest_brute_exclusion_and_nothing_left():
    targets = np.array([[-1.0, 0.0], [1.0, 0.0], [10.0, 1.0], [10.0, -1.0]])
    code = np.array([0, 1, 1, 1])
    queries = np.array([[0.0, 0.0], [0.0, 0.0], [10.0, 0.0], [10.0, 0.0], [0.0, 0.0]])
    dist, idx = dr.nearest_brute(targets, queries, code, np.array([0, -1, 0, 1, 1]))
    np.testing.assert_array_equal(idx, [1, 0, 2, 0, 0])
    np.testing.assert_array_equal(dist, [1.0, 1.0, 1.0, math.sqrt(121.0), 1.0])
    dist, idx = dr.nearest_brute(targets[1:], queries, code[1:], np.full(5, 1))
    np.testing.assert_array_equal(idx, np.full(5, -1))
    assert np.isposinf(dist).all()


def _assert_radius_brute_is_the_oracle(oracle, coords, r):
    indptr, indices = dr.radius_brute(coords, r)
    wp, wi = oracle.radius_neighbors(coords, r)
    np.testing.assert_array_equal(indptr, wp)
    np.testing.assert_array_equal(indices, wi)
    assert indptr.dtype == np.int64 and indices.dtype == np.int32
    return indptr, indices


@pytest.mark.parametrize("scale,radii", [(1.0, dr.LATTICE_RADII), (0.1, dr.SCALED_LATTICE_RADII)])
def test_radius_brute_is_the_oracle_on_lattice_ties(oracle, scale, radii):
    g = dr.lattice(25, seed=4) * scale
    for r in radii:
        indptr, _ = _assert_radius_brute_is_the_oracle(oracle, g, r)
        assert indptr[-1] > 0


def test_radius_brute_is_the_oracle_at_the_degree_steps_and_on_sparse_pairs(oracle):
    coords, r, degree = dr.degree_step_case()
    indptr, _ = _assert_radius_brute_is_the_oracle(oracle, coords, r)
    np.testing.assert_array_equal(np.diff(indptr), degree)
    assert set(degree.tolist()) == {0, 1, 30, 31, 32, 33, 34, 35, 64}
    coords, r = dr.sparse_pairs_case()
    indptr, _ = _assert_radius_brute_is_the_oracle(oracle, coords, r)
    assert 100 <= indptr[-1] < 1000 and (np.diff(indptr) == 0).mean() > 0.8
    assert (coords.max(axis=0) - coords.min(axis=0)).max() / r > 4096      # more bins of that size than the grid's cap


def test_pair_table_brute_by_hand():
    a = np.array([[0.0, 0.0], [3.0, 4.0]])
    b = np.array([[0.0, 0.0], [6.0, 8.0], [0.0, 1.0]])
    tot, mn, depth = dr.pair_table_brute(a, [0, 2, 2], b, [0, 1, 3])      # the second source group is empty
    np.testing.assert_array_equal(tot, [[5.0, math.fsum([10.0, 1.0, 5.0, math.sqrt(18.0)])], [0.0, 0.0]])
    np.testing.assert_array_equal(mn, [[0.0, 1.0], [np.inf, np.inf]])
    np.testing.assert_array_equal(depth, [[1 + 8 + 1, 2 + 8 + 1], [1 + 8 + 0, 2 + 8 + 0]])
    np.testing.assert_array_equal(dr.pair_depth([256, 257, 700], [1024]), [[1024 + 8 + 1], [1024 + 8 + 2], [1024 + 8 + 3]])
    assert dr.sum_bound(10, 4.0) == 10 * 2.0 ** -52 * 4.0


def test_profile_brute_by_hand():
    # rows: {1, 2}, {}, {0, 0, 1} with codes 1, 0, 1
    got = dr.profile_brute([0, 2, 2, 5], [1, 2, 0, 0, 1], [1, 0, 1], 3)
    np.testing.assert_array_equal(got, np.array([[1, 1, 0], [0, 0, 0], [1, 2, 0]], dtype=np.float32))
    assert got.dtype == np.float32


def test_the_stand_in_answers_through_the_restatement():
    targets, queries = dr.lattice_tie_case(8, seed=1)
    geo = dr.ScipyGeometry()
    d, i = geo.nearest(targets, queries)
    np.testing.assert_array_equal(i, dr.nearest_brute(targets, queries)[1])
    code = np.arange(len(targets)) % 3
    d2, i2 = geo.nearest_excluding(targets, code, queries, np.full(len(queries), -1))
    np.testing.assert_array_equal(i2, i)
    np.testing.assert_array_equal(d2, d)
    tot, mn = geo.pair_table(targets, [0, 10, 64], queries, [0, 192])
    want = cdist(targets, queries)
    np.testing.assert_allclose(tot[:, 0], [want[:10].sum(), want[10:].sum()], rtol=1e-13)
    np.testing.assert_array_equal(mn[:, 0], [want[:10].min(), want[10:].min()])


def test_the_pairwise_entry_points_refuse_non_finite_coordinates_on_the_host():
    """A NaN distance is kept by a sum and skipped by a minimum, so sc_pairwise_2d and sc_pair_table_2d refuse the
    coordinate, like every other entry point that reads coordinates -- on the host, before the context is looked at:
    the zeroed block that stands for it here is never read, and no device is needed to see the refusal."""
    import os

    from spatialcore_amd import _lib

    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "spatialcore_hip.h")).read()
    assert "sc_pairwise_2d and sc_pair_table_2d refuse a non-finite one" in header
    lib = _lib.load_library()
    a, b = np.arange(12.0).reshape(6, 2), np.arange(18.0).reshape(9, 2) + 0.5
    a_off, b_off = np.array([0, 2, 6], dtype=np.int64), np.array([0, 9], dtype=np.int64)
    tot, mn = np.zeros((2, 1)), np.zeros((2, 1))
    mean, least = _lib.c_double(0), _lib.c_double(0)
    p = _lib._ptr
    assert lib.sc_pair_table_2d(None, p(a), p(a_off), 2, p(b), p(b_off), 1, p(tot), p(mn)) == _lib.SC_ERR_INVALID
    assert b"sc_pair_table_2d: null pointer" in lib.sc_last_error()
    assert lib.sc_pairwise_2d(None, p(a), 6, p(b), 9, _lib.byref(mean), _lib.byref(least)) == _lib.SC_ERR_INVALID
    assert b"sc_pairwise_2d: null pointer" in lib.sc_last_error()
    no_ctx = np.zeros(1 << 17, dtype=np.int64)
    for value in (np.nan, np.inf, -np.inf):
        bad_a, bad_b = a.copy(), b.copy()
        bad_a[4, 1], bad_b[8, 0] = value, value
        for args, message in (((p(bad_a), p(a_off), 2, p(b), p(b_off), 1), b"sc_pair_table_2d: source coordinate 4 is not finite"),
                              ((p(a), p(a_off), 2, p(bad_b), p(b_off), 1), b"sc_pair_table_2d: target coordinate 8 is not finite")):
            assert lib.sc_pair_table_2d(p(no_ctx), *args, p(tot), p(mn)) == _lib.SC_ERR_INVALID
            assert lib.sc_last_error() == message
        for args, message in (((p(bad_a), 6, p(b), 9), b"sc_pairwise_2d: a coordinate 4 is not finite"),
                              ((p(a), 6, p(bad_b), 9), b"sc_pairwise_2d: b coordinate 8 is not finite")):
            assert lib.sc_pairwise_2d(p(no_ctx), *args, _lib.byref(mean), _lib.byref(least)) == _lib.SC_ERR_INVALID
            assert lib.sc_last_error() == message
