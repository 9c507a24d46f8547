"""GPU tests of sc_kmeans_fit at the edges of its kernels: several tiles per Lloyd workgroup, the FAST / general switch,
the seeding chunk (64) and group (4096) and the Lloyd tile (256) edges, n = K, exact ties and the ends of [0, 1) in the
draw search, relocation of several empty clusters, runs that share a call, and the "same partition" arm of the best-run
rule.

Every comparison is an equality with tests/kmeans_restated.py in its kernel_order mode, which takes every sum in the
kernels' own order.  ctx.kmeans takes the uniforms as an argument, so a test chooses every draw; each test asserts that
its input really reaches the edge it is about."""
import numpy as np
import pytest

import kmeans_restated as kr
from test_cpu_niches import blobs

pytestmark = pytest.mark.gpu


def _L(K):
    return 2 + int(np.log(K))


def _random_draws(seed, n_init, K):
    return np.random.RandomState(seed).random_sample((n_init, 1 + (K - 1) * _L(K)))


def _gpu(X, K, max_iter, draws):
    from spatialcore_amd import _lib

    tol = np.mean(np.var(X, axis=0)) * 1e-4
    return _lib.default_context(0).kmeans(X, K, draws.shape[0], max_iter, float(tol), X.mean(axis=0), draws)


def _assert_same(fit, ref):
    np.testing.assert_array_equal(fit["seeds"], ref["seeds"])
    np.testing.assert_array_equal(fit["labels"], ref["labels"])
    assert fit["centers"].dtype == ref["centers"].dtype
    np.testing.assert_array_equal(fit["centers"], ref["centers"])
    assert fit["inertia"] == ref["inertia"]
    assert fit["n_iter"] == ref["n_iter"]
    assert fit["strict"] == ref["strict"]
    assert fit["distinct"] == ref["distinct"]


def _check(X, K, max_iter, draws):
    """One call of the library against the restatement of that call; returns both."""
    fit = _gpu(X, K, max_iter, draws)
    ref = kr.fit(X, K, draws.shape[0], max_iter, draws, kernel_order=True)
    _assert_same(fit, ref)
    return fit, ref


def _lattice(dtype):
    """X = (P; -P), P integers in [-7, 7]^3 with rows 100:140 copies of row 17: the mean is exactly 0, and every D^2
    and every prefix sum is an integer below 2^24, exact in both types and the same in every summation order."""
    P = np.random.default_rng(4).integers(-7, 8, (2500, 3))
    P[100:140] = P[17]
    X = np.vstack([P, -P]).astype(dtype)
    assert not X.mean(axis=0).any()
    return X


# ---- 1. more than 256 tiles: a workgroup adds a second tile to its partial sums ---------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [65537, 66000])
def test_second_tile_of_a_workgroup(n, dtype):
    """65537: 257 tiles on 256 workgroups, workgroup 0's second tile holds one point.  66000: 258 tiles, workgroups 0
    and 1 have a second tile, the last one of 208 points."""
    C, K, n_init = 4, 3, 2
    assert kr.workgroups(n, C, K, n_init) == 256 < -(-n // 256)
    _check(blobs(n, C, K, 21, dtype), K, 300, _random_draws(21, n_init, K))


# ---- 2. the FAST / general switch at 64 | 65 --------------------------------------------------------------------------
@pytest.mark.parametrize("C,K,dtype", [
    (64, 64, np.float32), (65, 64, np.float32), (64, 65, np.float32),
    (64, 64, np.float64), (65, 64, np.float64),
])
def test_fast_path_edge(C, K, dtype):
    _check(blobs(1500, C, K, 22, dtype), K, 5, _random_draws(22, 2, K))


# ---- 3. chunk (64), tile (256), group (4096) edges and n = K ------------------------------------------------------------
def _edge_seeds(n):
    """n - 1, 0 and the two largest of the chunk, tile and group edges below n - 1."""
    inner = [i for i in (1, 2, 63, 64, 255, 256, 4095, 4096) if i < n - 1]
    return [n - 1, 0] + inner[-2:][::-1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [4, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097])
def test_chunk_tile_group_edges(n, dtype):
    """Run 0 is made to seed at the edge points themselves (draws_for_seeds); runs 1 and 2 draw at random."""
    C, K = 3, 4
    X = blobs(n, C, K, 23, dtype)
    draws = _random_draws(23, 3, K)
    seeds = _edge_seeds(n)
    draws[0] = kr.draws_for_seeds(X - X.mean(axis=0), seeds)
    fit, _ = _check(X, K, 300, draws)
    np.testing.assert_array_equal(fit["seeds"][0], seeds)


# ---- 4. exact ties in the draw search -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_draw_equal_to_a_prefix_value(dtype):
    """K = 2, one run per draw u with u * pot == prefix[i] exactly, both trials of the run at u: the second seed is
    searchsorted(prefix, u * pot, side="left") = i.  ">" in the group, chunk or point search would pass i by."""
    X = _lattice(dtype)
    n, q = X.shape[0], 17
    Xi = X.astype(np.int64)
    D = ((Xi - Xi[q]) ** 2).sum(axis=1)
    prefix = np.cumsum(D)
    pot = float(prefix[-1])
    assert prefix[-1] < 2 ** 24 and dtype(pot) == pot
    np.testing.assert_array_equal(kr.flat_prefix(D.astype(dtype)), prefix)
    ti, tu = kr.tie_draws(D.astype(dtype), pot)
    nxt = np.minimum(ti + 1, n - 1)
    before_zero_run = (D[ti] > 0) & (D[nxt] == 0) & (nxt > ti)
    chunk_end = ti % 64 == 63
    group_end = ti % 4096 == 4095
    assert before_zero_run.sum() >= 1 and chunk_end.sum() >= 1 and group_end.sum() >= 1
    assert np.any(before_zero_run & (ti == 99))          # the 40 copies of q at rows 100:140 follow point 99
    plain = np.flatnonzero(~(before_zero_run | chunk_end | group_end))[::50]
    pick = np.concatenate([np.flatnonzero(before_zero_run | chunk_end | group_end), plain])
    ti, tu = ti[pick], tu[pick]
    oracle = np.searchsorted(prefix, tu * pot, side="left")
    assert np.all(tu * pot == prefix[oracle]) and np.all(oracle <= ti)
    # where D^2[i] = 0 the prefix repeats and the first point of the repeat is chosen; elsewhere it is i itself
    np.testing.assert_array_equal(oracle[D[ti] > 0], ti[D[ti] > 0])
    draws = np.column_stack([np.full(ti.size, (q + 0.5) / n), tu, tu])
    expected = np.column_stack([np.full(ti.size, q), oracle])
    fit = _gpu(X, 2, 1, draws)
    np.testing.assert_array_equal(fit["seeds"], expected)
    ref = kr.fit(X, 2, ti.size, 1, draws, seeding_only=True)
    np.testing.assert_array_equal(ref["seeds"], expected)


# ---- 5. draws at the ends of [0, 1) -------------------------------------------------------------------------------------
def _zero_draws(n, K, firsts, seed):
    """Runs whose first centre is firsts[r] and whose later draws are all 0 (every later seed is point 0), then one
    ordinary random run."""
    draws = np.zeros((len(firsts) + 1, 1 + (K - 1) * _L(K)))
    draws[:-1, 0] = (np.asarray(firsts) + 0.5) / n
    draws[-1] = _random_draws(seed, 1, K)[0]
    return draws


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_draws_relocate_several_empty_clusters(dtype):
    """u = 0 picks point 0.  Run 0 (seeds 0, 0, ...) starts with K - 1 empty clusters, run 1 (q, 0, 0, ...) with K - 2
    filled from two donors in the same iteration, run 2 relocates nothing.  The three share a call, the two relocating
    runs share another, and each is also fitted alone, so that every run's relocation shows in a compared result."""
    n, C, K, q = 700, 5, 6, 350
    X = blobs(n, C, K, 24, dtype)
    draws = _zero_draws(n, K, [0, q], 24)
    fit, ref = _check(X, K, 300, draws)
    np.testing.assert_array_equal(fit["seeds"][:2], [[0] * K, [q] + [0] * (K - 1)])
    first0, first1 = ref["relocations"][0][0], ref["relocations"][1][0]
    assert first0["iteration"] == 0 and first0["empties"] == [1, 2, 3, 4, 5]
    assert first1["iteration"] == 0 and first1["empties"] == [2, 3, 4, 5] and sorted(set(first1["donors"])) == [0, 1]
    assert len(set(first0["distances"])) == K - 1 and min(first0["distances"]) > 0    # distinct, non-zero
    assert ref["relocations"][2] == []
    _check(X, K, 300, draws[:2])
    for r in range(3):
        _, one = _check(X, K, 300, draws[r:r + 1])
        assert one["distinct"] == K


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_relocation_ties_go_to_the_lowest_index(dtype):
    """On the integer lattice the farthest points are at equal distances: which of them move, and to which cluster, is
    decided by the point index alone."""
    X = _lattice(dtype)
    n, K = X.shape[0], 6
    draws = _zero_draws(n, K, [0, 17], 25)
    _check(X, K, 20, draws)
    _check(X, K, 20, draws[:2])
    for r in (0, 1):
        _, one = _check(X, K, 20, draws[r:r + 1])
        first = one["relocations"][0][0]
        assert first["tied"] and len(first["empties"]) > 1 and min(first["distances"]) > 0


def test_draw_above_the_total_takes_the_last_point():
    """float32 data whose potential rounds up: pot = float32(total) > total, and u = nextafter(1, 0) gives
    u * pot > total, so no group's running sum reaches the draw and the seed is n - 1."""
    n, C = 5000, 6
    X = blobs(n, C, 4, 26, np.float32)
    Xc = X - X.mean(axis=0)
    X64 = Xc.astype(np.float64)
    xn = kr._seq_dot(X64 * X64, np.ones(C))
    u = np.nextafter(1.0, 0.0)
    firsts = []
    for q in range(200):
        total = kr.hsum(kr._d2(X64, xn, q, np.float32))
        if u * float(np.float32(total)) > total:
            firsts.append(q)
    assert len(firsts) >= 20                      # about half of all first centres
    firsts = firsts[:6]
    draws = np.column_stack([(np.array(firsts) + 0.5) / n, np.full(len(firsts), u), np.full(len(firsts), u)])
    fit, _ = _check(X, 2, 300, draws)
    np.testing.assert_array_equal(fit["seeds"], [[q, n - 1] for q in firsts])


# ---- 6. runs do not see each other --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_joint_call_equals_single_run_calls(dtype):
    n, C, K = 3000, 6, 5
    # 12 tiles, and 12 workgroups for one run as for three: the four calls sum in the same order
    assert kr.workgroups(n, C, K, 1) == kr.workgroups(n, C, K, 3) == 12
    X = blobs(n, C, K, 27, dtype)
    draws = _random_draws(27, 3, K)
    joint, ref = _check(X, K, 300, draws)
    singles = [_gpu(X, K, 300, draws[r:r + 1]) for r in range(3)]
    for r in range(3):
        np.testing.assert_array_equal(joint["seeds"][r], singles[r]["seeds"][0])
        assert singles[r]["inertia"] == ref["inertias"][r]
    best = singles[ref["best_run"]]
    for key in ("labels", "centers"):
        np.testing.assert_array_equal(joint[key], best[key])
    for key in ("inertia", "n_iter", "strict", "distinct"):
        assert joint[key] == best[key]


# ---- 7. the best-run rule's "same partition" arm ------------------------------------------------------------------------
def test_lower_inertia_with_the_same_partition_does_not_replace():
    """One Lloyd pass from different seeds: later runs reach the first run's partition with other centres and a lower
    inertia.  _is_same_clustering keeps the first run; taking whatever is lower would return another run."""
    n, C, K, n_init = 2000, 4, 3, 10
    X = blobs(n, C, K, 5, np.float32, spread=3.0, noise=0.8)
    draws = _random_draws(5, n_init, K)
    fit, ref = _check(X, K, 1, draws)
    assert (True, True) in ref["decisions"]
    # no run is lower and different before the first lower-and-same one: that one meets the first run's partition
    first_same = ref["decisions"].index((True, True))
    assert (True, False) not in ref["decisions"][:first_same]
    assert ref["best_run"] != int(np.argmin(ref["inertias"]))
    assert fit["inertia"] == ref["inertias"][ref["best_run"]] > min(ref["inertias"])
