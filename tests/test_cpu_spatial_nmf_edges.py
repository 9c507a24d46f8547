"""The inputs of tests/test_gpu_spatial_nmf_edges.py without a GPU (tests/spatial_nmf_edge_inputs.py): each is what it
claims to be, and each separates the defect it is aimed at from the correct kernel -- shown on the restatement
(tests/spatial_nmf_restated.py) alone.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import nmf_restated as R
import spatial_nmf_edge_inputs as E
import spatial_nmf_restated as S


def _check_graph(A, n):
    assert A.has_canonical_format and A.shape == (n, n) and A.diagonal().sum() == 0
    assert (A != A.T).nnz == 0 and A.data.min() > 0 and np.isfinite(A.data).all()


# ---- 1. cell chunks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,G,K", E.CHUNK_TRIPLES)
def test_chunk_case_puts_the_planted_rows_on_the_chunk_boundary(n, G, K):
    X, A, W0, H0, facts = E.chunk_case(n, G, K)
    kp, special, deg = E.kp_of(K), facts["special"], np.diff(A.indptr)
    _check_graph(A, n)
    assert A.data.min() >= 0.1 and A.data.max() <= 3.0 and X.shape == (n, G) and W0.shape == (n, K) and H0.shape == (K, G)
    # a relabelling: the same degrees and weights, cell c on (c + 1010) mod n
    A0 = facts["unshifted"]
    to = (np.arange(n) + E.SHIFT) % n
    assert (A[to][:, to] != A0).nnz == 0
    assert special[0] == 1010 and deg[1010] == 0 and special[1] == 1009 and deg[1009] == 1
    planted = S.edge_degrees(kp) + [2 * kp + 3]
    assert all(deg[special[d]] == d for d in planted)
    cells = sorted(special.values())
    if n > 1033:
        assert cells[0] == 1009 and cells[-1] == 1009 + 3 * len(set(planted)) + 3 <= 1033
    assert A[1023, 1024 % n] > 0                              # the chain crosses 1023 | 1024 (n = 1024: it wraps to cell 0)
    chunks = -(-n // R.CELL_CHUNK)
    cross = E.cross_chunk_entries(A)
    print(f"n = {n}, K = {K}: {chunks} cell chunks, {cross} stored entries join two chunks, planted cells {cells}")
    assert chunks == (1 if n == 1024 else 3 if n == 2049 else 2)
    if (n, G, K) in E.CHUNK_ORDER_SHOWS:
        assert cross >= 8 and (cross == 22 or K != 3)
        assert kp == 1 or max(special[d] for d in planted) >= 1024 > special[3]   # planted rows in both chunks
    elif n == 1025:
        assert cross == 4                                     # cell 1024 alone: its two chain edges, stored twice
    else:
        assert cross == 0
    # the all-zero expression rows keep their graph neighbours
    assert X[n - 1].nnz == 0 and X[n // 3].nnz == 0 and deg[n - 1] >= 1 and deg[n // 3] >= 1


@pytest.mark.parametrize("n,G,K", E.CHUNK_TRIPLES)
def test_chunk_order_of_the_penalty_shows_in_its_bits(n, G, K):
    """A device that added the row penalties as one running sum (or whose chunk loop made one trip) would return another
    penalty wherever the two orders differ.  n = 1024 has one chunk and n = 1025 a second chunk of one cell, whose sum is
    that cell's own term: there the two orders are the same additions, and those two are bounds cases only."""
    X, A, W0, _, _ = E.chunk_case(n, G, K)
    final = E.restated("chunk", (n, G, K), E.LAMBDA, 3, 1e-4)
    for name, W in (("start", W0), ("after 3 iterations", final["W"])):
        chunked, running = E.penalty_sums(X, A, W)
        print(f"n = {n}, K = {K}, {name}: R by chunks {chunked!r}, as one running sum {running!r}")
        if (n, G, K) in E.CHUNK_ORDER_SHOWS:
            assert chunked != running
        else:
            assert chunked == running
    assert final["penalty"] == E.penalty_sums(X, A, final["W"])[0] / 2.0


@pytest.mark.parametrize("n,G,K,iters", E.CHUNK_RUNS)
def test_chunk_runs_are_finite_and_shaped(n, G, K, iters):
    r = E.restated("chunk", (n, G, K), E.LAMBDA, iters, 1e-4)
    assert r["n_iter"] == iters and len(r["objective_trace"]) == 1 + iters // 10
    assert np.isfinite(r["W"]).all() and np.isfinite(r["H"]).all() and r["penalty"] > 0
    assert iters == 3 or r["objective_trace"][1] < r["objective_trace"][0]


# ---- 2. the hub ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,G,K,iters", E.HUB_RUNS)
def test_hub_row_is_long_crosses_chunks_and_its_order_shows(n, G, K, iters):
    """A device that added the hub's a_e W[j_e][k] in any order but index order (here: the adjacent-pair tree of the same
    products) would return another g_ik, at the start and after the run."""
    X, A, W0, _, facts = E.hub_case(n, G, K)
    hub, deg, kp = facts["hub"], np.diff(A.indptr), E.kp_of(K)
    _check_graph(A, n)
    assert A.data.min() >= 0.1 and A.data.max() <= 3.0
    ends = [0, hub - 1, hub + 1, n - 1]                        # (the hub's chain edges are two of its n - 1)
    assert hub == 1100 and deg[hub] == n - 1 and np.all(deg[ends] == 2) and np.all(np.delete(deg, ends + [hub]) == 3)
    assert all(A[i, i + 1] > 0 for i in range(n - 1))
    row = A.indices[A.indptr[hub]:A.indptr[hub + 1]]
    assert np.sum(row < R.CELL_CHUNK) == 1024 and np.sum(row >= R.CELL_CHUNK) == n - 1025
    fetches = -(-deg[hub] // kp)
    print(f"n = {n}, K = {K}: the hub row has {deg[hub]} entries = {fetches} fetches of {kp}, tail {deg[hub] % kp}")
    assert fetches >= 20
    r = E.restated("hub", (n, G, K), E.LAMBDA, iters, 1e-4)
    assert r["n_iter"] == iters and np.isfinite(r["W"]).all() and np.isfinite(r["H"]).all()
    for name, W in (("start", W0), (f"after {iters} iterations", r["W"])):
        ordered, tree = E.hub_sums(A, W, hub)
        print(f"   {name}: {int(np.sum(ordered != tree))} of {K} components differ between index order and the tree")
        assert np.any(ordered != tree)


@pytest.mark.parametrize("n,G,K,iters", E.HUB_RUNS)
def test_hub_objective_falls_over_13_iterations(n, G, K, iters):
    X, A, W0, H0 = E.case("hub", n, G, K)
    r = E.restated("hub", (n, G, K), E.LAMBDA, 13, 1e-4) if iters == 13 else S.ordered(X, A, E.LAMBDA, W0, H0, max_iter=13, tol=1e-4)
    print(f"n = {n}, K = {K}: objective {r['objective_trace']}")
    assert r["n_iter"] == 13 and np.isfinite(r["W"]).all() and np.isfinite(r["H"]).all()
    assert r["objective_trace"][1] < r["objective_trace"][0]


# ---- 3. zeros in the start -------------------------------------------------------------------------------------------------------
def test_zero_start_takes_the_eps_branch_and_stays_zero():
    """A W pass without the den == 0 -> EPS guard would write 0 x (0 / 0) = NaN into 40 entries."""
    X, A, W0, H0, facts = E.zero_case()
    n, G, K = E.ZERO_TRIPLE
    rows, col, comp = facts["zero_rows"], facts["zero_column"], facts["zero_component"]
    deg = np.diff(A.indptr)
    assert rows[0] == 0 and deg[0] == 0 and deg[rows[1]] == E.kp_of(K) == 32 and col == K - 1 and comp == 2
    assert not W0[list(rows)].any() and not W0[:, col].any() and not H0[comp].any()
    assert np.count_nonzero(W0) == (n - 2) * (K - 1) and np.count_nonzero(H0) == (K - 1) * G
    num, den = E.first_w_pass_terms(X, A, E.LAMBDA, W0, H0)
    zero = den == 0
    print(f"first W pass: {int(zero.sum())} of {den.size} denominators are exactly zero")
    assert zero.sum() == 40 and den.size == 5180 and zero[list(rows)].all()
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.isnan(W0 * (num / den)).sum() == 40
    r = E.restated("zeros", (), E.LAMBDA, 13, 1e-4)
    assert r["n_iter"] == 13 and np.isfinite(r["W"]).all() and np.isfinite(r["H"]).all()
    assert np.isfinite(r["objective_trace"]).all() and np.isfinite(r["penalty"])
    assert not r["W"][list(rows)].any() and not r["W"][:, col].any() and not r["H"][comp].any()
    assert r["objective_trace"][1] < r["objective_trace"][0]


# ---- 4. float32 values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,G,K", E.F32_TRIPLES)
def test_float32_values_are_told_from_their_float64_source(n, G, K):
    """A device that read the float32 buffer as anything but float32 widened, or a caller that handed float64 over, would
    not give the restatement's bits: already the unrounded float64 values move every entry of W."""
    X, A, W0, H0, facts = E.f32_case(n, G, K)
    X64 = facts["X64"]
    assert X.dtype == np.float32 and X64.dtype == np.float64 and np.array_equal(X.indices, X64.indices)
    np.testing.assert_array_equal(X.data, np.log1p(E.edge_case(n, G, K)[0].data).astype(np.float32))
    changed = int(np.sum(X.data.astype(np.float64) != X64.data))
    print(f"n = {n}, K = {K}: {changed} of {X.nnz} values change when rounded to float32")
    assert changed > 0
    for iters in (3, 13):
        got = E.restated("f32", (n, G, K), E.LAMBDA, iters, 1e-4)
        other = S.ordered(X64, A, E.LAMBDA, W0, H0, max_iter=iters, tol=1e-4)
        differ = int(np.sum(got["W"] != other["W"]))
        print(f"   {iters} iterations: {differ} of {got['W'].size} entries of W differ in bits")
        assert differ > 0 and got["error_trace"][0] != other["error_trace"][0]     # (the start's error holds sum x^2: nmf_xconst)


# ---- 5. the stop rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam,tol,on_objective,on_error", E.STOP_RULES)
def test_stop_rule_on_the_objective_and_on_the_error_end_apart(lam, tol, on_objective, on_error):
    """Both figures come from the traces of the run that never stops (tol = 0).  One case stops earlier on the objective,
    the other later: a device that looked at the error would return another n_iter in each."""
    free = E.restated("stop", (), lam, 200, 0.0)
    assert free["n_iter"] == 200 and len(free["objective_trace"]) == len(free["error_trace"]) == 21
    obj, err = E.first_stop(free["objective_trace"], tol), E.first_stop(free["error_trace"], tol)
    print(f"lambda = {lam:g}, tol = {tol:g}: the rule stops at {obj} on the objective, at {err} on the error")
    assert (obj, err) == (on_objective, on_error) and obj != err
    stopped = E.restated("stop", (), lam, 200, tol)
    assert stopped["n_iter"] == obj and len(stopped["objective_trace"]) == 1 + obj // 10
    np.testing.assert_array_equal(stopped["objective_trace"], free["objective_trace"][:1 + obj // 10])


def test_stop_rules_differ_in_both_directions():
    (_, _, o1, e1), (_, _, o2, e2) = E.STOP_RULES
    assert o1 < e1 and o2 > e2


# ---- 6. extreme lambda and weights -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [3, 13])
@pytest.mark.parametrize("lam", E.EXTREME_LAMBDAS)
def test_extreme_lambda_stays_finite_and_is_felt(lam, iters):
    r = E.restated("edge", E.SMALL_TRIPLE, lam, iters, 1e-4)
    print(f"lambda = {lam:g}, {iters} iterations: objective {r['objective_trace']}, error {r['error_trace']}, penalty {r['penalty']}")
    assert r["n_iter"] == iters and np.isfinite(r["W"]).all() and np.isfinite(r["H"]).all()
    assert np.isfinite(r["objective_trace"]).all() and np.isfinite(r["error_trace"]).all() and np.isfinite(r["penalty"])
    X, A, W0, H0 = E.case("edge", *E.SMALL_TRIPLE)
    plain = S.ordered(X, A, 0.0, W0, H0, max_iter=iters, tol=1e-4)
    assert np.any(r["W"] != plain["W"])                          # even 1e-12 reaches the bits of W
    if lam > 1:
        assert r["objective_trace"][0] > 1000 * r["error_trace"][0]


def test_weights_over_twelve_decades_stay_finite():
    """The full range of the issue, u in [-6, 6], is kept: nothing had to be narrowed."""
    X, A, W0, H0, facts = E.decades_case()
    _check_graph(A, X.shape[0])
    base = E.edge_case(*E.SMALL_TRIPLE)[1]
    assert np.array_equal(A.indptr, base.indptr) and np.array_equal(A.indices, base.indices)
    ratio = A.data / base.data
    print(f"weights {A.data.min():.3e} .. {A.data.max():.3e}, factors {ratio.min():.3e} .. {ratio.max():.3e}")
    assert ratio.min() >= 1e-6 * (1 - 1e-12) and ratio.max() <= 1e6 * (1 + 1e-12) and ratio.min() < 1e-5 and ratio.max() > 1e5
    for iters in (3, 13):
        r = E.restated("decades", (), E.LAMBDA, iters, 1e-4)
        assert r["n_iter"] == iters and np.isfinite(r["W"]).all() and np.isfinite(r["H"]).all()
        assert np.isfinite(r["objective_trace"]).all() and np.isfinite(r["penalty"]) and r["penalty"] > 0


# ---- 7. iteration counts -----------------------------------------------------------------------------------------------------------
def test_iteration_counts_separate_the_tail_evaluation():
    X, A, W0, H0 = E.case("edge", *E.SMALL_TRIPLE)
    one, ten, eleven = (E.restated("edge", E.SMALL_TRIPLE, E.LAMBDA, it, 1e-4) for it in E.COUNT_ITERS)
    # one pass: the result is the other W buffer's; the first one still holds the start
    assert one["n_iter"] == 1 and len(one["objective_trace"]) == len(one["error_trace"]) == 1
    assert np.sum(one["W"] != W0) > W0.size // 2
    # ten: the check at the last iteration is the final evaluation
    assert ten["n_iter"] == 10 and len(ten["objective_trace"]) == 2 and ten["reconstruction_err"] == ten["error_trace"][-1]
    # eleven: the same check, one more pass, one tail evaluation
    assert eleven["n_iter"] == 11 and len(eleven["objective_trace"]) == 2
    np.testing.assert_array_equal(eleven["objective_trace"], ten["objective_trace"])
    assert eleven["reconstruction_err"] != eleven["error_trace"][-1] and eleven["penalty"] != ten["penalty"]
    assert one["reconstruction_err"] != one["error_trace"][0]
