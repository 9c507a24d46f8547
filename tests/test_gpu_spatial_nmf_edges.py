"""sc_nmf_fit_graph at the edges tests/test_gpu_spatial_nmf.py stops short of (inputs: tests/spatial_nmf_edge_inputs.py,
proved fair by tests/test_cpu_spatial_nmf_edges.py): more than one cell chunk with the graph term and two W buffers, graph
rows whose neighbours lie in another chunk, a hub row of n - 1 entries, exact zeros in the start (den == 0 -> EPS),
float32 values, a stop rule that must look at the objective, lambda and weights over many decades, max_iter = 1, 10, 11.

Everything is compared with spatial_nmf_restated.ordered bit for bit: W, H, both traces, the penalty, the final error
and n_iter.  There is no tolerance in this file."""
import numpy as np
import pytest

import spatial_nmf_edge_inputs as E

pytestmark = pytest.mark.gpu


def _device(X, A, lam, W0, H0, max_iter, tol):
    """The values go over in the dtype they have (float32 stays float32)."""
    from spatialcore_amd import _lib

    assert X.has_canonical_format and X.data.dtype in (np.float32, np.float64)
    return _lib.default_context(0).nmf_fit_graph(X.indptr, X.indices, X.data, X.shape[1], A.indptr, A.indices, A.data, lam,
                                                 W0, H0, max_iter, tol)


def _assert_same_bits(got, want):
    assert got["n_iter"] == want["n_iter"]
    for key in E.KEYS:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert got["penalty"] == want["penalty"] and got["reconstruction_err"] == want["reconstruction_err"]


def _both(kind, args, lam, max_iter, tol=1e-4):
    X, A, W0, H0 = E.case(kind, *args)
    return _device(X, A, lam, W0, H0, max_iter, tol), E.restated(kind, args, lam, max_iter, tol)


# ---- 1. cell chunks ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,G,K,iters", E.CHUNK_RUNS)
def test_cell_chunk_edges_with_the_graph_term(n, G, K, iters):
    """One, two and three cell chunks (PENPART, the ROWPEN pass of k_nmf_rowerr_chunks and both loops of k_nmf_obj_final
    past one trip), with cellsums(), h_pass(), k_nmf_rowerr and k_nmf_penalty reading W() after the flip; 13 iterations
    hold a check at iteration 10 and the tail evaluation.  n = 1024 and 1025 are bounds cases: the order of the chunk
    sums cannot show there."""
    got, want = _both("chunk", (n, G, K), E.LAMBDA, iters)
    assert len(got["objective_trace"]) == 1 + iters // 10
    _assert_same_bits(got, want)


def test_three_chunks_twice_give_the_same_bytes():
    X, A, W0, H0 = E.case("chunk", 2049, 23, 33)
    first, second = _device(X, A, E.LAMBDA, W0, H0, 13, 1e-4), _device(X, A, E.LAMBDA, W0, H0, 13, 1e-4)
    for key in E.KEYS:
        assert first[key].tobytes() == second[key].tobytes(), key
    assert first["penalty"] == second["penalty"] and first["reconstruction_err"] == second["reconstruction_err"]
    _assert_same_bits(second, E.restated("chunk", (2049, 23, 33), E.LAMBDA, 13, 1e-4))


# ---- 2. the hub ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,G,K,iters", E.HUB_RUNS)
def test_hub_row_across_the_chunks(n, G, K, iters):
    """Cell 1100 has n - 1 neighbours, 1024 of them in the first chunk: hundreds of fetches of lane_group_walk in index
    order, beside rows of two and three entries in the same wavefront (K < 64)."""
    got, want = _both("hub", (n, G, K), E.LAMBDA, iters)
    _assert_same_bits(got, want)
    assert np.isfinite(got["W"]).all() and np.isfinite(got["H"]).all()


# ---- 3. zeros in the start -------------------------------------------------------------------------------------------------------
def test_zeros_in_the_start_stay_zero_and_nothing_turns_nan():
    got, want = _both("zeros", (), E.LAMBDA, 13)
    _assert_same_bits(got, want)
    facts = E.zero_case()[4]
    assert np.isfinite(got["W"]).all() and np.isfinite(got["H"]).all()
    assert np.isfinite(got["objective_trace"]).all() and np.isfinite(got["error_trace"]).all() and np.isfinite(got["penalty"])
    assert not got["W"][list(facts["zero_rows"])].any() and not got["W"][:, facts["zero_column"]].any()
    assert not got["H"][facts["zero_component"]].any()


# ---- 4. float32 values -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [3, 13])
@pytest.mark.parametrize("n,G,K", E.F32_TRIPLES)
def test_float32_values_are_widened_exactly(n, G, K, iters):
    """The restatement runs on the float32 values widened to float64; on their float64 source every entry of W differs."""
    X = E.case("f32", n, G, K)[0]
    assert X.data.dtype == np.float32
    got, want = _both("f32", (n, G, K), E.LAMBDA, iters)
    _assert_same_bits(got, want)


# ---- 5. the stop rule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam,tol,on_objective,on_error", E.STOP_RULES)
def test_stop_rule_looks_at_the_objective(lam, tol, on_objective, on_error):
    got, want = _both("stop", (), lam, 200, tol)
    assert want["n_iter"] == on_objective != on_error
    assert got["n_iter"] == want["n_iter"] and len(got["objective_trace"]) == 1 + on_objective // 10
    _assert_same_bits(got, want)


# ---- 6. extreme lambda and weights -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [3, 13])
@pytest.mark.parametrize("lam", E.EXTREME_LAMBDAS)
def test_extreme_lambda(lam, iters):
    got, want = _both("edge", E.SMALL_TRIPLE, lam, iters)
    _assert_same_bits(got, want)
    assert np.isfinite(got["W"]).all() and np.isfinite(got["H"]).all()


@pytest.mark.parametrize("iters", [3, 13])
def test_weights_over_twelve_decades(iters):
    got, want = _both("decades", (), E.LAMBDA, iters)
    _assert_same_bits(got, want)
    assert np.isfinite(got["W"]).all() and np.isfinite(got["H"]).all() and np.isfinite(got["penalty"])


# ---- 7. iteration counts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", E.COUNT_ITERS)
def test_iteration_counts(iters):
    """max_iter = 1: the result lies in the second W buffer, one evaluation at the start and the tail's.  10: the check at
    the last iteration is the final evaluation.  11: that check, one more pass, one tail evaluation."""
    got, want = _both("edge", E.SMALL_TRIPLE, E.LAMBDA, iters)
    _assert_same_bits(got, want)
    assert got["n_iter"] == iters and len(got["objective_trace"]) == len(got["error_trace"]) == (1 if iters == 1 else 2)
    if iters == 1:
        assert np.any(got["W"] != E.case("edge", *E.SMALL_TRIPLE)[2])
    if iters == 10:
        assert got["reconstruction_err"] == got["error_trace"][-1]
    if iters == 11:
        assert got["reconstruction_err"] != got["error_trace"][-1]
