"""The inputs of tests/test_gpu_nmf_edges.py without a device: each case is what it says it is, and the restatement in the
device's order agrees with numpy's own products and with sklearn itself, over the same three iterations, within a
quarter of the tolerance the GPU test uses (TOL_SKLEARN = 1e-9 for the factors and the error against sklearn; rtol =
1e-12 for the error values against the restatement), so that the GPU tolerances have headroom from the reference alone."""
import numpy as np
import pytest

import lane_group_inputs as L
import nmf_restated as R
from test_cpu_annotation_lanes import _check_ladder
from test_cpu_nmf import TOL_SKLEARN, _rel

CASES = [("ladder", K, 200) for K in L.SWEEP_K] + [("ladder", L.KEY_K, G) for G in L.KEY_G] + [("tall", K, 70) for K in L.TALL_K]


def _case(kind, K, G):
    return L.nmf_tall_case(K) if kind == "tall" else L.nmf_case(K, G)


@pytest.mark.parametrize("K,G", [(K, 200) for K in L.SWEEP_K] + [(L.KEY_K, G) for G in L.KEY_G])
def test_ladder_has_the_structure_the_gpu_tests_rely_on(K, G):
    X, zero = L.nmf_counts(K, G)
    w = L.kp_of(K)
    facts = L.ladder_facts(X, w, zero)
    print(f"K={K} G={G}: {facts}")
    _check_ladder(facts, w, G, zero)
    assert w == {2: 2, 3: 4, 4: 4, 8: 8, 9: 16, 16: 16, 17: 32, 32: 32, 33: 64, 64: 64}[K] == 256 // R.w_rows_per_workgroup(K)
    if G == 256:
        assert facts["longest"] == 255 and zero == 0 and X.indices.max() == 255      # eight key bits, all of them used


def test_zero_gene_sits_at_both_ends_over_the_cases():
    assert {L.nmf_counts(K)[1] for K in L.SWEEP_K} == {0, 199}
    assert L.nmf_counts(L.KEY_K, 257)[1] == 0 and L.nmf_counts(L.KEY_K, 256)[1] == 0


@pytest.mark.parametrize("K", L.TALL_K)
def test_tall_case_has_the_stated_columns(K):
    X, W0, H0 = L.nmf_tall_case(K)
    zero = 0 if K % 2 == 0 else 69
    facts = L.tall_facts(X, L.kp_of(K), zero)
    print(f"tall nmf case K={K}: {facts}")
    assert facts["columns"] == [511, 512, 513, 1029] and facts["chunks_of_the_longest"] == 3
    assert (facts["n"], facts["G"]) == (L.TALL_N_NMF, 70) and facts["remainder"] == 1 and facts["cell_chunks"] == 2
    assert zero in facts["zero_columns"] and W0.shape == (L.TALL_N_NMF, K) and H0.shape == (K, 70)


@pytest.mark.parametrize("loss", L.LOSSES)
@pytest.mark.parametrize("kind,K,G", CASES)
def test_ordered_restatement_against_dense_and_sklearn(kind, K, G, loss):
    X, W0, H0 = _case(kind, K, G)
    got = L.nmf_ordered(kind, K, G, loss)
    free = R.dense(X, W0, H0, loss, max_iter=L.ITERS, tol=0.0)
    ref = R.sklearn_fit(X, W0, H0, loss, max_iter=L.ITERS, tol=0.0)
    assert got["n_iter"] == free["n_iter"] == ref["n_iter"] == L.ITERS
    d_dense = max(_rel(got["W"], free["W"]), _rel(got["H"], free["H"]))
    d_sk = max(_rel(got["W"], ref["W"]), _rel(got["H"], ref["H"]),
               abs(got["reconstruction_err"] - ref["reconstruction_err"]) / ref["reconstruction_err"])
    d_err = max(abs(got["reconstruction_err"] - free["reconstruction_err"]) / free["reconstruction_err"],
                abs(got["error_trace"][0] - free["error_trace"][0]) / free["error_trace"][0])
    print(f"nmf {kind} {X.shape} K={K} {loss}: ordered against dense {d_dense:.2e}, against sklearn {d_sk:.2e} (of max|.|), "
          f"errors against dense {d_err:.2e} (relative)")
    assert d_dense <= 0.25 * TOL_SKLEARN and d_sk <= 0.25 * TOL_SKLEARN
    assert d_err <= 0.25e-12
    assert got["reconstruction_err"] > 0 and np.all(np.isfinite(got["W"])) and got["W"].max() > 0


@pytest.mark.parametrize("loss", L.LOSSES)
@pytest.mark.parametrize("K", [32, 64])
def test_projection_restatement_against_dense_and_sklearn(K, loss):
    """update_H = False from sklearn's constant start, the programmes of the case's own start."""
    X, _, H0 = L.nmf_case(K)
    Wc = L.projection_start(X, K)
    got = L.nmf_ordered("ladder", K, 200, loss, update_H=False)
    free = R.dense(X, Wc, H0, loss, update_H=False, max_iter=L.ITERS, tol=0.0)
    d = _rel(got["W"], free["W"])
    print(f"nmf projection K={K} {loss}: ordered against dense {d:.2e} of max|.|")
    assert d <= 0.25 * TOL_SKLEARN and np.array_equal(got["H"], H0)
