"""sc_nmf.hip past one lane-group fetch (inputs: tests/lane_group_inputs.py, proved fair by tests/test_cpu_nmf_lanes.py):
every lane-group width kp = 2 .. 64 on rows of 0 to 3 kp + 3 and of all stored entries, groups of one wavefront with
different trip counts, the projection path, gene columns of several chunks at kp = 32 and 64, eight and nine sort-key bits.

Three iterations from a custom start without a check (tol = 0): W and the components bit for bit against the restatement
in the device's order, the error values at rtol = 1e-12, and the same run against sklearn itself at TOL_SKLEARN.  No
tolerance is new."""
import numpy as np
import pytest

import lane_group_inputs as L
from test_gpu_nmf import _adata, _against_sklearn, _fit

pytestmark = pytest.mark.gpu

CASES = [("ladder", K, 200) for K in L.SWEEP_K] + [("ladder", L.KEY_K, G) for G in L.KEY_G] + [("tall", K, 70) for K in L.TALL_K]


def _case(kind, K, G):
    return L.nmf_tall_case(K) if kind == "tall" else L.nmf_case(K, G)


def _run(X, K, loss, W0, H0):
    return _fit(X, K, loss, init="custom", W=W0, H=H0, max_iter=L.ITERS, tol=0.0)


@pytest.mark.parametrize("loss", L.LOSSES)
@pytest.mark.parametrize("kind,K,G", CASES)
def test_three_iterations_are_the_ordered_restatement(kind, K, G, loss):
    X, W0, H0 = _case(kind, K, G)
    exact = L.nmf_ordered(kind, K, G, loss)
    W, info = _run(X, K, loss, W0, H0)
    np.testing.assert_array_equal(W, exact["W"])
    np.testing.assert_array_equal(info["components"], exact["H"])
    assert info["n_iter"] == L.ITERS and info["converged"] and len(info["error_trace"]) == 1
    # the errors hold a log and a square root: not bit for bit
    np.testing.assert_allclose(info["error_trace"][0], exact["error_trace"][0], rtol=1e-12)
    np.testing.assert_allclose(info["reconstruction_err"], exact["reconstruction_err"], rtol=1e-12)
    empty = np.flatnonzero(np.diff(X.indptr) == 0)
    assert (empty.size >= 1 or kind == "tall") and not W[empty].any()             # the ladder's rows without a trip
    assert not info["components"][:, np.diff(X.tocsc().indptr) == 0].any()         # the all-zero gene, at either end


@pytest.mark.parametrize("loss", L.LOSSES)
@pytest.mark.parametrize("kind,K,G", CASES)
def test_three_iterations_match_sklearn(kind, K, G, loss):
    X, W0, H0 = _case(kind, K, G)
    W, info = _run(X, K, loss, W0, H0)
    _against_sklearn(X, W0, H0, loss, W, info, max_iter=L.ITERS, tol=0.0)


@pytest.mark.parametrize("loss", L.LOSSES)
@pytest.mark.parametrize("K", [32, 64])
def test_projection_on_the_ladder_is_the_ordered_restatement(K, loss):
    from spatialcore_amd.nmf import project_nmf

    X, _, H0 = L.nmf_case(K)
    exact = L.nmf_ordered("ladder", K, 200, loss, update_H=False)
    ad = project_nmf(_adata(X), H0, [f"g{j}" for j in range(X.shape[1])], beta_loss=loss, max_iter=L.ITERS, tol=0.0)
    np.testing.assert_array_equal(ad.obsm["X_nmf"], exact["W"])
    np.testing.assert_array_equal(ad.uns["nmf"]["components"], H0)
    assert ad.uns["nmf"]["n_iter"] == L.ITERS
    np.testing.assert_allclose(ad.uns["nmf"]["reconstruction_err"], exact["reconstruction_err"], rtol=1e-12)


@pytest.mark.parametrize("loss", L.LOSSES)
def test_two_calls_give_identical_bytes(loss):
    X, W0, H0 = L.nmf_case(32)
    (W, info), (W2, info2) = _run(X, 32, loss, W0, H0), _run(X, 32, loss, W0, H0)
    assert W.tobytes() == W2.tobytes() and info["components"].tobytes() == info2["components"].tobytes()
    assert info["reconstruction_err"] == info2["reconstruction_err"]
    np.testing.assert_array_equal(info["error_trace"], info2["error_trace"])
