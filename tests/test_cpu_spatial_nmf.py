"""fit_spatial_nmf without a GPU: the numpy restatement of sc_nmf_fit_graph (tests/spatial_nmf_restated.py) against
sc_nmf_fit's restatement at lambda = 0, against the same definition with scipy / numpy products, the descent Cai et
al. (2011) prove, the effect of the penalty, the planted graph edges, and every argument error of the public function."""
import functools

import numpy as np
import pytest
from scipy import sparse

import nmf_restated as R
import spatial_nmf_restated as S
from conftest import make_adata

K = 4
LAMBDAS = (0.0, 1.0, 10.0, 100.0)
MIN_DROP = 1e-6     # a numpy prototype of these updates measured 7.9e-5 at lambda = 0 and more for the others


@functools.lru_cache(maxsize=None)
def _planted():
    X, xy, _ = S.planted(600, 30, 4, 1)
    return X, S.knn_union(xy, 6), R.start(X, K, 0)


@functools.lru_cache(maxsize=None)
def _descent(lam):
    X, A, (W0, H0) = _planted()
    return S.ordered(X, A, lam, W0, H0, max_iter=200, tol=0.0)


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


def _drops(trace):
    t = np.asarray(trace)
    return (t[:-1] - t[1:]) / t[:-1]


def test_ordered_with_lambda_zero_is_the_plain_restatement_bit_for_bit():
    X, xy, _ = S.planted(300, 25, 4, 0)
    A = S.knn_union(xy, 6)
    W0, H0 = R.start(X, K, 0)
    got = S.ordered(X, A, 0.0, W0, H0, max_iter=20, tol=1e-4)
    want = R.ordered(X, W0, H0, R.LOSS_FRO, True, max_iter=20, tol=1e-4)
    assert got["n_iter"] == want["n_iter"] == 20
    for key in ("W", "H", "error_trace"):
        np.testing.assert_array_equal(got[key], want[key])
    assert got["reconstruction_err"] == want["reconstruction_err"]
    np.testing.assert_array_equal(got["objective_trace"], got["error_trace"])    # F = D + 0
    assert got["penalty"] > 0


def test_ordered_against_dense():
    """Measured on planted(600, 30, 4, seed 1), kNN union k = 6, K = 4, lambda = 10, 20 iterations: the largest
    difference of W is 2.0e-15 and of H 2.7e-15 of max|.|; the bounds are ten times those."""
    X, A, (W0, H0) = _planted()
    o = S.ordered(X, A, 10.0, W0, H0, max_iter=20, tol=1e-4)
    d = S.dense(X, A, 10.0, W0, H0, max_iter=20, tol=1e-4)
    dw, dh = _rel(o["W"], d["W"]), _rel(o["H"], d["H"])
    print(f"ordered against dense: W {dw:.2e}, H {dh:.2e} of max|.|")
    assert o["n_iter"] == d["n_iter"] == 20
    assert dw < 2.0e-14 and dh < 2.7e-14
    assert abs(o["penalty"] - d["penalty"]) < 1e-10 * d["penalty"]
    np.testing.assert_allclose(o["objective_trace"], d["objective_trace"], rtol=1e-12)
    np.testing.assert_allclose(o["error_trace"], d["error_trace"], rtol=1e-12)


@pytest.mark.parametrize("lam", LAMBDAS)
def test_the_objective_never_rises(lam):
    r = _descent(lam)
    trace = r["objective_trace"]
    assert r["n_iter"] == 200 and trace.size == 21
    drops = _drops(trace)
    print(f"lambda = {lam:g}: smallest relative drop between checks {drops.min():.2e}")
    assert np.all(np.diff(trace) < 0)
    assert drops.min() > MIN_DROP


def test_the_objective_never_rises_on_the_edge_graph():
    X, _, (W0, H0) = _planted()
    A, _ = S.edge_graph(X.shape[0], 4, 3)
    r = S.ordered(X, A, 5.0, W0, H0, max_iter=200, tol=0.0)
    drops = _drops(r["objective_trace"])
    print(f"edge graph, lambda = 5: smallest relative drop between checks {drops.min():.2e}")
    assert r["objective_trace"].size == 21 and np.all(np.diff(r["objective_trace"]) < 0)
    assert drops.min() > MIN_DROP


def test_the_penalty_smooths_the_usages():
    """Scale-invariant roughness (columns of W at unit norm) along lambda = 0, 1, 10, 100; measured 4.48, 4.00, 3.79, 3.48."""
    _, A, _ = _planted()
    rough = [S.roughness(_descent(lam)["W"], A) for lam in LAMBDAS]
    print("roughness along lambda:", ", ".join(f"{r:.3f}" for r in rough))
    assert all(a > b for a, b in zip(rough[:-1], rough[1:]))


def test_the_stopping_rule_is_sklearns_on_the_objective():
    X, A, (W0, H0) = _planted()
    r = S.ordered(X, A, 1.0, W0, H0, max_iter=200, tol=1e-2)
    t = r["objective_trace"]
    assert r["n_iter"] == 10 * (t.size - 1) < 200
    rel = (t[:-1] - t[1:]) / t[0]
    assert np.all(rel[:-1] >= 1e-2) and rel[-1] < 1e-2


@pytest.mark.parametrize("n,kp", [(777, 1), (130, 4), (259, 32), (150, 64)])
def test_edge_graph_is_what_it_says(n, kp):
    A, special = S.edge_graph(n, kp, 5)
    assert A.has_canonical_format and A.shape == (n, n) and A.diagonal().sum() == 0
    assert (A != A.T).nnz == 0 and A.data.min() >= 0.1 and A.data.max() <= 3.0
    deg = np.diff(A.indptr)
    assert deg[0] == 0 and deg[n - 1] == 1 and special[0] == 0 and special[1] == n - 1
    for d in S.edge_degrees(kp) + [2 * kp + 3]:
        assert deg[special[d]] == d
    rows = R.w_rows_per_workgroup(kp)
    src = np.repeat(np.arange(n), deg)
    assert np.any(src // rows != A.indices // rows)          # neighbours in other workgroups
    assert all(A[i, i + 1] > 0 for i in range(1, n - 1))     # the chain


def test_union_of_knn_matches_the_tree():
    from spatialcore_amd.nmf.spatial import union_of_knn
    from scipy.spatial import cKDTree

    xy = np.random.default_rng(3).uniform(size=(200, 2))
    _, idx = cKDTree(xy).query(xy, k=7)
    A = union_of_knn(idx[:, 1:].astype(np.int32), None, 200)
    want = S.knn_union(xy, 6)
    assert A.has_canonical_format and (A != want).nnz == 0 and np.all(A.data == 1.0)
    rows = np.arange(100, 200)
    _, idx = cKDTree(xy[rows]).query(xy[rows], k=4)
    B = union_of_knn(idx[:, 1:].astype(np.int32), rows, 200)
    assert B[:100].nnz == 0 and B[:, :100].nnz == 0 and (B[100:, 100:] != S.knn_union(xy[rows], 3)).nnz == 0


def _adata(n=40, G=6, seed=0):
    rng = np.random.default_rng(seed)
    ad = make_adata(rng.uniform(size=(n, 2)), sparse.csr_matrix(rng.poisson(1.0, size=(n, G)).astype(np.float64)))
    ad.obs["slide"] = np.where(np.arange(n) < 5, "a", "b")
    return ad


def test_argument_errors_are_raised_without_a_gpu(monkeypatch):
    from spatialcore_amd import _lib
    from spatialcore_amd.nmf import fit_spatial_nmf

    def no_context(*a, **k):
        raise AssertionError("an argument error must be raised before a context is created")

    monkeypatch.setattr(_lib, "default_context", no_context)
    ad = _adata()
    n = ad.n_obs
    ring = sparse.csr_matrix((np.ones(n), (np.arange(n), (np.arange(n) + 1) % n)), shape=(n, n))
    sym = (ring + ring.T).tocsr()
    lopsided = sym.copy()
    lopsided.data[0] = 2.0
    cases = [
        (dict(spatial_alpha=-1.0), "spatial_alpha"),
        (dict(spatial_alpha=float("nan")), "spatial_alpha"),
        (dict(spatial_alpha="1"), "spatial_alpha"),
        (dict(spatial_key="nowhere"), "not found"),
        (dict(graph=sym, batch_key="slide"), "batch_key"),
        (dict(graph=ring), "symmetric"),
        (dict(graph=lopsided), "symmetric"),
        (dict(graph=sym[:-1]), f"{n} x {n}"),
        (dict(graph="nowhere"), "obsp"),
        (dict(graph=np.eye(n)), "scipy sparse"),
        (dict(graph=-sym), "positive"),
        (dict(n_neighbors=5, batch_key="slide"), "smallest batch"),
        (dict(n_neighbors=n), "smallest data set"),
        (dict(n_neighbors=0), "n_neighbors"),
        (dict(n_neighbors=2.5), "n_neighbors"),
        (dict(batch_key="nope"), "adata.obs"),
        (dict(max_iter=0), "max_iter"),
        (dict(tol=-1.0), "tol"),
        (dict(init="nndsvd"), "init"),
        (dict(init="custom"), "custom"),
        (dict(W=np.ones((n, 3))), "custom"),
        (dict(genes=["g0", "nope"]), "not found"),
        (dict(random_state="seed"), "random_state"),
    ]
    for kw, fragment in cases:
        with pytest.raises(ValueError, match=fragment):
            fit_spatial_nmf(ad, 3, **kw)
    for k in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="n_components"):
            fit_spatial_nmf(ad, k)
    bad = _adata()
    bad.obsm["spatial"] = np.zeros((n, 3))
    with pytest.raises(ValueError, match="2-D"):
        fit_spatial_nmf(bad, 3)
    bad.obsm["spatial"] = np.full((n, 2), np.nan)
    with pytest.raises(ValueError, match="NaN"):
        fit_spatial_nmf(bad, 3)
    with pytest.raises(TypeError):
        fit_spatial_nmf(ad, 3, 1.0, sym)      # everything after spatial_alpha is keyword-only
    assert "spatial_nmf" not in ad.uns and "X_spatial_nmf" not in ad.obsm and "spatialcore_metadata" not in ad.uns


def test_without_a_gpu_a_valid_call_reaches_the_device_and_fails_there():
    from spatialcore_amd import _lib
    from spatialcore_amd.nmf import fit_spatial_nmf

    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(_lib.SpatialCoreHipError):
        fit_spatial_nmf(_adata(), 3)


def test_the_entry_point_is_declared_exported_and_bound():
    import spatialcore_amd.nmf as nmf
    from spatialcore_amd import _lib

    assert nmf.__all__ == ["fit_nmf", "project_nmf", "fit_spatial_nmf"]
    assert "sc_nmf_fit_graph" in _lib.SYMBOLS and hasattr(_lib.load_library(), "sc_nmf_fit_graph")
