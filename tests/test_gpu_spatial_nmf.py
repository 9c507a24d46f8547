"""fit_spatial_nmf on the device: sc_nmf_fit_graph against the numpy restatement in the device's summation order
(tests/spatial_nmf_restated.py), bit for bit -- W, H, both traces, the penalty -- at the lane and workgroup edges of
the W pass with the graph term, against sc_nmf_fit at lambda = 0, the public function, and the C entry's refusals.

Shapes are the smallest at which the kernels can go wrong: K = 1, 3, 20, 33, 64 (one lane; padded lanes; 8, 4 and 4 rows
per workgroup with n not a multiple), graph rows of degree 0, 1, Kp - 1, Kp, Kp + 1 and 2 Kp + 3 (a lane group's fetch
not filled, filled, one and two fetches over), neighbours in other workgroups."""
import ctypes
import functools
import logging

import numpy as np
import pytest
from scipy import sparse

import nmf_restated as R
import spatial_nmf_restated as S
from conftest import make_adata

pytestmark = pytest.mark.gpu

LAMBDA = 2.5
TRIPLES = [(777, 37, 1), (130, 21, 3), (259, 37, 20), (150, 19, 33), (150, 23, 64)]   # n, G, K


def _kp(K):
    return 256 // R.w_rows_per_workgroup(K)


@functools.lru_cache(maxsize=None)
def _case(n, G, K, graph):
    """(X, A, W0, H0).  "knn": planted counts on uniform coordinates and their kNN union; "edge": nmf_restated's counts
    (all-zero rows n // 3, inside the chain, and n - 1, the chain's end) on edge_graph."""
    if graph == "knn":
        X, xy, _ = S.planted(n, G, 3, 100 + K)
        A = S.knn_union(xy, 6)
    else:
        X = R.counts(n, G, 3, 200 + K)
        A, special = S.edge_graph(n, _kp(K), 300 + K)
        assert X[n - 1].nnz == 0 and A[n - 1].nnz == 1 and X[n // 3].nnz == 0 and A[n // 3].nnz >= 2
        assert A[0].nnz == 0 and X[0].nnz > 0
    W0, H0 = R.start(X, K, 7)
    return X, A, W0, H0


def _device(X, A, lam, W0, H0, max_iter, tol):
    from spatialcore_amd import _lib

    X = sparse.csr_matrix(X, dtype=np.float64)
    return _lib.default_context(0).nmf_fit_graph(X.indptr, X.indices, X.data, X.shape[1], A.indptr, A.indices, A.data, lam,
                                                 W0, H0, max_iter, tol)


def _assert_same_bits(got, want):
    assert got["n_iter"] == want["n_iter"]
    for key in ("W", "H", "objective_trace", "error_trace"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert got["penalty"] == want["penalty"] and got["reconstruction_err"] == want["reconstruction_err"]


@pytest.mark.parametrize("iters", [3, 20])
@pytest.mark.parametrize("graph", ["knn", "edge"])
@pytest.mark.parametrize("n,G,K", TRIPLES)
def test_device_equals_the_ordered_restatement_bit_for_bit(n, G, K, graph, iters):
    """On "edge" a W pass that updated W in place would fail: the chain puts a neighbour of almost every row into another
    workgroup, and the hub and the degree-(Kp +- 1) rows read rows that an earlier group of the same workgroup has
    already replaced.  The pass reads the previous iteration's W for every row (Jacobi), as the restatement does."""
    X, A, W0, H0 = _case(n, G, K, graph)
    want = S.ordered(X, A, LAMBDA, W0, H0, max_iter=iters, tol=1e-4)
    got = _device(X, A, LAMBDA, W0, H0, iters, 1e-4)
    assert len(got["objective_trace"]) == 1 + want["n_iter"] // 10
    _assert_same_bits(got, want)
    assert got["penalty"] > 0 and np.all(got["objective_trace"] >= got["error_trace"])


def test_tol_zero_still_records_the_traces():
    X, A, W0, H0 = _case(130, 21, 3, "edge")
    got = _device(X, A, LAMBDA, W0, H0, 25, 0.0)
    _assert_same_bits(got, S.ordered(X, A, LAMBDA, W0, H0, max_iter=25, tol=0.0))
    assert got["n_iter"] == 25 and len(got["objective_trace"]) == 3 and np.all(np.diff(got["objective_trace"]) < 0)


@pytest.mark.parametrize("n,G,K", [(130, 21, 3), (150, 23, 64)])
def test_lambda_zero_equals_sc_nmf_fit_byte_for_byte(n, G, K):
    from spatialcore_amd import _lib

    X, A, W0, H0 = _case(n, G, K, "edge")
    X = sparse.csr_matrix(X, dtype=np.float64)
    plain = _lib.default_context(0).nmf_fit(X.indptr, X.indices, X.data, G, W0, H0, R.LOSS_FRO, True, 30, 1e-4)
    got = _device(X, A, 0.0, W0, H0, 30, 1e-4)
    assert got["n_iter"] == plain["n_iter"]
    for key in ("W", "H", "error_trace"):
        assert got[key].tobytes() == plain[key].tobytes(), key
    assert got["reconstruction_err"] == plain["reconstruction_err"]
    np.testing.assert_array_equal(got["objective_trace"], got["error_trace"])
    empty = sparse.csr_matrix((n, n), dtype=np.float64)          # no graph entry at all: the plain fit whatever lambda is
    alone = _device(X, empty, 3.0, W0, H0, 30, 1e-4)
    assert alone["W"].tobytes() == plain["W"].tobytes() and alone["H"].tobytes() == plain["H"].tobytes() and alone["penalty"] == 0.0


# ---- the public function ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _public_case():
    X, xy, _ = S.planted(500, 20, 3, 5)
    return X, xy, S.knn_union(xy, 6)


def _fit(ad, K=3, **kw):
    from spatialcore_amd.nmf import fit_spatial_nmf

    return fit_spatial_nmf(ad, K, **kw)


def test_public_function_run_to_run_dtypes_and_outputs():
    from spatialcore_amd.nmf import fit_nmf

    X, xy, A = _public_case()
    ad = make_adata(xy, X)
    fit_nmf(ad, 3, max_iter=20)
    before = (ad.obsm["X_nmf"].copy(), ad.uns["nmf"]["components"].copy(), sorted(ad.uns["nmf"]))
    assert _fit(ad, spatial_alpha=4.0, max_iter=30) is ad
    W, info = ad.obsm["X_spatial_nmf"], ad.uns["spatial_nmf"]
    # fit_nmf's outputs are untouched
    assert ad.obsm["X_nmf"].tobytes() == before[0].tobytes() and ad.uns["nmf"]["components"].tobytes() == before[1].tobytes()
    assert sorted(ad.uns["nmf"]) == before[2]
    # against the restatement from the same start, and the keys
    W0, H0 = R.start(X, 3, 0)
    want = S.ordered(X, A, 4.0, W0, H0, max_iter=30, tol=1e-4)
    np.testing.assert_array_equal(W, want["W"])
    np.testing.assert_array_equal(info["components"], want["H"])
    np.testing.assert_array_equal(info["objective_trace"], want["objective_trace"])
    np.testing.assert_array_equal(info["error_trace"], want["error_trace"])
    assert info["penalty"] == want["penalty"] and info["reconstruction_err"] == want["reconstruction_err"]
    assert set(info) == {"components", "genes", "reconstruction_err", "n_iter", "converged", "error_trace", "params",
                         "spatial_alpha", "penalty", "objective_trace", "graph"}
    assert info["spatial_alpha"] == 4.0 and info["n_iter"] == want["n_iter"] and W.dtype == np.float64
    assert info["graph"] == {"source": "knn_union", "n_neighbors": 6, "stored_entries": int(A.nnz)}
    op = ad.uns["spatialcore_metadata"]["operations"][-1]
    assert op["function"] == "fit_spatial_nmf" and op["parameters"]["spatial_alpha"] == 4.0
    assert op["outputs"] == {"obsm": "X_spatial_nmf", "uns": "spatial_nmf"}
    # run to run
    again = _fit(make_adata(xy, X), spatial_alpha=4.0, max_iter=30)
    assert again.obsm["X_spatial_nmf"].tobytes() == W.tobytes()
    assert again.uns["spatial_nmf"]["components"].tobytes() == info["components"].tobytes()
    # float32 (the fp64 result rounded once), integer counts, a dense matrix
    f32 = _fit(make_adata(xy, X.astype(np.float32)), spatial_alpha=4.0, max_iter=30)
    assert f32.obsm["X_spatial_nmf"].dtype == np.float32
    np.testing.assert_array_equal(f32.obsm["X_spatial_nmf"], W.astype(np.float32))
    i64 = _fit(make_adata(xy, X.astype(np.int64)), spatial_alpha=4.0, max_iter=30)
    assert i64.obsm["X_spatial_nmf"].tobytes() == W.tobytes()
    dense = _fit(make_adata(xy, np.asarray(X.todense())), spatial_alpha=4.0, max_iter=30)
    assert dense.obsm["X_spatial_nmf"].tobytes() == W.tobytes()


def test_gene_subset_copy_and_named_graph():
    X, xy, A = _public_case()
    genes = [f"g{i}" for i in (7, 2, 11, 5, 0, 19, 3)]
    ad = make_adata(xy, X)
    ad.obsp["touching"] = A + sparse.identity(A.shape[0], format="csr")      # the diagonal is dropped
    out = _fit(ad, genes=genes, graph="touching", spatial_alpha=2.0, max_iter=20, key_added="prog", copy=True)
    assert out is not ad and "prog" not in ad.uns and "X_prog" not in ad.obsm
    info = out.uns["prog"]
    assert info["genes"] == genes and info["components"].shape == (3, len(genes))
    assert info["graph"] == {"source": "obsp['touching']", "n_neighbors": None, "stored_entries": int(A.nnz)}
    Xs = X[:, [7, 2, 11, 5, 0, 19, 3]].tocsr()
    Xs.sum_duplicates()        # fancy column indexing leaves the rows unsorted
    W0, H0 = R.start(Xs, 3, 0)
    want = S.ordered(Xs, A, 2.0, W0, H0, max_iter=20, tol=1e-4)
    np.testing.assert_array_equal(out.obsm["X_prog"], want["W"])
    np.testing.assert_array_equal(info["components"], want["H"])
    # graph="name" reproduces graph=None when the matrix is the one the search builds; so does the matrix itself
    searched = _fit(make_adata(xy, X), genes=genes, spatial_alpha=2.0, max_iter=20)
    assert searched.obsm["X_spatial_nmf"].tobytes() == out.obsm["X_prog"].tobytes()
    assert searched.uns["spatial_nmf"]["graph"]["stored_entries"] == int(A.nnz)
    given = _fit(make_adata(xy, X), genes=genes, graph=A.tocoo(), spatial_alpha=2.0, max_iter=20)
    assert given.obsm["X_spatial_nmf"].tobytes() == out.obsm["X_prog"].tobytes()
    # a custom start
    custom = _fit(make_adata(xy, X), genes=genes, graph=A, spatial_alpha=2.0, max_iter=20, init="custom", W=W0, H=H0)
    assert custom.obsm["X_spatial_nmf"].tobytes() == out.obsm["X_prog"].tobytes()


def test_batch_key_never_connects_two_slides():
    X, xy, _ = _public_case()
    m = 250
    both = np.concatenate([xy[:m], xy[:m]])                    # the second slide lies exactly on the first
    ad = make_adata(both, X)
    ad.obs["slide"] = np.where(np.arange(2 * m) < m, "s1", "s2")
    block = S.knn_union(xy[:m], 6)
    A = sparse.block_diag([block, block], format="csr")
    got = _fit(ad, spatial_alpha=3.0, batch_key="slide", max_iter=20)
    info = got.uns["spatial_nmf"]
    assert info["graph"] == {"source": "knn_union within obs['slide']", "n_neighbors": 6, "stored_entries": int(A.nnz)}
    want = _fit(make_adata(both, X), spatial_alpha=3.0, graph=A, max_iter=20)
    assert got.obsm["X_spatial_nmf"].tobytes() == want.obsm["X_spatial_nmf"].tobytes()
    assert info["penalty"] == want.uns["spatial_nmf"]["penalty"]
    # interleaved batches: rows are remapped to the cells' own indices
    order = np.random.default_rng(0).permutation(2 * m)
    mixed = make_adata(both[order], X[order])
    mixed.obs["slide"] = np.asarray(ad.obs["slide"])[order]
    P = sparse.csr_matrix((np.ones(2 * m), (np.arange(2 * m), order)), shape=(2 * m, 2 * m))
    Am = (P @ A @ P.T).tocsr()
    Am.sort_indices()
    _fit(mixed, spatial_alpha=3.0, batch_key="slide", max_iter=20)
    ref = _fit(make_adata(both[order], X[order]), spatial_alpha=3.0, graph=Am, max_iter=20)
    assert mixed.obsm["X_spatial_nmf"].tobytes() == ref.obsm["X_spatial_nmf"].tobytes()
    # without batch_key the coincident cells are each other's nearest neighbours
    joined = _fit(make_adata(both, X), spatial_alpha=3.0, max_iter=20)
    assert joined.obsm["X_spatial_nmf"].tobytes() != got.obsm["X_spatial_nmf"].tobytes()


@pytest.fixture
def package_log(caplog):
    """The package logger's records (it does not propagate to the root logger, where caplog listens)."""
    log = logging.getLogger("spatialcore_amd")
    log.propagate = True
    try:
        with caplog.at_level(logging.WARNING, logger="spatialcore_amd"):
            yield caplog
    finally:
        log.propagate = False


def test_convergence_warning_and_converged(package_log):
    X, xy, _ = _public_case()
    info = _fit(make_adata(xy, X), max_iter=7).uns["spatial_nmf"]
    assert info["n_iter"] == 7 and not info["converged"] and len(info["objective_trace"]) == 1
    assert any("Maximum number of iterations 7 reached" in r.getMessage() for r in package_log.records)
    package_log.clear()
    info = _fit(make_adata(xy, X), max_iter=25, tol=0.0).uns["spatial_nmf"]        # tol = 0: to max_iter, no warning
    assert info["n_iter"] == 25 and info["converged"] and len(info["objective_trace"]) == 3 and not package_log.records
    info = _fit(make_adata(xy, X), tol=1e-2).uns["spatial_nmf"]
    assert info["n_iter"] < 200 and info["n_iter"] % 10 == 0 and info["converged"]
    assert len(info["objective_trace"]) == len(info["error_trace"]) == 1 + info["n_iter"] // 10


# ---- the C entry's refusals ------------------------------------------------------------------------------------------
def test_the_c_entry_refuses_every_graph_defect():
    from spatialcore_amd import _lib

    ctx = _lib.default_context(0)
    X = sparse.csr_matrix(np.array([[1.0, 0, 0, 2.0], [0, 0, 0, 0], [0, 0.5, 3.0, 4.0]]))
    W0, H0 = np.ones((3, 2)), np.ones((2, 4))
    gp, gi, gv = np.array([0, 1, 3, 4]), np.array([1, 0, 2, 1]), np.array([0.5, 0.5, 2.0, 2.0])

    def call(p=gp, i=gi, v=gv, lam=1.0):
        return ctx.nmf_fit_graph(X.indptr, X.indices, X.data, 4, p, i, v, lam, W0, H0, 10, 1e-4)

    assert call()["n_iter"] == 10
    defects = [
        (dict(p=np.array([0, 1, 2, 3]), i=np.array([1, 0, 1]), v=np.array([0.5, 0.5, 2.0])), "entry 2 \\(row 2, column 1\\) has no mirror"),
        (dict(v=np.array([0.5, 0.5, 2.0, 2.5])), "entry 2 \\(row 1, column 2\\) and its mirror differ"),
        (dict(p=np.array([0, 1, 4, 5]), i=np.array([1, 0, 1, 2, 1]), v=np.array([0.5, 0.5, 1.0, 2.0, 2.0])), "entry 2 is on the diagonal"),
        (dict(i=np.array([1, 2, 0, 1])), "row 1 is not canonical"),
        (dict(i=np.array([1, 0, 2, 3])), "row 2 is not canonical"),
        (dict(v=np.array([0.5, 0.5, 2.0, 0.0])), "weight 3 \\(row 2, column 1\\) must be finite and > 0"),
        (dict(v=np.array([-0.5, -0.5, 2.0, 2.0])), "weight 0 \\(row 0, column 1\\) must be finite and > 0"),
        (dict(v=np.array([0.5, 0.5, 2.0, np.nan])), "weight 3 \\(row 2, column 1\\) must be finite and > 0"),
        (dict(lam=-1.0), "lambda must be finite and >= 0"),
        (dict(lam=float("nan")), "lambda must be finite and >= 0"),
    ]
    for kw, message in defects:
        with pytest.raises(ValueError, match="sc_nmf_fit_graph: .*" + message):
            call(**kw)
    # null pointers, through the raw entry
    lib = _lib.load_library()
    Xp, Xi, Xv = X.indptr.astype(np.int64), X.indices.astype(np.int32), X.data
    gp64, gi32 = gp.astype(np.int64), gi.astype(np.int32)
    obj, err = np.zeros(2), np.zeros(2)
    checks, iters, recon, pen = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_double(0), ctypes.c_double(0)
    P, Wc, Hc = _lib._ptr, W0.copy(), H0.copy()
    for gptr, gidx, gval in ((None, gi32, gv), (gp64, None, gv), (gp64, gi32, None)):
        rc = lib.sc_nmf_fit_graph(ctx._h, P(Xp), P(Xi), P(Xv), _lib.SC_F64, 3, 4, 2, P(gptr), P(gidx), P(gval), 1.0, 10, 1e-4,
                                  P(Wc), P(Hc), P(obj), P(err), ctypes.byref(checks), ctypes.byref(iters),
                                  ctypes.byref(recon), ctypes.byref(pen))
        assert rc == _lib.SC_ERR_INVALID and b"null pointer" in lib.sc_last_error()
    assert call()["n_iter"] == 10      # the context is as usable as before
