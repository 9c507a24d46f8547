"""fit_nmf / project_nmf without a GPU: the numpy restatement of sc_nmf_fit against sklearn itself, the host's replay of
sklearn's random start, the argument checks (all of them before a device context exists) and the no-fallback rule."""
import numpy as np
import pytest
from scipy import sparse

import nmf_restated as R
from conftest import make_adata

TOL_SKLEARN = 1e-9      # fp64 reorderings of this update measure <= 4.4e-13 of max|.|, float32 arithmetic >= 9e-7


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / np.max(np.abs(b)))


@pytest.mark.parametrize("loss", [R.LOSS_FRO, R.LOSS_KL])
@pytest.mark.parametrize("n,G,K,seed", [(300, 9, 1, 1), (777, 37, 5, 2)])
def test_ordered_restatement_is_sklearn(n, G, K, seed, loss):
    X = R.counts(n, G, max(K, 3), seed)
    W0, H0 = R.start(X, K, seed)
    got = R.ordered(X, W0, H0, loss)
    # an exact n_iter means something only away from the threshold of the stopping rule
    assert R.guard_margin(got["error_trace"], 1e-4) >= 1e-3
    ref = R.sklearn_fit(X, W0, H0, loss)
    assert got["n_iter"] == ref["n_iter"]
    assert _rel(got["W"], ref["W"]) <= TOL_SKLEARN
    assert _rel(got["H"], ref["H"]) <= TOL_SKLEARN
    assert abs(got["reconstruction_err"] - ref["reconstruction_err"]) <= TOL_SKLEARN * ref["reconstruction_err"]
    free = R.dense(X, W0, H0, loss)
    assert free["n_iter"] == ref["n_iter"] and _rel(free["W"], ref["W"]) <= TOL_SKLEARN


def test_update_h_off_is_sklearn_transform():
    X, X2 = R.counts(400, 23, 4, 3), R.counts(150, 23, 4, 4)
    W0, H0 = R.start(X, 4, 3)
    for loss in (R.LOSS_FRO, R.LOSS_KL):
        model = R.sklearn_fit(X, W0, H0, loss, max_iter=40)["model"]
        ref = model.transform(X2)
        Wc = np.full((150, 4), np.sqrt(X2.mean() / 4))
        got = R.ordered(X2, Wc, model.components_, loss, update_H=False, max_iter=model.max_iter, tol=model.tol)
        assert R.guard_margin(got["error_trace"], model.tol) >= 1e-3
        assert _rel(got["W"], ref) <= TOL_SKLEARN
        np.testing.assert_array_equal(got["H"], model.components_)


@pytest.mark.parametrize("seed", [0, 7, 123456])
def test_random_start_replays_sklearn(seed):
    """Through public sklearn only: init="random" with a seed and init="custom" from the replayed draws are one fit."""
    from sklearn.decomposition import NMF

    X = R.counts(211, 17, 3, 5)
    W0, H0 = R.start(X, 6, seed)
    kw = dict(n_components=6, solver="mu", max_iter=30, tol=0.0)
    a = NMF(init="random", random_state=seed, **kw)
    Wa = a.fit_transform(X)
    b = NMF(init="custom", **kw)
    Wb = b.fit_transform(X, W=W0.copy(), H=H0.copy())
    np.testing.assert_array_equal(Wa, Wb)
    np.testing.assert_array_equal(a.components_, b.components_)


def _adata(X):
    return make_adata(np.zeros((X.shape[0], 2)), X)


def test_argument_errors_need_no_gpu():
    from spatialcore_amd.nmf import fit_nmf, project_nmf

    X = R.counts(60, 8, 3, 6)
    ad = _adata(X)
    W0, H0 = R.start(X, 3, 0)
    for kw in (dict(beta_loss="itakura-saito"), dict(beta_loss=1.5), dict(beta_loss=2), dict(init="nndsvda"), dict(init=None),
               dict(init="nndsvd"), dict(solver="cd"), dict(alpha_W=0.1), dict(alpha_H=0.5)):
        with pytest.raises(ValueError, match="supported: beta_loss"):
            fit_nmf(ad, 3, **kw)
    for k in (0, 65, -1, 2.5):
        with pytest.raises(ValueError, match="n_components"):
            fit_nmf(ad, k)
    with pytest.raises(ValueError, match="max_iter"):
        fit_nmf(ad, 3, max_iter=0)
    with pytest.raises(ValueError, match="tol"):
        fit_nmf(ad, 3, tol=-1.0)
    with pytest.raises(ValueError, match="Genes not found"):
        fit_nmf(ad, 3, genes=["g0", "nope"])
    with pytest.raises(ValueError, match="repeat"):
        fit_nmf(ad, 3, genes=["g0", "g1", "g0"])
    with pytest.raises(ValueError, match="needs both W"):
        fit_nmf(ad, 3, init="custom", W=W0)
    with pytest.raises(ValueError, match="only used with"):
        fit_nmf(ad, 3, W=W0, H=H0)
    with pytest.raises(ValueError, match=r"wrong shape passed to NMF \(input W\)"):
        fit_nmf(ad, 3, init="custom", W=W0[:-1], H=H0)
    with pytest.raises(ValueError, match=r"wrong shape passed to NMF \(input H\)"):
        fit_nmf(ad, 3, init="custom", W=W0, H=H0[:, :-1])
    with pytest.raises(ValueError, match=r"Negative values in data passed to NMF \(input H\)"):
        fit_nmf(ad, 3, init="custom", W=W0, H=-H0)
    with pytest.raises(ValueError, match="random_state"):
        fit_nmf(ad, 3, random_state="seed")
    neg = X.toarray()
    neg[3, 2] = -1.0
    for bad in (neg, sparse.csr_matrix(neg), sparse.csc_matrix(neg)):
        with pytest.raises(ValueError, match="Negative values in data passed to NMF"):
            fit_nmf(_adata(bad), 3)
    for v in (np.nan, np.inf):
        nonfinite = X.toarray()
        nonfinite[0, 0] = v
        with pytest.raises(ValueError, match="NaN or infinite"):
            fit_nmf(_adata(nonfinite), 3)
    with pytest.raises(ValueError, match="all zero"):
        fit_nmf(_adata(np.zeros((20, 4))), 2)
    with pytest.raises(ValueError, match="all zero"):
        fit_nmf(_adata(sparse.csr_matrix((np.zeros(2), ([0, 1], [1, 2])), shape=(20, 4))), 2)
    # project_nmf
    genes = [f"g{i}" for i in range(8)]
    with pytest.raises(ValueError, match="supported: beta_loss"):
        project_nmf(ad, H0, genes, beta_loss="itakura-saito")
    with pytest.raises(ValueError, match=r"wrong shape passed to NMF \(input H\)"):
        project_nmf(ad, H0, genes[:-1])
    with pytest.raises(ValueError, match="n_components"):
        project_nmf(ad, np.ones((65, 8)), genes)
    with pytest.raises(ValueError, match="Genes not found"):
        project_nmf(ad, H0, genes[:-1] + ["nope"])
    with pytest.raises(ValueError, match="2-D"):
        project_nmf(ad, H0[0], genes)
    assert "nmf" not in ad.uns and "X_nmf" not in ad.obsm and "spatialcore_metadata" not in ad.uns


def test_host_hands_over_one_canonical_matrix():
    """Dense, CSR, CSC, unsorted CSR with duplicates and CSR with stored zeros become the same arrays; the caller's matrix stays."""
    from spatialcore_amd._sparse_input import canonical_csr as _canonical_csr

    X = R.counts(50, 12, 3, 8)
    A = X.toarray()
    cols = np.arange(12)
    coo = X.tocoo()
    half = sparse.coo_matrix((np.concatenate([coo.data / 2, coo.data / 2]), (np.concatenate([coo.row, coo.row]),
                                                                            np.concatenate([coo.col, coo.col]))), shape=X.shape)
    dup = half.tocsr()
    dup.has_canonical_format = False
    zeros = sparse.csr_matrix(np.ones_like(A))      # every entry stored, row by row ...
    zeros.data[:] = A.ravel()                       # ... most of them as explicit zeros
    forms = [A, X, X.tocsc(), coo, half, dup, zeros, A.astype(np.int32), sparse.csr_matrix(A.astype(np.int64))]
    ref, dt = _canonical_csr(X, cols, 12)
    assert dt == np.float64 and ref.has_canonical_format
    before = X.copy()
    for F in forms:
        got, dt = _canonical_csr(F, cols, 12)
        assert dt == np.float64 and got.data.dtype == np.float64
        for a, b in ((got.indptr, ref.indptr), (got.indices, ref.indices), (got.data, ref.data)):
            np.testing.assert_array_equal(a, b)
    assert (X != before).nnz == 0 and zeros.nnz > X.nnz
    got, dt = _canonical_csr(X.astype(np.float32), cols, 12)
    assert dt == np.float32 and got.data.dtype == np.float32
    sub, _ = _canonical_csr(X, np.array([7, 2, 9]), 12)
    np.testing.assert_array_equal(sub.toarray(), A[:, [7, 2, 9]])


def test_no_cpu_fallback():
    from spatialcore_amd import _lib
    from spatialcore_amd.nmf import fit_nmf, project_nmf

    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    X = R.counts(60, 8, 3, 6)
    with pytest.raises(_lib.SpatialCoreHipError):
        fit_nmf(_adata(X), 3)
    with pytest.raises(_lib.SpatialCoreHipError):
        project_nmf(_adata(X), np.ones((3, 8)), [f"g{i}" for i in range(8)])
