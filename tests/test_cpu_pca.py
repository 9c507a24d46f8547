"""spatialcore_amd.pca without a GPU: the argument errors of pca / project_pca (refused before any device work), the
restatements the GPU tests lean on (tests/pca_restated.py) pinned against sklearn, the host part of pca/decompose.py fed
numpy's Gram matrix, and SimpleAnnData.varm.

TOL = 1e-9 of the reference's largest entry, as tests/test_gpu_pca.py; its header says where the figure comes from."""
import numpy as np
import pandas as pd
import pytest
from scipy import sparse

import pca_restated as R
from spatialcore_amd import SimpleAnnData
from spatialcore_amd.pca import decompose as D
from spatialcore_amd.pca import pca, project_pca

TOL = 1e-9
CASES = [(n, G, K, False) for n, G, K in R.SHAPES] + [(*R.LANE_SHAPE, K, True) for K in R.LANE_COMPS]


def _adata(n=30, G=8, seed=3, **kw):
    X = R.counts(n, G, seed)
    return SimpleAnnData(X.copy(), var_names=[f"g{i}" for i in range(G)], **kw)


@pytest.fixture(autouse=True)
def _no_device(monkeypatch):
    """Every call of this file must be refused before it asks for a context."""
    from spatialcore_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the device was asked for")

    monkeypatch.setattr(_lib, "default_context", refuse)


# ---- argument errors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, 65, -1, 2.5, True, "3", None])
def test_n_comps_must_be_an_integer_in_range(bad):
    with pytest.raises(ValueError, match=r"n_comps must be an integer in 1\.\.64"):
        pca(_adata(), bad)


def test_n_comps_is_bounded_by_cells_and_genes():
    with pytest.raises(ValueError, match=r"n_comps=8 exceeds min\(64, cells - 1, genes\) = 7"):
        pca(_adata(8, 9), 8)
    with pytest.raises(ValueError, match=r"n_comps=9 exceeds min\(64, cells - 1, genes\) = 8"):
        pca(_adata(30, 8), 9)


def test_gene_and_cell_limits_are_named():
    big = SimpleAnnData(sparse.csr_matrix((3, 4097), dtype=np.float64))
    with pytest.raises(ValueError, match=r"limited to 4096 genes.*got 4097"):
        pca(big, 2)
    one = SimpleAnnData(np.ones((1, 5)))
    with pytest.raises(ValueError, match=r"2 <= cells <= 2\^31 - 1, got 1"):
        pca(one, 1)


@pytest.mark.parametrize("kw,match", [
    ({"dtype": "float16"}, "dtype='float16' is not supported"),
    ({"dtype": "int32"}, "is not supported"),
    ({"normalize": 1}, "normalize must be True or False"),
    ({"scale": "yes"}, "scale must be True or False"),
    ({"target_sum": 0}, "target_sum must be a finite number > 0"),
    ({"target_sum": float("inf")}, "target_sum must be a finite number > 0"),
    ({"key_added": ""}, "key_added must be None or a non-empty string"),
    ({"key_added": 3}, "key_added must be None or a non-empty string"),
    ({"genes": ["g1", "nope"]}, "Genes not found"),
    ({"genes": ["g1", "g1"]}, "must not repeat"),
    ({"genes": []}, "at least one gene"),
])
def test_option_errors(kw, match):
    with pytest.raises(ValueError, match=match):
        pca(_adata(), 2, **kw)


def test_matrix_errors():
    ad = _adata()
    bad = ad.X.toarray()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or infinite"):
        pca(SimpleAnnData(bad), 2)
    neg = ad.X.toarray()
    neg[2, 1] = -1.0
    with pytest.raises(ValueError, match="normalize=True needs non-negative"):
        pca(SimpleAnnData(neg), 2, normalize=True)
    with pytest.raises(ValueError, match="all zero"):
        pca(SimpleAnnData(np.zeros((6, 4))), 2)
    with pytest.raises(KeyError):
        pca(ad, 2, layer="missing")


def _fake_result(ad, K=2, key=None, normalize=False):
    """A stored decomposition written by hand: orthonormal loadings, the gene means."""
    G = ad.n_vars
    obsm, varm, uns = D._keys(key)
    Q = np.linalg.qr(np.random.default_rng(5).normal(size=(G, K)))[0]
    ad.varm[varm] = Q
    ad.uns[uns] = {"variance": np.ones(K), "variance_ratio": np.full(K, 0.1), "mean": np.asarray(ad.X.mean(axis=0)).ravel(),
                   "scale": np.ones(G), "genes": list(ad.var_names),
                   "params": {"n_comps": K, "normalize": normalize, "target_sum": 1e4, "scale": False, "dtype": "float64", "layer": None}}
    return ad


def test_project_errors():
    src = _fake_result(_adata())
    with pytest.raises(ValueError, match="source must be an AnnData-like"):
        project_pca(_adata(), 3)
    with pytest.raises(ValueError, match="holds no PCA result"):
        project_pca(_adata(), _adata())
    with pytest.raises(ValueError, match="holds no PCA result"):
        project_pca(_adata(), src, key_added="other")
    fewer = SimpleAnnData(R.counts(30, 8, 3)[:, :6].copy(), var_names=[f"g{i}" for i in range(6)])
    with pytest.raises(ValueError, match=r"not found in adata.var_names: \['g6', 'g7'\]"):
        project_pca(fewer, src)
    info = dict(src.uns["pca"])
    with pytest.raises(ValueError, match=r"loadings must be \(genes, n_comps\)"):
        project_pca(_adata(), (info, np.zeros((5, 2))))
    with pytest.raises(ValueError, match="lacks \\['scale'\\]"):
        project_pca(_adata(), ({k: v for k, v in info.items() if k != "scale"}, src.varm["PCs"]))
    bad = dict(info, scale=np.zeros(8))
    with pytest.raises(ValueError, match="scale positive"):
        project_pca(_adata(), (bad, src.varm["PCs"]))
    with pytest.raises(ValueError, match="key_added"):
        project_pca(_adata(), src, key_added="")
    neg = _adata()
    neg.X = neg.X.toarray()
    neg.X[0, 0] = -2.0
    with pytest.raises(ValueError, match="normalize=True needs non-negative"):
        project_pca(neg, _fake_result(_adata(), normalize=True))


# ---- the restatements ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("n,G,K,lane", CASES)
def test_dense_pca_matches_sklearn(n, G, K, lane, mode):
    C, X, ref, mask = R.reference_case(n, G, K, mode, lane)
    assert (~mask).sum() <= K // 4, "the gap filter may exclude at most a quarter of the components"
    mine = R.dense_pca(X.toarray(), K, scale=mode == "normalize_scale")
    d = R.differences(mine, ref, mask)
    print(f"dense_pca vs sklearn covariance_eigh {n}x{G} K={K} {mode}: excluded {(~mask).sum()}, "
          f"variance {d[0]:.2e} ratio {d[1]:.2e} loadings {d[2]:.2e} scores {d[3]:.2e}")
    assert max(d) <= TOL, d


@pytest.mark.parametrize("mode", ["counts", "normalize_scale"])
@pytest.mark.parametrize("n,G,K,lane", [CASES[2], CASES[5], CASES[-1]])
def test_ordered_project_matches_dense_pca(n, G, K, lane, mode):
    C, X, _, _ = R.reference_case(n, G, K, mode, lane)
    mine = R.dense_pca(X.toarray(), K, scale=mode == "normalize_scale")
    Vs = mine["components"] / mine["scale"]
    got = R.ordered_project(X, Vs, R.offsets(Vs, mine["mean"]))
    # |x| |v| per entry, G entries a row: a few G ulp of the row's absolute sum
    bound = 4 * G * np.finfo(float).eps * (abs(X) @ np.abs(Vs.T) + np.abs(Vs) @ np.abs(mine["mean"]))
    assert np.all(np.abs(got - mine["scores"]) <= np.asarray(bound))
    if n >= 9:
        np.testing.assert_array_equal(got[n // 3], -R.offsets(Vs, mine["mean"]))      # the all-zero cell


def test_log1p_norm_is_the_plain_formula():
    C = R.counts(777, 37, R.SEED)
    A = C.toarray()
    s = A.sum(axis=1, keepdims=True)        # integer counts: exact in any order
    want = np.log1p(np.divide(A, s, out=np.zeros_like(A), where=s > 0) * 1e4)
    np.testing.assert_array_equal(R.log1p_norm(C).toarray(), want)
    assert not R.log1p_norm(C)[777 // 3].nnz or not R.log1p_norm(C)[777 // 3].data.any()


# ---- the host part of decompose.py ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("n,G,K", [(5, 3, 2), (777, 37, 5), (2500, 130, 50)])
def test_host_decompose_on_numpy_gram(n, G, K, scale):
    A = R.log1p_norm(R.counts(n, G, R.SEED)).toarray()
    host = D.host_decompose(A.T @ A, A.sum(axis=0), n, K, scale)
    want = R.dense_pca(A, K, scale=scale)
    for key in ("mean", "scale"):
        np.testing.assert_allclose(host[key], want[key], rtol=1e-13, atol=0)
    mask = R.separated(want["spectrum"], K)
    host["scores"] = want["scores"]
    assert max(R.differences(host, want, mask)) <= TOL
    V, lam = host["components"], host["variance"]
    assert V.shape == (K, G) and lam.shape == (K,) and host["variance_ratio"].shape == (K,)
    assert np.all(np.diff(lam) <= 0) and np.all(lam >= 0)
    assert np.max(np.abs(V @ V.T - np.eye(K))) <= 1e-12
    assert np.all(V[np.arange(K), np.argmax(np.abs(V), axis=1)] > 0)
    if G >= 4:
        assert not V[:, G // 2].any() and host["scale"][G // 2] == 1.0
    if not scale:
        assert np.all(host["scale"] == 1.0)
    Vs, off = D.projection_operands(V, host["mean"], host["scale"])
    np.testing.assert_array_equal(Vs, V / host["scale"])
    np.testing.assert_array_equal(off, R.offsets(Vs, host["mean"]))


def test_negative_eigenvalues_are_clipped_and_signs_follow_the_largest_entry():
    C = np.diag([3.0, -1e-18, 1.0])
    C[0, 2] = C[2, 0] = -0.5
    lam, ratio, V = D.eigen_decompose(C, 3)
    assert lam[2] == 0.0 and np.all(np.diff(lam) <= 0)
    np.testing.assert_allclose(ratio.sum(), 1.0, rtol=1e-15)
    assert np.all(V[np.arange(3), np.argmax(np.abs(V), axis=1)] > 0)
    np.testing.assert_allclose(C @ V[0], lam[0] * V[0], atol=1e-15)


def test_correlation_scaling_treats_a_constant_gene_as_standard_scaler_does():
    rng = np.random.default_rng(2)
    A = rng.normal(size=(50, 4))
    A[:, 1] = 0.0
    A[:, 3] = 7.25        # constant and not zero: its variance is rounding noise
    mean, C = D.covariance_from_gram(A.T @ A, A.sum(axis=0), 50)
    sigma, Cs = D.correlation_scaling(C, mean, 50)
    assert sigma[1] == 1.0 and sigma[3] == 1.0 and not Cs[1].any() and not Cs[:, 3].any()
    np.testing.assert_allclose(sigma[[0, 2]], A[:, [0, 2]].std(axis=0, ddof=1), rtol=1e-13)
    np.testing.assert_allclose(np.diag(Cs)[[0, 2]], 1.0, rtol=1e-15)


# ---- SimpleAnnData.varm ------------------------------------------------------------------------------------------------------------
def test_varm_travels_through_copy_and_column_slicing():
    L = np.arange(16.0).reshape(8, 2)
    ad = _adata(varm={"PCs": L})
    assert SimpleAnnData(np.zeros((2, 2))).varm == {}
    cp = ad.copy()
    cp.varm["PCs"][0, 0] = -1.0
    assert ad.varm["PCs"][0, 0] == 0.0 and set(cp.varm) == {"PCs"}
    sub = ad[:, ["g5", "g1"]]
    np.testing.assert_array_equal(sub.varm["PCs"], L[[5, 1]])
    assert list(sub.var_names) == ["g5", "g1"]
    assert isinstance(ad.obs, pd.DataFrame)
