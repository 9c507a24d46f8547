"""ingest without a GPU: the numpy restatement (tests/ingest_restated.py) against sklearn's KNeighborsClassifier and
KNeighborsRegressor, the properties the device tests rely on, and the argument checks of the Python layer, all of which
come before the first call into the library.

The bounds against sklearn (shared with tests/test_gpu_ingest.py through ``sklearn_bounds``).  u = 2^-53.
  * uniform weights: a probability is count / k on both sides: equal.  A regressed value is the mean of k values added in
    another order: the standard bound for a sum of k terms and one division, (k + 3) u max|Y|.
  * distance weights: sklearn's brute force takes its distances in the Gram form |q|^2 + |r|^2 - 2 q.r, whose absolute
    error is at most (2 d + 6) u (|q|^2 + |r|^2) (two norms and a dot product of d terms, three more operations), while
    the lists' d2 is the direct form with relative error (d + 2) u.  A weight d2^(-1/2) therefore differs relatively by
    at most rho = max over the lists' entries of ((2 d + 6) u (|q|^2 + |r|^2) / d2 + (d + 2) u) / 2, plus 3 u for the square
    root, the division and sklearn's own rounding.  A ratio of sums of such weights moves by at most 2 rho' times its
    value (rho' = rho + 3 u), and the two summation orders add (k + 3) u: probabilities within 2 rho' + (k + 3) u,
    regressed values within (2 rho' + (k + 3) u) max|Y|.
"""
import numpy as np
import pandas as pd
import pytest

import ingest_restated as IR
import neighbors_restated as NR
from conftest import make_adata

U = 2.0 ** -53
GAP = 1e-9


def sklearn_bounds(Q, R, idx, d2, Ymax, weighting):
    """(bound on a probability, bound on a regressed value) between the lists' results and sklearn's, as derived above."""
    k, d = idx.shape[1], R.shape[1]
    summation = (k + 3) * U
    if weighting == "uniform":
        return 0.0, summation * Ymax
    Q64, R64 = np.asarray(Q, dtype=np.float64), np.asarray(R, dtype=np.float64)
    nq, nr = (Q64 * Q64).sum(axis=1), (R64 * R64).sum(axis=1)
    rho = 0.5 * ((2 * d + 6) * U * ((nq[:, None] + nr[idx]) / d2).max() + (d + 2) * U) + 3 * U
    return 2 * rho + summation, (2 * rho + summation) * Ymax


@pytest.fixture(scope="module")
def pair():
    """pca_like(3000, 50) and a second draw of 400 queries: every k-th gap exceeds GAP (asserted)."""
    R = NR.pca_like(3000, 50, 0)
    Q = NR.pca_like(400, 50, 7)
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 7, size=R.shape[0])
    Y = rng.standard_normal((R.shape[0], 3))
    return Q, R, codes, Y


@pytest.mark.parametrize("k", [1, 15])
@pytest.mark.parametrize("weighting", ["uniform", "distance"])
def test_restatement_agrees_with_sklearn(pair, k, weighting):
    from sklearn.neighbors import KNeighborsClassifier, KNeighborsRegressor

    Q, R, codes, Y = pair
    assert IR.kth_gap(Q, R, k).min() > GAP          # no pair so close that sklearn's Gram-form distances may swap it
    idx, d2 = IR.cross_knn(Q, R, k)
    clf = KNeighborsClassifier(n_neighbors=k, algorithm="brute", weights=weighting).fit(R, codes)
    dist, ind = clf.kneighbors(Q)
    np.testing.assert_array_equal(ind, idx)
    label, conf, proba = IR.vote(idx, d2, codes, 7, weighting)
    tol_p, tol_y = sklearn_bounds(Q, R, idx, d2, np.abs(Y).max(), weighting)
    sk_proba = clf.predict_proba(Q)
    print(f"k={k} {weighting}: max |proba - sklearn| = {np.abs(proba - sk_proba).max():.3e} (bound {tol_p:.3e})")
    assert np.abs(proba - sk_proba).max() <= tol_p
    top = np.sort(proba, axis=1)
    decided = top[:, -1] - (top[:, -2] if proba.shape[1] > 1 else 0.0) > tol_p
    np.testing.assert_array_equal(label[decided], clf.predict(Q)[decided])
    np.testing.assert_array_equal(conf, proba[np.arange(len(label)), label])
    out = IR.regress(idx, d2, Y, weighting)
    sk_out = KNeighborsRegressor(n_neighbors=k, algorithm="brute", weights=weighting).fit(R, Y).predict(Q)
    print(f"k={k} {weighting}: max |regress - sklearn| = {np.abs(out - sk_out).max():.3e} (bound {tol_y:.3e})")
    assert np.abs(out - sk_out).max() <= tol_y


def test_uniform_vote_is_the_integer_count_with_ties_to_the_lowest_code(pair):
    Q, R, codes, _ = pair
    idx, d2 = IR.cross_knn(Q, R, 8)
    label, conf, proba = IR.vote(idx, d2, codes, 7, "uniform")
    want_label, want_conf, counts = IR.uniform_count_vote(idx, codes, 7)
    np.testing.assert_array_equal(label, want_label)
    np.testing.assert_array_equal(conf, want_conf)
    np.testing.assert_array_equal(proba, counts / 8.0)
    assert ((counts == counts.max(axis=1, keepdims=True)).sum(axis=1) > 1).any()      # the sample holds ties


def test_a_constructed_tie_goes_to_the_lowest_code():
    d2 = np.array([[1.0, 1.0, 4.0, 4.0]])
    # uniform: the list's classes are 5, 5, 2, 2 -- two votes each; the class met first is not the lowest
    label, conf, proba = IR.vote(np.array([[3, 1, 2, 0]], dtype=np.int32), d2, np.array([2, 5, 2, 5]), 6, "uniform")
    assert label[0] == 2 and conf[0] == 0.5 and proba[0, 2] == proba[0, 5] == 0.5
    # distance: class 4 holds the weights 1 and 1/2 (entries 0 and 3), class 1 the same (entries 1 and 2): 1.5 each
    label, conf, proba = IR.vote(np.array([[0, 1, 2, 3]], dtype=np.int32), d2, np.array([4, 1, 1, 4]), 5, "distance")
    assert proba[0, 4] == proba[0, 1] == 0.5 and label[0] == 1 and conf[0] == 0.5


def test_zero_distances_take_the_vote_and_the_average_alone():
    idx = np.array([[4, 2, 0, 1], [0, 1, 2, 3]], dtype=np.int32)
    d2 = np.array([[0.0, 0.0, 1.0, 9.0], [0.0, 0.25, 0.25, 4.0]])
    codes = np.array([0, 0, 1, 0, 2])
    Y = np.arange(10.0).reshape(5, 2)
    w = IR.weights(d2, "distance")
    np.testing.assert_array_equal(w, [[1, 1, 0, 0], [1, 0, 0, 0]])
    label, conf, proba = IR.vote(idx, d2, codes, 3, "distance")
    np.testing.assert_array_equal(proba, [[0, 0.5, 0.5], [1, 0, 0]])
    np.testing.assert_array_equal(label, [1, 0])
    np.testing.assert_array_equal(IR.regress(idx, d2, Y, "distance"), [(Y[4] + Y[2]) / 2.0, Y[0]])
    np.testing.assert_array_equal(IR.weights(d2, "uniform"), np.ones((2, 4)))


def test_cross_search_on_one_set_is_the_self_search_plus_the_cell_itself():
    """cross_knn(X, X, k + 1) without j = i (or without its last entry) equals knn(X, k), duplicates included."""
    import diffusion_restated as DR

    for X in (NR.pca_like(300, 9, 2), NR.lattice(300, 2), NR.duplicates(20, 6, 5)):
        k = 4
        ci, cd = IR.cross_knn(X, X, k + 1)
        si, sd = DR.knn(X, k)
        got_i, got_d = self_from_cross(ci, cd)
        np.testing.assert_array_equal(got_i, si)
        np.testing.assert_array_equal(got_d, sd)


def self_from_cross(ci, cd):
    """Remove j = i from every row of a (k + 1)-list where present, otherwise its last entry."""
    n, k1 = ci.shape
    own = ci == np.arange(n)[:, None]
    drop = np.where(own.any(axis=1), own.argmax(axis=1), k1 - 1)
    keep = np.ones_like(ci, dtype=bool)
    keep[np.arange(n), drop] = False
    return ci[keep].reshape(n, k1 - 1), cd[keep].reshape(n, k1 - 1)


def test_mixed_dtypes_widen_each_array_on_its_own():
    R = NR.pca_like(200, 5, 1)
    Q32 = NR.pca_like(50, 5, 2).astype(np.float32)
    a = IR.cross_knn(Q32, R, 3)
    b = IR.cross_knn(Q32.astype(np.float64), R, 3)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


# ---- the Python layer's argument checks: all before the library is loaded ---------------------------------------------------------------
def _objects(n_ref=30, n=10, d=4):
    rng = np.random.default_rng(0)
    ref = make_adata(np.zeros((n_ref, 2)), np.zeros((n_ref, 3)))
    ref.obsm["X_pca"] = rng.standard_normal((n_ref, d))
    ref.obsm["X_umap"] = rng.standard_normal((n_ref, 2))
    ref.obs["cluster"] = pd.Categorical(rng.integers(0, 3, n_ref).astype(str), categories=["0", "1", "2", "unused"])
    ad = make_adata(np.zeros((n, 2)), np.zeros((n, 3)))
    ad.obsm["X_pca"] = rng.standard_normal((n, d))
    return ad, ref


def _snapshot(ad):
    return (sorted(ad.obs.columns), sorted(ad.obsm), sorted(ad.uns))


@pytest.mark.parametrize("change, kwargs, fragment", [
    (None, dict(), "at least one of obs"),
    (None, dict(obs="cluster", weights="gauss"), "weights must be one of"),
    (None, dict(obs="cluster", n_neighbors=0), "n_neighbors must be an integer in 1..32"),
    (None, dict(obs="cluster", n_neighbors=33), "n_neighbors must be an integer in 1..32"),
    (None, dict(obs="cluster", n_neighbors=31), "at most the 30 reference cells"),
    (None, dict(obs="cluster", n_neighbors=2.0), "n_neighbors must be an integer"),
    (None, dict(obs="nope"), "is not in adata_ref.obs"),
    (None, dict(obsm="nope"), "is not in adata_ref.obsm"),
    (None, dict(obs=["cluster", "cluster"]), "names a key twice"),
    (None, dict(obs="cluster", key_added=""), "key_added must be a non-empty string"),
    (None, dict(obs="cluster", use_rep="X_other"), "is not an entry of adata.obsm"),
    ("no_query_rep", dict(obs="cluster"), "project_pca(adata, adata_ref)"),
    ("columns", dict(obs="cluster"), "columns in adata and"),
    ("nan_rep", dict(obs="cluster"), "NaN or infinite"),
    ("missing", dict(obs="cluster"), "missing values"),
    ("floats", dict(obs="score"), "must be categorical, string, bool or integer"),
    ("wide", dict(obsm="wide"), "1..64 are supported"),
    ("nan_obsm", dict(obsm="X_umap"), "NaN or infinite"),
    ("ragged", dict(obsm="flat"), "real 2-D array"),
])
def test_ingest_refuses_and_writes_nothing(change, kwargs, fragment):
    from spatialcore_amd.neighbors import ingest

    ad, ref = _objects()
    if change == "no_query_rep":
        del ad.obsm["X_pca"]
    elif change == "columns":
        ad.obsm["X_pca"] = ad.obsm["X_pca"][:, :3]
    elif change == "nan_rep":
        ad.obsm["X_pca"][3, 1] = np.nan
    elif change == "missing":
        ref.obs["cluster"] = pd.Categorical([None] + ["1"] * 29, categories=["0", "1"])
    elif change == "floats":
        ref.obs["score"] = np.linspace(0, 1, 30)
    elif change == "wide":
        ref.obsm["wide"] = np.zeros((30, 65))
    elif change == "nan_obsm":
        ref.obsm["X_umap"][0, 0] = np.inf
    elif change == "ragged":
        ref.obsm["flat"] = np.zeros(30)
    before = _snapshot(ad), _snapshot(ref)
    with pytest.raises(ValueError, match=fragment.replace("(", r"\(").replace(")", r"\)").replace(".", r"\.")):
        ingest(ad, ref, **kwargs)
    assert (_snapshot(ad), _snapshot(ref)) == before


def test_query_neighbors_checks_its_arguments():
    from spatialcore_amd.neighbors import query_neighbors

    ad, ref = _objects()
    with pytest.raises(ValueError, match="n_neighbors must be an integer in 1..32"):
        query_neighbors(ad, ref, n_neighbors=0)
    del ad.obsm["X_pca"]
    with pytest.raises(ValueError, match="project_pca"):
        query_neighbors(ad, ref)


def test_codes_keep_categories_or_sort_unique_values():
    from spatialcore_amd.neighbors.ingest import _codes

    _, ref = _objects()
    codes, cats = _codes(ref, "cluster")
    assert list(cats) == ["0", "1", "2", "unused"] and codes.dtype == np.int32
    np.testing.assert_array_equal(np.asarray(cats)[codes], ref.obs["cluster"].astype(str).values)
    ref.obs["s"] = ["b", "a", "c"] * 10
    ref.obs["i"] = np.array([7, -1, 3] * 10)
    ref.obs["flag"] = np.array([True, False, True] * 10)
    for col, want in (("s", ["a", "b", "c"]), ("i", [-1, 3, 7]), ("flag", [False, True])):
        codes, cats = _codes(ref, col)
        assert list(cats) == want
        np.testing.assert_array_equal(np.asarray(cats)[codes], ref.obs[col].values)
