"""sc_knn_dense_gram and spatialcore_amd.neighbors on the device: the certified Gram-form search against the numpy
restatement (tests/diffusion_restated.py: knn), against sc_knn_dense byte for byte, and against sklearn's brute force.

Shapes come from the kernel's constants: an MFMA block is 16 candidates x 16 queries, a wavefront owns 16 queries, a
workgroup 128, a candidate tile holds 64; the kept list is k + slack long, TopK<8 / 16 / 32> re-ranks it.  The recipes and
the margins the certification counts rest on are checked on the host in tests/test_cpu_neighbors.py."""
import functools

import numpy as np
import pytest
from scipy import sparse

import diffusion_restated as R
import neighbors_restated as N
from conftest import make_adata

pytestmark = pytest.mark.gpu


def _ctx():
    from spatialcore_amd import _lib

    return _lib.default_context(0)


@functools.lru_cache(maxsize=None)
def _features(n, d):
    X = R.traj(n, d, 7 * n + d)[0]
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def _truth(n, d, k):
    return R.knn(_features(n, d), k)


def _same(a, b):
    return a[0].dtype == b[0].dtype and a[1].dtype == b[1].dtype and a[0].tobytes() == b[0].tobytes() \
        and a[1].tobytes() == b[1].tobytes()


# (n, d, k): every n, d and k of the cross at least twice; k = n - 1 where it is legal (n = 3, 17)
EQUALITY = [
    (3, 1, 2), (3, 33, 2), (3, 64, 2),
    (17, 1, 9), (17, 3, 16), (17, 8, 2), (17, 50, 8), (17, 64, 16),
    (129, 1, 32), (129, 3, 16), (129, 33, 17), (129, 50, 9), (129, 64, 2),
    (257, 1, 9), (257, 3, 17), (257, 8, 32), (257, 33, 8), (257, 50, 2), (257, 64, 16),
    (1000, 1, 2), (1000, 3, 8), (1000, 8, 9), (1000, 33, 16), (1000, 50, 17), (1000, 64, 32),
    (3000, 1, 16), (3000, 3, 32), (3000, 8, 17), (3000, 33, 2), (3000, 50, 9), (3000, 50, 32), (3000, 64, 8),
]


@pytest.mark.parametrize("n, d, k", EQUALITY, ids=[f"n{n}-d{d}-k{k}" for n, d, k in EQUALITY])
def test_gram_path_equals_restatement_and_direct_search(n, d, k):
    X = _features(n, d)
    ctx = _ctx()
    idx, d2, info = ctx.knn_dense_gram(X, k, path=2)
    assert info["path"] == 2 and info["list_length"] == k + N.SLACK_DEFAULT
    assert info["rows_certified"] + info["rows_fallback"] == n
    assert idx.dtype == np.int32 and d2.dtype == np.float64
    assert _same((idx, d2), _truth(n, d, k))
    assert _same((idx, d2), ctx.knn_dense(X, k))


@pytest.mark.parametrize("k", [15, 32])
def test_pca_like_is_certified_by_the_filter(k):
    X = N.pca_like(3000, 50, N.CERT_SEED)
    truth = R.knn(X, k)
    ctx = _ctx()
    for slack in (0, 1):
        idx, d2, info = ctx.knn_dense_gram(X, k, path=2, slack=slack)
        print(f"pca_like k={k} slack={slack}: {info}")
        assert info["list_length"] == k + (slack or N.SLACK_DEFAULT)
        assert _same((idx, d2), truth)
        assert info["rows_fallback"] == 0 and info["rows_certified"] == 3000      # margins >= 1e6 max E: test_cpu_neighbors.py


def test_forty_fold_duplicates_all_take_the_fallback():
    X, k = N.duplicates(100, 40, 50, 0), 15
    truth = R.knn(X, k)
    assert np.all(truth[1] == 0.0)
    ctx = _ctx()
    for slack in (0, 1):
        idx, d2, info = ctx.knn_dense_gram(X, k, path=2, slack=slack)
        assert info["rows_fallback"] == X.shape[0] and info["rows_certified"] == 0
        assert _same((idx, d2), truth)


@pytest.mark.parametrize("d, dtype, k, slack, m", N.LISTED_EDGE, ids=N.LISTED_EDGE_IDS)
def test_fallback_at_listed_row_block_edges(d, dtype, k, slack, m):
    """Exactly the ``m`` copies are listed for the fallback (the margins: test_cpu_neighbors.py), with ``m`` at the edges
    of its scan's query block; their lists and everybody else's are the exact search's."""
    X = N.far_copies(d, m, dtype)
    truth = R.knn(X, k)
    ctx = _ctx()
    idx, d2, info = ctx.knn_dense_gram(X, k, path=2, slack=slack)
    print(f"far_copies d={d} {np.dtype(dtype).name} k={k} slack={slack} m={m}: {info}")
    assert info["rows_fallback"] == m
    assert info["rows_certified"] == 1000
    assert _same((idx, d2), truth)
    assert _same((idx, d2), ctx.knn_dense(X, k))


def test_lattice_is_certified_in_part():
    X, k = N.lattice(2000, 2), 15
    truth = R.knn(X, k)
    ctx = _ctx()
    idx, d2, info = ctx.knn_dense_gram(X, k, path=2)
    print(f"lattice: {info}")
    assert 0 < info["rows_fallback"] < 2000
    assert _same((idx, d2), truth)
    again = ctx.knn_dense_gram(X, k, path=2, slack=1)
    assert _same(again[:2], truth)


@pytest.mark.parametrize("name", ["offset_1e6", "tiny", "huge", "float32"])
def test_scaled_offset_and_float32_recipes(name):
    X, k = N.recipes(1000)[name], 15
    truth = R.knn(X, k)
    ri, rd, certified, _ = N.filtered_knn(X, k)
    assert _same(N.with_fallback(X, k, ri, rd, certified), truth)      # the restatement itself
    idx, d2, info = _ctx().knn_dense_gram(X, k, path=2)
    print(f"{name}: {info}")
    assert _same((idx, d2), truth)


def test_paths_agree_and_a_second_call_is_identical():
    X, k = _features(1000, 50), 17
    ctx = _ctx()
    direct = ctx.knn_dense(X, k)
    one = ctx.knn_dense_gram(X, k, path=1)
    assert one[2] == {"path": 1, "list_length": k, "rows_certified": 0, "rows_fallback": 0}
    assert _same(one[:2], direct)
    auto = ctx.knn_dense_gram(X, k, path=0)
    assert auto[2]["path"] in (1, 2)
    assert _same(auto[:2], direct)
    a = ctx.knn_dense_gram(X, k, path=2)
    b = ctx.knn_dense_gram(X, k, path=2)
    assert _same(a[:2], direct) and _same(a[:2], b[:2]) and a[2] == b[2]


def test_path_0_takes_the_filter_where_the_rule_says_so():
    """10,000 cells at a padded width of 40: the first size at which path 0 leaves the direct kernels."""
    X, k = _features(10000, 40), 15
    ctx = _ctx()
    direct = ctx.knn_dense(X, k)
    idx, d2, info = ctx.knn_dense_gram(X, k, path=0)
    assert info["path"] == 2 and info["list_length"] == k + N.SLACK_DEFAULT
    assert info["rows_certified"] + info["rows_fallback"] == 10000
    assert _same((idx, d2), direct)
    below = ctx.knn_dense_gram(X[:9999], k, path=0)
    assert below[2]["path"] == 1 and _same(below[:2], ctx.knn_dense(X[:9999], k))
    narrow = ctx.knn_dense_gram(X[:, :32], k, path=0)
    assert narrow[2]["path"] == 1


def test_lists_stay_resident_for_the_graph():
    """sc_diffmap_graph follows the Gram path unchanged: the same graph as after sc_knn_dense."""
    X, k = _features(1000, 50), 15
    ctx = _ctx()
    assert ctx.knn_dense_gram(X, k, fetch=False, path=2)[:2] == (None, None)
    info = ctx.diffmap_graph()
    got = ctx.diffmap_graph_get(transition=True)
    ctx.knn_dense(X, k, fetch=False)
    ref_info = ctx.diffmap_graph()
    ref = ctx.diffmap_graph_get(transition=True)
    assert np.array_equal(info["s2"], ref_info["s2"]) and info["n_edges"] == ref_info["n_edges"]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref))


def test_against_sklearn_brute_force():
    from sklearn.neighbors import NearestNeighbors

    X, k = N.pca_like(3000, 50, 0), 15
    dist, ref = NearestNeighbors(n_neighbors=k + 1, algorithm="brute").fit(X).kneighbors(X)
    assert np.array_equal(ref[:, 0], np.arange(3000))
    idx, d2, _ = _ctx().knn_dense_gram(X, k, path=2)
    assert np.array_equal(idx, ref[:, 1:])
    rel = np.max(np.abs(np.sqrt(d2) - dist[:, 1:]) / dist[:, 1:])
    print(f"max relative difference of the distances to sklearn's brute force: {rel:.2e}")
    assert rel <= 1e-12


# ---- the public call ----------------------------------------------------------------------------------------------------
def _adata(X, key="X_pca"):
    ad = make_adata(np.zeros((X.shape[0], 2)), np.zeros((X.shape[0], 1)))
    ad.obsm[key] = X
    return ad


def test_neighbors_writes_the_graph_louvain_and_diffusion_map_take():
    from spatialcore_amd.cluster import louvain
    from spatialcore_amd.diffusion import diffusion_map
    from spatialcore_amd.neighbors import neighbors

    n, k = 1000, 15
    X = _features(n, 40)
    ad = _adata(X)
    assert neighbors(ad, n_neighbors=k) is ad
    assert set(ad.obsp) == {"distances", "connectivities"}
    info = ad.uns["neighbors"]
    assert info["connectivities_key"] == "connectivities" and info["distances_key"] == "distances"
    assert info["params"] == {"n_neighbors": k, "method": "gauss", "metric": "euclidean", "use_rep": "X_pca", "n_features": 40}
    assert set(info["search"]) == {"path", "list_length", "rows_certified", "rows_fallback"}
    assert ad.uns["spatialcore_metadata"]["operations"][-1]["function"] == "neighbors"

    g = R.graph(X, k)
    D = ad.obsp["distances"]
    assert sparse.isspmatrix_csr(D) and D.shape == (n, n) and D.dtype == np.float64
    assert np.array_equal(np.diff(D.indptr), np.full(n, k)) and D.has_sorted_indices
    order = np.argsort(g["idx"], axis=1, kind="stable")
    assert np.array_equal(D.indices.reshape(n, k), np.take_along_axis(g["idx"], order, axis=1))
    assert np.array_equal(D.data.reshape(n, k), np.sqrt(np.take_along_axis(g["d2"], order, axis=1)))

    C = ad.obsp["connectivities"]
    assert sparse.isspmatrix_csr(C) and C.shape == (n, n) and C.dtype == np.float64
    assert np.array_equal(C.indptr, g["indptr"]) and np.array_equal(C.indices, g["indices"])
    rel = np.max(np.abs(C.data - g["w"]) / g["w"])
    print(f"max relative difference of the connectivities to numpy's exp: {rel:.2e}")
    assert rel <= 1e-13
    assert (C != C.T).nnz == 0

    own = louvain(_adata(X), use_rep="X_pca", n_neighbors=k)
    louvain(ad, graph="connectivities")
    assert np.array_equal(np.asarray(ad.obs["louvain"].astype(str)), np.asarray(own.obs["louvain"].astype(str)))
    ref = diffusion_map(_adata(X), use_rep="X_pca", n_neighbors=k, n_comps=5)
    diffusion_map(ad, graph="connectivities", n_comps=5)
    assert ad.obsm["X_diffmap"].tobytes() == ref.obsm["X_diffmap"].tobytes()
    assert np.array_equal(ad.uns["diffmap_evals"], ref.uns["diffmap_evals"])


def test_neighbors_key_added_copy_and_zero_distances():
    from spatialcore_amd.neighbors import neighbors

    X = _features(300, 8).copy()
    X[17] = X[4]                       # one exact duplicate: a stored zero distance, not a dropped entry
    ad = _adata(X, key="rep")
    out = neighbors(ad, n_neighbors=6, use_rep="rep", key_added="x", copy=True)
    assert out is not ad and not ad.obsp and "x" not in ad.uns
    assert set(out.obsp) == {"x_distances", "x_connectivities"} and "neighbors" not in out.uns
    assert out.uns["x"]["connectivities_key"] == "x_connectivities" and out.uns["x"]["distances_key"] == "x_distances"
    D = out.obsp["x_distances"]
    assert np.array_equal(np.diff(D.indptr), np.full(300, 6))
    row = D.indices[D.indptr[4]:D.indptr[5]]
    assert 17 in row and D.data[D.indptr[4]:D.indptr[5]][list(row).index(17)] == 0.0


def test_neighbors_zero_scale_raises_and_writes_nothing():
    from spatialcore_amd.neighbors import neighbors

    X = _features(200, 5).copy()
    X[51:56] = X[50]
    ad = _adata(X)
    with pytest.raises(ValueError, match="local scale of cell 50 is zero.*duplicates"):
        neighbors(ad, n_neighbors=6)
    assert not ad.obsp and "neighbors" not in ad.uns and "spatialcore_metadata" not in ad.uns


# ---- the drivers where path 0 takes the filter: their own search against the direct one --------------------------------
# 10,000 cells at a padded width of 40 (test_path_0_takes_the_filter_where_the_rule_says_so), k = 15: a trajectory, and the
# wide lattice, whose tied rows go through the exact fallback (test_cpu_neighbors.py checks the recipe on the host)
ABOVE_THE_RULE = {"traj": lambda: _features(10000, 40), "lattice": lambda: N.lattice_wide(10000, 2)}
K_DRIVERS = 15


@functools.lru_cache(maxsize=None)
def _direct_kernel_graph(name):
    """(features, the kernel matrix on the lists of sc_knn_dense): the reference, built without the code under test."""
    X = ABOVE_THE_RULE[name]()
    X.setflags(write=False)
    ctx = _ctx()
    ctx.knn_dense(X, K_DRIVERS, fetch=False)
    ctx.diffmap_graph()
    indptr, indices, w = ctx.diffmap_graph_get()
    return X, sparse.csr_matrix((w, indices, indptr), shape=(X.shape[0], X.shape[0]))


def _takes_the_filter(name, X):
    info = _ctx().knn_dense_gram(X, K_DRIVERS)[2]
    print(f"{name}: {info}")
    assert info["path"] == 2
    if name == "lattice":
        assert info["rows_fallback"] > 0


@pytest.mark.parametrize("name", list(ABOVE_THE_RULE))
def test_diffusion_map_own_search_above_the_rule_equals_the_direct_search(name):
    from spatialcore_amd.diffusion import diffusion_map

    X, ref = _direct_kernel_graph(name)
    _takes_the_filter(name, X)
    ad = diffusion_map(_adata(X), use_rep="X_pca", n_neighbors=K_DRIVERS, n_comps=5, store_graph=True)
    C = ad.obsp["diffmap_connectivities"]
    for part in ("indptr", "indices", "data"):
        a, b = getattr(C, part), getattr(ref, part)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), part
    given = diffusion_map(_adata(X), graph=ref, n_comps=5)
    assert ad.obsm["X_diffmap"].tobytes() == given.obsm["X_diffmap"].tobytes()
    assert ad.uns["diffmap_evals"].tobytes() == given.uns["diffmap_evals"].tobytes()


@pytest.mark.parametrize("name", list(ABOVE_THE_RULE))
def test_louvain_own_search_above_the_rule_equals_the_direct_search(name):
    from spatialcore_amd.cluster import louvain
    from spatialcore_amd.cluster.communities import quantise_weights, resolution_units, run_levels

    X = _direct_kernel_graph(name)[0]
    _takes_the_filter(name, X)
    ctx = _ctx()
    ctx.knn_dense(X, K_DRIVERS, fetch=False)
    ctx.diffmap_graph()
    try:
        ctx.louvain_begin_resident(quantise_weights(ctx.louvain_resident_weights())[0], resolution_units(1.0), 500)
        want = run_levels(ctx, X.shape[0])[0]
    finally:
        ctx.louvain_end()
    ad = louvain(_adata(X), use_rep="X_pca", n_neighbors=K_DRIVERS)
    assert np.array_equal(np.asarray(ad.obs["louvain"].cat.codes), want)
