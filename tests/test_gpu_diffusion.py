"""spatialcore_amd.diffusion on the device, against the numpy restatement (tests/diffusion_restated.py: bit for bit except
where exp enters), sklearn's kd_tree, sc_knn_2d and dense / ARPACK eigensolvers.

Shapes come from the kernels' constants.  The search keeps a query's row in registers up to a padded width of 32 columns
(256 queries per workgroup, candidate tiles of 128) and in LDS beyond (64 queries, tiles of 32); below 100 000 queries the
candidates are split over workgroups in whole tiles; its lists are TopK<8 / 16 / 32>.  Every dot product of the Lanczos
step is cut into chunks of 1024 cells."""
import functools

import numpy as np
import pytest
from scipy import sparse

import diffusion_restated as R
from conftest import make_adata

pytestmark = pytest.mark.gpu

TOL = 1e-10
EPS = 2.0 ** -52


def _ctx():
    from spatialcore_amd import _lib

    return _lib.default_context(0)


def _adata(X, key="X_rep"):
    ad = make_adata(np.zeros((X.shape[0], 2)), np.zeros((X.shape[0], 1)))
    ad.obsm[key] = X
    return ad


def _integer_features(n, seed):
    return np.random.default_rng(seed).integers(0, 3, size=(n, 3)).astype(np.float64)


# name: (n, d, k, dtype, forced splits) -- and which edge it is
SEARCH = {
    # every feature width class: 1 and 2 and 7 pad to 8 registers, 33 and 64 take the LDS form (padded 40, 64)
    "d1": (300, 1, 15, np.float64, 0), "d2": (300, 2, 15, np.float64, 0), "d7": (300, 7, 15, np.float64, 0),
    "d33": (300, 33, 15, np.float64, 0), "d64": (300, 64, 15, np.float64, 0),
    # the other register widths: 16, 24, 32 columns
    "d9": (300, 9, 15, np.float64, 0), "d20": (300, 20, 15, np.float64, 0), "d32": (300, 32, 15, np.float64, 0),
    # every list width, and k at a width exactly (8, 16, 32)
    "k2": (300, 7, 2, np.float64, 0), "k8": (300, 7, 8, np.float64, 0), "k16": (300, 7, 16, np.float64, 0),
    "k32": (300, 7, 32, np.float64, 0), "k32_lds": (300, 40, 32, np.float64, 0),
    # n = k + 1: every other cell is a neighbour
    "n_k_plus_1": (16, 3, 15, np.float64, 0), "n_k_plus_1_lds": (33, 40, 32, np.float64, 0),
    # one below, at and one above the candidate tile (128; LDS form 32), one above the query block (256; 64)
    "tile-1": (127, 7, 5, np.float64, 1), "tile": (128, 7, 5, np.float64, 1), "tile+1": (129, 7, 5, np.float64, 1),
    "block+1": (257, 7, 5, np.float64, 1),
    "lds_tile-1": (31, 40, 5, np.float64, 1), "lds_tile": (32, 40, 5, np.float64, 1), "lds_tile+1": (33, 40, 5, np.float64, 1),
    "lds_block+1": (65, 40, 5, np.float64, 1),
    # candidate splits: the library's choice (n = 1000: 8 splits of 128, the last with 104; LDS form 32 of 32, the last
    # with 8) and a forced 3 (384, 384, 232); splits of 32 candidates (the last of 8) hold fewer than k = 32 and leave
    # sentinels for the merge
    "split_auto": (1000, 7, 15, np.float64, 0), "split_auto_lds": (1000, 40, 15, np.float64, 0),
    "split_3": (1000, 7, 15, np.float64, 3), "split_short": (200, 40, 32, np.float64, 7),
    "f32": (300, 7, 15, np.float32, 0), "f32_lds": (300, 33, 15, np.float32, 0),
}


@pytest.mark.parametrize("name", list(SEARCH))
def test_search_bit_for_bit(name):
    n, d, k, dtype, splits = SEARCH[name]
    X = R.traj(n, d, 100 + n + d)[0].astype(dtype)
    idx, d2 = _ctx().knn_dense(X, k, splits=splits)
    ref_idx, ref_d2 = R.knn(X.astype(np.float64), k)
    assert np.array_equal(idx, ref_idx)
    assert np.array_equal(d2, ref_d2)


@pytest.mark.parametrize("splits", [0, 1, 5])
def test_search_ties_and_duplicates(splits):
    """Integer features 0..2 in three columns: 27 distinct points among 500 cells, so almost every comparison is a tie
    and the lists are decided by the index alone."""
    X = _integer_features(500, 7)
    idx, d2 = _ctx().knn_dense(X, 15, splits=splits)
    ref_idx, ref_d2 = R.knn(X, 15)
    assert (ref_d2 == 0).sum() > 500 and len(np.unique(ref_d2)) < 10
    assert np.array_equal(idx, ref_idx)
    assert np.array_equal(d2, ref_d2)


def test_search_does_not_depend_on_the_split():
    X = R.traj(3000, 12, 5)[0]
    ctx = _ctx()
    one = ctx.knn_dense(X, 16, splits=1)
    for splits in (0, 2, 24):
        other = ctx.knn_dense(X, 16, splits=splits)
        assert np.array_equal(one[0], other[0]) and np.array_equal(one[1], other[1])


def test_search_agrees_with_the_planar_search():
    X = R.traj(2000, 2, 9)[0]
    ctx = _ctx()
    idx, d2 = ctx.knn_dense(X, 15)
    assert np.all(np.diff(d2, axis=1) > 0)
    assert np.array_equal(idx, ctx.knn(X, 15))


# ---- graph ------------------------------------------------------------------------------------------------------------
def _device_graph(X, k):
    ctx = _ctx()
    idx, d2 = ctx.knn_dense(X, k)
    info = ctx.diffmap_graph()
    indptr, indices, w, T = ctx.diffmap_graph_get(transition=True)
    return idx, d2, info, indptr, indices, w, T


@pytest.mark.parametrize("n,d,k", [(300, 2, 15), (777, 7, 16), (1200, 64, 32), (600, 33, 5)], ids=["odd", "even", "wide32", "odd5"])
def test_graph_against_restatement(n, d, k):
    X = R.traj(n, d, n)[0]
    idx, d2, info, indptr, indices, w, T = _device_graph(X, k)
    g = R.graph(X, k)
    assert np.array_equal(info["s2"], g["s2"])
    assert np.array_equal(indptr, g["indptr"]) and np.array_equal(indices, g["indices"])
    assert info["n_edges"] == g["indices"].size and info["n_components"] == 1
    rel = np.max(np.abs(w - g["w"]) / g["w"])
    print(f"n={n}, d={d}, k={k}: max relative difference of w to numpy's exp: {rel:.2e}")
    assert rel <= 1e-13
    # from the device's own w on, everything is + x / sqrt: exact
    T_ref, _, _ = R.transition(indptr, indices, w)
    assert np.array_equal(T, T_ref)
    W = sparse.csr_matrix((w, indices, indptr), shape=(n, n))
    assert (W != W.T).nnz == 0


def test_graph_with_a_hub():
    """One point at the centre of a Gaussian cloud of 3000 in 33 dimensions is a neighbour of most of them: a row of the
    union with thousands of entries, a sort with one dominant key prefix."""
    rng = np.random.default_rng(33)
    X = rng.standard_normal((3000, 33))
    X[0] = 0.0
    idx, d2, info, indptr, indices, w, T = _device_graph(X, 15)
    g = R.graph(X, 15)
    in_degree = int((g["idx"] == 0).sum())
    assert in_degree >= 300
    assert indptr[1] - indptr[0] >= in_degree
    assert np.array_equal(idx, g["idx"]) and np.array_equal(info["s2"], g["s2"])
    assert np.array_equal(indptr, g["indptr"]) and np.array_equal(indices, g["indices"])
    rel = np.max(np.abs(w - g["w"]) / g["w"])
    print(f"hub of in-degree {in_degree}: max relative difference of w: {rel:.2e}")
    assert rel <= 1e-13
    assert np.array_equal(T, R.transition(indptr, indices, w)[0])


def test_zero_scale_is_an_error():
    from spatialcore_amd.diffusion import diffusion_map

    X = R.traj(200, 4, 2)[0]
    X[50:58] = X[50]          # eight copies: more than half of the 9 nearest neighbours of each are duplicates
    with pytest.raises(ValueError, match="local scale of cell 50 is zero.*duplicates"):
        diffusion_map(_adata(X), "X_rep", n_neighbors=9, n_comps=3)


def test_disconnected_graph_is_an_error():
    from spatialcore_amd.diffusion import diffusion_map

    X = R.traj(700, 3, 8)[0]
    ad = _adata(X)
    with pytest.raises(ValueError, match="7 connected components.*larger n_neighbors"):
        diffusion_map(ad, "X_rep", n_neighbors=2, n_comps=3)
    assert "X_diffmap" not in ad.obsm


# ---- Lanczos ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2 * R.CHUNK + 1, 700, R.CHUNK], ids=["2_chunks+1", "below_a_chunk", "one_chunk"])
def test_lanczos_steps_bit_for_bit(n):
    """A caller's kernel matrix: T is built from + x / sqrt only, so the whole recurrence is restatable."""
    X = R.traj(n, 5, n)[0]
    g = R.graph(X, 10)
    ctx = _ctx()
    assert ctx.diffmap_graph_csr(g["indptr"], g["indices"], g["w"]) == R.n_components(g["indptr"], g["indices"])
    T = ctx.diffmap_graph_get(transition=True)[3]
    assert np.array_equal(T, g["T"])
    start = np.random.RandomState(0).standard_normal(n)
    ctx.lanczos_begin(start, 40)
    try:
        alpha, beta = ctx.lanczos_run(10)
        alpha, beta = ctx.lanczos_run(14)          # continues where the first call stopped
        V, a_ref, b_ref = R.lanczos(g["indptr"], g["indices"], g["T"], start, 24)
        assert alpha.size == 24 and beta.size == 25
        assert np.array_equal(alpha, np.asarray(a_ref))
        assert np.array_equal(beta, np.asarray(b_ref))
        theta, S = np.linalg.eigh(np.diag(a_ref) + np.diag(b_ref[1:24], 1) + np.diag(b_ref[1:24], -1))
        vecs, res = ctx.lanczos_ritz(S[:, -3:], theta[-3:])
        v_ref, r_ref = R.ritz(g["indptr"], g["indices"], g["T"], V, S[:, -3:], theta[-3:])
        assert np.array_equal(vecs, v_ref) and np.array_equal(res, r_ref)
    finally:
        ctx.lanczos_end()


# ---- the public call ----------------------------------------------------------------------------------------------------
PUBLIC = [(300, 2, 15), (1500, 7, 15), (1031, 20, 15), (1200, 64, 32)]


@functools.lru_cache(maxsize=None)
def _public_input(n, d, k):
    return R.traj(n, d, n)[0]


@functools.lru_cache(maxsize=None)
def _dense_oracle(n, d, k):
    """numpy.linalg.eigh of the dense T that belongs to the device's own kernel matrix (T follows from it exactly)."""
    from spatialcore_amd.diffusion import diffusion_map

    ad = diffusion_map(_adata(_public_input(n, d, k)), "X_rep", n_neighbors=k, n_comps=2, store_graph=True)
    W = ad.obsp["diffmap_connectivities"]
    T = R.transition(W.indptr.astype(np.int64), W.indices, W.data)[0]
    lam, vec = np.linalg.eigh(R.dense(W.indptr, W.indices, T))
    return lam[::-1].copy(), R.sign(vec[:, ::-1])


@pytest.mark.parametrize("n_comps", [2, 15, 33])
@pytest.mark.parametrize("n,d,k", PUBLIC)
def test_public_call_against_dense_oracle(n, d, k, n_comps):
    from spatialcore_amd.diffusion import diffusion_map

    lam_ref, vec_ref = _dense_oracle(n, d, k)
    gap = float(np.min(-np.diff(lam_ref[:n_comps + 1])))
    assert gap >= 1e-4
    X = _public_input(n, d, k)
    ad = diffusion_map(_adata(X), "X_rep", n_neighbors=k, n_comps=n_comps)
    lam, vec, info = ad.uns["diffmap_evals"], ad.obsm["X_diffmap"], ad.uns["diffmap"]
    d_lam, d_vec = np.max(np.abs(lam - lam_ref[:n_comps])), np.max(np.abs(vec - vec_ref[:, :n_comps]))
    print(f"n={n}, d={d}, k={k}, n_comps={n_comps}: {info['n_steps']} steps, residual {info['residuals'].max():.2e}, "
          f"|dlambda| {d_lam:.2e} (bound {4 * n * EPS:.2e}), |dpsi| {d_vec:.2e} (bound {2 * max(TOL, n * EPS) / gap:.2e})")
    assert vec.shape == (n, n_comps) and vec.dtype == np.float64 and lam.shape == (n_comps,)
    assert np.all(np.diff(lam) < 0)
    assert d_lam <= 4 * n * EPS
    assert d_vec <= 2 * max(TOL, n * EPS) / gap
    assert info["residuals"].shape == (n_comps,) and info["residuals"].max() <= TOL
    assert info["n_features"] == d and info["use_rep"] == "X_rep" and info["n_edges"] > n * k
    assert ad.uns["spatialcore_metadata"]["operations"][-1]["function"] == "diffusion_map"
    again = diffusion_map(_adata(X), "X_rep", n_neighbors=k, n_comps=n_comps)
    assert again.obsm["X_diffmap"].tobytes() == vec.tobytes()
    assert again.uns["diffmap_evals"].tobytes() == lam.tobytes()
    assert again.uns["diffmap"]["residuals"].tobytes() == info["residuals"].tobytes()


def test_mid_size_against_kd_tree_and_arpack():
    """30 000 cells in 10 dimensions: 118 query blocks x 17 candidate splits, 30 chunks per dot product."""
    from scipy.sparse.linalg import eigsh
    from sklearn.neighbors import NearestNeighbors

    from spatialcore_amd.diffusion import diffusion_map

    n, d, k, n_comps = 30000, 10, 15, 15
    X = R.traj(n, d, n)[0]
    idx, d2 = _ctx().knn_dense(X, k)
    assert np.all(np.diff(d2, axis=1) > 0)
    ref = NearestNeighbors(n_neighbors=k + 1, algorithm="kd_tree").fit(X).kneighbors(X, return_distance=False)
    assert np.array_equal(idx, ref[:, 1:])
    ad = diffusion_map(_adata(X), "X_rep", n_neighbors=k, n_comps=n_comps, store_graph=True)
    W = ad.obsp["diffmap_connectivities"]
    T = R.transition(W.indptr.astype(np.int64), W.indices, W.data)[0]
    lam_ref, vec_ref = eigsh(sparse.csr_matrix((T, W.indices, W.indptr), shape=(n, n)), k=n_comps + 1, which="LA", tol=0,
                             v0=np.ones(n))
    lam_ref, vec_ref = lam_ref[::-1], R.sign(vec_ref[:, ::-1])
    gap = float(np.min(-np.diff(lam_ref)))
    assert gap >= 1e-4
    lam, vec, info = ad.uns["diffmap_evals"], ad.obsm["X_diffmap"], ad.uns["diffmap"]
    d_lam, d_vec = np.max(np.abs(lam - lam_ref[:n_comps])), np.max(np.abs(vec - vec_ref[:, :n_comps]))
    print(f"n={n}: {info['n_steps']} steps, residual {info['residuals'].max():.2e}, |dlambda| {d_lam:.2e}, |dpsi| {d_vec:.2e}, "
          f"gap {gap:.2e}")
    assert d_lam <= 4 * n * EPS
    assert d_vec <= 2 * max(TOL, n * EPS) / gap
    assert info["residuals"].max() <= TOL


# ---- errors and chains --------------------------------------------------------------------------------------------------
def test_running_out_of_basis_is_an_error():
    from spatialcore_amd.diffusion import diffusion_map

    ad = _adata(_public_input(1500, 7, 15))
    with pytest.raises(RuntimeError, match="did not converge.*max_basis=20.*worst residual"):
        diffusion_map(ad, "X_rep", n_neighbors=15, n_comps=15, max_basis=20)
    assert "X_diffmap" not in ad.obsm


def test_stored_graph_round_trips():
    from spatialcore_amd.diffusion import diffusion_map

    X = _public_input(1031, 20, 15)
    ad = diffusion_map(_adata(X), "X_rep", n_neighbors=15, n_comps=10, store_graph=True)
    W = ad.obsp["diffmap_connectivities"]
    assert W.dtype == np.float64 and W.has_sorted_indices and (W != W.T).nnz == 0
    by_name = diffusion_map(ad, graph="diffmap_connectivities", n_comps=10, key_added="again")
    assert np.array_equal(by_name.uns["again_evals"], ad.uns["diffmap_evals"])
    assert np.array_equal(by_name.obsm["X_again"], ad.obsm["X_diffmap"])
    by_matrix = diffusion_map(_adata(X), graph=W.tocoo(), n_comps=10)
    assert np.array_equal(by_matrix.uns["diffmap_evals"], ad.uns["diffmap_evals"])
    assert by_matrix.uns["diffmap"]["n_edges"] == ad.uns["diffmap"]["n_edges"] and by_matrix.uns["diffmap"]["use_rep"] is None


def test_nmf_to_pseudotime_chain():
    from scipy.stats import spearmanr

    from spatialcore_amd.diffusion import diffusion_map, diffusion_pseudotime
    from spatialcore_amd.nmf import fit_nmf

    rng = np.random.default_rng(4)
    n, G = 500, 40
    t = rng.uniform(0, 1, n)
    rate = 0.2 + 6.0 * np.exp(-((t[:, None] - np.linspace(0, 1, G)[None, :]) / 0.25) ** 2)
    ad = make_adata(np.zeros((n, 2)), sparse.csr_matrix(rng.poisson(rate).astype(np.float64)))
    fit_nmf(ad, 4)
    diffusion_map(ad, n_neighbors=15, n_comps=10)          # use_rep defaults to the usages
    diffusion_pseudotime(ad, int(np.argmin(t)))
    assert ad.uns["diffmap"]["use_rep"] == "X_nmf" and ad.uns["diffmap"]["n_features"] == 4
    dpt = ad.obs["dpt_pseudotime"].to_numpy()
    assert dpt.min() == 0.0 and dpt.max() == 1.0
    rho = spearmanr(dpt, t).correlation
    print(f"nmf -> diffusion map -> pseudotime: Spearman with the trajectory parameter {rho:.3f}")
    assert rho >= 0.9
