"""spatialcore_amd.diffusion without a GPU: the numpy restatement (tests/diffusion_restated.py) against independent
references -- sklearn's kd_tree for the neighbour lists, numpy.linalg.eigh of the dense transition matrix for the
eigenpairs, the Markov property of D^-1/2 T D^1/2, the known first pair (1, sqrt(D)), the trajectory parameter for the
pseudotime -- and everything the two public functions do on the host: every ValueError (raised before any device call) and
diffusion_pseudotime end to end on a stored map."""
import functools

import numpy as np
import pandas as pd
import pytest
from scipy import sparse
from scipy.stats import spearmanr

import diffusion_restated as R
from spatialcore_amd import SimpleAnnData, _lib
from spatialcore_amd.diffusion import diffusion_map, diffusion_pseudotime

# n, d, k, seed: every graph is connected and the 17 leading eigenvalues are at least 1.6e-4 apart (asserted below)
SHAPES = [(257, 1, 5, 1), (300, 2, 15, 300), (1500, 7, 15, 1500), (1031, 20, 15, 1031), (2500, 33, 31, 2500),
          (1200, 64, 32, 1200), (4097, 10, 15, 4097), (5000, 10, 30, 5000)]
N_COMPS = 15
TOL = 1e-10
EPS = 2.0 ** -52


@functools.lru_cache(maxsize=None)
def _case(n, d, k, seed):
    X, t = R.traj(n, d, seed)
    g = R.graph(X, k)
    g["X"], g["t"] = X, t
    return g


@functools.lru_cache(maxsize=None)
def _oracle(n, d, k, seed):
    """numpy.linalg.eigh of the dense T: (values descending, vectors signed by the project's rule)."""
    g = _case(n, d, k, seed)
    lam, vec = np.linalg.eigh(R.dense(g["indptr"], g["indices"], g["T"]))
    return lam[::-1].copy(), R.sign(vec[:, ::-1])


@functools.lru_cache(maxsize=None)
def _restated_pairs(n, d, k, seed):
    g = _case(n, d, k, seed)
    return R.eigenpairs(g["indptr"], g["indices"], g["T"], N_COMPS, tol=TOL)


@pytest.mark.parametrize("n,d,k,seed", SHAPES)
def test_neighbours_equal_kd_tree(n, d, k, seed):
    from sklearn.neighbors import NearestNeighbors

    g = _case(n, d, k, seed)
    assert np.all(np.diff(g["d2"], axis=1) > 0), "the input is meant to be tie-free"
    ref = NearestNeighbors(n_neighbors=k + 1, algorithm="kd_tree").fit(g["X"]).kneighbors(g["X"], return_distance=False)
    assert np.array_equal(ref[:, 0], np.arange(n))
    assert np.array_equal(g["idx"], ref[:, 1:])


@pytest.mark.parametrize("n,d,k,seed", SHAPES)
def test_kernel_is_symmetric_and_connected(n, d, k, seed):
    g = _case(n, d, k, seed)
    W = sparse.csr_matrix((g["w"], g["indices"], g["indptr"]), shape=(n, n))
    assert (W != W.T).nnz == 0                       # bit for bit
    Tm = sparse.csr_matrix((g["T"], g["indices"], g["indptr"]), shape=(n, n))
    assert (Tm != Tm.T).nnz == 0
    assert R.n_components(g["indptr"], g["indices"]) == 1


@pytest.mark.parametrize("n,d,k,seed", SHAPES)
def test_transition_rows_sum_to_one(n, d, k, seed):
    g = _case(n, d, k, seed)
    rows = np.repeat(np.arange(n), np.diff(g["indptr"]))
    P = g["T"] * np.sqrt(g["D"][g["indices"]]) / np.sqrt(g["D"][rows])
    sums = np.bincount(rows, weights=P, minlength=n)
    # each of a row's <= max-degree terms carries a few roundings of relative size 2^-52
    assert np.max(np.abs(sums - 1.0)) <= 8 * np.diff(g["indptr"]).max() * EPS


@pytest.mark.parametrize("n,d,k,seed", SHAPES)
def test_eigenpairs_against_dense_eigh(n, d, k, seed):
    g = _case(n, d, k, seed)
    lam_ref, vec_ref = _oracle(n, d, k, seed)
    lam, vec, res, steps = _restated_pairs(n, d, k, seed)
    gap = float(np.min(-np.diff(lam_ref[:N_COMPS + 1])))
    assert gap >= 1e-4
    print(f"n={n}: {steps} steps, max residual {res.max():.2e}, max |dlambda| {np.abs(lam - lam_ref[:N_COMPS]).max():.2e}, "
          f"max |dpsi| {np.abs(vec - vec_ref[:, :N_COMPS]).max():.2e}, gap {gap:.2e}")
    assert res.max() <= TOL
    assert np.all(np.diff(lam) < 0)
    assert np.max(np.abs(lam - lam_ref[:N_COMPS])) <= 4 * n * EPS
    assert np.max(np.abs(vec - vec_ref[:, :N_COMPS])) <= 2 * max(TOL, n * EPS) / gap
    # a sum of n squares is off by at most n 2^-52 relative, its root by half of that: once in the scaling, once here
    assert np.max(np.abs(np.linalg.norm(vec, axis=0) - 1.0)) <= n * EPS
    # the first pair is known in closed form: lambda_0 = 1, psi_0 proportional to sqrt(D)
    assert abs(lam[0] - 1.0) <= 4 * n * EPS
    stationary = np.sqrt(g["D"]) / np.linalg.norm(np.sqrt(g["D"]))
    assert np.max(np.abs(vec[:, 0] - stationary)) <= 2 * max(TOL, n * EPS) / gap


@pytest.mark.parametrize("n,d,k,seed", [SHAPES[2], SHAPES[6]])
@pytest.mark.parametrize("n_dcs", [10, 15])
def test_pseudotime_orders_the_trajectory(n, d, k, seed, n_dcs):
    g = _case(n, d, k, seed)
    lam, vec, _, _ = _restated_pairs(n, d, k, seed)
    dpt = R.pseudotime(vec, lam, int(np.argmin(g["t"])), n_dcs)
    rho = spearmanr(dpt, g["t"]).correlation
    print(f"n={n}, n_dcs={n_dcs}: Spearman {rho:.4f}")
    assert rho >= 0.95


def test_disconnected_input_is_what_it_claims():
    X, _ = R.traj(700, 3, 8)
    idx, _ = R.knn(X, 2)
    assert R.n_components(*R.union_edges(idx)) == 7


def test_dot_order_is_not_the_plain_sum():
    """The restated dot product is a definite order of its own: it must differ in bits from numpy's somewhere, and agree
    with it to rounding."""
    rng = np.random.default_rng(3)
    differs = 0
    for n in (5, 1024, 1025, 2049 + 17):
        a, b = rng.standard_normal(n), rng.standard_normal(n)
        mine, ref = R.dots(a, b)[0], float(np.dot(a, b))
        assert abs(mine - ref) <= n * EPS * float(np.abs(a) @ np.abs(b))
        differs += mine != ref
    assert differs


# ---- the public functions on the host -----------------------------------------------------------------------------------
def _adata(n=40, d=3, seed=0, **obsm):
    X, _ = R.traj(n, d, seed)
    obs = pd.DataFrame(index=[f"cell{i}" for i in range(n)])
    return SimpleAnnData(np.zeros((n, 2)), obs=obs, obsm={"X_nmf": X, "spatial": X[:, :2].copy(), **obsm})


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a device call was made before the arguments were checked")

    monkeypatch.setattr(_lib, "default_context", refuse)


def _ring(n):
    i = np.arange(n)
    return sparse.csr_matrix((np.ones(2 * n), (np.r_[i, i], np.r_[(i + 1) % n, (i - 1) % n])), shape=(n, n))


BAD_MAP = [
    (dict(use_rep="X_pca"), "not an entry of adata.obsm"),
    (dict(use_rep=3), "not an entry of adata.obsm"),
    (dict(use_rep="wide"), "65 columns"),
    (dict(use_rep="empty"), "0 columns"),
    (dict(use_rep="flat"), "real 2-D array"),
    (dict(use_rep="cplx"), "real 2-D array"),
    (dict(use_rep="text"), "real 2-D array"),
    (dict(use_rep="nan"), "NaN or infinite"),
    (dict(use_rep="inf"), "NaN or infinite"),
    (dict(use_rep="huge"), "2\\^500"),
    (dict(n_neighbors=1), "n_neighbors must be an integer in 2..32"),
    (dict(n_neighbors=33), "n_neighbors must be an integer in 2..32"),
    (dict(n_neighbors=40), "below the 40 cells"),
    (dict(n_neighbors=15.0), "n_neighbors must be an integer"),
    (dict(n_neighbors=True), "n_neighbors must be an integer"),
    (dict(n_comps=1), "n_comps must be an integer in 2..64"),
    (dict(n_comps=65), "n_comps must be an integer in 2..64"),
    (dict(n_comps=40), "below the 40 cells"),
    (dict(n_comps=2.5), "n_comps must be an integer"),
    (dict(tol=0), "tol must be a finite number > 0"),
    (dict(tol=-1e-3), "tol must be a finite number > 0"),
    (dict(tol=float("nan")), "tol must be a finite number > 0"),
    (dict(tol=float("inf")), "tol must be a finite number > 0"),
    (dict(tol="tight"), "tol must be a finite number > 0"),
    (dict(max_basis=3, n_comps=5), "max_basis must be an integer >= n_comps"),
    (dict(max_basis=20.0), "max_basis must be an integer"),
    (dict(random_state=-1), "random_state must be an integer"),
    (dict(random_state=None), "random_state must be an integer"),
    (dict(key_added=""), "key_added must be a non-empty string"),
    (dict(graph="missing"), "not an entry of adata.obsp"),
    (dict(graph=np.eye(40)), "scipy sparse matrix"),
    (dict(graph=_ring(39)), "must be 40 x 40"),
    (dict(graph="directed"), "must be symmetric"),
    (dict(graph="weights_differ"), "must be symmetric"),
    (dict(graph="negative"), "non-negative"),
    (dict(graph="nan"), "NaN or infinite"),
    (dict(graph="lonely"), "empty rows"),
    (dict(graph="zeros"), "empty rows"),
    (dict(graph="cplx"), "must be real"),
]


@pytest.mark.parametrize("kw,message", BAD_MAP, ids=[f"{i}-{sorted(kw)[0]}" for i, (kw, _) in enumerate(BAD_MAP)])
def test_diffusion_map_rejects(no_device, kw, message):
    n = 40
    base, _ = R.traj(n, 3, 0)
    ad = _adata(n, wide=np.zeros((n, 65)), empty=np.zeros((n, 0)), flat=np.zeros(n), cplx=base.astype(complex),
                text=base.astype(str), nan=np.where(np.arange(3) == 1, np.nan, base),
                inf=np.where(np.arange(3) == 2, np.inf, base), huge=base * 2.0 ** 501)
    ring = _ring(n)
    directed = ring.tolil(copy=True)
    directed[0, 1] = 0
    skew = ring.tolil(copy=True)
    skew[0, 1] = 2.0
    neg = ring.tolil(copy=True)
    neg[0, 1] = neg[1, 0] = -1.0
    nan = ring.tolil(copy=True)
    nan[0, 1] = nan[1, 0] = np.nan
    lonely = ring.tolil(copy=True)
    lonely[5, :] = 0
    lonely[:, 5] = 0
    zeros = sparse.csr_matrix((np.zeros(ring.nnz), ring.indices, ring.indptr), shape=(n, n))   # explicit zeros only
    ad.obsp.update(directed=directed.tocsr(), weights_differ=skew.tocsr(), negative=neg.tocsr(), nan=nan.tocsr(),
                   lonely=lonely.tocsr(), zeros=zeros, cplx=ring.astype(complex))
    before = (set(ad.obsm), set(ad.uns), set(ad.obsp))
    with pytest.raises(ValueError, match=message):
        diffusion_map(ad, **kw)
    assert (set(ad.obsm), set(ad.uns), set(ad.obsp)) == before


def test_messages_name_what_is_supported(no_device):
    with pytest.raises(ValueError, match="supported: a finite float32 or float64 representation with 1..64 columns"):
        diffusion_map(_adata(), n_neighbors=99)


def _stored_map(n=600, d=5, k=10, seed=5, n_comps=12):
    X, t = R.traj(n, d, seed)
    g = R.graph(X, k)
    lam, vec, res, _ = R.eigenpairs(g["indptr"], g["indices"], g["T"], n_comps)
    ad = _adata(n, d, seed)
    ad.obsm["X_diffmap"] = vec
    ad.uns["diffmap_evals"] = lam
    return ad, lam, vec, t


@functools.lru_cache(maxsize=None)
def _stored():
    return _stored_map()


def test_pseudotime_end_to_end_on_a_stored_map():
    ad, lam, vec, t = _stored()
    ad = ad.copy()
    root = int(np.argmin(t))
    out = diffusion_pseudotime(ad, root, n_dcs=10)
    assert out is ad
    dpt = ad.obs["dpt_pseudotime"].to_numpy()
    assert dpt.dtype == np.float64
    assert np.array_equal(dpt, R.pseudotime(vec, lam, root, 10))
    assert dpt[root] == 0.0 and dpt.max() == 1.0 and np.all(dpt >= 0)
    assert ad.uns["dpt_pseudotime"] == {"root": root, "n_dcs": 10, "key": "diffmap"}
    assert ad.uns["spatialcore_metadata"]["operations"][-1]["function"] == "diffusion_pseudotime"
    assert spearmanr(dpt, t).correlation >= 0.9
    # the root by name, another output key, a copy
    by_name = diffusion_pseudotime(ad, f"cell{root}", n_dcs=10, key_added="dpt2", copy=True)
    assert by_name is not ad and "dpt2" not in ad.obs
    assert np.array_equal(by_name.obs["dpt2"].to_numpy(), dpt)
    # n_dcs at both ends of its range
    assert np.array_equal(diffusion_pseudotime(ad, root, n_dcs=2, copy=True).obs["dpt_pseudotime"].to_numpy(),
                          R.pseudotime(vec, lam, root, 2))
    assert np.array_equal(diffusion_pseudotime(ad, root, n_dcs=12, copy=True).obs["dpt_pseudotime"].to_numpy(),
                          R.pseudotime(vec, lam, root, 12))


BAD_DPT = [
    (dict(root=0, key="other"), "no diffusion map is stored under key='other'"),
    (dict(root=-1), "not a row number"),
    (dict(root=600), "not a row number"),
    (dict(root="nobody"), "neither a row number nor an entry"),
    (dict(root=1.5), "root must be a row number or an entry"),
    (dict(root=True), "root must be a row number or an entry"),
    (dict(root=0, n_dcs=1), "n_dcs must be an integer in 2..12"),
    (dict(root=0, n_dcs=13), "n_dcs must be an integer in 2..12"),
    (dict(root=0, n_dcs=3.0), "n_dcs must be an integer in 2..12"),
    (dict(root=0, key_added=""), "key_added must be a non-empty string"),
    (dict(root=0, key=""), "key must be a non-empty string"),
]


@pytest.mark.parametrize("kw,message", BAD_DPT, ids=[str(i) for i in range(len(BAD_DPT))])
def test_diffusion_pseudotime_rejects(no_device, kw, message):
    ad = _stored()[0].copy()
    with pytest.raises(ValueError, match=message):
        diffusion_pseudotime(ad, **kw)
    assert "dpt_pseudotime" not in ad.obs


def test_pseudotime_rejects_a_broken_store(no_device):
    ad = _stored()[0].copy()
    ad.uns["diffmap_evals"] = ad.uns["diffmap_evals"][:5]
    with pytest.raises(ValueError, match="eigenvalues for 600 cells"):
        diffusion_pseudotime(ad, 0, n_dcs=3)
    ad = _stored()[0].copy()
    lam = ad.uns["diffmap_evals"].copy()
    lam[1] = 1.0
    ad.uns["diffmap_evals"] = lam
    with pytest.raises(ValueError, match="disconnected"):
        diffusion_pseudotime(ad, 0, n_dcs=3)


def test_package_exports():
    import spatialcore_amd

    assert spatialcore_amd.diffusion.diffusion_map is diffusion_map
    assert set(_lib.SYMBOLS) >= {"sc_knn_dense", "sc_diffmap_graph", "sc_diffmap_graph_csr", "sc_diffmap_graph_get",
                                 "sc_lanczos_begin", "sc_lanczos_run", "sc_lanczos_ritz", "sc_lanczos_end"}
    _lib.load_library()      # every declared symbol is in the built library
