"""GPU tests of identify_niches / sc_kmeans_fit: the reference's own results (tests/golden/ref_niches.npz), the numpy
restatement of the kernels (tests/kmeans_restated.py) on random inputs, determinism, the workflow end to end, and
one run at size (10^6 cells x 20 cell types, K = 8, the reference's defaults)."""
import time
import warnings

import numpy as np
import pytest

import kmeans_restated as kr
from conftest import load_golden, make_adata
from test_cpu_niches import BLOB_SHAPES, CASES, LATTICE_TIES, ari, blobs

pytestmark = pytest.mark.gpu

G = load_golden("ref_niches.npz")


def _adata(P):
    from spatialcore_amd import SimpleAnnData

    return SimpleAnnData(np.zeros((P.shape[0], 1)), var_names=["g0"], obsm={"neighborhood_profile": P})


def _run(P, **kw):
    from spatialcore_amd.spatial import identify_niches

    a = _adata(P)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        identify_niches(a, **kw)
    return a, [str(w.message) for w in caught if type(w.message).__name__ == "ConvergenceWarning"]


def _ctx_fit(X, K, n_init, max_iter, random_state):
    from spatialcore_amd import _lib
    from spatialcore_amd.spatial.neighborhoods import kmeans_draws

    tol = np.mean(np.var(X, axis=0)) * 1e-4
    draws = kmeans_draws(random_state, n_init, K)
    return _lib.default_context(0).kmeans(X, K, n_init, max_iter, float(tol), X.mean(axis=0), draws), draws


@pytest.mark.parametrize("name", CASES)
def test_niches_match_reference(name):
    P = G[f"profile_{G[f'{name}_kind']}"]
    K, n_init, rs, max_iter = (int(G[f"{name}_{k}"]) for k in ("n_niches", "n_init", "random_state", "max_iter"))
    fit, _ = _ctx_fit(P, K, n_init, max_iter, rs)
    stable = G[f"{name}_seed_stable"]
    np.testing.assert_array_equal(fit["seeds"][stable], G[f"{name}_seeds"][stable])
    a, warn = _run(P, n_niches=K, random_state=rs, n_init=n_init, max_iter=max_iter)
    cat = a.obs["niche"]
    assert list(cat.cat.categories) == [str(c) for c in G[f"{name}_categories"]]
    prm = dict(a.uns["niche_params"])
    ref_inertia = float(G[f"{name}_inertia"])
    assert prm.pop("inertia") == pytest.approx(ref_inertia, rel=2e-2 if name in LATTICE_TIES else 1e-5,
                                               abs=1e-9)
    assert prm == {"n_niches": K, "method": "kmeans", "neighborhood_key": "neighborhood_profile",
                   "random_state": rs, "n_init": n_init, "max_iter": max_iter}
    assert a.uns["niche_centroids"].dtype == P.dtype
    codes = cat.cat.codes.to_numpy()
    if name.startswith("dup"):
        assert ari(codes, G[f"{name}_labels"]) == 1.0
        assert warn == [str(G[f"{name}_warning"])]
        return
    assert warn == []
    if name in LATTICE_TIES:
        return
    assert ari(codes, G[f"{name}_labels"]) == 1.0
    np.testing.assert_allclose(a.uns["niche_centroids"], G[f"{name}_centroids"], rtol=0, atol=1e-3)


@pytest.mark.parametrize("n,C,K,n_init,max_iter,dtype,seed", BLOB_SHAPES)
def test_kmeans_matches_restatement(n, C, K, n_init, max_iter, dtype, seed):
    """Equality throughout: the restatement sums in the kernels' own orders (kernel_order=True)."""
    X = blobs(n, C, K, seed, dtype)
    fit, draws = _ctx_fit(X, K, n_init, max_iter, seed)
    ref = kr.fit(X, K, n_init, max_iter, draws, kernel_order=True)
    np.testing.assert_array_equal(fit["seeds"], ref["seeds"])
    np.testing.assert_array_equal(fit["labels"], ref["labels"])
    assert fit["inertia"] == ref["inertia"]
    assert fit["n_iter"] == ref["n_iter"] and fit["strict"] == ref["strict"] and fit["distinct"] == ref["distinct"]
    assert fit["centers"].dtype == X.dtype
    np.testing.assert_array_equal(fit["centers"], ref["centers"])


def test_kmeans_is_bit_reproducible():
    X = blobs(20000, 12, 8, 9, np.float32)
    a, _ = _ctx_fit(X, 8, 10, 300, 0)
    b, _ = _ctx_fit(X, 8, 10, 300, 0)
    for k in ("labels", "centers", "seeds"):
        np.testing.assert_array_equal(a[k], b[k])
    assert a["inertia"] == b["inertia"]


def test_profile_then_niches_end_to_end():
    from spatialcore_amd.spatial import compute_neighborhood_profile, identify_niches

    rng = np.random.default_rng(2)
    n = 5000
    coords = rng.uniform(0, 700, (n, 2))
    labels = np.where(coords[:, 0] < 350, rng.choice(["A", "B", "C"], n, p=[.7, .2, .1]),
                      rng.choice(["A", "B", "C"], n, p=[.1, .2, .7]))
    ad = make_adata(coords, np.zeros((n, 1)), labels)
    compute_neighborhood_profile(ad, celltype_column="cell_type", k=10)
    identify_niches(ad, n_niches=3)
    assert ad.obs["niche"].cat.categories.tolist() == ["niche_1", "niche_2", "niche_3"]
    assert ad.uns["niche_centroids"].shape == (3, 3)
    ops = [o["function"] for o in ad.uns["spatialcore_metadata"]["operations"]]
    assert ops == ["compute_neighborhood_profile", "identify_niches"]


def test_minibatch_is_answered_by_lloyd():
    X = blobs(4000, 6, 5, 11, np.float32)
    a, _ = _run(X, n_niches=5, method="kmeans")
    b, _ = _run(X, n_niches=5, method="minibatch_kmeans")
    np.testing.assert_array_equal(a.obs["niche"].cat.codes.to_numpy(), b.obs["niche"].cat.codes.to_numpy())
    assert b.uns["niche_params"]["method"] == "minibatch_kmeans"
    entry = b.uns["spatialcore_metadata"]["operations"][-1]
    assert entry["parameters"]["algorithm"] == "lloyd" and entry["parameters"]["method"] == "minibatch_kmeans"


def test_niches_at_size():
    """10^6 cells x 20 cell types, K = 8, n_init = 10, max_iter = 300."""
    from spatialcore_amd.spatial import identify_niches

    n, C, K = 1_000_000, 20, 8
    rng = np.random.default_rng(0)
    mix = rng.dirichlet(np.full(C, 0.5), size=12)
    P = rng.dirichlet(np.ones(C), size=n) * 0.3 + mix[rng.integers(0, 12, n)] * 0.7
    P = P.astype(np.float32)
    fit, draws = _ctx_fit(P, K, 10, 300, 0)
    ref = kr.fit(P, K, 10, 300, draws, seeding_only=True)
    np.testing.assert_array_equal(fit["seeds"], ref["seeds"])
    X64 = P.astype(np.float64)
    d = kr._dist_all(X64, fit["centers"].astype(np.float64))
    ds = np.sort(d, axis=1)
    clear = (ds[:, 1] - ds[:, 0]) > 1e-5 * ds[:, 1]     # a near-tie may round either way once X_mean is added back
    np.testing.assert_array_equal(fit["labels"][clear], np.argmin(d, axis=1)[clear])
    if fit["strict"]:
        for k in range(K):
            np.testing.assert_allclose(X64[fit["labels"] == k].mean(axis=0), fit["centers"][k], rtol=0, atol=1e-6)
    a = _adata(P)
    t0 = time.perf_counter()
    identify_niches(a, n_niches=K)
    wall = time.perf_counter() - t0
    print(f"identify_niches 10^6 x 20, K=8, n_init=10: {wall:.3f} s, n_iter {fit['n_iter']}, strict {fit['strict']}")
    np.testing.assert_array_equal(a.obs["niche"].cat.codes.to_numpy(), fit["labels"])
